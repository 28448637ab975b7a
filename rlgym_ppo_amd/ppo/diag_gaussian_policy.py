"""DiagGaussianPolicy -- the continuous head of Stable-Baselines3 / CleanRL / rl_games (not in the reference): an unbounded mean
from the network and ONE learnable, state-independent `log_std` vector (include/rlppo.h, "[diag]").

Against ContinuousPolicy (the reference's head): no tanh on the mean, sigma = exp(log_std) is a parameter and not a network output
mapped into `continuous_var_range`, the sample is not clamped, the log-probability is that of the sample actually drawn, and a
row's entropy is the SUM over the action dimensions of Normal.entropy() (no division by k).  `log_std` lives in the tail of the
policy's arena, behind the layers: the optimiser, the gradient exchange and checkpoints cover it with the arena.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from ..engine import ptr, stream_ptr
from ._mlp import ArenaModule, build_body
from .continuous_policy import _no_action_mask

ENTROPY_CONST = 1.4189385332046727  # 1/2 + 1/2 log(2 pi)


def check_log_std_init(value):
    v = float(value)
    if not math.isfinite(v):
        raise ValueError(f"log_std_init must be a finite number, got {value!r}")
    return v


class DiagGaussianPolicy(ArenaModule):
    def __init__(self, input_shape, output_shape, layer_sizes, device, log_std_init=0.0):
        super().__init__()
        k = int(output_shape)
        if not 1 <= k <= N.DIAG_MAX_K:
            raise ValueError(f"DiagGaussianPolicy: {k} action dimensions, 1 .. {N.DIAG_MAX_K} (RLPPO_DIAG_MAX_K) are supported")
        log_std_init = check_log_std_init(log_std_init)
        self.model = build_body(input_shape, layer_sizes, k)   # plain bias on the last layer: the mean is unbounded
        # a constant fill, created after the body: it consumes nothing from the CPU generator
        self.log_std = nn.Parameter(torch.full((k,), log_std_init, dtype=torch.float32))
        self.n_out = k
        self._arena_tail = (self.log_std,)
        self._finish(device)

    @torch.no_grad()
    def fill_log_std(self, value):
        """log_std <- value in every dimension (in place, in the arena: the next call of any kernel sees it)."""
        self._log_std_dev().fill_(check_log_std_init(value))

    def _log_std_dev(self):
        """The parameter where the kernels read it: its slice of the arena (re-bound first if somebody moved it)."""
        a = self.arena
        if not a.is_bound():
            a.bind()
        return self.log_std

    @torch.no_grad()
    def get_output(self, obs, action_mask=None):
        """-> (mean [n, k], std [k]) on the device."""
        _no_action_mask(action_mask)
        rows = self.arena.stage_obs(obs)
        return self.arena.forward(rows, out_tanh=False)[:, :self.n_out], self._log_std_dev().detach().exp()

    @torch.no_grad()
    def get_action(self, obs, deterministic=False, noise=None, standardize=None, action_mask=None):
        _no_action_mask(action_mask)
        a = self.arena
        if deterministic:   # the mean, row by row
            rows = a.stage_obs(obs, standardize)
            return a.forward(rows, out_tanh=False)[:, :self.n_out].cpu(), 0
        out = self._graph_act(obs, noise, standardize)  # small host batches: one hipGraph replay (ppo/_mlp.py)
        if out is not None:
            return out
        rows = a.stage_obs(obs, standardize)
        actions, logp = self.act_padded(rows, noise)
        return actions.cpu(), logp.cpu()

    # ---- hooks of the graph-replayed rollout step (ppo/_mlp.py::ActGraph)
    def _noise_shape(self, n):
        return (n, self.n_out)

    def _draw_noise(self, n, device=None):
        if device is not None and self.noise_mode == "device":
            return torch.empty(n, self.n_out, device=device).normal_(0, 1)  # fast mode: torch's HIP generator
        return torch.empty(n, self.n_out).normal_(0, 1)  # the stream ContinuousPolicy._draw_noise draws

    def _action_buffer(self, cap, device=None):
        return torch.empty((cap, self.n_out), dtype=torch.float32, device=device)

    def _act_launch(self, rows, n, noise, actions, logp, ws, opts=None, mask_words=None):   # (mask_words: never given, act_padded refuses a mask)
        a = self.arena
        # (log_std's ADDRESS is an argument: the kernel reads the values when it runs, so a captured call follows the parameter)
        N.check(N.lib().rlppo_diag_gaussian_act(stream_ptr(), a.dims_c, a.n_layers, ptr(a.packed), ptr(rows), rows.shape[1], n,
                                                ptr(noise), ptr(self._log_std_dev()), ptr(actions), ptr(logp), ptr(ws), ws.numel(),
                                                a.act_opts(opts)))

    def act_padded(self, rows, noise=None, action_mask=None):
        _no_action_mask(action_mask)
        return super().act_padded(rows, noise)

    @staticmethod
    def logpdf(x, mean, log_std):
        """torch.distributions.Normal(mean, exp(log_std)).log_prob(x), term by term."""
        var = torch.exp(log_std) ** 2
        return -((x - mean) ** 2) / (2 * var) - log_std - math.log(math.sqrt(2 * math.pi))

    def get_backprop_data(self, obs, acts, action_mask=None):
        """Compatibility accessor with an autograd graph (stock torch, like the other heads'); unused by PPOLearner.
        -> (log_probs [n], entropy): the row entropy sum_j (1/2 + 1/2 log 2 pi + log_std_j), the same for every row."""
        _no_action_mask(action_mask)
        dev = self.arena.device
        if not isinstance(obs, torch.Tensor):
            obs = torch.as_tensor(np.asarray(obs), dtype=torch.float32, device=dev)
        acts = torch.as_tensor(acts, dtype=torch.float32).to(dev)
        mean = self.model(obs.to(dev))
        log_probs = self.logpdf(acts, mean, self.log_std).sum(dim=1)
        entropy = (ENTROPY_CONST + self.log_std).sum()
        return log_probs, entropy
