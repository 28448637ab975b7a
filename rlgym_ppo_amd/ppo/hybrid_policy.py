"""HybridPolicy -- Gaussian axes and categorical buttons in one action (include/rlppo.h, "[hybrid]"): the network
has k + sum(bins) outputs, the first k the unbounded means of DiagGaussianPolicy's distribution (one learnable `log_std` k-vector in
the tail of the arena), the rest the logits of MultiDiscreteFF's len(bins) independent categoricals.

An action row is k + len(bins) float32 values: the k samples as drawn (not clamped), then the bin indices.  log p is the sum of the two
halves', a row's entropy the sum of Normal.entropy() over the k dimensions and of the heads' entropies (no division by anything).

Noise: `_draw_noise` draws the Gaussian half's N(0, 1) numbers [n, k] and then the categorical half's Exp(1) numbers
[n * len(bins), max(bins)] -- the streams DiagGaussianPolicy and MultiDiscreteFF draw, in that order -- as ONE flat tensor; a caller's
`noise` is that flat tensor or the pair (eps, q).  Both noise modes work; the small-batch graph replay is not taken (eager path)."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from .. import _native as N
from ..engine import host_exponential, ptr, stream_ptr
from ._mlp import ArenaModule, build_body
from .continuous_policy import _no_action_mask
from .diag_gaussian_policy import ENTROPY_CONST, DiagGaussianPolicy, check_log_std_init
from .multi_discrete_policy import check_bins


class HybridPolicy(ArenaModule):
    def __init__(self, input_shape, k, bins, layer_sizes, device, log_std_init=0.0):
        super().__init__()
        k = int(k)
        if not 1 <= k <= N.DIAG_MAX_K:
            raise ValueError(f"HybridPolicy: k={k} Gaussian dimensions, 1 .. {N.DIAG_MAX_K} (RLPPO_DIAG_MAX_K) are supported")
        bins = check_bins(bins)
        log_std_init = check_log_std_init(log_std_init)
        self.k, self.splits = k, bins
        self.n_heads, self.max_bins, self.n_logits = len(bins), max(bins), sum(bins)
        self.n_out = k + self.n_logits
        self.act_dim = k + self.n_heads
        self.model = build_body(input_shape, layer_sizes, self.n_out)   # plain bias on the last layer
        # a constant fill, created after the body: it consumes nothing from the CPU generator
        self.log_std = nn.Parameter(torch.full((k,), log_std_init, dtype=torch.float32))
        self._arena_tail = (self.log_std,)
        self._nvec_c = (ctypes.c_int32 * len(bins))(*bins)   # HOST memory the library reads during a call
        self._finish(device)
        self.act_graphs = False   # the captured small call is not built for this head: get_action takes the eager path

    fill_log_std = DiagGaussianPolicy.fill_log_std
    _log_std_dev = DiagGaussianPolicy._log_std_dev

    def _heads(self, logits):
        return torch.split(logits, self.splits, dim=-1)

    @torch.no_grad()
    def get_output(self, obs, action_mask=None):
        """-> (mean [n, k], std [k], logits [n, sum(bins)]) on the device."""
        _no_action_mask(action_mask)
        y = self.arena.forward(self.arena.stage_obs(obs), out_tanh=False)
        return y[:, :self.k], self._log_std_dev().detach().exp(), y[:, self.k:self.n_out]

    @torch.no_grad()
    def get_action(self, obs, deterministic=False, noise=None, standardize=None, action_mask=None):
        _no_action_mask(action_mask)
        a = self.arena
        rows = a.stage_obs(obs, standardize)
        if deterministic:   # the means, and each head's arg-max of its logits, row by row
            y = a.forward(rows, out_tanh=False)
            idx = [z.argmax(dim=-1).float() for z in self._heads(y[:, self.k:self.n_out])]
            return torch.cat([y[:, :self.k], torch.stack(idx, dim=1)], dim=1).cpu(), 0
        actions, logp = self.act_padded(rows, noise)
        return actions.cpu(), logp.cpu()

    # ---- hooks of ArenaModule.act_padded
    def _noise_shape(self, n):
        return (n * (self.k + self.n_heads * self.max_bins),)

    def _draw_noise(self, n, device=None):
        q_shape = (n * self.n_heads, self.max_bins)
        if device is not None and self.noise_mode == "device":   # fast mode: torch's HIP generator
            return torch.cat([torch.empty(n * self.k, device=device).normal_(0, 1), torch.empty(q_shape, device=device).exponential_(1).flatten()])
        return torch.cat([torch.empty(n, self.k).normal_(0, 1).flatten(), host_exponential(q_shape).flatten()])

    def _action_buffer(self, cap, device=None):
        return torch.empty((cap, self.act_dim), dtype=torch.float32, device=device)

    def _act_launch(self, rows, n, noise, actions, logp, ws, opts=None, mask_words=None):   # (mask_words: never given, act_padded refuses a mask)
        a = self.arena
        q = ctypes.c_void_p(noise.data_ptr() + 4 * n * self.k)   # the Exp(1) numbers lie behind the n * k N(0, 1) ones
        N.check(N.lib().rlppo_hybrid_act(stream_ptr(), a.dims_c, a.n_layers, ptr(a.packed), ptr(rows), rows.shape[1], n, self.k, self._nvec_c,
                                         self.n_heads, ptr(noise), q, ptr(self._log_std_dev()), ptr(actions), ptr(logp), ptr(ws), ws.numel(),
                                         a.act_opts(opts)))

    def act_padded(self, rows, noise=None, action_mask=None):
        _no_action_mask(action_mask)
        if isinstance(noise, (tuple, list)):   # (eps [n, k], q [n * H, B]) -> the flat tensor
            noise = torch.cat([torch.as_tensor(x, dtype=torch.float32).flatten() for x in noise])
        return super().act_padded(rows, noise)

    def get_backprop_data(self, obs, acts, action_mask=None):
        """Compatibility accessor with an autograd graph (stock torch, like the other heads'); unused by PPOLearner.
        -> (log_probs [n], entropy): the mean over the rows of the row entropy."""
        _no_action_mask(action_mask)
        dev = self.arena.device
        if not isinstance(obs, torch.Tensor):
            obs = torch.as_tensor(np.asarray(obs), dtype=torch.float32, device=dev)
        acts = torch.as_tensor(acts, dtype=torch.float32).to(dev)
        y = self.model(obs.to(dev))
        log_probs = DiagGaussianPolicy.logpdf(acts[:, :self.k], y[:, :self.k], self.log_std).sum(dim=1)
        entropy = (ENTROPY_CONST + self.log_std).sum()
        for h, z in enumerate(self._heads(y[:, self.k:])):
            cat = torch.distributions.Categorical(logits=z)
            log_probs = log_probs + cat.log_prob(acts[:, self.k + h].long())
            entropy = entropy + cat.entropy().mean()
        return log_probs, entropy
