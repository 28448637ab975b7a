"""MultiDiscreteFF -- drop-in for rlgym_ppo/ppo/multi_discrete_policy.py:16-89 (+ MultiDiscreteRolv,
util/torch_functions.py:81-122) on librlppo's fused forward + 8-way categorical sampling kernel.

`bins` (not in the reference, whose bins are literals): the nvec of a MultiDiscrete(nvec) action space -- H = len(bins) heads,
sum(bins) outputs, every head padded to B = max(bins) where the reference pads its 2-way heads to 3.  None or the reference's own
list [3, 3, 3, 3, 3, 2, 2, 2] is the reference's policy on the fixed kernels, launch for launch; anything else runs the general
kernels (rlppo_multidiscrete_act_nvec; limits: include/rlppo.h, RLPPO_MD_MAX_*).

`action_mask` (not in the reference): invalid-action masking per component, the sb3-contrib MaskablePPO convention -- one entry per
LOGIT, [n, sum(bins)] bool / 0-1 (host or device, or util.action_mask.Packed), head h owning columns [s_h, s_h + b_h).  A head's
distribution is the Categorical over its valid bins; every head of every row needs at least one (a host mask is checked, naming row
and head).  A masked call always runs the general kernels, also on the reference's bins; get_output returns logits, which no mask
changes, and keeps refusing one.  A host mask on a small host batch rides a masked hipGraph like the unmasked small call
(ppo/_mlp.py::ActGraph, cached under (bucket, True)): the mask is packed and checked on the host and its words are staged with the
observations; a device mask or a Packed one takes the eager path."""
import ctypes

import numpy as np
import torch

from .. import _native as N
from ..engine import host_exponential, ptr, stream_ptr
from ..util import action_mask as AM
from ..util import torch_functions
from ._mlp import ArenaModule, build_body


def _no_action_mask(action_mask):
    if action_mask is not None:
        raise ValueError("action_mask: get_output of the multi-discrete head returns logits, which no mask changes -- pass the mask to "
                         "get_action / act_padded / get_backprop_data")


REFERENCE_BINS = (3, 3, 3, 3, 3, 2, 2, 2)  # multi_discrete_policy.py:20


def check_bins(bins):
    """bins -> a list of ints within the library's limits (ValueError otherwise)."""
    try:
        out = [int(b) for b in bins]
        exact = all(float(b) == float(i) for b, i in zip(bins, out))
    except (TypeError, ValueError):
        raise ValueError(f"multi-discrete bins must be a sequence of integers, got {bins!r}") from None
    if not exact or not 1 <= len(out) <= N.MD_MAX_HEADS:
        raise ValueError(f"multi-discrete bins: 1 .. {N.MD_MAX_HEADS} integer entries, got {bins!r}")
    if min(out) < 1 or max(out) > N.MD_MAX_BINS:
        raise ValueError(f"multi-discrete bins: every entry must be in 1 .. {N.MD_MAX_BINS}, got {bins!r}")
    if sum(out) > N.MD_MAX_LOGITS:
        raise ValueError(f"multi-discrete bins: at most {N.MD_MAX_LOGITS} logits in all, got {sum(out)}")
    return out


class MultiDiscreteFF(ArenaModule):
    def __init__(self, input_shape, layer_sizes, device, bins=None):
        super().__init__()
        bins = list(REFERENCE_BINS) if bins is None else check_bins(bins)
        self.model = build_body(input_shape, layer_sizes, sum(bins))
        self.splits = bins
        self.n_heads, self.max_bins, self.n_logits = len(bins), max(bins), sum(bins)
        self.mask_layout = AM.Layout(self.n_logits, bins)   # one mask entry per logit
        # the general kernels' nvec (HOST memory the library reads during a call); None = the reference's bins on the fixed kernels.
        # (`_force_general`: measurements run the general kernels on the reference's bins -- tools/multidiscrete_bins_cost.py)
        self._force_general = False
        self._nvec_c = (ctypes.c_int32 * len(bins))(*bins)
        self._general = tuple(bins) != REFERENCE_BINS
        self.multi_discrete = torch_functions.MultiDiscreteRolv(bins)
        self._finish(device)

    @property
    def md_nvec(self):
        """The ctypes nvec the library's general kernels take, or None where the fixed kernels (the reference's bins) run."""
        return self._nvec_c if (self._general or self._force_general) else None

    @torch.no_grad()
    def get_output(self, obs, action_mask=None):
        _no_action_mask(action_mask)
        rows = self.arena.stage_obs(obs)
        return self.arena.forward(rows)[:, :self.n_logits]

    @torch.no_grad()
    def get_action(self, obs, deterministic=False, noise=None, standardize=None, action_mask=None):
        a = self.arena
        if deterministic:
            logits = self.get_output(obs)
            if action_mask is not None:  # the arg-max over each head's valid bins
                logits = logits.masked_fill(~self.mask_layout.valid(action_mask, logits.device), float("-inf"))
            action, start = [], 0
            for split in self.splits:
                action.append(logits[..., start:start + split].argmax(dim=-1))
                start += split
            return torch.stack(action).cpu().numpy(), 0
        # small host batches: one hipGraph replay (ppo/_mlp.py), with a host mask too (its words are staged with the observations)
        out = self._graph_act(obs, noise, standardize, action_mask)
        if out is not None:
            return out
        rows = a.stage_obs(obs, standardize)
        actions, logp = self.act_padded(rows, noise, action_mask)
        return actions.cpu(), logp.cpu()

    # ---- hooks of the graph-replayed rollout step (ppo/_mlp.py::ActGraph)
    _masked_chain = True  # a masked graph's body: the layer chain + rlppo_multidiscrete_act_nvec_masked (no one-launch step here)

    def _noise_shape(self, n):
        return (n * self.n_heads, self.max_bins)

    def _draw_noise(self, n, device=None):
        if device is not None and self.noise_mode == "device":
            return torch.empty(self._noise_shape(n), device=device).exponential_(1)  # fast mode: torch's HIP generator, not the reference's CPU stream
        # Categorical.sample -> multinomial on [n*H, B]: torch.empty(n*H, B).exponential_(1)
        return host_exponential(self._noise_shape(n), device=device)

    def _action_buffer(self, cap, device=None):
        return torch.empty((cap, self.n_heads), dtype=torch.int64, device=device)

    def _act_launch(self, rows, n, noise, actions, logp, ws, opts=None, mask_words=None):
        a = self.arena
        nvec = self.md_nvec
        opts = a.act_opts(opts)
        if mask_words is not None:  # a masked call runs the general kernel, also on the reference's bins
            N.check(N.lib().rlppo_multidiscrete_act_nvec_masked(stream_ptr(), a.dims_c, a.n_layers, ptr(a.packed), ptr(rows), rows.shape[1],
                                                                n, ptr(noise), ptr(actions), ptr(logp), ptr(ws), ws.numel(), opts,
                                                                self._nvec_c, self.n_heads, ptr(mask_words), mask_words.shape[1]))
        elif nvec is None:
            N.check(N.lib().rlppo_multidiscrete_act(stream_ptr(), a.dims_c, a.n_layers, ptr(a.packed), ptr(rows), rows.shape[1],
                                                    n, ptr(noise), ptr(actions), ptr(logp), ptr(ws), ws.numel(), opts))
        else:
            N.check(N.lib().rlppo_multidiscrete_act_nvec(stream_ptr(), a.dims_c, a.n_layers, ptr(a.packed), ptr(rows), rows.shape[1],
                                                         n, ptr(noise), ptr(actions), ptr(logp), ptr(ws), ws.numel(),
                                                         opts, nvec, self.n_heads))

    def get_backprop_data(self, obs, acts, action_mask=None):
        """Compatibility accessor with an autograd graph (multi_discrete_policy.py:76-89); unused by PPOLearner.
        action_mask (optional): the masked semantics of the update -- invalid logits -inf before make_distribution."""
        if not isinstance(obs, torch.Tensor):
            obs = torch.as_tensor(np.asarray(obs), dtype=torch.float32, device=self.arena.device)
        dist = self.multi_discrete
        logits = self.model(obs)
        if action_mask is not None:
            logits = logits.masked_fill(~self.mask_layout.valid(action_mask, logits.device).view(logits.shape), float("-inf"))
        dist.make_distribution(logits)
        return dist.log_prob(acts), dist.entropy().mean()
