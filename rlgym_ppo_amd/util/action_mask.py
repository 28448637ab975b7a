"""Action masks at the library boundary (include/rlppo.h, rlppo_act_opts.action_mask / rlppo_minibatch_args.action_mask).

A mask row marks each of the A actions valid (1 / True) or invalid (0 / False).  The kernels read it packed: W = ceil(A / 32)
32-bit words per row, bit c % 32 of word c / 32 set = action c valid, bits at and beyond A clear.  `pack` builds that form on
the device from a bool / 0-1 array or tensor [n, A] (host or device); `unpack` is its inverse for the accessors.

The multi-discrete head (MultiDiscrete(nvec)) uses the same encoding with one bit per LOGIT: A = S = sum(nvec), head h owns bits
[s_h, s_h + b_h).  `pack(..., heads=nvec)` / `check_heads` hold a host mask to the per-head rule: every head of every row keeps at
least one valid bin.
"""
import numpy as np
import torch


class Packed(object):
    """Masks already in the kernels' form: int32 device words [n, W] + the action count they describe (what a device-resident
    rollout hands from the collector to the buffer without unpacking)."""
    __slots__ = ("words", "n_actions")

    def __init__(self, words, n_actions):
        self.words, self.n_actions = words, int(n_actions)

    @property
    def shape(self):
        return (self.words.shape[0], self.n_actions)

    def unpack(self):
        return unpack(self.words, self.n_actions)


def mask_words(n_actions):
    """Words per row: ceil(A / 32)."""
    return (int(n_actions) + 31) // 32


_STARTS = {}


def _heads_ok(m, heads):
    """bool [n, sum(heads)], heads a tuple of ints >= 1 -> True when every head of every row keeps a valid bin: one pass over the
    rows for all heads (this runs per small get_action call of a masked multi-discrete rollout).  False = look closer (the callers'
    loops word the error)."""
    starts = _STARTS.get(heads)
    if starts is None:
        if not heads or min(heads) < 1 or len(_STARTS) > 64:
            return False
        starts = _STARTS[heads] = np.cumsum((0,) + heads[:-1])
    return m.shape[0] > 0 and bool(np.logical_or.reduceat(m, starts, axis=1).all())


def check_heads(mask, heads):
    """Host bool / 0-1 [n, sum(heads)]: a head without a valid bin raises ValueError naming the row and the head (a head with
    exactly one valid bin is fine: it contributes log-probability 0 and entropy 0)."""
    m = np.asarray(mask)
    if m.ndim == 1:
        m = m.reshape(1, -1)
    heads = [int(b) for b in heads]
    if m.ndim != 2 or m.shape[1] != sum(heads):
        raise ValueError(f"action mask shape {tuple(m.shape)} != (n, {sum(heads)}) for bins {tuple(heads)}")
    m = m != 0
    if _heads_ok(m, tuple(heads)):
        return
    s = 0
    for h, b in enumerate(heads):
        empty = np.flatnonzero(~m[:, s:s + b].any(axis=1))
        if empty.size:
            raise ValueError(f"action mask: row {int(empty[0])}, head {h} (bins {s} .. {s + b - 1}) has no valid bin")
        s += b


def pack_host(mask, n_actions, heads=None):
    """numpy bool / 0-1 [n, A] -> int32 words [n, W]; a row without a valid action raises ValueError naming it (heads: the
    multi-discrete head's nvec -- a head without a valid bin raises, naming row and head)."""
    m = np.asarray(mask)
    if m.ndim == 1:
        m = m.reshape(1, -1)
    if m.ndim != 2 or m.shape[1] != int(n_actions):
        raise ValueError(f"action mask shape {tuple(m.shape)} != (n, {int(n_actions)})")
    m = m != 0
    if heads is None or not _heads_ok(m, tuple(int(b) for b in heads)):   # (every head with a valid bin: every row with a valid action)
        if heads is not None:
            check_heads(m, heads)
        empty = np.flatnonzero(~m.any(axis=1))
        if empty.size:
            raise ValueError(f"action mask: row {int(empty[0])} has no valid action")
    w = mask_words(n_actions)
    padded = np.zeros((m.shape[0], w * 32), dtype=bool)
    padded[:, :m.shape[1]] = m
    by = np.packbits(padded, axis=1, bitorder="little")           # byte k of a row = actions 8 k .. 8 k + 7, LSB first
    return np.ascontiguousarray(by).view("<u4").astype(np.uint32, copy=False).view(np.int32).reshape(m.shape[0], w)


def pack(mask, n_actions, device, heads=None):
    """bool / 0-1 array or tensor [n, A], host or device -> int32 words [n, W] on `device`.  Host input is checked for rows
    without a valid action (ValueError naming the row) and, with heads = the multi-discrete head's nvec (A = sum(heads)), for
    heads without a valid bin (ValueError naming row and head); device input is not read back -- the kernels treat such a row
    (such a head) as all-valid."""
    A = int(n_actions)
    if isinstance(mask, Packed):
        if mask.n_actions != A:
            raise ValueError(f"packed action mask of {mask.n_actions} actions != {A}")
        return mask.words.to(device).contiguous()
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        m = mask.detach()
        if m.dim() == 1:
            m = m.view(1, -1)
        if m.dim() != 2 or m.shape[1] != A:
            raise ValueError(f"action mask shape {tuple(m.shape)} != (n, {A})")
        w = mask_words(A)
        bits = torch.zeros((m.shape[0], w * 32), dtype=torch.int32, device=m.device)
        bits[:, :A] = (m != 0).to(torch.int32)
        shifts = torch.arange(32, dtype=torch.int32, device=m.device)
        # distinct bits: the int32 sum is their OR (bit 31 wraps into the sign, the word's bit pattern)
        words = (bits.view(m.shape[0], w, 32) << shifts).sum(-1, dtype=torch.int32)
        return words.to(device).contiguous()
    if isinstance(mask, torch.Tensor):
        mask = mask.detach().numpy()
    return torch.from_numpy(pack_host(mask, A, heads)).to(device, non_blocking=False)


def unpack(words, n_actions):
    """int32 words [n, W] (tensor, any device) -> bool tensor [n, A] on the same device."""
    A = int(n_actions)
    w = mask_words(A)
    t = words.reshape(-1, w).to(torch.int64)
    shifts = torch.arange(32, device=t.device)
    bits = ((t.unsqueeze(-1) >> shifts) & 1).reshape(t.shape[0], w * 32)
    return bits[:, :A] != 0
