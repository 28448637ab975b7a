"""Action masks at the library boundary (include/rlppo.h, rlppo_act_opts.action_mask / rlppo_minibatch_args.action_mask).

A mask row marks each of the A actions valid (1 / True) or invalid (0 / False).  The kernels read it packed: W = ceil(A / 32)
32-bit words per row, bit c % 32 of word c / 32 set = action c valid, bits at and beyond A clear.

The multi-discrete head (MultiDiscrete(nvec)) uses the same encoding with one bit per LOGIT: A = S = sum(nvec), head h owns bits
[s_h, s_h + b_h).

`Layout` is the one owner of that geometry and of its rules: how wide a mask row of a policy is, which bins each head owns, that
every head of every row of a HOST mask keeps at least one valid bin (the discrete head is one head: every row keeps a valid
action), and that a head which keeps none -- possible only in a device mask, which is never read back -- counts as all-valid, as in
the kernels.  A policy that masks states its layout as `policy.mask_layout`; everybody else asks `Layout.of(policy)`.  The module
functions below are the same operations for callers that hold a width (and bins) instead of a policy.
"""
import numpy as np
import torch

REFUSAL = "invalid-action masking is an option of the discrete head (DiscreteFF) and of the multi-discrete head (MultiDiscreteFF)"


def mask_words(n_actions):
    """Words per row: ceil(A / 32)."""
    return (int(n_actions) + 31) // 32


class Layout(object):
    """width: entries of a mask row; heads: the multi-discrete head's bins (a tuple, sum = width) or None for the discrete head;
    words: int32 words of a packed row; starts: the first entry of every head (the discrete head: one head at 0).  Immutable."""
    __slots__ = ("width", "heads", "words", "starts")

    def __init__(self, width, heads=None):
        width = int(width)
        if heads is not None:
            heads = tuple(int(b) for b in heads)
            if not heads or min(heads) < 1 or sum(heads) != width:
                raise ValueError(f"action mask layout: bins {heads} do not add up to {width} entries of at least one bin each")
        elif width < 1:
            raise ValueError(f"action mask layout: {width} actions")
        set_ = object.__setattr__
        set_(self, "width", width), set_(self, "heads", heads), set_(self, "words", mask_words(width))
        set_(self, "starts", np.cumsum((0,) + heads[:-1]) if heads is not None else np.zeros(1, dtype=np.int64))
        self.starts.flags.writeable = False

    def __setattr__(self, name, value):
        raise AttributeError("Layout is immutable")

    def __repr__(self):
        return f"Layout({self.width}, heads={self.heads})"

    @classmethod
    def of(cls, policy):
        """The layout of a policy's masks: policy.mask_layout; for a policy of another class, what its (n_logits, splits) or its
        n_actions say; a policy with none of them cannot be masked."""
        lay = getattr(policy, "mask_layout", None)
        if lay is not None:
            return lay
        n_logits, splits = getattr(policy, "n_logits", None), getattr(policy, "splits", None)
        if n_logits is not None and splits is not None:
            return cls(n_logits, splits)
        if getattr(policy, "n_actions", None) is not None:
            return cls(policy.n_actions)
        raise ValueError(f"{REFUSAL}, not of {type(policy).__name__} (a policy of another class states its layout as "
                         "policy.mask_layout, as policy.n_logits, policy.splits or as policy.n_actions)")

    def rows(self, mask):
        """A host mask, bool / 0-1 [n, width] or one row [width] -> bool [n, width]."""
        m = np.asarray(mask)
        if m.ndim == 1:
            m = m.reshape(1, -1)
        if m.ndim != 2 or m.shape[1] != self.width:
            raise ValueError(f"action mask shape {tuple(m.shape)} != (n, {self.width})"
                             + (f" for bins {self.heads}" if self.heads is not None else ""))
        return m if m.dtype == bool else m != 0

    def first_empty(self, m):
        """bool [n, width] -> None when every head of every row keeps a valid bin (a head with exactly one is fine: it contributes
        log-probability 0 and entropy 0), else (row, head) of the first one that does not, rows first -- head None for the
        discrete head.  One pass over the rows for all heads: this runs per small get_action call of a masked rollout."""
        ok = np.logical_or.reduceat(m, self.starts, axis=1)   # [n, H]: head h keeps a valid bin
        if ok.all():
            return None
        r, h = np.argwhere(~ok)[0]
        return int(r), (int(h) if self.heads is not None else None)

    def what(self, head):
        """The tail of the error for first_empty's head: callers put "action mask: row r" / "... worker p, agent a" in front."""
        if head is None:
            return " has no valid action"
        s = int(self.starts[head])
        return f", head {head} (bins {s} .. {s + self.heads[head] - 1}) has no valid bin"

    def checked(self, mask):
        """rows(mask), held to the rule: ValueError naming the first row (and head) without a valid bin."""
        m = self.rows(mask)
        bad = self.first_empty(m)
        if bad is not None:
            raise ValueError(f"action mask: row {bad[0]}{self.what(bad[1])}")
        return m

    def pack_host(self, mask):
        """Host mask -> int32 numpy words [n, words], checked."""
        m = self.checked(mask)
        padded = np.zeros((m.shape[0], self.words * 32), dtype=bool)
        padded[:, :self.width] = m
        by = np.packbits(padded, axis=1, bitorder="little")           # byte k of a row = actions 8 k .. 8 k + 7, LSB first
        return np.ascontiguousarray(by).view("<u4").astype(np.uint32, copy=False).view(np.int32).reshape(m.shape[0], self.words)

    def pack(self, mask, device):
        """bool / 0-1 array or tensor [n, width], host or device, or Packed -> int32 words [n, words] on `device`.  Host input is
        checked; device input is not read back -- the kernels treat a head without a valid bin as all-valid."""
        if isinstance(mask, Packed):
            if mask.n_actions != self.width:
                raise ValueError(f"packed action mask of {mask.n_actions} actions != {self.width}")
            return mask.words.to(device).contiguous()
        if isinstance(mask, torch.Tensor) and mask.is_cuda:
            m = mask.detach()
            if m.dim() == 1:
                m = m.view(1, -1)
            if m.dim() != 2 or m.shape[1] != self.width:
                raise ValueError(f"action mask shape {tuple(m.shape)} != (n, {self.width})")
            bits = torch.zeros((m.shape[0], self.words * 32), dtype=torch.int32, device=m.device)
            bits[:, :self.width] = (m != 0).to(torch.int32)
            shifts = torch.arange(32, dtype=torch.int32, device=m.device)
            # distinct bits: the int32 sum is their OR (bit 31 wraps into the sign, the word's bit pattern)
            words = (bits.view(m.shape[0], self.words, 32) << shifts).sum(-1, dtype=torch.int32)
            return words.to(device).contiguous()
        if isinstance(mask, torch.Tensor):
            mask = mask.detach().numpy()
        return torch.from_numpy(self.pack_host(mask)).to(device, non_blocking=False)

    def unpack(self, words):
        """int32 words [n, words] (tensor, any device) -> bool tensor [n, width] on the same device."""
        t = words.reshape(-1, self.words).to(torch.int64)
        shifts = torch.arange(32, device=t.device)
        bits = ((t.unsqueeze(-1) >> shifts) & 1).reshape(t.shape[0], self.words * 32)
        return bits[:, :self.width] != 0

    def valid(self, mask, device):
        """A mask in any accepted form -> bool tensor [n, width] on `device` as the kernels read it: a head without a valid bin
        counts as all-valid (only a tensor or Packed words can hold one: a host array is checked)."""
        if isinstance(mask, Packed):
            m = self.unpack(self.pack(mask, mask.words.device))   # (pack: the words as they are, held to this width)
        elif isinstance(mask, torch.Tensor):
            m = mask.detach() != 0
        else:
            m = torch.from_numpy(self.checked(mask))
        m = m.to(device).view(-1, self.width)
        if self.heads is None:
            return torch.where(m.any(dim=-1, keepdim=True), m, torch.ones_like(m))
        parts = [torch.where(p.any(dim=-1, keepdim=True), p, torch.ones_like(p)) for p in torch.split(m, self.heads, dim=-1)]
        return torch.cat(parts, dim=-1)


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


def check_heads(mask, heads):
    """Host bool / 0-1 [n, sum(heads)]: a head without a valid bin raises ValueError naming the row and the head."""
    heads = tuple(heads)
    Layout(sum(int(b) for b in heads), heads).checked(mask)


def pack_host(mask, n_actions, heads=None):
    """numpy bool / 0-1 [n, A] -> int32 words [n, W]; a row without a valid action raises ValueError naming it (heads: the
    multi-discrete head's nvec -- a head without a valid bin raises, naming row and head)."""
    return Layout(n_actions, heads).pack_host(mask)


def pack(mask, n_actions, device, heads=None):
    """Layout(n_actions, heads).pack(mask, device)."""
    return Layout(n_actions, heads).pack(mask, device)


def unpack(words, n_actions):
    """int32 words [n, W] (tensor, any device) -> bool tensor [n, A] on the same device."""
    return Layout(n_actions).unpack(words)
