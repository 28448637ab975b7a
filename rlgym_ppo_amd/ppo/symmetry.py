"""Symmetry -- the mirror symmetry of an environment, for PPOLearner.set_symmetry / Learner(symmetry=...).

With one set, every pass of learn() trains on each minibatch row a second time as its mirror image (rsl_rl's symmetry_cfg with
use_data_augmentation, Mittal et al. 2024): the observation permuted and sign-flipped, the action mapped, the stored log-probability,
advantage and value target kept.  This class only DESCRIBES the map and checks that it is well formed; rlppo_mirror_batch
(csrc/mirror.hip) applies it on the device.  Whether the maps describe a true symmetry of the environment -- that the mirrored
observation is one the environment could have produced, and the mirrored action the one that mirrors its effect -- is the USER'S
responsibility: nothing here can check it, and training on a map that is not a symmetry trains on wrong data.
"""
import numpy as np

from .. import _native as N

ZERO = 0xFFFFFFFF  # RLPPO_MIRROR_ZERO


def _perm(name, p, n=None):
    a = np.asarray(p)
    if a.ndim != 1 or a.size == 0 or a.dtype.kind not in "iu":
        raise ValueError(f"Symmetry: {name} must be a non-empty 1-D integer array, got {p!r}")
    a = a.astype(np.int64)
    if n is not None and a.size != n:
        raise ValueError(f"Symmetry: {name} has {a.size} entries, expected {n}")
    seen = np.zeros(a.size, bool)
    for i, v in enumerate(a):
        if not 0 <= v < a.size or seen[v]:
            raise ValueError(f"Symmetry: {name} is not a permutation of range({a.size}): entry {int(v)} at index {i}")
        seen[v] = True
    return a


def _sign(name, s, n):
    a = np.asarray(s, np.float64)
    if a.shape != (n,):
        raise ValueError(f"Symmetry: {name} has shape {a.shape}, expected ({n},)")
    for i, v in enumerate(a):
        if v not in (-1.0, 1.0):
            raise ValueError(f"Symmetry: {name} must hold -1 or +1: entry {float(v)!r} at index {i}")
    return a


def _packed(perm, sign, ld):
    """[ld] uint32: source column with the sign in bit 31; RLPPO_MIRROR_ZERO in the padded columns."""
    t = np.full(ld, ZERO, np.uint32)
    t[:perm.size] = perm.astype(np.uint32) | np.where(sign < 0, np.uint32(0x80000000), np.uint32(0))
    return t


class Symmetry(object):
    """Symmetry(obs_perm, obs_sign, action=..., critic_obs_perm=None, critic_obs_sign=None)

    Mirrored observation: y[j] = obs_sign[j] * x[obs_perm[j]] (critic_obs_* likewise for a critic with observations of its own).
    `action` by policy head:
      discrete        an index array amap: the mirrored action is amap[a];
      multi-discrete  (hperm, binmaps): component h of the mirror is binmaps[h][a[hperm[h]]]; hperm None = identity, binmaps None or
                      a None entry = identity; hperm may only map between components of equal bin count;
      Gaussian heads  (aperm, asign): asign[j] * a[aperm[j]].
    A ValueError names the field and the index of the first offending entry.  What only a policy can decide -- the widths, the bins
    -- is checked by tables(), which PPOLearner.set_symmetry calls.  Whether the maps are a true symmetry of the environment is the
    user's responsibility (module docstring)."""

    def __init__(self, obs_perm, obs_sign, action=None, critic_obs_perm=None, critic_obs_sign=None):
        self.obs_perm = _perm("obs_perm", obs_perm)
        self.obs_sign = _sign("obs_sign", obs_sign, self.obs_perm.size)
        if (critic_obs_perm is None) != (critic_obs_sign is None):
            raise ValueError("Symmetry: critic_obs_perm and critic_obs_sign come together")
        self.critic_obs_perm = self.critic_obs_sign = None
        if critic_obs_perm is not None:
            self.critic_obs_perm = _perm("critic_obs_perm", critic_obs_perm)
            self.critic_obs_sign = _sign("critic_obs_sign", critic_obs_sign, self.critic_obs_perm.size)
        if action is None:
            raise ValueError("Symmetry: action is required (an index array, (hperm, binmaps) or (aperm, asign))")
        self.action = action

    # the three readings of `action`, each checked against what the policy says
    def _discrete(self, n_actions):
        if isinstance(self.action, tuple):
            raise ValueError("Symmetry: action is a pair, but the discrete head takes an index array amap")
        return _perm("action", self.action, n_actions)

    def _pair(self, what):
        if not isinstance(self.action, tuple) or len(self.action) != 2:
            raise ValueError(f"Symmetry: action must be the pair {what} for this policy head, got {self.action!r}")
        return self.action

    def _multi_discrete(self, bins):
        hperm, maps = self._pair("(hperm, binmaps)")
        H = len(bins)
        hperm = np.arange(H) if hperm is None else _perm("action hperm", hperm, H)
        maps = [None] * H if maps is None else list(maps)
        if len(maps) != H:
            raise ValueError(f"Symmetry: action binmaps has {len(maps)} entries, the policy has {H} components")
        for h in range(H):
            if bins[hperm[h]] != bins[h]:
                raise ValueError(f"Symmetry: action hperm maps component {int(hperm[h])} ({bins[hperm[h]]} bins) onto component {h} "
                                 f"({bins[h]} bins) at index {h}: unequal bin count")
            maps[h] = np.arange(bins[h]) if maps[h] is None else _perm(f"action binmaps[{h}]", maps[h], bins[h])
        return hperm, maps

    def _gaussian(self, k):
        aperm, asign = self._pair("(aperm, asign)")
        aperm = _perm("action aperm", aperm, k)
        return aperm, _sign("action asign", asign, k)

    def host_tables(self, head, obs_dim, obs_ld, n_actions=None, bins=None, act_dim=None, critic_dim=None, critic_ld=None):
        """The packed tables as numpy uint32 arrays (include/rlppo.h, "[mirror]"), every entry range-checked: {obs, critic or None, act,
        mask or None, n_actions, act_dim}.  head: RLPPO_HEAD_*; obs_dim / critic_dim: the networks' input widths; obs_ld / critic_ld: the
        rows' leading dimensions; n_actions (discrete), bins (multi-discrete) or act_dim (Gaussian heads): the policy's."""
        if self.obs_perm.size != obs_dim:
            raise ValueError(f"Symmetry: obs_perm has {self.obs_perm.size} entries, the policy observes {obs_dim} features")
        out = dict(obs=_packed(self.obs_perm, self.obs_sign, obs_ld), critic=None, mask=None)
        if critic_dim is not None:
            if self.critic_obs_perm is None:
                raise ValueError("Symmetry: critic_obs_perm / critic_obs_sign are required: the critic has observations of its own")
            if self.critic_obs_perm.size != critic_dim:
                raise ValueError(f"Symmetry: critic_obs_perm has {self.critic_obs_perm.size} entries, the critic observes {critic_dim} features")
            out["critic"] = _packed(self.critic_obs_perm, self.critic_obs_sign, critic_ld)
        if head == N.HEAD_DISCRETE:
            amap = self._discrete(n_actions)
            inv = np.argsort(amap)
            out.update(act=amap.astype(np.uint32), n_actions=int(n_actions), act_dim=1)
        elif head == N.HEAD_MULTIDISCRETE:
            bins = [int(b) for b in bins]
            hperm, maps = self._multi_discrete(bins)
            starts = np.concatenate(([0], np.cumsum(bins)[:-1])).astype(np.int64)
            H, S = len(bins), int(sum(bins))
            out.update(act=np.concatenate([hperm, 3 * H + starts, bins] + maps).astype(np.uint32), n_actions=S, act_dim=H)
            # logit (h, b) of the mirror is valid iff logit (hperm[h], binmaps[h]^-1(b)) of the source is
            inv = np.concatenate([starts[hperm[h]] + np.argsort(maps[h]) for h in range(H)])
        else:
            aperm, asign = self._gaussian(act_dim)
            out.update(act=_packed(aperm, asign, aperm.size), n_actions=0, act_dim=int(act_dim))
            return out
        words = (out["n_actions"] + 31) // 32
        out["mask"] = np.full(32 * words, ZERO, np.uint32)
        out["mask"][:inv.size] = inv.astype(np.uint32)
        return out


class BoundSymmetry(object):
    """A Symmetry's tables on the device, built once for one learner (PPOLearner.set_symmetry), and the rlppo_symmetry that names them."""

    def __init__(self, sym, host, head, device):
        import torch
        self.symmetry = sym
        up = lambda a: None if a is None else torch.as_tensor(a.view(np.int32)).to(device)
        self.obs, self.critic, self.act, self.mask = (up(host[k]) for k in ("obs", "critic", "act", "mask"))
        d = self.desc = N.SymmetryArg()
        d.head, d.act_dim, d.n_actions = head, host["act_dim"], host["n_actions"]
        d.mask_words = 0 if self.mask is None else self.mask.numel() // 32
        d.obs_ld, d.obs_tab = self.obs.numel(), self.obs.data_ptr()
        if self.critic is not None:
            d.critic_ld, d.critic_tab = self.critic.numel(), self.critic.data_ptr()
        d.act_tab = self.act.data_ptr()
        if self.mask is not None:
            d.mask_tab = self.mask.data_ptr()
