"""rlppo_mirror_batch (csrc/mirror.hip) against numpy, bit for bit: permutations, sign flips and bit moves are exact, so there is no
tolerance.  Shapes cover both row layouts (several rows per wave up to 128 floats, a wave per row above), a lone row, a ragged last
wave and several workgroups; the minibatch wraps around the ring; the whole staging region is compared, so every byte outside the
seven arrays (the gaps behind them and a band behind the region) must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

from hip_pass import L, stream   # noqa: F401 -- L is a fixture
from mirror_reference import mirror_actions, mirror_mask, mirror_rows, obs_symmetry, pack
from rlgym_ppo_amd import _native as N
from rlgym_ppo_amd.ppo import Symmetry
from rlgym_ppo_amd.ppo.symmetry import BoundSymmetry

pytestmark = pytest.mark.gpu
BINS = [3, 3, 2, 7, 7]
BAND = 4096   # bytes behind the staging region
# name -> (head, action description, n_actions, act_dim, bins, masked)
HEADS = {
    "discrete33": (N.HEAD_DISCRETE, np.arange(33)[::-1].copy(), 33, 1, None, False),
    "discrete33-masked": (N.HEAD_DISCRETE, np.arange(33)[::-1].copy(), 33, 1, None, True),   # one bit in the second word
    "discrete90": (N.HEAD_DISCRETE, np.arange(90)[::-1].copy(), 90, 1, None, False),
    "discrete90-masked": (N.HEAD_DISCRETE, np.arange(90)[::-1].copy(), 90, 1, None, True),
    "nvec": (N.HEAD_MULTIDISCRETE, ([0, 1, 2, 4, 3], [None, [2, 1, 0], None, None, None]), 22, 5, BINS, False),
    "nvec-masked": (N.HEAD_MULTIDISCRETE, ([0, 1, 2, 4, 3], [None, [2, 1, 0], None, None, None]), 22, 5, BINS, True),
    "gaussian-critic": (N.HEAD_DIAG_GAUSSIAN, ([1, 0, 2, 3], [1, 1, -1, 1]), 0, 4, None, False),   # + a critic matrix of another width
}


@pytest.mark.parametrize("head_name", list(HEADS))
@pytest.mark.parametrize("mb", [1, 17, 300])
@pytest.mark.parametrize("d, ld", [(5, 16), (107, 112), (107, 128), (231, 256)])
def test_mirror_batch_is_numpy_bit_for_bit(L, d, ld, mb, head_name):
    head, desc, n_actions, k, bins, masked = HEADS[head_name]
    rs = np.random.RandomState(1000 * d + 10 * mb + len(head_name))
    n, base = mb + 7, mb + 4                       # the ring: capacity n, logical row 0 three rows before its end
    idx = rs.permutation(n)[:mb].astype(np.int64)
    phys = (idx + base) % n
    perm, sign = obs_symmetry(d)
    with_critic = head_name.endswith("critic")
    dc, ldc = ((231, 256) if ld <= 128 else (5, 16)) if with_critic else (None, 0)
    cperm, csign = obs_symmetry(dc) if with_critic else (None, None)

    def rows(width, lead):
        x = np.zeros((n, lead), np.float32)
        x[:, :width] = rs.randn(n, width) * (rs.rand(n, width) > 0.1)   # (some exact zeros: a flipped zero is -0)
        return x
    states, cstates = rows(d, ld), rows(dc, ldc) if with_critic else None
    if head == N.HEAD_DISCRETE:
        acts = rs.randint(0, n_actions, (n, 1)).astype(np.float32)
    elif head == N.HEAD_MULTIDISCRETE:
        acts = np.stack([rs.randint(0, b, n) for b in bins], 1).astype(np.float32)
    else:
        acts = rs.randn(n, k).astype(np.float32)
    old, tgt, adv = (rs.randn(n).astype(np.float32) for _ in range(3))
    W = (n_actions + 31) // 32 if masked else 0
    if masked:
        valid = rs.rand(n, n_actions) < 0.6
        valid[:, 0] |= ~valid.any(1)
        words = pack(valid, W)
        words[1::2, -1] |= np.uint32((0xFFFFFFFF << (n_actions % 32)) & 0xFFFFFFFF)   # stale bits beyond the logits: copied, never mirrored

    sym = Symmetry(perm, sign, action=desc, critic_obs_perm=cperm, critic_obs_sign=csign)
    kw = {0: dict(n_actions=n_actions), 1: dict(bins=bins)}.get(head, dict(act_dim=k))
    if with_critic:
        kw.update(critic_dim=dc, critic_ld=ldc)
    bound = BoundSymmetry(sym, sym.host_tables(head, d, ld, **kw), head, "cuda")
    # the test's own tables are honest: every map is an involution on the host
    assert np.array_equal(mirror_rows(mirror_rows(states[:, :d], perm, sign, ld)[:, :d], perm, sign, ld), states)
    assert np.array_equal(mirror_actions(head, desc, mirror_actions(head, desc, acts if k > 1 else acts[:, 0], bins), bins), acts if k > 1 else acts[:, 0])
    if masked:
        assert np.array_equal(mirror_mask(head, desc, mirror_mask(head, desc, valid, bins), bins), valid)

    off = (ctypes.c_int64 * 7)()
    nbytes = int(L.rlppo_mirror_staging_bytes(mb, ld, ldc, k, W, off))
    prefill = rs.randint(0, 256, nbytes + BAND).astype(np.uint8)
    want = prefill.copy()

    def put(i, original, mirrored):
        both = np.ascontiguousarray(np.concatenate([original, mirrored], 0))
        want[off[i]:off[i] + both.nbytes] = both.view(np.uint8).reshape(-1)
    put(0, states[phys], mirror_rows(states[phys, :d], perm, sign, ld))
    if with_critic:
        put(1, cstates[phys], mirror_rows(cstates[phys, :dc], cperm, csign, ldc))
    put(2, acts[phys], mirror_actions(head, desc, acts[phys] if k > 1 else acts[phys, 0], bins).reshape(mb, k))
    for i, x in ((3, old), (4, tgt), (5, adv)):
        put(i, x[phys], x[phys])
    if masked:
        put(6, words[phys], pack(mirror_mask(head, desc, valid[phys], bins), W))

    dev = lambda x: None if x is None else torch.as_tensor(x.view(np.int32) if x.dtype == np.uint32 else x).cuda()
    t = dict(states=dev(states), cstates=dev(cstates), acts=dev(acts), old=dev(old), tgt=dev(tgt), adv=dev(adv), idx=dev(idx),
             words=dev(words) if masked else None, staging=dev(prefill))
    a = N.MinibatchArgs()
    a.head, a.act_dim, a.mb, a.ld_states, a.ring_base, a.ring_cap = head, k, mb, ld, base, n
    a.states, a.actions, a.old_logp, a.targets, a.advantages, a.idx = (t[f].data_ptr() for f in ("states", "acts", "old", "tgt", "adv", "idx"))
    if masked:
        a.action_mask, a.mask_words = t["words"].data_ptr(), W
    cr = N.CriticRows(t["cstates"].data_ptr(), ldc) if with_critic else None
    rc = L.rlppo_mirror_batch(stream(), ctypes.byref(a), ctypes.byref(cr) if with_critic else None, ctypes.byref(bound.desc),
                              ctypes.c_void_p(t["staging"].data_ptr()), nbytes)
    assert rc == 0, L.rlppo_last_error()
    torch.cuda.synchronize()
    got = t["staging"].cpu().numpy()
    assert np.array_equal(got[nbytes:], prefill[nbytes:]), "the launch wrote behind the staging region"
    for i, name in enumerate(("states", "critic rows", "actions", "old_logp", "targets", "advantages", "mask")):
        end = off[i + 1] if i < 6 else nbytes
        assert np.array_equal(got[off[i]:end], want[off[i]:end]), f"{name}: {np.flatnonzero(got[off[i]:end] != want[off[i]:end])[:8]} (byte offsets)"
