"""The masked small rollout call on the one-launch, late-noise path: rlppo_discrete_step with rlppo_act_opts.action_mask AND
noise_ctl (the mask words staged before the launch, the noise published after it), and DiscreteFF.get_action(obs, action_mask=m)
on small host batches through ActGraph.  Every comparison is bit for bit: the reference is the same library's masked call with its
noise up front, which tests/test_gpu_action_mask.py pins to torch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hip_pass import L, P, check, stream  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 5, 16, 17, 80, 256)


def policy(d, A, hidden, seed):
    from rlgym_ppo_amd.ppo import DiscreteFF
    torch.manual_seed(seed)
    return DiscreteFF(d, A, hidden, "cuda:0")


def special_rows(A):
    """Mask rows every shape must get right: exactly one valid action at the word boundaries, all valid, none valid."""
    out = []
    for c in (0, 31, 32, 63, 64, A - 1):
        if c < A and all(c != o[1] for o in out):
            row = np.zeros(A, bool)
            row[c] = True
            out.append((row, c))
    out.append((np.ones(A, bool), None))
    out.append((np.zeros(A, bool), None))      # through the C ABI only: all-valid on the device
    return out


def make_mask(rs, n, A):
    """Seeded random mask, two-thirds valid, every row with a valid action; from row 1 on the special rows (as many as fit)."""
    m = rs.rand(n, A) < 2.0 / 3.0
    m[np.arange(n), rs.randint(0, A, n)] = True
    single = {}
    for k, (row, c) in enumerate(special_rows(A)):
        if 1 + k < n:
            m[1 + k] = row
            if c is not None:
                single[1 + k] = c
    return m, single


def pack_words(m, W):
    """bool [n, A] -> uint32 words [n, W] without the host form's validation (an all-zero row stays all-zero)."""
    n, A = m.shape
    bits = np.zeros((n, W * 32), bool)
    bits[:, :A] = m
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4").reshape(n, W).astype(np.uint32)


@pytest.mark.parametrize("d,hidden,A", [(40, (64, 64), 33), (40, (64, 64), 64), (40, (128, 128), 3), (40, (128, 128), 128), (107, (256, 256, 256), 90)],
                         ids=["h64_A33_idle_wave", "h64_A64_no_idle_wave", "h128_A3", "h128_A128_four_words", "h256x3_A90"])
def test_masked_step_takes_its_noise_while_it_runs(L, d, hidden, A):
    """rlppo_discrete_step with a mask and noise_ctl through the C ABI: observations, mask words, control words and noise live in
    a host window; the host stages observations + mask words + {sequence, live rows}, flushes, launches, and only then publishes
    the noise.  Actions and log-probabilities equal the masked call that had its noise before the launch, bit for bit; the launch
    covers more rows than are live, the rows beyond carry stale non-zero mask words and store nothing.
    Which late-noise fetch site serves a row depends on host timing where the head layer has an idle wave (A = 33, 3, 90): the
    idle-wave fetch into LDS if the host has published by the time the head layer starts, else the wait-then-read after the last
    layer.  Only the shapes without an idle wave (A = 64 on 64 wide, A = 128 on 128 wide) pin a site: every row is read after the
    layers.  The host publishes at once here, so the idle-wave site is the likely one for the others, not a guaranteed one."""
    from rlgym_ppo_amd import _native as N
    pol = policy(d, A, hidden, seed=A + hidden[0])
    a = pol.arena
    a.ensure_packed()
    W = (A + 31) // 32
    cap_max = max(ROWS) + 16
    r256 = lambda x: (x + 255) // 256 * 256
    obs_bytes, q_bytes = r256(4 * cap_max * d), r256(4 * cap_max * A)
    win = ctypes.c_void_p()
    check(L, L.rlppo_host_window_alloc(256 + obs_bytes + q_bytes + 4 * cap_max * W, ctypes.byref(win)))
    ctl_p, obs_p = win.value, win.value + 256
    q_p, mask_p = obs_p + obs_bytes, obs_p + obs_bytes + q_bytes
    V = ctypes.c_void_p
    rs = np.random.RandomState(A * 7 + hidden[0])
    ws = torch.empty(int(L.rlppo_discrete_step_workspace_bytes(a.dims_c, a.n_layers, cap_max)), dtype=torch.uint8, device="cuda")
    done = torch.zeros(int(L.rlppo_act_done_words(cap_max)), dtype=torch.int32).pin_memory()
    hdr = np.zeros(2, dtype=np.uint32)

    def step(opts, n, obs_ptr, noise_ptr, act, logp):
        return L.rlppo_discrete_step(stream(), a.dims_c, a.n_layers, P(a.packed), V(obs_ptr), 0, d, n, 0, 0.0, 1.0, None, None, V(noise_ptr), P(act), None,
                                     P(logp), None, 0, P(ws), ws.numel(), opts)

    try:
        opts = N.ActOpts(N.PRECISION_DEFAULT, 1, done.data_ptr(), ctl_p)
        opts.action_mask, opts.mask_words = mask_p, W
        unmasked = N.ActOpts(N.PRECISION_DEFAULT, 1, done.data_ptr(), ctl_p)
        for seq, n in enumerate(ROWS, start=1):
            cap = (n // 16 + 1) * 16                         # the launched capacity: always more rows than are live
            n_words = int(L.rlppo_act_done_words(cap))
            # a masked late-noise call is one launch wherever the unmasked one is
            assert L.rlppo_discrete_step_one_launch(a.dims_c, a.n_layers, cap, ctypes.byref(unmasked)) == 1
            assert L.rlppo_discrete_step_one_launch(a.dims_c, a.n_layers, cap, ctypes.byref(opts)) == 1
            obs = np.clip(rs.randn(cap, d), -5, 5).astype(np.float32)
            m, single = make_mask(rs, n, A)
            words = np.full((cap, W), 0xA5A5A5A5, dtype=np.uint32)       # stale non-zero words beyond the live rows
            words[:n] = pack_words(m, W)
            q = torch.from_numpy(rs.exponential(size=(n, A)).astype(np.float32)).pin_memory()

            # the reference: the same library's masked call on the n live rows with its noise up front
            ref_opts = N.ActOpts()
            words_d = torch.from_numpy(words[:n].view(np.int32).copy()).cuda()
            ref_opts.action_mask, ref_opts.mask_words = words_d.data_ptr(), W
            obs_d = torch.from_numpy(obs[:n].copy()).cuda()
            ref_a, ref_l = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, device="cuda")
            check(L, step(ctypes.byref(ref_opts), n, obs_d.data_ptr(), q.data_ptr(), ref_a, ref_l))
            torch.cuda.synchronize()
            ref_a, ref_l = ref_a.cpu(), ref_l.cpu()

            act, logp = torch.full((cap,), -1, dtype=torch.int64).pin_memory(), torch.full((cap,), float("nan")).pin_memory()
            done.zero_()
            hdr[:] = (seq, n)
            check(L, L.rlppo_host_push(V(obs_p), V(obs.ctypes.data), obs.nbytes, None, 0))
            check(L, L.rlppo_host_push(V(mask_p), V(words.ctypes.data), words.nbytes, None, 0))
            check(L, L.rlppo_host_push(V(ctl_p), V(hdr.ctypes.data), 8, None, 0))
            check(L, L.rlppo_host_window_flush(V(ctl_p)))
            opts.done_value = seq
            check(L, step(ctypes.byref(opts), cap, obs_p, q_p, act, logp))  # (the noise matrix holds the previous round's numbers)
            check(L, L.rlppo_host_push(V(q_p), V(q.data_ptr()), 4 * n * A, V(ctl_p + 8), seq))
            assert L.rlppo_host_wait_words(P(done), n_words, seq, 5_000_000) == 0, (n, done.numpy()[:n_words].astype(np.uint32).tolist())
            torch.cuda.synchronize()
            diff = int((act[:n] != ref_a).sum()), int((logp[:n] != ref_l).sum())
            print(f"[masked late noise] hidden={hidden} A={A} n={n} cap={cap}: actions differing {diff[0]}, log-probs differing {diff[1]}")
            assert torch.equal(act[:n], ref_a) and torch.equal(logp[:n], ref_l), (n, diff)
            assert (act[n:] == -1).all() and torch.isnan(logp[n:]).all(), n        # rows at and beyond the live-row word store nothing
            act_h = act[:n].numpy()
            ok = np.where(m.any(1, keepdims=True), m, True)                         # a row without a valid action: all-valid
            assert ok[np.arange(n), act_h].all(), n
            for row, c in single.items():                                           # one valid action: that one, with log(1)
                assert act_h[row] == c and float(logp[row]) == 0.0, (n, row, c, act_h[row], float(logp[row]))
    finally:
        torch.cuda.synchronize()
        check(L, L.rlppo_host_window_free(win))


def _pair(d=107, A=90, hidden=(256, 256, 256), seed=3):
    return policy(d, A, hidden, seed), policy(d, A, hidden, seed)


def _problem(n, d, A, seed):
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    m = rs.rand(n, A) < 2.0 / 3.0
    m[np.arange(n), rs.randint(0, A, n)] = True
    q = torch.from_numpy(rs.exponential(size=(n, A)).astype(np.float32))
    return obs, m, q


@pytest.mark.parametrize("n", [8, 80, 300])
def test_masked_get_action_rides_the_graph(L, n):
    """DiscreteFF.get_action(obs, action_mask=m) on a small host batch: equal to the general path with the same explicit noise;
    with drawn noise equal between two policies seeded alike (graph against general path) with the generator left in the same
    state; the masked graph counts the calls and takes late noise up to 256 rows; an all-valid mask gives the unmasked call."""
    from rlgym_ppo_amd.ppo._mlp import _bucket
    d, A = 107, 90
    g_pol, e_pol = _pair(d, A)
    e_pol.act_graphs = False
    obs, m, q = _problem(n, d, A, n)
    a0, l0 = g_pol.get_action(obs, noise=q, action_mask=m)
    a1, l1 = e_pol._get_action_general(obs, False, q, None, m)
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
    assert m[np.arange(n), a0.numpy()].all()
    key = (_bucket(n), True)
    assert set(g_pol._graphs) == {key} and not e_pol._graphs        # cached beside the unmasked ones, keyed (bucket, masked)
    g = g_pol._graphs[key]
    assert g.masked and g.calls == 1 and g.cap == _bucket(n)
    if n <= 256 and g.push:
        assert g.late                                               # host window granted: the late-noise form
    if n > 256:
        assert not g.late
    # drawn noise: the same generator stream as the unmasked call ([n][A] numbers), the same state afterwards
    for k in range(3):
        obs, m, _ = _problem(n, d, A, 100 + n + k)
        torch.manual_seed(77 + k)
        a0, l0 = g_pol.get_action(obs, action_mask=m)
        s0 = torch.get_rng_state()
        torch.manual_seed(77 + k)
        a1, l1 = e_pol.get_action(obs, action_mask=m)
        s1 = torch.get_rng_state()
        assert torch.equal(a0, a1) and torch.equal(l0, l1) and torch.equal(s0, s1), k
        assert m[np.arange(n), a0.numpy()].all()
    assert g.calls == 4 and g.late_retries == 0
    # a torch bool mask is a host mask too; an all-valid mask gives the unmasked call's results bit for bit
    obs, m, q = _problem(n, d, A, 999 + n)
    a0, l0 = g_pol.get_action(obs, noise=q, action_mask=torch.from_numpy(m))
    a1, l1 = e_pol._get_action_general(obs, False, q, None, m)
    assert torch.equal(a0, a1) and torch.equal(l0, l1) and g.calls == 5
    a0, l0 = g_pol.get_action(obs, noise=q, action_mask=np.ones((n, A), bool))
    a1, l1 = g_pol.get_action(obs, noise=q)
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
    assert set(g_pol._graphs) == {key, _bucket(n)} and g.calls == 6 and g_pol._graphs[_bucket(n)].calls == 1
    assert not g_pol._graphs[_bucket(n)].masked


def test_a_mask_row_without_a_valid_action_raises_and_the_next_call_works(L):
    d, A, n = 107, 90, 8
    g_pol, e_pol = _pair(d, A)
    e_pol.act_graphs = False
    obs, m, q = _problem(n, d, A, 5)
    a0, l0 = g_pol.get_action(obs, noise=q, action_mask=m)          # (the graph exists: the failing call is a replay's)
    bad = m.copy()
    bad[5] = False
    with pytest.raises(ValueError, match="row 5 has no valid action"):
        g_pol.get_action(obs, noise=q, action_mask=bad)
    with pytest.raises(ValueError, match="rows"):
        g_pol.get_action(obs, noise=q, action_mask=m[:7])
    g = g_pol._graphs[(16, True)]
    assert g.calls == 1                                             # nothing was staged or launched for the refused calls
    a1, l1 = g_pol.get_action(obs, noise=q, action_mask=m)
    a2, l2 = e_pol._get_action_general(obs, False, q, None, m)
    assert torch.equal(a0, a1) and torch.equal(l0, l1) and torch.equal(a1, a2) and torch.equal(l1, l2) and g.calls == 2


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from rlgym_ppo_amd.ppo import DiscreteFF
out = {}
for n in (8, 80, 300):
    torch.manual_seed(3)
    pol = DiscreteFF(107, 90, (256, 256, 256), "cuda:0")
    rs = np.random.RandomState(n)
    obs = np.clip(rs.randn(n, 107), -5, 5).astype(np.float32)
    m = rs.rand(n, 90) < 2.0 / 3.0
    m[np.arange(n), rs.randint(0, 90, n)] = True
    q = torch.from_numpy(rs.exponential(size=(n, 90)).astype(np.float32))
    a, l = pol.get_action(obs, noise=q, action_mask=m)
    g = list(pol._graphs.values())
    assert len(g) == 1 and g[0].masked and g[0].calls == 1, "the masked graph did not serve the call"
    out["a%d" % n], out["l%d" % n] = a.numpy(), l.numpy()
    out["push%d" % n], out["late%d" % n] = np.asarray(g[0].push), np.asarray(g[0].late)
np.savez(sys.argv[2], **out)
"""


def test_masked_graph_with_pinned_inputs_in_a_fresh_process(L, tmp_path):
    """RLPPO_ACT_PUSH=0 (inputs, mask words and noise in pinned host memory, no late noise): the same results.  The switch is read
    when a graph is built, per process: a child process started afresh."""
    script, res = tmp_path / "child.py", tmp_path / "out.npz"
    script.write_text(_CHILD)
    env = dict(os.environ, RLPPO_ACT_PUSH="0")
    subprocess.run([sys.executable, str(script), ROOT, str(res)], check=True, env=env, timeout=120)
    got = np.load(res)
    for n in (8, 80, 300):
        assert not got["push%d" % n] and not got["late%d" % n]
        pol = policy(107, 90, (256, 256, 256), 3)
        pol.act_graphs = False
        obs, m, q = _problem(n, 107, 90, n)
        a, l = pol._get_action_general(obs, False, q, None, m)
        assert np.array_equal(got["a%d" % n], a.numpy()) and np.array_equal(got["l%d" % n], l.numpy()), n
