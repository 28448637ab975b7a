"""The masked small rollout call of the multi-discrete head as a hipGraph: MultiDiscreteFF.get_action(obs, action_mask=m) with a host
mask on a small host batch rides ActGraph(pol, cap, masked=True) -- the layer chain reading the host window, then
rlppo_multidiscrete_act_nvec_masked with completion words, the mask words staged behind the noise with the observations.  The
yardstick is the same library's eager masked call (act_graphs = False) under the same generator state, which
tests/test_gpu_multidiscrete_mask.py pins to the float64 yardstick and to torch's Categorical; every comparison here is bit for bit
on actions and log-probabilities."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import masked_multidiscrete_yardstick as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 5, 16, 17, 80, 256)
D = 23
REFERENCE = [3, 3, 3, 3, 3, 2, 2, 2]
BINS = {"one_word": [2, 7, 3, 11, 2],            # S = 25
        "straddling": [30, 5, 64, 3],            # S = 102: head 1 straddles words 0 | 1, head 2 spans words 1, 2 and 3
        "reference": REFERENCE}                  # the fixed bins: a masked call gives them to the general kernel


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rlgym_ppo_amd import _native as N
    return N.lib()


def policy(bins, seed=4, general=False):
    from rlgym_ppo_amd.ppo import MultiDiscreteFF
    torch.manual_seed(seed)
    pol = MultiDiscreteFF(D, (64, 64), "cuda:0", bins=None if bins == REFERENCE else bins)
    pol._force_general = general
    return pol


def problem(bins, n, seed):
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    m = M.rand_mask(rs, n, bins)
    q = torch.from_numpy(rs.exponential(size=(n * len(bins), max(bins))).astype(np.float32))
    return obs, m, q


def valid(m, bins, act):
    return bool(np.take_along_axis(M.head_valid(m, bins), act.numpy()[..., None], -1).all())


def same(x, y):
    return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])


@pytest.mark.parametrize("case", list(BINS))
def test_masked_small_call_rides_the_graph_and_equals_the_eager_call(L, case):
    """Rows 1 .. 256, given noise and drawn noise: actions and log-probabilities of the graph call equal the eager masked call's bit
    for bit, the generator is left in the same state, every sampled action is valid under its row's mask; the graph is cached under
    (bucket, True) beside the unmasked ones and counts its calls; counter 6 (runs of the general kernels) rises once per call,
    graph or eager, the graph's first call included; the eager policy builds no graph; an all-valid mask gives the unmasked graph
    call's results."""
    from rlgym_ppo_amd.ppo._mlp import _bucket
    bins = BINS[case]
    S, H = sum(bins), len(bins)
    g_pol, e_pol, u_pol = policy(bins), policy(bins), policy(bins, general=True)
    e_pol.act_graphs = False
    assert g_pol.n_logits == S and (g_pol.md_nvec is None) == (case == "reference")
    calls = {}
    for n in ROWS:
        key = (_bucket(n), True)
        obs, m, q = problem(bins, n, 100 + n)
        assert m.shape == (n, S) and M.head_valid(m, bins).any(-1).all()
        if n >= 8:      # rand_mask's special rows: one bin per head, all valid, the last bin of every head
            assert (M.head_valid(m, bins).sum(-1) == 1).all(-1).any() and m.all(1).any() and not m.all()
        c6 = L.rlppo_dbg_counter(6)
        got = g_pol.get_action(obs, noise=q, action_mask=m)
        assert L.rlppo_dbg_counter(6) == c6 + 1, "the graph call must count as one run of the general kernel (its first call too)"
        want = e_pol.get_action(obs, noise=q, action_mask=m)
        assert L.rlppo_dbg_counter(6) == c6 + 2
        diff = int((got[0] != want[0]).sum()), int((got[1] != want[1]).sum())
        print(f"[masked nvec small call] {case} n={n}: actions differing {diff[0]}, log-probs differing {diff[1]}")
        assert same(got, want), (n, diff)
        assert got[0].dtype == torch.int64 and tuple(got[0].shape) == (n, H) and got[1].dtype == torch.float32 and tuple(got[1].shape) == (n,)
        assert valid(m, bins, got[0]), n
        calls[key] = calls.get(key, 0) + 1
        g = g_pol._graphs[key]
        assert g.masked and g.cap == _bucket(n) and g.calls == calls[key] and g.mask_words == (S + 31) // 32 and not g.late
        # drawn noise: the unmasked call's stream ([n H, B] numbers), the same generator state afterwards
        obs, m, _ = problem(bins, n, 200 + n)
        torch.manual_seed(77 + n)
        got = g_pol.get_action(obs, action_mask=m)
        s0 = torch.get_rng_state()
        torch.manual_seed(77 + n)
        want = e_pol.get_action(obs, action_mask=m)
        assert same(got, want) and torch.equal(s0, torch.get_rng_state()) and valid(m, bins, got[0]), n
        # a torch bool mask is a host mask too
        got = g_pol.get_action(obs, noise=q, action_mask=torch.from_numpy(m))
        assert same(got, e_pol.get_action(obs, noise=q, action_mask=m))
        calls[key] += 2
        assert g.calls == calls[key]
        # an all-valid mask: the unmasked graph call of the general kernel, bit for bit
        ones = np.ones((n, S), bool)
        got = g_pol.get_action(obs, noise=q, action_mask=ones)
        plain = u_pol.get_action(obs, noise=q)
        assert same(got, plain), n
        assert not u_pol._graphs[_bucket(n)].masked and u_pol._graphs[_bucket(n)].mask_words == 0
        if case == "reference":      # ... and the fixed kernel's actions (its log-probability is summed in another order)
            fixed = g_pol.get_action(obs, noise=q)
            assert torch.equal(got[0], fixed[0]) and float((got[1] - fixed[1]).abs().max()) < 1e-5
        calls[key] += 1
    assert not e_pol._graphs
    masked_keys = {k for k in g_pol._graphs if isinstance(k, tuple)}
    assert masked_keys == set(calls) == {(16, True), (32, True), (80, True), (256, True)}
    assert all(g_pol._graphs[k].calls == c and g_pol._graphs[k].polled + g_pol._graphs[k].poll_timeouts >= c for k, c in calls.items())
    assert all(isinstance(k, int) and not g.masked for k, g in u_pol._graphs.items()) and len(u_pol._graphs) == 4


def test_stale_words_of_an_earlier_call_do_no_harm(L):
    """A 16-row call whose every head keeps one bin, then a 3-row call in the same bucket under other masks: rows 3 .. 15 of the
    window keep the first call's words (and its observations), their results are ignored, and the second call equals the eager one."""
    bins = BINS["straddling"]
    S = sum(bins)
    g_pol, e_pol = policy(bins), policy(bins)
    e_pol.act_graphs = False
    rs = np.random.RandomState(9)
    obs, _, q = problem(bins, 16, 1)
    tight = np.zeros((16, S), bool)
    for s, b in zip(M.starts(bins), bins):
        tight[np.arange(16), s + rs.randint(0, b, 16)] = True
    got = g_pol.get_action(obs, noise=q, action_mask=tight)
    assert same(got, e_pol.get_action(obs, noise=q, action_mask=tight))
    want_act = np.stack([tight[:, s:s + b].argmax(1) for s, b in zip(M.starts(bins), bins)], 1)
    assert np.array_equal(got[0].numpy(), want_act) and (got[1] == 0).all()          # one valid bin per head: that one, log(1)
    obs3, m3, q3 = problem(bins, 3, 2)
    assert not np.array_equal(m3, tight[:3])
    got = g_pol.get_action(obs3, noise=q3, action_mask=m3)
    assert same(got, e_pol.get_action(obs3, noise=q3, action_mask=m3)) and valid(m3, bins, got[0])
    assert set(g_pol._graphs) == {(16, True)} and g_pol._graphs[(16, True)].calls == 2


def test_an_empty_head_raises_before_anything_is_staged(L):
    bins = BINS["one_word"]
    g_pol, e_pol = policy(bins), policy(bins)
    e_pol.act_graphs = False
    obs, m, q = problem(bins, 8, 5)
    first = g_pol.get_action(obs, noise=q, action_mask=m)               # (the graph exists: the failing call is a replay's)
    g = g_pol._graphs[(16, True)]
    bad = m.copy()
    bad[5, 2:9] = False
    c6 = L.rlppo_dbg_counter(6)
    with pytest.raises(ValueError, match=r"row 5, head 1 \(bins 2 \.\. 8\) has no valid bin"):
        g_pol.get_action(obs, noise=q, action_mask=bad)
    with pytest.raises(ValueError, match="rows"):
        g_pol.get_action(obs, noise=q, action_mask=m[:7])
    with pytest.raises(ValueError, match="shape"):
        g_pol.get_action(obs, noise=q, action_mask=np.ones((8, len(bins)), bool))
    assert g.calls == 1 and L.rlppo_dbg_counter(6) == c6 and set(g_pol._graphs) == {(16, True)}
    again = g_pol.get_action(obs, noise=q, action_mask=m)
    assert same(first, again) and same(again, e_pol.get_action(obs, noise=q, action_mask=m)) and g.calls == 2


def test_device_and_packed_masks_take_the_eager_path_and_the_gaussian_head_refuses(L):
    from rlgym_ppo_amd.ppo import ContinuousPolicy
    from rlgym_ppo_amd.ppo._mlp import ActGraph
    from rlgym_ppo_amd.util import action_mask as AM
    bins = BINS["straddling"]
    S = sum(bins)
    pol, e_pol = policy(bins), policy(bins)
    e_pol.act_graphs = False
    obs, m, q = problem(bins, 8, 6)
    want = e_pol.get_action(obs, noise=q, action_mask=m)
    for form in (torch.from_numpy(m).cuda(), AM.Packed(AM.pack(m, S, "cuda:0", heads=bins), S)):
        c6 = L.rlppo_dbg_counter(6)
        assert same(pol.get_action(obs, noise=q, action_mask=form), want)
        assert not pol._graphs and L.rlppo_dbg_counter(6) == c6 + 1
    torch.manual_seed(1)
    gauss = ContinuousPolicy(D, 8, (64, 64), "cuda:0")
    with pytest.raises(ValueError, match="ActGraph: a masked graph needs"):
        ActGraph(gauss, 16, masked=True)


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_multidiscrete_masked_small_call as T
out = {}
for case, bins in T.BINS.items():
    for n in (8, 80, 256):
        pol = T.policy(bins)
        obs, m, q = T.problem(bins, n, 100 + n)
        a, l = pol.get_action(obs, noise=q, action_mask=m)
        g = list(pol._graphs.values())
        assert len(g) == 1 and g[0].masked and g[0].calls == 1 and list(pol._graphs) == [(g[0].cap, True)], "the masked graph did not serve the call"
        assert g[0].window is None and g[0].mask_pin is not None and g[0].mask_pin.is_pinned()
        obs, m, q = T.problem(bins, 3, 300 + n)                       # stale words in pinned memory, too
        a3, l3 = pol.get_action(obs, noise=q, action_mask=m)
        k = "%s%d" % (case, n)
        out["a" + k], out["l" + k], out["a3" + k], out["l3" + k], out["push" + k] = a.numpy(), l.numpy(), a3.numpy(), l3.numpy(), np.asarray(g[0].push)
np.savez(sys.argv[2], **out)
"""


def test_masked_graph_with_pinned_inputs_in_a_fresh_process(L, tmp_path):
    """RLPPO_ACT_PUSH=0 (observations, noise and mask words in pinned host memory): the same results.  The switch is read when a
    graph is built, per process: a child process started afresh."""
    script, res = tmp_path / "child.py", tmp_path / "out.npz"
    script.write_text(_CHILD)
    env = dict(os.environ, RLPPO_ACT_PUSH="0")
    subprocess.run([sys.executable, str(script), ROOT, str(res)], check=True, env=env, timeout=120)
    got = np.load(res)
    for case, bins in BINS.items():
        pol = policy(bins)
        pol.act_graphs = False
        for n in (8, 80, 256):
            k = "%s%d" % (case, n)
            assert not got["push" + k]
            obs, m, q = problem(bins, n, 100 + n)
            a, l = pol.get_action(obs, noise=q, action_mask=m)
            assert np.array_equal(got["a" + k], a.numpy()) and np.array_equal(got["l" + k], l.numpy()), k
            obs, m, q = problem(bins, 3, 300 + n)
            a, l = pol.get_action(obs, noise=q, action_mask=m)
            assert np.array_equal(got["a3" + k], a.numpy()) and np.array_equal(got["l3" + k], l.numpy()), k
