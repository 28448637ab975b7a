"""PopArt's weight-preserving step through the C ABI (rlppo_value_norm_update_popart) and through ValueNorm.update(preserve=critic),
against tests/popart_yardstick.py (numpy float64) and, for the statistic, bit for bit against rlppo_value_norm_update."""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import popart_yardstick as PY  # noqa: E402
from hip_pass import L, P, check, dev, stream  # noqa: E402,F401

# targets: one thread | two workgroups, the second ragged | more than the grid cap (128 workgroups, each striding)
SIZES = [1, 513, 70001]
# last-layer weights: one | a ragged pass of the 256 threads | an exact one | one more | several passes and a ragged last
WEIGHTS = [1, 255, 256, 257, 1031]
SENT = 0x7FC5A5A5          # (a quiet NaN with a payload: a guard word read as a weight poisons it)
LEAD, TAIL = 7, 9          # guard words in front of w (an ODD float offset: w is 4-byte aligned only) and behind b


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def fresh_stat():
    from rlgym_ppo_amd import _native as N
    return (torch.zeros(4, dtype=torch.float64, device="cuda"), dev([0.0, 1.0, 1.0, 0.0]),
            torch.zeros(N.VALUE_NORM_WS_BYTES, dtype=torch.uint8, device="cuda"))


class Layer(object):
    """n_w weights and the bias behind them, as in a flat arena, inside a buffer of guard words."""

    def __init__(self, w, b):
        self.n_w = len(w)
        self.raw = torch.full((LEAD + self.n_w + 1 + TAIL,), SENT, dtype=torch.int32, device="cuda")
        self.f = self.raw.view(torch.float32)
        self.w, self.b = self.f[LEAD:LEAD + self.n_w], self.f[LEAD + self.n_w:LEAD + self.n_w + 1]
        self.w.copy_(dev(w))
        self.b.copy_(dev([b]))
        assert self.w.data_ptr() % 8 == 4

    def host(self):
        return self.w.cpu().numpy().copy(), self.b.cpu().numpy().copy()

    def guards_intact(self):
        g = torch.cat([self.raw[:LEAD], self.raw[LEAD + self.n_w + 1:]])
        return bool((g == SENT).all())


def popart_update(L, x, stat, layer):
    state, scale, ws = stat
    xd = dev(x)
    w, n_w, b = (None, 0, None) if layer is None else (layer.w, layer.n_w, layer.b)
    check(L, L.rlppo_value_norm_update_popart(stream(), P(xd), xd.numel(), P(state), P(scale), P(ws), P(w), n_w, P(b)))
    torch.cuda.synchronize()
    return state.cpu().numpy().copy(), scale.cpu().numpy().copy()


def plain_update(L, x, stat):
    state, scale, ws = stat
    xd = dev(x)
    check(L, L.rlppo_value_norm_update(stream(), P(xd), xd.numel(), P(state), P(scale), P(ws)))
    torch.cuda.synchronize()
    return state.cpu().numpy().copy(), scale.cpu().numpy().copy()


def batches(n, seed):
    rs = np.random.RandomState(seed)
    return [(50.0 + 7.0 * rs.randn(n)).astype(np.float32), (-300.0 + 0.02 * rs.randn(n)).astype(np.float32), (4e4 + 900.0 * rs.randn(n)).astype(np.float32)]


def make_layer(n_w, seed):
    rs = np.random.RandomState(1000 + seed)
    return (rs.randn(n_w) / np.sqrt(n_w)).astype(np.float32), np.float32(0.3 * rs.randn())


def check_step(L, x, stat, twin, layer, what):
    """One finite batch: state and scale are the plain entry's bits on the twin, w' the yardstick's bits, b' within 1 ulp of it."""
    w0, b0 = layer.host()
    s0 = stat[1].cpu().numpy().copy()
    got = popart_update(L, x, stat, layer)
    want = plain_update(L, x, twin)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (what, got, want)
    w1, b1 = layer.host()
    w_want, b_want = PY.rescale(w0, b0, s0, got[1])
    assert w1.tobytes() == w_want.tobytes(), (what, int((w1 != w_want).sum()))
    assert abs(float(b1[0]) - float(b_want)) <= ulp32(b_want), (what, b1, b_want)
    assert layer.guards_intact(), what
    return got


@pytest.mark.parametrize("n_w", WEIGHTS)
@pytest.mark.parametrize("n", SIZES)
def test_three_updates_from_a_fresh_statistic(L, n, n_w):
    runs = []
    for run in range(2):
        stat, twin, layer = fresh_stat(), fresh_stat(), Layer(*make_layer(n_w, n_w))
        for k, x in enumerate(batches(n, n)):               # three calls on one ws, zeroed once
            got = check_step(L, x, stat, twin, layer, f"n={n} n_w={n_w} update {k}")
            assert got[0][0] == (k + 1) * n and got[0][3] == 0.0
        w, b = layer.host()
        assert not np.array_equal(w, make_layer(n_w, n_w)[0])
        runs.append(w.tobytes() + b.tobytes() + got[0].tobytes() + got[1].tobytes())
    assert runs[0] == runs[1]                                # two runs: the same bits


@pytest.mark.parametrize("n_w", WEIGHTS)
@pytest.mark.parametrize("n", SIZES)
def test_a_rejected_batch_stores_nothing_and_rearms_the_ticket(L, n, n_w):
    stat, twin, layer = fresh_stat(), fresh_stat(), Layer(*make_layer(n_w, n_w))
    xs = batches(n, 7 + n)
    check_step(L, xs[0], stat, twin, layer, "first")
    w0, b0 = layer.host()
    s0, c0 = stat[0].cpu().numpy().copy(), stat[1].cpu().numpy().copy()
    for k, where in enumerate(sorted({0, n // 2, n - 1})):   # (anywhere: the pivot x_0 too)
        bad = xs[1].copy()
        bad[where] = np.nan if k % 2 == 0 else np.inf
        s1, c1 = popart_update(L, bad, stat, layer)
        w1, b1 = layer.host()
        assert w1.tobytes() == w0.tobytes() and b1.tobytes() == b0.tobytes(), where
        assert s1[:3].tobytes() == s0[:3].tobytes() and c1.tobytes() == c0.tobytes() and s1[3] == k + 1, (where, s1, s0)
        assert layer.guards_intact()
        twin[0][3] += 1.0                                    # (the twin's count follows: it never saw the batch)
    got = check_step(L, xs[2], stat, twin, layer, "after the rejected batches")   # the ticket was re-armed on the rejected path
    assert got[0][0] == 2 * n


@pytest.mark.parametrize("n", SIZES)
def test_without_a_layer_it_is_the_plain_entry_point(L, n):
    stat, twin = fresh_stat(), fresh_stat()
    for x in batches(n, 3 * n):
        got, want = popart_update(L, x, stat, None), plain_update(L, x, twin)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert stat[2].cpu().numpy().tobytes() == twin[2].cpu().numpy().tobytes()      # (and the workspace as the plain entry leaves it)


# ================================================================================================ through ValueEstimator
D, ACTIONS, ROWS = 21, 8, 48


def build_ppo(hid, seed=5):
    from rlgym_ppo_amd.ppo import PPOLearner
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = PPOLearner(D, ACTIONS, 0, hid, hid, (0.1, 1.0), 3000, 1, 3e-4, 3e-4, 0.2, 0.005, 1500, "cuda:0")
    g = torch.Generator(device="cuda").manual_seed(seed)
    for t in (learner.value_optimizer.exp_avg, learner.value_optimizer.exp_avg_sq):     # (moments with bits to keep)
        t.copy_(torch.rand(t.shape, device="cuda", generator=g))
    return learner


def real_outputs(net, rows, vn):
    v = net.forward_padded(rows).cpu().numpy()
    return v, PY.real_units32(v, vn.scale.cpu().numpy())


@pytest.mark.parametrize("hid", [(64, 64), (256, 256, 256)], ids=["64x2", "256x3"])
def test_value_estimator_keeps_its_real_unit_outputs(hid):
    rs = np.random.RandomState(len(hid))
    obs = np.clip(rs.randn(ROWS, D), -5, 5).astype(np.float32)
    targets = dev((50.0 + 7.0 * rs.randn(3000)).astype(np.float32))                    # mean 50, deviation 7, a fresh statistic
    ratios = {}
    for preserve in (True, False):
        learner = build_ppo(hid)
        learner.set_value_normalization(True, preserve_outputs=preserve)
        net, vn = learner.value_net, learner.value_norm
        arena = net.arena
        rows = arena.stage_obs(obs)
        layers = [(l.weight.detach().cpu().numpy().copy(), l.bias.detach().cpu().numpy().copy()) for l in arena.linears]
        h = PY.hidden64(layers, obs)
        s0 = vn.scale.cpu().numpy().copy()
        v0, V0 = real_outputs(net, rows, vn)
        x3_before = arena.ensure_packed_x3().clone()
        assert arena.packed_is_current() and arena._packed_x3_key == arena._pack_key()
        packed0, flat0 = arena.packed.clone(), arena.flat.clone()
        keep = [t.clone() for t in (learner.value_optimizer.exp_avg, learner.value_optimizer.exp_avg_sq, learner.policy.arena.flat)]
        if preserve:
            vn.update(targets, preserve=net)
        else:
            learner.update_value_norm(targets)                                          # (the learner's own call, the option off)
        torch.cuda.synchronize()
        s1 = vn.scale.cpu().numpy().copy()
        assert abs(s1[0] - 50.0) < 1.0 and abs(s1[2] - 7.0) < 0.5
        assert arena.packed_is_current() is (not preserve)                              # stale right after the rescale
        for t, was in zip((learner.value_optimizer.exp_avg, learner.value_optimizer.exp_avg_sq, learner.policy.arena.flat), keep):
            assert torch.equal(t, was)                                                  # moments and the policy: their bits
        w_last, b_last = layers[-1]
        if preserve:
            w2, b2 = PY.rescale(w_last, b_last, s0, s1)
            n_last = w_last.size + 1
            assert torch.equal(arena.flat[:-n_last], flat0[:-n_last])                   # the hidden layers were not touched
            assert arena.linears[-1].weight.detach().cpu().numpy().tobytes() == w2.tobytes()
            assert abs(float(arena.linears[-1].bias.item()) - float(b2)) <= ulp32(b2)
            assert arena._packed_x3_key != arena._pack_key()
        else:
            w2, b2 = w_last, b_last[0]
            assert torch.equal(arena.flat, flat0)
        v1, V1 = real_outputs(net, rows, vn)                                            # (ensure_packed rebuilds the image first)
        assert arena.packed_is_current()
        if preserve:
            assert not torch.equal(arena.packed, packed0) and not np.array_equal(v1, v0)    # the forward read the new weights
            x3_after = arena.ensure_packed_x3()
            assert arena._packed_x3_key == arena._pack_key() and x3_after.shape == x3_before.shape
        allow = PY.allowance(w_last, b_last, w2 if preserve else w_last, b2, h, s0, s1)
        ratio = np.abs(V1.astype(np.float64) - V0.astype(np.float64)) / allow
        ratios[preserve] = ratio
        print(f"[popart] hidden {hid}, preserve={preserve}: |V1 - V0| / allowance in [{ratio.min():.3g}, {ratio.max():.3g}]")
    assert ratios[True].max() <= 1.0, ratios[True].max()                                # every row within the derived allowance
    assert ratios[False].min() >= 1000.0, ratios[False].min()                           # the bare update misses it a thousandfold
