"""What happens to a gradient AFTER the minibatch pass, held to float64 truth element for element (tests/optim_yardstick.py; its
bounds are derived there and shown neither too tight nor too loose by tests/test_optim_yardstick_host.py): rlppo_clip_adam, every
fused form of it DIRECTLY (not through rlppo_clip_adam), rlppo_net_pack's image, rlppo_adv_stats, the many-slot sum and the strict
decisions of rlppo_kl_gate / rlppo_kl_gate_lr, and the writer of kl_slots in the loss launches.  Truth is evaluated one step at a
time from the float32 state the device itself produced in the step before, so errors do not compound and the per-step bound holds.
Every test prints a "[fp64 gate]" line with max(err / bound) for HIP and for the CPU float32 oracle."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets  # noqa: E402
import optim_yardstick as Y  # noqa: E402
from hip_pass import L, P, check, dev, run_pass, stream  # noqa: E402,F401

KEYS = ("g", "m", "v", "p")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def within(got, truth, bound, what):
    """Element for element |got - truth| <= bound, no element left out.  -> max(err / bound)."""
    err = np.abs(np.asarray(got, np.float64) - truth)
    worst = Y.worst(got, truth, bound)
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (what, f"{bad.size} elements outside, worst err/bound {worst:.3g}", bad[:5], err[bad[:5]], bound[bad[:5]])
    return worst


def gnorm2_check(got, g, what):
    """The squared norm: positive terms, so n 2^-53 relative bounds ANY summation order in double."""
    exact = Y.exact_sum_squares(g)
    assert abs(got - exact) <= g.size * 2.0 ** -53 * exact, (what, got, exact)
    return exact


# ------------------------------------------------------------------------------------------------ a. rlppo_clip_adam
def hip_clip_adam(L, p, g, m, v, max_norm, lr, b1, b2, eps, step):
    dp, dg, dm, dv = dev(p), dev(g), dev(m), dev(v)
    gn = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    check(L, L.rlppo_clip_adam(stream(), P(dp), P(dg), P(dm), P(dv), dp.numel(), max_norm, lr, b1, b2, eps, step, P(gn)))
    torch.cuda.synchronize()
    return dict(g=dg.cpu().numpy(), m=dm.cpu().numpy(), v=dv.cpu().numpy(), p=dp.cpu().numpy()), gn.item()


def cpu_oracle_worst(state, hyper):
    got, norm2 = Y.torch_adam32(*state, *hyper)
    truth, bound = Y.clip_adam64(*state, norm2, *hyper)
    return {k: Y.worst(got[k], truth[k], bound[k]) for k in KEYS}


def report(label, hip, cpu):
    fmt = lambda w: " ".join(f"{k}' {w[k]:.3f}" for k in KEYS if k in hip)
    print(f"[fp64 gate] {label}: max(err/bound) HIP {fmt(hip)} | CPU fp32 oracle {fmt(cpu)}")


@pytest.mark.parametrize("case", Y.ADAM_CASES, ids=[c[0] for c in Y.ADAM_CASES])
def test_clip_adam_against_float64(L, case):
    name, n, step, kind, max_norm, (b1, b2) = case
    state = Y.adam_state(case)
    hyper = (max_norm, Y.LR, b1, b2, Y.EPS, step)
    got, norm2 = hip_clip_adam(L, *state, *hyper)
    exact = gnorm2_check(norm2, state[1], name)
    truth, bound = Y.clip_adam64(*state, norm2, *hyper)
    hip = {k: within(got[k], truth[k], bound[k], (name, k)) for k in KEYS}
    report(f"clip+Adam {name}", hip, cpu_oracle_worst(state, hyper))
    if max_norm / (math.sqrt(exact) + 1e-6) > 1.001:   # an unclipped step returns the gradient bit for bit
        assert np.array_equal(bits(got["g"]), bits(state[1]))
    else:
        assert max_norm / (math.sqrt(exact) + 1e-6) < 0.999   # (no row of the table sits on the clamp's edge)


def test_clip_adam_exact_edges(L):
    rs = np.random.RandomState(5)
    n = 513
    p = (rs.randn(n) * 0.2).astype(np.float32)
    zero = np.zeros(n, np.float32)
    # an all-zero gradient on fresh moments: nothing moves, nothing becomes NaN (0 / (0 + eps))
    got, norm2 = hip_clip_adam(L, p, zero, zero, zero, 0.5, Y.LR, 0.9, 0.999, Y.EPS, 3)
    assert norm2 == 0.0
    for k, before in (("p", p), ("m", zero), ("v", zero), ("g", zero)):
        assert np.array_equal(bits(got[k]), bits(before)) and np.isfinite(got[k]).all(), k
    # elements with g = m = v = 0 inside a non-zero arena keep p bit for bit and m = v = 0, clipped or not
    for max_norm in (0.5, 1e9):
        case = ("edge", n, 2, "wide", max_norm, (0.9, 0.999))
        p, g, m, v = Y.adam_state(case)
        dead = rs.permutation(n)[:40]
        g[dead] = m[dead] = v[dead] = 0.0
        got, _ = hip_clip_adam(L, p, g, m, v, max_norm, Y.LR, 0.9, 0.999, Y.EPS, 2)
        assert np.array_equal(bits(got["p"][dead]), bits(p[dead]))
        assert not got["m"][dead].any() and not got["v"][dead].any() and not got["g"][dead].any()
        live = np.setdiff1d(np.arange(n), dead)
        assert (got["p"][live] != p[live]).mean() > 0.5


def test_clip_adam_denormal_second_moments_are_reported_not_gated(L):
    """|g| ~ 1e-21: (1 - beta2) g^2 ~ 1e-45 is a float32 denormal.  How the device rounds there has not been measured by anybody:
    the figures are printed, nothing is asserted beyond a finite result."""
    rs = np.random.RandomState(6)
    n = 300
    p = (rs.randn(n) * 0.2).astype(np.float32)
    g = (1e-21 * rs.uniform(0.5, 1.5, n) * np.where(rs.rand(n) < 0.5, -1, 1)).astype(np.float32)
    zero = np.zeros(n, np.float32)
    hyper = (1e9, Y.LR, 0.9, 0.999, Y.EPS, 1)
    got, norm2 = hip_clip_adam(L, p, g, zero, zero, *hyper)
    truth, bound = Y.clip_adam64(p, g, zero, zero, norm2, *hyper)
    hip = {k: Y.worst(got[k], truth[k], bound[k]) for k in KEYS}
    report("clip+Adam denormal v' (not gated)", hip, cpu_oracle_worst((p, g, zero, zero), hyper))
    print(f"[fp64 gate]   device v' zero on {(got['v'] == 0).mean():.2f} of the elements, truth's largest v' {truth['v'].max():.2e}")
    assert all(np.isfinite(got[k]).all() for k in KEYS)


# ------------------------------------------------------------------------------------------------ b. the fused forms
PAIRS = {
    "plain": ([107, 256, 256, 90], [107, 256, 256, 1]),
    # ~0.9 M elements: above the 196,608 that 128 workgroups x 6 register elements x 256 threads hold, so the stride loop behind the
    # barrier runs; most workgroups of the 14-element net own no element at all
    "big_and_tiny": ([231, 512, 512, 512, 512, 16], [13, 1]),
    "odd": ([7, 33, 5], [300, 130, 257, 64, 1500]),
}
# (pair, entry point, one launch with the grid barrier?, (tail_a, tail_b))
FUSED = [
    ("plain", "pack2", True, (0, 0)), ("plain", "pack2", False, (0, 0)), ("plain", "lr", True, (0, 0)),
    ("big_and_tiny", "pack2", True, (0, 0)), ("big_and_tiny", "lr", False, (0, 0)), ("big_and_tiny", "tail", False, (0, 0)),
    ("odd", "tail", True, (0, 0)), ("odd", "tail", True, (3, 256)), ("odd", "tail", False, (256, 3)), ("odd", "lr", True, (3, 0)),
    ("odd", "pack2", False, (0, 0)),
]
HYPER = ((0.5, 3e-4, 0.9, 0.999, 1e-8), (1e-3, 1e-3, 0.8, 0.99, 1e-8))   # (max_norm, lr, beta1, beta2, eps) of network a / b
KINDS = ("wide", "small", "big")   # the gradient of step 1 / 2 / 3: clipped, unclipped (network a), clipped


class FusedNet:
    def __init__(self, L, dims, tail, seed):
        from rlgym_ppo_amd import _native as N
        self.dims, self.tail = dims, tail
        self.dc, self.nl = N.dims_array(dims), len(dims) - 1
        self.nf = int(L.rlppo_flat_floats(self.dc, self.nl))
        self.n = self.nf + tail
        rs = np.random.RandomState(seed)
        self.rs = rs
        self.p = dev((rs.randn(self.n) * 0.1).astype(np.float32))
        self.m, self.v, self.g = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.packed = torch.full((int(L.rlppo_packed_floats(self.dc, self.nl)),), float("nan"), device="cuda")
        check(L, L.rlppo_net_pack(stream(), self.dc, self.nl, P(self.p), P(self.packed)))
        self.gn = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        self.skip = torch.zeros(1, dtype=torch.int32, device="cuda")

    def desc(self, hyper, step, lr_in_desc):
        from rlgym_ppo_amd import _native as N
        d = N.OptNet()
        d.dims, d.n_layers = ctypes.cast(self.dc, ctypes.POINTER(ctypes.c_int32)), self.nl
        d.params, d.grads, d.exp_avg, d.exp_avg_sq = self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        d.packed, d.gnorm2, d.skip_word = self.packed.data_ptr(), self.gn.data_ptr(), self.skip.data_ptr()
        d.max_norm, _, d.beta1, d.beta2, d.eps = hyper
        d.lr, d.step = lr_in_desc, step
        return d

    def snapshot(self):
        return tuple(t.cpu().numpy() for t in (self.p, self.g, self.m, self.v))

    def image_is_exact(self, L):
        """`packed` == the documented image of the CURRENT flat arena, bit for bit, padding included; a tail is never in it."""
        want = Y.packed_image(self.dims, self.p.cpu().numpy()[:self.nf], L)
        return np.array_equal(bits(self.packed.cpu().numpy()), bits(want))


def fused_call(L, entry, a, b, sync, tails, rates):
    if entry == "pack2":
        return L.rlppo_clip_adam_pack2(stream(), ctypes.byref(a), ctypes.byref(b), P(sync))
    if entry == "tail":
        return L.rlppo_clip_adam_pack2_tail(stream(), ctypes.byref(a), ctypes.byref(b), P(sync), tails[0], tails[1])
    return L.rlppo_clip_adam_pack2_lr(stream(), ctypes.byref(a), ctypes.byref(b), P(sync), tails[0], tails[1],
                                      ctypes.c_void_p(rates.data_ptr()), ctypes.c_void_p(rates.data_ptr() + 8))


@pytest.mark.parametrize("pair,entry,one_launch,tails", FUSED,
                         ids=[f"{p}-{e}-{'one_launch' if o else 'three_operations'}-tails{t[0]}_{t[1]}" for p, e, o, t in FUSED])
def test_fused_forms_against_float64(L, pair, entry, one_launch, tails):
    from rlgym_ppo_amd import _native as N
    assert entry != "pack2" or tails == (0, 0)
    net = [FusedNet(L, dims, tail, 11 + k) for k, (dims, tail) in enumerate(zip(PAIRS[pair], tails))]
    assert all(x.image_is_exact(L) for x in net)
    sync = torch.zeros(N.OPT_SYNC_BYTES // 4, dtype=torch.int32, device="cuda") if one_launch else None   # zeroed ONCE
    # the "lr" entry point reads its rates from two adjacent device doubles; the descriptors then carry a rate nobody may use
    rates = torch.tensor([HYPER[0][1], HYPER[1][1]], dtype=torch.float64, device="cuda")
    worst_hip, worst_cpu = {k: 0.0 for k in "mvp"}, {k: 0.0 for k in "mvp"}
    for step in (1, 2, 3):
        before = []
        for x in net:
            x.g.copy_(dev(Y.gradient(KINDS[step - 1], x.n, x.rs)))
            before.append(x.snapshot())
        descs = [x.desc(h, step, 123.0 if entry == "lr" else h[1]) for x, h in zip(net, HYPER)]
        check(L, fused_call(L, entry, descs[0], descs[1], sync, tails, rates))
        torch.cuda.synchronize()
        for k, (x, h, state) in enumerate(zip(net, HYPER, before)):
            what = (pair, entry, step, "ab"[k])
            hyper = (h[0], h[1], h[2], h[3], h[4], step)
            norm2 = x.gn.item()
            gnorm2_check(norm2, state[1], what)
            truth, bound = Y.clip_adam64(*state, norm2, *hyper, lr_device=h[1] if entry == "lr" else None)
            got = dict(zip(("p", "g", "m", "v"), x.snapshot()))
            for key in "mvp":   # (the tail behind the layers is part of the arena: clipped, updated and bounded like the rest)
                worst_hip[key] = max(worst_hip[key], within(got[key], truth[key], bound[key], what + (key,)))
            assert not got["g"].any(), what                      # gradients are left exactly zero
            assert x.image_is_exact(L), what
            if x.tail and step == 3:   # ("big": every element's update is of the order of the rate)
                assert (got["p"][x.nf:] != state[0][x.nf:]).all(), what   # the tail is updated
            cpu = cpu_oracle_worst(state, hyper)
            for key in "mvp":
                worst_cpu[key] = max(worst_cpu[key], cpu[key])
    if one_launch:   # the barrier's block: arrival counter back at 0, one generation per call, no wait that gave up
        w = sync.cpu().numpy()
        assert w[0] == 0 and w[1] == 3 and w[2] == 0, w[:4]
    assert rates.cpu().tolist() == [HYPER[0][1], HYPER[1][1]]   # the call never writes a rate
    report(f"fused {pair} {entry} {'one launch' if one_launch else 'three operations'} tails {tails}", worst_hip, worst_cpu)


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "three_operations"])
@pytest.mark.parametrize("skipped", [0, 1], ids=["skip_a", "skip_b"])
def test_fused_skip_word_leaves_one_network_untouched(L, one_launch, skipped):
    from rlgym_ppo_amd import _native as N
    tails = (3, 0)
    net = [FusedNet(L, dims, tail, 21 + k) for k, (dims, tail) in enumerate(zip(PAIRS["odd"], tails))]
    sync = torch.zeros(N.OPT_SYNC_BYTES // 4, dtype=torch.int32, device="cuda") if one_launch else None
    for x in net:   # moments that are not zero, so that "untouched" says something
        x.m.copy_(dev((x.rs.randn(x.n) * 1e-2).astype(np.float32)))
        x.v.copy_(dev((x.rs.rand(x.n) * 1e-4).astype(np.float32)))
        x.g.copy_(dev(Y.gradient("wide", x.n, x.rs)))
    net[skipped].skip.fill_(7)
    before = [x.snapshot() for x in net]
    packed_before = [x.packed.clone() for x in net]
    descs = [x.desc(h, 4, h[1]) for x, h in zip(net, HYPER)]
    check(L, fused_call(L, "tail", descs[0], descs[1], sync, tails, None))
    torch.cuda.synchronize()
    s, o = net[skipped], net[1 - skipped]
    for a, b in zip(before[skipped], s.snapshot()):
        assert np.array_equal(bits(a), bits(b))
    assert torch.equal(s.packed.view(torch.int32), packed_before[skipped].view(torch.int32))
    h, state = HYPER[1 - skipped], before[1 - skipped]
    norm2 = o.gn.item()
    gnorm2_check(norm2, state[1], "the network that was not skipped")
    truth, bound = Y.clip_adam64(*state, norm2, h[0], h[1], h[2], h[3], h[4], 4)
    got = dict(zip(("p", "g", "m", "v"), o.snapshot()))
    hip = {k: within(got[k], truth[k], bound[k], ("skip", k)) for k in "mvp"}
    assert not got["g"].any() and o.image_is_exact(L)
    if one_launch:
        w = sync.cpu().numpy()
        assert w[0] == 0 and w[1] == 1 and w[2] == 0, w[:4]
    report(f"fused skip_word on network {'ab'[skipped]}, the other one", hip, cpu_oracle_worst(state, (h[0], h[1], h[2], h[3], h[4], 4)))


@pytest.mark.parametrize("pair", list(PAIRS))
def test_net_pack_builds_the_documented_image(L, pair):
    """rlppo_net_pack on a destination full of NaN: every float of the image is written -- W[Pout][Pin], W^T[Pin][Pout], b[Pout] per
    layer, zero wherever no parameter lands -- so the caller owes no zero fill (include/rlppo.h says so)."""
    from rlgym_ppo_amd import _native as N
    for k, dims in enumerate(PAIRS[pair]):
        dc, nl = N.dims_array(dims), len(dims) - 1
        rs = np.random.RandomState(31 + k)
        flat = (rs.randn(int(L.rlppo_flat_floats(dc, nl))) * 0.1).astype(np.float32)
        flat[rs.permutation(flat.size)[:3]] = (-0.0, 0.0, 1e-40)[:min(3, flat.size)]
        packed = torch.full((int(L.rlppo_packed_floats(dc, nl)),), float("nan"), device="cuda")
        check(L, L.rlppo_net_pack(stream(), dc, nl, P(dev(flat)), P(packed)))
        torch.cuda.synchronize()
        assert np.array_equal(bits(packed.cpu().numpy()), bits(Y.packed_image(dims, flat, L))), dims


# ------------------------------------------------------------------------------------------------ c. rlppo_adv_stats
@pytest.mark.parametrize("n,kind,idx_kind,ring", Y.ADV_CASES, ids=[f"n{c[0]}_{c[1]}_{c[2]}_{'ring' if c[3] else 'plain'}" for c in Y.ADV_CASES])
def test_adv_stats_against_float64(L, n, kind, idx_kind, ring):
    from rlgym_ppo_amd import _native as N
    adv, idx, base, cap = Y.adv_case(n, kind, idx_kind, ring)
    rows = Y.ring_rows(idx, base, cap)
    assert rows.min() >= 0 and rows.max() < adv.size
    d_adv, d_idx = dev(adv), dev(idx, torch.int64)
    ws = torch.zeros(N.ADV_STATS_WS_BYTES // 4, dtype=torch.int32, device="cuda")   # zeroed ONCE; every call leaves it armed
    outs = []
    for _ in range(3):
        out = torch.full((2,), float("nan"), device="cuda")
        check(L, L.rlppo_adv_stats(stream(), P(d_idx), n, P(d_adv), base, cap, P(out), P(ws)))
        torch.cuda.synchronize()
        assert ws[0].item() == 0   # the ticket word is back at 0
        outs.append(out.cpu().numpy())
    assert all(np.array_equal(bits(outs[0]), bits(o)) for o in outs[1:])
    mean, scale = float(outs[0][0]), float(outs[0][1])
    t_mean, t_scale, b_mean, b_scale = Y.adv_stats64(adv, idx, base, cap)
    a32 = torch.as_tensor(adv[rows])
    cpu = (float(a32.mean()), float(1.0 / (a32.std() + 1e-8))) if n > 1 else (0.0, 1.0)
    ratio = lambda got, want, bound: 0.0 if got == want else (abs(got - want) / bound if bound > 0 else float("inf"))
    print(f"[fp64 gate] adv_stats n={n} {kind} {idx_kind} {'ring' if ring else 'plain'}: err/bound HIP mean {ratio(mean, t_mean, b_mean):.3f} "
          f"scale {ratio(scale, t_scale, b_scale):.3f} | CPU fp32 oracle (float32 sums) mean {ratio(cpu[0], t_mean, b_mean):.3g} "
          f"scale {ratio(cpu[1], t_scale, b_scale):.3g}")
    if n == 1:
        assert np.array_equal(bits(outs[0]), bits([0.0, 1.0]))
        return
    assert abs(mean - t_mean) <= b_mean and abs(scale - t_scale) <= b_scale, (mean, t_mean, b_mean, scale, t_scale, b_scale)
    if kind == "constant":
        a = np.float32(adv[0])
        assert np.array_equal(bits(outs[0][:1]), bits([a])) and np.float32(outs[0][1]) * (a - np.float32(outs[0][0])) == 0


# ------------------------------------------------------------------------------------------------ d. the KL gate
SLOT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
KL_STRIDE = 1024   # doubles per pass region >= 2 + 1000
GATE_CASES = [(c,) for c in SLOT_COUNTS] + [(63, 257, 1000), SLOT_COUNTS]   # n_passes 1, 3 and 8


def kl_regions(counts, seed=0, nan_at=None):
    """-> (flat float64 image, [(mb_ratio, slots)]).  Slot values spread over six decades, unequal mb_ratio per pass, NaN in every
    double behind a pass's last slot: the gate must not read there."""
    rs = np.random.RandomState(40 + seed + len(counts))
    img = np.full(len(counts) * KL_STRIDE, np.nan)
    regions = []
    for p, c in enumerate(counts):
        slots = 10.0 ** rs.uniform(-8.0, -2.0, c)
        ratio = float(np.float32(1.0 / (2.0 + 1.7 * p)))
        if nan_at == p:
            slots[c // 2] = np.nan
        img[p * KL_STRIDE:p * KL_STRIDE + 2 + c] = np.concatenate([[float(c), ratio], slots])
        regions.append((ratio, slots))
    return img, regions


class GateRun:
    def __init__(self, L, img, n_passes, rates=(3e-4, 1e-3), stop=0, threshold=1e30, batch=4):
        from rlgym_ppo_amd import _native as N
        self.L = L
        self.slots = dev(img, torch.float64)
        self.rates = torch.tensor(rates, dtype=torch.float64, device="cuda")
        self.kl = torch.tensor([-7.0], dtype=torch.float64, device="cuda")
        self.exchange = torch.full((2,), float("nan"), device="cuda")
        self.stop = torch.tensor([stop], dtype=torch.int32, device="cuda")
        self.host = torch.full((2,), -1, dtype=torch.int32).pin_memory()
        g, a = N.KlGateArgs(), N.LrAdaptArgs()
        g.kl_slots, g.slot_stride, g.n_passes, g.threshold = self.slots.data_ptr(), KL_STRIDE, n_passes, threshold
        g.exchange, g.batch, g.done_value = self.exchange.data_ptr(), batch, 77
        g.stop_word, g.host_words = self.stop.data_ptr(), self.host.data_ptr()
        a.lr, a.n_lr, a.desired_kl, a.factor, a.lr_min, a.lr_max = self.rates.data_ptr(), len(rates), 0.01, 1.5, 1e-5, 1e-2
        a.kl_out = self.kl.data_ptr()
        self.g, self.a = g, a

    def run(self, phase, lr_entry):
        self.g.phase = phase
        if lr_entry:
            check(self.L, self.L.rlppo_kl_gate_lr(stream(), ctypes.byref(self.g), ctypes.byref(self.a)))
        else:
            check(self.L, self.L.rlppo_kl_gate(stream(), ctypes.byref(self.g)))
        torch.cuda.synchronize()
        return self


@pytest.mark.parametrize("counts", GATE_CASES, ids=["slots_" + "_".join(map(str, c)) for c in GATE_CASES])
def test_kl_gate_sum_against_float64(L, counts):
    img, regions = kl_regions(counts)
    truth, bound = Y.kl_batch64(regions)
    assert bound > 0 and truth > 0
    # through kl_out (phase 0 of rlppo_kl_gate_lr), twice: the same bits
    kls = [GateRun(L, img, len(counts), threshold=1e30).run(0, True).kl.item() for _ in range(2)]
    assert kls[0] == kls[1]
    assert abs(kls[0] - truth) <= bound, (kls[0], truth, bound)
    # through the phase-1 words of both entry points: identical words, and hi + lo is KL_b up to the float32 rounding of lo
    # (|lo| <= 2^-24 KL_b, rounded once more: 2^-48 KL_b -- two floats carry 48 bits, tests/optim_yardstick.py)
    words = []
    for lr_entry in (False, True, True):
        r = GateRun(L, img, len(counts)).run(1, lr_entry)
        assert r.stop.item() == 0 and r.host.tolist() == [-1, -1] and r.kl.item() == -7.0   # phase 1 writes the two words only
        assert r.rates.cpu().tolist() == [3e-4, 1e-3]
        words.append(r.exchange.cpu().numpy())
    assert all(np.array_equal(bits(words[0]), bits(w)) for w in words[1:])
    hi, lo = float(words[0][0]), float(words[0][1])
    assert hi == float(np.float32(kls[0])) and abs((hi + lo) - kls[0]) <= Y.exchange_bound(kls[0])
    assert abs((hi + lo) - truth) <= bound + Y.exchange_bound(truth)
    print(f"[fp64 gate] kl_gate {len(counts)} passes, slots {counts}: err/bound HIP {abs(kls[0] - truth) / bound:.3f} (kl_out) "
          f"{abs(hi + lo - truth) / (bound + Y.exchange_bound(truth)):.3f} (hi + lo) | CPU float64 left-to-right "
          f"{abs(sum(r * float(np.sum(s)) for r, s in regions) - truth) / bound:.3f}")


@pytest.mark.parametrize("lr_entry", [False, True], ids=["kl_gate", "kl_gate_lr"])
def test_kl_gate_decisions_are_strict(L, lr_entry):
    from rlgym_ppo_amd.ppo.lr_schedule import adapt_lr
    counts = (63, 257, 1000)
    img, _ = kl_regions(counts)
    kl_b = GateRun(L, img, 3).run(0, True).kl.item()   # what the device itself reports
    rates = [3e-4, 1e-3]
    # (the rate rule of the lr entry point, desired_kl 0.01: a gate that runs and does not stop moves both rates)
    moved = [adapt_lr(r, kl_b, 0.01, 1e-5, 1e-2) for r in rates] if lr_entry else rates
    assert kl_b > 0 and (moved != rates) == lr_entry
    r = GateRun(L, img, 3, threshold=kl_b).run(0, lr_entry)                                # KL_b == threshold: no stop
    assert r.stop.item() == 0 and r.host.tolist() == [0, 77] and r.rates.cpu().tolist() == moved
    r = GateRun(L, img, 3, threshold=float(np.nextafter(kl_b, 0.0)), batch=9).run(0, lr_entry)   # one ulp below: stop = batch + 1
    assert r.stop.item() == 10 and r.host.tolist() == [10, 77] and r.rates.cpu().tolist() == rates   # (a gate that stops moves no rate)
    r = GateRun(L, img, 3, stop=3, threshold=float(np.nextafter(kl_b, 0.0)), batch=9).run(0, lr_entry)   # a set stop word stays
    assert r.stop.item() == 3 and r.host.tolist() == [3, 77] and r.rates.cpu().tolist() == rates
    r = GateRun(L, img, 3, stop=3, threshold=1e30).run(0, lr_entry)                        # ... also when KL_b is below the threshold
    assert r.stop.item() == 3 and r.host.tolist() == [3, 77]
    nan_img, _ = kl_regions(counts, nan_at=1)
    r = GateRun(L, nan_img, 3, threshold=0.0).run(0, lr_entry)                             # a NaN slot: no stop, no rate moves
    assert r.stop.item() == 0 and r.host.tolist() == [0, 77] and r.rates.cpu().tolist() == rates
    if lr_entry:
        assert math.isnan(r.kl.item())
    # phase 2 decides from the exchanged words, strictly too
    r = GateRun(L, img, 3, threshold=kl_b).run(1, lr_entry)
    r.exchange.copy_(torch.tensor([np.float32(kl_b), 0.0]))
    summed = float(np.float32(kl_b))
    r.g.threshold = summed
    assert r.run(2, lr_entry).stop.item() == 0 and r.host.tolist() == [0, 77]
    r.g.threshold = float(np.nextafter(summed, 0.0))
    assert r.run(2, lr_entry).stop.item() == 5 and r.host.tolist() == [5, 77]


# ------------------------------------------------------------------------------------------------ e. the writer of kl_slots
def armed_pass(L, head, mb, mb_ratio, seed, stop=None):
    """One rlppo_ppo_minibatch pass over mb rows (obs 20 -> (32,) -> 7 actions) with kl_slots armed and NaN-filled.
    -> (slots region, stats)."""
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    k = 7
    pol, val = nets.init_mlp(20, (32,), k if head == "discrete" else 2 * k), nets.init_mlp(20, (32,), 1)
    obs = rs.randn(mb, 20).astype(np.float32)
    acts = rs.randint(0, k, mb).astype(np.float32) if head == "discrete" else rs.uniform(-0.9, 0.9, (mb, k)).astype(np.float32)
    with torch.no_grad():
        logp = nets.backprop(head, pol, torch.as_tensor(obs), torch.as_tensor(acts))[0].reshape(-1).numpy()
    old = (logp + 0.1 * rs.randn(mb)).astype(np.float32)
    adv, tgt = rs.randn(mb).astype(np.float32), rs.randn(mb).astype(np.float32)
    r = run_pass(L, pol, val, obs, acts, old, tgt, adv, np.arange(mb), head=head, mb_ratio=mb_ratio, kl_slots=True, stop=stop)
    lr = logp.astype(np.float64) - old.astype(np.float64)
    return r["kl"], r["stats"], float(np.mean(np.expm1(lr) - lr))


@pytest.mark.parametrize("mb", [1, 255, 256, 257, 1000, 70001])
@pytest.mark.parametrize("head", ["discrete", "gaussian"])
def test_kl_slots_writer(L, head, mb):
    """The contract of rlppo_minibatch_args.kl_slots (include/rlppo.h): [0] = the workgroups of the policy loss launch, [1] =
    mb_ratio, [2 + w] = THE double workgroup w adds to stats[RLPPO_STAT_KL] -- its share of mean((ratio - 1) - log ratio), not
    weighted by mb_ratio -- so the pass's increment of stats[RLPPO_STAT_KL] is the sum of its slots up to the order of the double
    additions: (rows) 2^-53 relative; nothing behind slot 2 + [0] is written."""
    mb_ratio = 0.3
    r, stats, kl_cpu = armed_pass(L, head, mb, mb_ratio, 50 + mb % 97)
    n_slots = int(L.rlppo_kl_slots_doubles(mb))
    assert r.size == n_slots
    assert r[0] == int(r[0]) and 1 <= r[0] <= n_slots - 2, r[0]
    assert r[1] == float(np.float32(mb_ratio))
    nw = int(r[0])
    slots = r[2:2 + nw]
    assert np.isfinite(slots).all() and np.isnan(r[2 + nw:]).all()
    total, scale = math.fsum(slots.tolist()), math.fsum(np.abs(slots).tolist())
    assert abs(stats[1] - total) <= mb * 2.0 ** -53 * scale, (stats[1], total)
    print(f"[fp64 gate] kl_slots {head} mb={mb}: {nw} slots, sum {total:.6e} vs stats[KL] {stats[1]:.6e} (diff "
          f"{abs(stats[1] - total) / max(mb * 2.0 ** -53 * scale, 1e-300):.3f} of the bound); CPU fp32 oracle's KL {kl_cpu:.6e}")


def test_kl_slots_are_written_under_a_set_stop_word(L):
    """A set stop word keeps the pass out of `stats` and not out of its slots (the gate of a stopped batch still reads them)."""
    free, stats_free, _ = armed_pass(L, "discrete", 1000, 0.3, 60)
    held, stats_held, _ = armed_pass(L, "discrete", 1000, 0.3, 60, stop=2)
    nw = int(free[0])
    assert np.array_equal(free[:2 + nw], held[:2 + nw]) and np.isnan(held[2 + nw:]).all()
    assert stats_free[1] > 0 and not stats_held[:5].any()
