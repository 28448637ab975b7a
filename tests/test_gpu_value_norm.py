"""Value normalisation through the C ABI: rlppo_value_norm_update (the running statistic), rlppo_gae_norm (the scan on normalised
values) and rlppo_ppo_minibatch_vnorm (the value loss on normalised targets), against tests/value_norm_yardstick.py (numpy
float64) and, where the arithmetic is exact, bit for bit against the entry points that existed before."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_gate  # noqa: E402
import gae_bootstrap_yardstick as GY  # noqa: E402
import hip_pass as HP  # noqa: E402
import value_norm_yardstick as VY  # noqa: E402
from hip_pass import L, P, check, dev, stream  # noqa: E402,F401
from oracle import nets  # noqa: E402

GAMMA, LMBDA = 0.99, 0.95
CHUNK = 2048


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ================================================================================================ 1. the statistic
# one thread | a ragged workgroup | an exact one | one more | several workgroups | more than the grid cap (128 workgroups x 512)
STAT_SIZES = [1, 255, 256, 257, 4097, 70001]
U = 2.0 ** -52


def fresh_stat():
    from rlgym_ppo_amd import _native as N
    return (torch.zeros(4, dtype=torch.float64, device="cuda"), dev([0.0, 1.0, 1.0, 0.0]),
            torch.zeros(N.VALUE_NORM_WS_BYTES, dtype=torch.uint8, device="cuda"))


def stat_update(L, x, state, scale, ws):
    xd = dev(x)
    check(L, L.rlppo_value_norm_update(stream(), P(xd), xd.numel(), P(state), P(scale), P(ws)))
    torch.cuda.synchronize()
    return state.cpu().numpy().copy(), scale.cpu().numpy().copy()


def batch_bounds(x):
    """The bound tests/optim_yardstick.py (adv_stats64) derives for adv_stats_kernel's shifted double sums, restated for a state kept
    in double (no float32 rounding of the results).  With d = x - x_0, t0 = sum d, t1 = sum d^2 (n additions in any order: n 2^-53
    sum|terms| each, doubled), m = t0 / n, mean_b = x_0 + m, M2_b = t1 - t0 m:
        |mean_b err| <= n 2^-52 mean|d| + 2^-52 |mean_b|
        |M2_b err|   <= n 2^-52 t1 + 2 |m| n 2^-52 sum|d| + 2^-52 (|t0 m| + |t1 - t0 m|)
    (the sum of squares; t0 m = t0^2 / n through t0's error; the product and the cancelling subtraction)."""
    a = np.asarray(x, np.float32).astype(np.float64)
    n = a.size
    d = a - a[0]
    sum_abs = math.fsum(np.abs(d).tolist())
    t0, t1 = math.fsum(d.tolist()), math.fsum((d * d).tolist())
    m = t0 / n
    e_mean = n * U * (sum_abs / n) + U * abs(a[0] + m)
    e_m2 = n * U * t1 + 2.0 * abs(m) * n * U * sum_abs + U * (abs(t0 * m) + abs(t1 - t0 * m))
    return e_mean, e_m2


def merged_bounds(prev, prev_err, batch, batch_err, new):
    """Chan's merge propagates the two means' errors into mean' (weights <= 1) and, through delta^2 count n_b / tot, into M2'; every one
    of its own operations (4 for the mean, 7 for M2) rounds once: 2^-52 of the result's magnitude each, with a factor 2 of slack."""
    (c, mean, m2), (e_mean, e_m2) = prev, prev_err
    (nb, mean_b, m2_b), (e_mb, e_m2b) = batch, batch_err
    tot, mean_n, m2_n = new
    delta = abs(mean_b - mean)
    e_delta = e_mean + e_mb + U * delta
    w = c * nb / tot
    e_mean_n = e_mean + e_delta + 8 * U * max(abs(mean_n), abs(mean), abs(mean_b))
    e_m2_n = e_m2 + e_m2b + (2.0 * delta * e_delta + e_delta * e_delta) * w + 14 * U * (m2_n + delta * delta * w)
    return e_mean_n, e_m2_n


def check_scale(state, scale):
    """scale = {mu, 1/sigma, sigma, 0} of the device's own double state, each rounded once; 1 ulp allowed on 1/sigma and sigma (the
    device's double sqrt and division against the host's)."""
    want = VY.scale64(state[:3])
    assert scale[0] == np.float32(want[0]) and scale[3] == 0.0, (scale, want)
    for k in (1, 2):
        assert abs(float(scale[k]) - want[k]) <= ulp32(want[k]), (k, scale, want)


@pytest.mark.parametrize("n", STAT_SIZES)
def test_statistic_follows_chans_merge_over_three_updates(L, n):
    rs = np.random.RandomState(n)
    batches = [(5e3 + 30.0 * rs.randn(n)).astype(np.float32), (6e3 + 30.0 * rs.randn(n)).astype(np.float32), np.full(n, 5500.0, np.float32)]
    state, scale, ws = fresh_stat()
    truth, err = (0.0, 0.0, 0.0), (0.0, 0.0)
    for k, x in enumerate(batches):           # three calls on one ws, zeroed once
        got, sc = stat_update(L, x, state, scale, ws)
        bm = VY.batch_moments(x)
        new = VY.merge(truth, bm)
        err = merged_bounds(truth, err, bm, batch_bounds(x), new)
        truth = new
        print(f"[value norm stat] n={n} update {k}: mean err {abs(got[1] - truth[1]):.3e} (bound {err[0]:.3e})  "
              f"M2 err {abs(got[2] - truth[2]):.3e} (bound {err[1]:.3e})")
        assert got[0] == truth[0] == (k + 1) * n and got[3] == 0.0
        assert abs(got[1] - truth[1]) <= err[0], (k, got[1], truth[1], err[0])
        assert abs(got[2] - truth[2]) <= err[1], (k, got[2], truth[2], err[1])
        check_scale(got, sc)


@pytest.mark.parametrize("n", STAT_SIZES)
def test_statistic_constant_batch_nan_batch_and_reproducibility(L, n):
    # a constant first batch: M2 == 0 exactly, mean the constant, sigma = fl32(sqrt(1e-5))
    state, scale, ws = fresh_stat()
    got, sc = stat_update(L, np.full(n, 7.25, np.float32), state, scale, ws)
    assert got.tolist() == [float(n), 7.25, 0.0, 0.0]
    assert sc[0] == np.float32(7.25) and sc[2] == np.float32(np.sqrt(1e-5)) and abs(float(sc[1]) - 1.0 / math.sqrt(1e-5)) <= ulp32(1.0 / math.sqrt(1e-5))
    # one NaN (anywhere: the pivot x_0 too) leaves state[0..2] and scale bit-identical and counts the batch
    rs = np.random.RandomState(100 + n)
    x = (5e3 + 30.0 * rs.randn(n)).astype(np.float32)
    s0, c0 = stat_update(L, x, state, scale, ws)
    for k, where in enumerate(sorted({0, n // 2, n - 1})):
        bad = x.copy()
        bad[where] = np.nan if k % 2 == 0 else np.inf
        s1, c1 = stat_update(L, bad, state, scale, ws)
        assert s1[:3].tobytes() == s0[:3].tobytes() and c1.tobytes() == c0.tobytes() and s1[3] == k + 1, (where, s1, s0)
    # two runs from the same state: the same bits (and the rejected batches left the ticket block armed)
    y = (4e3 + 10.0 * rs.randn(n)).astype(np.float32)
    twin_state, twin_scale, twin_ws = state.clone(), scale.clone(), torch.zeros_like(ws)
    a = stat_update(L, y, state, scale, ws)
    b = stat_update(L, y, twin_state, twin_scale, twin_ws)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[0][0] == 3 * n


# ================================================================================================ 2. the scan
# single ragged chunk | exact chunk | chunk + 1 | n mod 4, 8, 512, 2048 all non-zero | three chunks and a ragged last wave
SIZES = [1, 7, 2047, 2048, 2049, 5003, 3 * 2048 + 300]


@pytest.fixture(params=[1, 0], ids=["lookback", "two_launch"])
def form(L, request):
    check(L, L.rlppo_dbg_set(1, request.param))
    try:
        yield request.param
    finally:
        check(L, L.rlppo_dbg_set(1, 1))


def run_gae(L, rews, dones, trunc, values, boot, std, scale="boot_entry"):
    """scale = "boot_entry": rlppo_gae_boot; None: rlppo_gae_norm with value_scale == NULL; else rlppo_gae_norm with the four floats."""
    n = len(rews)
    vt, adv, ret = (torch.full((n,), 7.0, device="cuda") for _ in range(3))
    ws = torch.empty(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    ws[:16] = 0
    r, d, t, v = dev(rews), dev(dones), dev(trunc), dev(values)
    b = None if boot is None else dev(boot)
    s = float("nan") if std is None else float(std)
    if isinstance(scale, str):
        check(L, L.rlppo_gae_boot(stream(), P(r), P(d), P(t), P(v), P(b), n, GAMMA, LMBDA, s, P(vt), P(adv), P(ret), P(ws), ws.numel()))
    else:
        sc = None if scale is None else dev(scale)
        check(L, L.rlppo_gae_norm(stream(), P(r), P(d), P(t), P(v), P(b), P(sc), n, GAMMA, LMBDA, s, P(vt), P(adv), P(ret), P(ws), ws.numel()))
    assert int(ws[4:8].view(torch.int32).item()) == 0, "a look-back wait timed out in a normal run"
    return vt.cpu().numpy(), adv.cpu().numpy(), ret.cpu().numpy()


def same_bits(got, want, what):
    for k, name in enumerate(("value_targets", "advantages", "returns")):
        assert got[k].tobytes() == want[k].tobytes(), (what, name)


MU, SIGMA = -212.7, 37.3


def assert_close_norm(got, want, vmax, what):
    """The existing GAE tests' tolerance (rtol 2e-6, atol 2e-6 against the float64 recurrence) plus what one float32 rounding of every
    V = fmaf(v^, sigma, mu) can move an advantage or a target by: delta_t = r + gamma V_{t+1} - V_t moves by at most
    (1 + gamma) max|V| 2^-24 and A_t = sum_k (gamma lambda)^k delta_{t+k} by that over (1 - gamma lambda)
    (value_norm_yardstick.gae_value_rounding).  Returns do not read the values: the old tolerance alone."""
    extra = VY.gae_value_rounding(vmax, GAMMA, LMBDA)
    for k, name in enumerate(("value_targets", "advantages", "returns")):
        g, w = np.asarray(got[k]), np.asarray(want[k], np.float32)
        assert np.isfinite(g).all(), f"{what}: {name} not finite"
        atol = GY.ATOL + (extra if k < 2 else 0.0)
        err = np.abs(g.astype(np.float64) - w.astype(np.float64)) - GY.RTOL * np.abs(w.astype(np.float64))
        assert err.max() <= atol, (what, name, float(err.max()), atol)


@pytest.mark.parametrize("std", [None, 1.3], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("with_boot", [True, False], ids=["boot", "plain"])
@pytest.mark.parametrize("n", SIZES)
def test_gae_norm(L, form, n, with_boot, std):
    rews, dones, trunc, vhat, boot_hat = GY.make_case(n, seed=n)          # boot: NaN at every entry that is not to be used
    rs = np.random.RandomState(7 * n + 1)
    b_of = lambda b: b if with_boot else None
    # (a) exact: v^ multiples of 1/256 in [-4, 4], sigma = 8, mu = 3.5 -- the fma is exact, so the outputs are rlppo_gae_boot's on V
    q = (rs.randint(-1024, 1025, n + 1) / 256.0).astype(np.float32)
    qb = np.where(np.isnan(boot_hat), np.float32(np.nan), (rs.randint(-1024, 1025, n) / 256.0).astype(np.float32)).astype(np.float32)
    V, Vb = q * np.float32(8.0) + np.float32(3.5), qb * np.float32(8.0) + np.float32(3.5)
    assert np.array_equal(V.astype(np.float64), q.astype(np.float64) * 8.0 + 3.5)
    same_bits(run_gae(L, rews, dones, trunc, q, b_of(qb), std, scale=[3.5, 0.125, 8.0, 0.0]), run_gae(L, rews, dones, trunc, V, b_of(Vb), std), f"exact n={n}")
    # (b) general: against the float64 yardstick
    got = run_gae(L, rews, dones, trunc, vhat, b_of(boot_hat), std, scale=[MU, 1.0 / SIGMA, SIGMA, 0.0])
    s32 = np.asarray([MU, SIGMA], np.float32).astype(np.float64)
    want = VY.gae(rews, dones, trunc, vhat, b_of(boot_hat), s32[0], s32[1], GAMMA, LMBDA, std)
    vmax = np.nanmax(np.abs(np.concatenate([vhat, boot_hat if with_boot else vhat[:1]]).astype(np.float64) * s32[1] + s32[0]))
    assert_close_norm(got, want, vmax, f"general n={n}")
    # (c) value_scale == NULL and (d) the identity scale: rlppo_gae_boot's bits
    ref = run_gae(L, rews, dones, trunc, vhat, b_of(boot_hat), std)
    same_bits(run_gae(L, rews, dones, trunc, vhat, b_of(boot_hat), std, scale=None), ref, f"NULL n={n}")
    same_bits(run_gae(L, rews, dones, trunc, vhat, b_of(boot_hat), std, scale=[0.0, 1.0, 1.0, 0.0]), ref, f"identity n={n}")


def test_gae_norm_on_more_chunks_than_resident_workgroups(L):
    """(e) A grid beyond the resident workgroups takes the kernel's chunk loop.  One truncated step per 128."""
    n = 1100 * CHUNK + 300
    rs = np.random.RandomState(11)
    rews, vhat = rs.randn(n).astype(np.float32), rs.randn(n + 1).astype(np.float32)
    dones, trunc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    trunc[127::128] = 1.0
    boot = np.full(n, np.nan, np.float32)
    boot[127::128] = rs.randn(len(boot[127::128])).astype(np.float32)
    got = run_gae(L, rews, dones, trunc, vhat, boot, 1.7, scale=[MU, 1.0 / SIGMA, SIGMA, 0.0])
    s32 = np.asarray([MU, SIGMA], np.float32).astype(np.float64)
    vmax = max(np.abs(vhat).max(), np.nanmax(np.abs(boot))) * s32[1] + abs(s32[0])
    assert_close_norm(got, VY.gae(rews, dones, trunc, vhat, boot, s32[0], s32[1], GAMMA, LMBDA, 1.7), vmax, "loop form")


def test_gae_norm_under_graph_capture_follows_the_scale(L):
    """(f) Under capture the stateless two-launch form runs and reads value_scale when it runs: the four floats change between
    replays and the outputs follow."""
    n = 3 * CHUNK + 300
    rews, dones, trunc, vhat, boot = GY.make_case(n, seed=3)
    vt, adv, ret = (torch.empty(n, device="cuda") for _ in range(3))
    ws = torch.empty(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    r, d, t, v, b = dev(rews), dev(dones), dev(trunc), dev(vhat), dev(boot)
    sc = dev([0.0, 1.0, 1.0, 0.0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            check(L, L.rlppo_gae_norm(ctypes.c_void_p(side.cuda_stream), P(r), P(d), P(t), P(v), P(b), P(sc), n, GAMMA, LMBDA, 1.7,
                                      P(vt), P(adv), P(ret), P(ws), ws.numel()))
    seen = []
    for mu, sigma in ((0.0, 1.0), (MU, SIGMA), (3.5, 8.0)):
        sc.copy_(dev([mu, 1.0 / sigma, sigma, 0.0]))
        g.replay()
        torch.cuda.synchronize()
        got = (vt.cpu().numpy(), adv.cpu().numpy(), ret.cpu().numpy())
        s32 = np.asarray([mu, sigma], np.float32).astype(np.float64)
        vmax = max(np.abs(vhat).max(), np.nanmax(np.abs(boot))) * s32[1] + abs(s32[0])
        assert_close_norm(got, VY.gae(rews, dones, trunc, vhat, boot, s32[0], s32[1], GAMMA, LMBDA, 1.7), vmax, f"replay mu={mu}")
        seen.append(got[1].copy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ================================================================================================ 3. the value loss in the pass
OBS, HID, ACTIONS = 21, (32, 32), 8
# update.hip: `twin` -- the paired (and folded value head) ReLU form -- is taken from PAIRED_MIN_ROWS = 262144 rows per pass up, on
# layers twin_ok() accepts (equal shapes, padded widths that are multiples of 128): the smallest mb that selects it by itself
PAIRED_MIN_ROWS = 262144
PAIRED_HID = (128, 128)
COUNTER_PAIRED_PASS = 3
MBS = [1, 257, 1500]


def make_nets(hid=HID, obs=OBS, cobs=None, seed=0):
    torch.manual_seed(seed)
    pol = nets.init_mlp(obs, hid, ACTIONS)
    val = nets.init_mlp(obs if cobs is None else cobs, hid, 1)
    return pol, val


def make_rows(n, seed, obs=OBS, cobs=None):
    rs = np.random.RandomState(seed)
    out = dict(obs=np.clip(rs.randn(n, obs), -5, 5).astype(np.float32), acts=rs.randint(0, ACTIONS, n).astype(np.float32),
               old=(-2.0 + 0.3 * rs.randn(n)).astype(np.float32), tgt=(40.0 + 25.0 * rs.randn(n)).astype(np.float32),
               adv=rs.randn(n).astype(np.float32))
    if cobs is not None:
        out["cobs"] = np.clip(rs.randn(n, cobs), -5, 5).astype(np.float32)
    return out


def run_pass(L, pol, val, rows, idx, entry, scale=None, vclip=0.0, act="relu", tgt=None, adv=None):
    """hip_pass.run_pass over rows[idx] (the critic on rows["cobs"] when present) -> (pol_grad, val_grad, stats) on the host."""
    r = HP.run_pass(L, pol, val, rows["obs"], rows["acts"], rows["old"], rows["tgt"] if tgt is None else tgt, rows["adv"] if adv is None else adv,
                    idx, head="discrete", entry=entry, precision="fp32", pol_act=act, val_act=act, cobs=rows.get("cobs"), scale=scale,
                    value_clip=vclip, join=True)
    return r["gp"].cpu(), r["gv"].cpu(), r["stats"]


def same_pass(a, b, what, policy=True):
    assert torch.equal(a[1], b[1]), (what, "val_grad")
    if policy:
        assert torch.equal(a[0], b[0]), (what, "pol_grad")
        assert a[2].tobytes() == b[2].tobytes(), (what, "stats", a[2], b[2])
    else:
        assert a[2][2] == b[2][2], (what, "VLOSS", a[2][2], b[2][2])


SCALE = np.asarray([38.7, 1.0 / 24.3, 24.3, 0.0], np.float32)


def pick(n_rows, mb, seed):
    return np.random.RandomState(seed).permutation(n_rows)[:mb].astype(np.int64)


@pytest.mark.parametrize("mb", MBS)
def test_vnorm_pass_is_the_plain_pass_on_host_normalised_targets(L, mb):
    """(a) value_clip = 0: targets t under scale == rlppo_ppo_minibatch on fl32(fl32(t - mu) * s), bit for bit -- val_grad, pol_grad, stats.
    (d) vnorm == NULL == rlppo_ppo_minibatch_critic's bits."""
    pol, val = make_nets()
    rows, idx = make_rows(mb + 37, mb), pick(mb + 37, mb, mb)
    tn = VY.normalise_targets32(rows["tgt"], SCALE[0], SCALE[1])
    got = run_pass(L, pol, val, rows, idx, "vnorm", scale=SCALE)
    same_pass(got, run_pass(L, pol, val, rows, idx, "plain", tgt=tn), f"(a) mb={mb}")
    raw = run_pass(L, pol, val, rows, idx, "plain")
    assert not torch.equal(got[1], raw[1])                                  # (the scale is not a no-op on these targets)
    same_pass(run_pass(L, pol, val, rows, idx, "vnorm", scale=None), run_pass(L, pol, val, rows, idx, "critic"), f"(d) mb={mb}")
    same_pass(run_pass(L, pol, val, rows, idx, "vnorm", scale=None), raw, f"(d) plain mb={mb}")


def test_vnorm_pass_in_the_paired_form(L):
    """(a) at mb = PAIRED_MIN_ROWS, the smallest pass update.hip pairs (and folds the value head of) by itself."""
    mb = PAIRED_MIN_ROWS
    pol, val = make_nets(PAIRED_HID)
    rows, idx = make_rows(mb, 5), pick(mb, mb, 5)
    tn = VY.normalise_targets32(rows["tgt"], SCALE[0], SCALE[1])
    c0 = int(L.rlppo_dbg_counter(COUNTER_PAIRED_PASS))
    got = run_pass(L, pol, val, rows, idx, "vnorm", scale=SCALE)
    assert int(L.rlppo_dbg_counter(COUNTER_PAIRED_PASS)) == c0 + 1, "the pass was not paired"
    want = run_pass(L, pol, val, rows, idx, "plain", tgt=tn)
    assert int(L.rlppo_dbg_counter(COUNTER_PAIRED_PASS)) == c0 + 2
    same_pass(got, want, f"(a) paired, mb={mb}")


@pytest.mark.parametrize("mb", MBS)
def test_vnorm_pass_clips_in_normalised_units(L, mb):
    """(b) value_clip = 0.25 on dyadic inputs (t, A, mu multiples of 1/64, s = 2^-3: every normalisation is exact): val_grad and
    stats[VLOSS] are the plain pass's on (t^, A s), bit for bit."""
    pol, val = make_nets()
    rows, idx = make_rows(mb + 37, 10 + mb), pick(mb + 37, mb, mb)
    rs = np.random.RandomState(mb)
    n = mb + 37
    mu, s = np.float32(-1.5), np.float32(0.125)
    rows["tgt"] = (rs.randint(-640, 641, n) / 64.0).astype(np.float32)       # t^ in [-1.06, 1.44]: around the critic's outputs
    rows["adv"] = (rs.randint(-256, 257, n) / 64.0).astype(np.float32)
    tn, an = (rows["tgt"] - mu) * s, rows["adv"] * s
    assert np.array_equal(tn.astype(np.float64), (rows["tgt"].astype(np.float64) + 1.5) / 8) and np.array_equal(an.astype(np.float64), rows["adv"].astype(np.float64) / 8)
    got = run_pass(L, pol, val, rows, idx, "vnorm", scale=[mu, s, 8.0, 0.0], vclip=0.25)
    want = run_pass(L, pol, val, rows, idx, "plain", vclip=0.25, tgt=tn, adv=an)
    same_pass(got, want, f"(b) mb={mb}", policy=False)
    if mb > 1:
        zero = (got[1] == 0).all().item()
        assert not zero and not torch.equal(got[1], run_pass(L, pol, val, rows, idx, "vnorm", scale=[mu, s, 8.0, 0.0])[1])   # clipping bites


def critic64(val, obs, masks, loss_fn):
    """float64 forward of the critic under imposed ReLU masks, the yardstick's loss on its outputs, backward -> (grads, loss)."""
    f = lambda t: np.asarray(t, np.float64)
    h, acts = f(obs), []
    for l, (w, b) in enumerate(val):
        acts.append(h)
        h = h @ f(w).T + f(b)
        if l + 1 < len(val):
            h = h * masks[l]
    loss, g = loss_fn(h[:, 0])
    gout = g[:, None]
    grads = [None] * len(val)
    for l in range(len(val) - 1, -1, -1):
        grads[l] = (gout.T @ acts[l], gout.sum(0))
        if l:
            gout = (gout @ f(val[l][0])) * masks[l - 1]
    return grads, loss


def critic32(val, obs, tn, v_old, c):
    ps = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in val]
    h = torch.as_tensor(obs)
    for l, (w, b) in enumerate(ps):
        h = torch.nn.functional.linear(h, w, b)
        if l + 1 < len(ps):
            h = torch.relu(h)
    vo = torch.as_tensor(v_old)
    torch.nn.functional.mse_loss(vo + torch.clamp(h.view(-1) - vo, -c, c), torch.as_tensor(tn)).backward()
    return [(w.grad, b.grad) for w, b in ps]


@pytest.mark.parametrize("mb", [257, 1500])
def test_vnorm_clipped_value_loss_matches_float64(L, mb):
    """(c) general inputs, value_clip = 0.25, about half of the rows outside the band: the critic's gradient against float64 truth under the
    HIP's own ReLU decisions within the gate tests/fp64_gate.py holds the critic to -- err <= max(1e-5, 1.5 err(CPU float32)) -- and VLOSS
    at 1e-5 relative."""
    c = 0.25
    pol, val = make_nets(seed=3)
    rows = make_rows(mb, 20 + mb)
    idx = np.arange(mb, dtype=np.int64)
    rs = np.random.RandomState(mb)
    mu, inv_sd, sd = (float(x) for x in SCALE[:3])
    v0 = nets.value_forward(val, rows["obs"]).flatten().numpy().astype(np.float64)
    rows["tgt"] = ((v0 + 0.5 * rs.randn(mb)) * sd + mu).astype(np.float32)          # t^ near v^
    v_old_real = (v0 + 0.3 * rs.randn(mb)) * sd + mu                                # |v^ - v^_old| > 0.25 for ~40 %
    rows["adv"] = (rows["tgt"].astype(np.float64) - v_old_real).astype(np.float32)
    gp, gv, stats = run_pass(L, pol, val, rows, idx, "vnorm", scale=SCALE, vclip=c)
    masks = fp64_gate.hip_masks(L, val, rows["obs"])
    loss_fn = lambda v: VY.value_loss64(v, rows["tgt"], rows["adv"], mu, inv_sd, c)
    truth, loss64 = critic64(val, rows["obs"], masks, loss_fn)
    v_old_n = ((rows["tgt"] - rows["adv"]).astype(np.float32).astype(np.float64) - mu) * inv_sd
    outside = float((np.abs(v0 - v_old_n) > c).mean())
    assert 0.2 <= outside <= 0.7, outside
    got = [(w.numpy(), b.numpy()) for w, b in nets.unflatten(gv, val)]
    tn64 = (rows["tgt"].astype(np.float64) - mu) * inv_sd
    cpu = critic32(val, rows["obs"], tn64.astype(np.float32), v_old_n.astype(np.float32), c)
    cpu_truth, _ = critic64(val, rows["obs"], fp64_gate.cpu_masks(val, rows["obs"]), loss_fn)
    e_hip, e_cpu = fp64_gate.grads_err(got, truth), fp64_gate.grads_err(cpu, cpu_truth)
    print(f"[fp64 gate] normalised clipped value loss, mb={mb}: err(HIP)={e_hip:.2e} err(CPU fp32)={e_cpu:.2e}, {outside:.0%} outside; "
          f"VLOSS {stats[2]:.9g} vs {loss64:.9g}")
    assert e_hip <= max(1e-5, 1.5 * e_cpu), (e_hip, e_cpu)
    assert abs(stats[2] - loss64) <= 1e-5 * abs(loss64), (stats[2], loss64)


def test_vnorm_pass_with_tanh_networks_and_with_critic_rows(L):
    """(e) the combinations run and match (a)'s construction: the same entry point's pass without vnorm on host-normalised targets."""
    mb = 257
    idx = pick(mb + 37, mb, 2)
    tn = lambda rows: VY.normalise_targets32(rows["tgt"], SCALE[0], SCALE[1])
    pol, val = make_nets(seed=1)
    rows = make_rows(mb + 37, 31)
    same_pass(run_pass(L, pol, val, rows, idx, "vnorm", scale=SCALE, act="tanh"), run_pass(L, pol, val, rows, idx, "ex", act="tanh", tgt=tn(rows)), "(e) tanh")
    assert not torch.equal(run_pass(L, pol, val, rows, idx, "vnorm", scale=SCALE, act="tanh")[1], run_pass(L, pol, val, rows, idx, "vnorm", scale=SCALE)[1])
    pol, val = make_nets(cobs=29, seed=2)
    rows = make_rows(mb + 37, 32, cobs=29)
    from rlgym_ppo_amd import _native as N
    c0 = int(L.rlppo_dbg_counter(N.COUNTER_CRITIC_ROWS_PASS))
    same_pass(run_pass(L, pol, val, rows, idx, "vnorm", scale=SCALE), run_pass(L, pol, val, rows, idx, "critic", tgt=tn(rows)), "(e) critic rows")
    assert int(L.rlppo_dbg_counter(N.COUNTER_CRITIC_ROWS_PASS)) == c0 + 2
