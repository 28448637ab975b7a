"""The hybrid head's kernels (csrc/hybrid.hip) through the C ABI: the sampling step decomposes bit for bit into the diag head's samples and
the [nvec] head's indices, and the loss step meets a float64 torch-autograd restatement (Normal + Categoricals, the clipped surrogate, the
entropy bonus) within the allowance of tests/fp64_gate.py: err(HIP, fp64) <= max(1e-5, 1.5 x err(float32 torch, fp64)), errors as
max|got - want| / max|want|, statistics at 1e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hip_pass import L, Net, P, check, dev, stream  # noqa: E402,F401
from rlgym_ppo_amd import _native as N  # noqa: E402

# (k, nvec): the smallest head; a controller; 19 heads (lanes carry two, a one-bin head among them) with k past 16; 512 logits
CASES = {"1+[2]": (1, [2]), "5+[2,2,2]": (5, [2, 2, 2]), "17+19heads": (17, [3, 1, 64, 2, 7] + [5] * 14), "3+[64]*8": (3, [64] * 8)}
ROWS = (1, 63, 257)   # one row; a partial tile and a partial 16-lane group; a second workgroup with one row
CLIP, ENT, MB_RATIO = 0.2, 0.005, 0.5


def inputs(name, n):
    k, nvec = CASES[name]
    rs = np.random.RandomState(1000 * n + k)
    y = (1.5 * rs.randn(n, k + sum(nvec))).astype(np.float32)
    log_std = rs.uniform(-0.7, 0.3, k).astype(np.float32)
    eps = rs.randn(n, k).astype(np.float32)
    q = rs.exponential(size=(n * len(nvec), max(nvec))).astype(np.float32) + 1e-6
    return k, nvec, rs, y, log_std, eps, q


def rows_at(y, ld):
    out = torch.full((y.shape[0], ld), float("nan"))
    out[:, :y.shape[1]] = torch.as_tensor(y)
    return out.cuda()


def selector(rows, width):
    """One layer whose output j is input rows[j] times 1.0: the chain's outputs are the inputs, exactly, whatever order the product sums in."""
    w = torch.zeros(len(rows), width)
    w[torch.arange(len(rows)), torch.as_tensor(rows)] = 1.0
    return [(w, torch.zeros(len(rows)))]


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(CASES))
def test_sampling_decomposes_into_the_two_heads(L, name, n):
    k, nvec, _, y, log_std, eps, q = inputs(name, n)
    H, S, W = len(nvec), sum(nvec), k + sum(nvec)
    nv, lsd, epsd, qd = N.dims_array(nvec), dev(log_std), dev(eps), dev(q)
    nets = [Net(L, selector(r, W)) for r in (range(W), range(k), range(k, W))]
    obs = nets[0].pad(y)
    act, logp = torch.full((n, k + H), -7.0, device="cuda"), torch.empty(n, device="cuda")
    a_d, lp_d = torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
    a_n, lp_n = torch.empty(n, H, dtype=torch.int64, device="cuda"), torch.empty(n, device="cuda")
    hy, dg, md = nets
    ws = [x.ws(n) for x in nets]
    check(L, L.rlppo_hybrid_act(stream(), hy.dims_c, 1, P(hy.packed), P(obs), hy.ld_in, n, k, nv, H, P(epsd), P(qd), P(lsd), P(act), P(logp),
                                P(ws[0]), ws[0].numel(), None))
    check(L, L.rlppo_diag_gaussian_act(stream(), dg.dims_c, 1, P(dg.packed), P(obs), dg.ld_in, n, P(epsd), P(lsd), P(a_d), P(lp_d), P(ws[1]),
                                       ws[1].numel(), None))
    check(L, L.rlppo_multidiscrete_act_nvec(stream(), md.dims_c, 1, P(md.packed), P(obs), md.ld_in, n, P(qd), P(a_n), P(lp_n), P(ws[2]),
                                            ws[2].numel(), None, nv, H))
    # ... and the kernel alone on rows of a leading dimension the chain does not produce
    act2, logp2 = torch.empty_like(act), torch.empty_like(logp)
    wide = rows_at(y, hy.ld_out + 36)
    check(L, L.rlppo_dbg_hybrid_sample(stream(), P(wide), wide.shape[1], n, k, nv, H, P(epsd), P(qd), P(lsd), P(act2), P(logp2)))
    torch.cuda.synchronize()
    assert torch.equal(act[:, :k], a_d) and torch.equal(act[:, k:], a_n.float())
    assert torch.equal(act, act2) and torch.equal(logp, logp2)
    want = (lp_d + lp_n).cpu().numpy()
    scale = np.maximum(np.abs(lp_d.cpu().numpy()), np.abs(lp_n.cpu().numpy()))
    ulps = float((np.abs(logp.cpu().numpy() - want) / np.spacing(scale.astype(np.float32))).max())
    print(f"[hybrid] {name}, {n} rows: log p within {ulps:.1f} float32 ulps of the two heads' sum")
    assert ulps <= 8.0   # (observed: at most 4; the diag head sums up to 32 float terms serially, the hybrid all terms in double)


def loss64(y, log_std, acts, old, adv, k, nvec, dtype):
    """The loss in torch autograd at `dtype` -> (dL/dy, dL/dlog_std, [entropy, kl, -, clip fraction, policy loss], ratio)."""
    t = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    y, ls = t(y).requires_grad_(), t(log_std).requires_grad_()
    acts, old, adv = t(acts), t(old), t(adv)
    gauss = torch.distributions.Normal(y[:, :k], ls.exp())
    logp, ent = gauss.log_prob(acts[:, :k]).sum(-1), gauss.entropy().sum(-1).expand(y.shape[0])
    s = k
    for h, b in enumerate(nvec):
        cat = torch.distributions.Categorical(logits=y[:, s:s + b])
        logp, ent, s = logp + cat.log_prob(acts[:, k + h].long()), ent + cat.entropy(), s + b
    ratio = (logp - old).exp()
    surr = torch.min(ratio * adv, ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * adv)
    (MB_RATIO * (-surr.mean() - ENT * ent.mean())).backward()
    with torch.no_grad():
        st = [ent.mean(), ((ratio - 1) - (logp - old)).mean(), 0.0, ((ratio - 1).abs() > CLIP).double().mean(), -surr.mean()]
    return y.grad.numpy(), ls.grad.numpy(), np.asarray([float(x) for x in st]), ratio.detach().numpy()


def rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


@pytest.mark.parametrize("ld_extra", (0, 36))
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("name", list(CASES))
def test_loss_against_float64_autograd(L, name, n, ld_extra):
    k, nvec, rs, y, log_std, eps, _ = inputs(name, n)
    H, S, W = len(nvec), sum(nvec), k + sum(nvec)
    acts = np.concatenate([y[:, :k] + np.exp(log_std) * eps, (rs.rand(n, H) * np.asarray(nvec)).astype(np.int64)], 1).astype(np.float32)
    adv = rs.randn(n).astype(np.float32)
    lp0 = np.log(loss64(y, log_std, acts, np.zeros(n), adv, k, nvec, torch.float64)[3])
    old = (lp0 + 0.25 * rs.randn(n)).astype(np.float32)   # ratios on both sides of both clip edges
    dy64, dls64, st64, ratio = loss64(y, log_std, acts, old, adv, k, nvec, torch.float64)
    assert np.minimum(np.abs(ratio - (1 - CLIP)), np.abs(ratio - (1 + CLIP))).min() > 1e-5   # no row float32 rounding could decide either way
    dy32, dls32, _, _ = loss64(y, log_std, acts, old, adv, k, nvec, torch.float32)
    ld = int(L.rlppo_padded_out(W)) + ld_extra
    sb = int(L.rlppo_diag_scratch_bytes(n, k))
    runs, (actd, oldd, advd, lsd) = [], (dev(x) for x in (acts, old, adv, log_std))
    for _ in range(2):
        yd, gls = rows_at(y, ld), torch.zeros(k, device="cuda")
        stats, scratch = torch.zeros(8, dtype=torch.float64, device="cuda"), torch.full((sb,), 0xFF, dtype=torch.uint8, device="cuda")
        check(L, L.rlppo_dbg_hybrid_loss(stream(), P(yd), ld, k, N.dims_array(nvec), H, P(actd), P(oldd), P(advd), n, CLIP, ENT, MB_RATIO,
                                         P(lsd), P(gls), P(scratch), sb, P(stats), 0))
        torch.cuda.synchronize()
        runs.append((yd.cpu().numpy(), gls.cpu().numpy(), stats.cpu().numpy()))
    (dy, dls, st), again = runs
    assert all(np.array_equal(a, b) for a, b in zip(runs[0], again))   # the same bits, the log_std gradient included
    assert (dy[:, W:] == 0).all() and np.isfinite(dy).all()
    if 1 in nvec:   # a head of one bin: nothing behind it
        assert (dy[:, k + int(np.cumsum([0] + nvec)[nvec.index(1)])] == 0).all()
    e_dy, e_ls, c_dy, c_ls = rel(dy[:, :W], dy64), rel(dls, dls64), rel(dy32, dy64), rel(dls32, dls64)
    print(f"[hybrid] {name}, {n} rows, ld {ld}: dL/dy err {e_dy:.2e} (float32 torch {c_dy:.2e}), dL/dlog_std err {e_ls:.2e} ({c_ls:.2e})")
    assert e_dy <= max(1e-5, 1.5 * c_dy) and e_ls <= max(1e-5, 1.5 * c_ls)
    for i in (0, 1, 4):
        assert abs(st[i] - st64[i]) <= 1e-5 * max(abs(st64[i]), 1e-3) + 1e-7, (i, st[i], st64[i])
    assert abs(st[3] - st64[3]) <= 0.5 / n + 1e-9   # the gate's allowance for the clip fraction without edge rows: less than one row
