"""The hidden-activation choice on the GPU (include/rlppo.h, "[act]"; Learner(hidden_activation=...), ppo.LayerSizes): the three new
GEMM epilogues, one update pass, the rollout entry points, PPOLearner.learn and the Learner loop with tanh / ELU (alpha = 1) hidden
layers, against the float64 yardstick of tests/ppo_yardstick.py under the project's tolerance rule:
err(HIP, float64) <= max(1e-5, 1.5 x err(float32 yardstick, float64)).

Inputs are built on the CPU and checked there, from float64 alone, before anything runs on the GPU (no ratio near a clip edge; the
cap on ill-conditioned Adam steps).  With tanh / ELU no hidden decision is discrete (ppo_yardstick's docstring), so there is
no counterpart of the ReLU tests' assert_relu_clear."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets  # noqa: E402
import ppo_yardstick as A  # noqa: E402
import diag_gaussian_env as E  # noqa: E402
from diag_gaussian_yardstick import assert_clear_of_clip_edges, logp_terms  # noqa: E402
from hip_pass import L, Net, P, check, dev, run_pass, stream  # noqa: E402,F401

U32 = 2.0 ** -24
CLIP, ENT = 0.2, 0.005
ACTS = ("tanh", "elu")
EPI_TANH, EPI_MASK, EPI_ELU, EPI_DTANH, EPI_DELU = 2, 3, 4, 5, 6
NS, KS = (32, 64, 96, 128, 256), (16, 48, 256)   # every tile width of gemm_nt_dma_kernel; BK = 16 (K = 16, 48) and BK = 32 (K = 256 at N = 32)


def counters(L, *keys):
    return [int(L.rlppo_dbg_counter(k)) for k in keys]


# ------------------------------------------------------------------------------------------------ 1. kernel epilogues
def gemm_nt(L, A_, B_, bias, mask, M, N, K, epi):
    C = torch.full((M, N), float("nan"), device="cuda")
    check(L, L.rlppo_dbg_gemm_nt(stream(), P(A_), A_.shape[1], P(B_), K, P(bias), P(mask), N, P(C), N, M, N, K, epi))
    return C.cpu()


def product_bound(A_, B_, bias, K):
    """Elementwise bound of a float32 dot product of K terms (+ bias) against the float64 one of the same operands:
    (K + 8) u (sum_k |a_k b_k| + |bias|)."""
    s = A_.abs().double() @ B_.abs().double().T
    return (K + 8) * U32 * (s + (bias.abs().double() if bias is not None else 0.0))


@pytest.mark.parametrize("M", [1, 130, 1100])   # the few-row kernel, a row tail, 128-row tiles above SK_MAX_ROWS = 1024
@pytest.mark.parametrize("epi", [EPI_TANH, EPI_ELU], ids=["tanh", "elu"])
def test_forward_epilogues_against_float64(L, epi, M):
    """C = f(A.B^T + bias), f = tanh / ELU, against float64 of the same float32 operands.  Both are 1-Lipschitz, so the allowance is
    the product's own float32 bound + 4 u |f| for the evaluation of f itself (expm1f / tanhf are good to a few ulp)."""
    f = torch.tanh if epi == EPI_TANH else torch.nn.functional.elu
    for N in NS:
        for K in KS:
            g = torch.Generator().manual_seed(1000 * epi + M + N + K)
            A_ = torch.randn(M, K + 32, generator=g)      # lda > K
            B_ = torch.randn(N, K, generator=g) * (2.0 / K ** 0.5)   # pre-activations of O(1): both sides of 0, some saturated
            bias = torch.randn(N, generator=g) * 0.5
            if M > 1:   # row 1 x the first half of the columns: tiny pre-activations BY CONSTRUCTION (ELU near 0: the expm1 evaluation)
                A_[1, :K] *= 1e-4
                bias[:N // 2] *= 1e-4
            C = gemm_nt(L, dev(A_), dev(B_), dev(bias), None, M, N, K, epi)
            pre = A_[:, :K].double() @ B_.double().T + bias.double()
            want = f(pre)
            allow = product_bound(A_[:, :K], B_, bias, K) + 4 * U32 * want.abs() + 1e-30
            worst = float(((C.double() - want).abs() / allow).max())
            assert worst <= 1.0, (epi, M, N, K, worst)
            assert (pre < 0).any() and (pre > 0).any()
            if M > 1:
                tiny = pre[1, :N // 2]
                assert tiny.abs().max() < 2e-3 and (tiny < 0).any() and (tiny > 0).any()


@pytest.mark.parametrize("M", [130, 1100])
@pytest.mark.parametrize("epi", [EPI_DTANH, EPI_DELU], ids=["dtanh", "delu"])
def test_derivative_epilogues_against_float64(L, epi, M):
    """C = (A.B^T) f'(h) with the saved activation h read from mask_src as EPI_MASK reads it.  h holds exact 0 and +-1 (tanh) /
    exact 0 and values just below 0 (ELU).  |f'| <= 1 on the range of h, so the allowance is the product's bound times |f'| + the
    rounding of the factor (below) and of the multiplication (4 u |want|)."""
    for N in NS:
        for K in KS:
            g = torch.Generator().manual_seed(1000 * epi + M + N + K)
            A_ = torch.randn(M, K + 32, generator=g)
            B_ = torch.randn(N, K, generator=g)
            ld_mask = N + 4   # ld_mask > N
            if epi == EPI_DTANH:
                h = torch.tanh(torch.randn(M, ld_mask, generator=g) * 2)
                h[0, :8] = torch.tensor([0.0, 1.0, -1.0, -0.0, 1.0, -1.0, 0.5, -0.5])
                fp = 1.0 - h.double() ** 2
            else:
                h = torch.nn.functional.elu(torch.randn(M, ld_mask, generator=g) * 2)
                h[0, :8] = torch.tensor([0.0, -0.0, -1e-7, -1e-30, 1e-7, -0.999999, 3.0, -0.5])
                fp = torch.where(h > 0, torch.ones_like(h, dtype=torch.float64), h.double() + 1.0)
            C = torch.full((M, N), float("nan"), device="cuda")
            Ad, Bd, hd = dev(A_), dev(B_), dev(h)
            check(L, L.rlppo_dbg_gemm_nt(stream(), P(Ad), A_.shape[1], P(Bd), K, None, P(hd), ld_mask, P(C), N, M, N, K, epi))
            prod = A_[:, :K].double() @ B_.double().T
            want = prod * fp[:, :N]
            # (the factor itself is evaluated in float32: h * h and the subtraction / h + 1 round once each at magnitude <= 2 -- an
            # ABSOLUTE error of up to 2 u in f', which matters where tanh is saturated and f' is tiny)
            allow = product_bound(A_[:, :K], B_, None, K) * fp[:, :N].abs() + 2 * U32 * prod.abs() + 4 * U32 * want.abs() + 1e-30
            worst = float(((C.cpu().double() - want).abs() / allow).max())
            assert worst <= 1.0, (epi, M, N, K, worst)
    # a missing mask operand is an argument error, as for the ReLU mask
    assert L.rlppo_dbg_gemm_nt(stream(), P(Ad), A_.shape[1], P(Bd), K, None, None, 0, P(C), N, M, N, K, epi) == 1001


@pytest.mark.parametrize("epi", [EPI_TANH, EPI_ELU], ids=["tanh", "elu"])
def test_few_row_and_large_tile_forward_agree_bit_for_bit(L, epi):
    """M = 130 through gemm_nt_skinny_kernel and (rlppo_dbg_set(40, 0)) through gemm_nt_dma_kernel: the same arithmetic, the same
    activation function on the same accumulators -- what tests/test_gpu_kernels.py::test_gemm_nt_skinny requires for ReLU."""
    M = 130
    for N in NS:
        for K in KS:
            g = torch.Generator().manual_seed(epi + N + K)
            A_, B_, bias = dev(torch.randn(M, K, generator=g)), dev(torch.randn(N, K, generator=g) / K ** 0.5), dev(torch.randn(N, generator=g))
            outs = []
            for skinny in (1, 0):
                check(L, L.rlppo_dbg_set(40, skinny))
                try:
                    outs.append(gemm_nt(L, A_, B_, bias, None, M, N, K, epi))
                finally:
                    check(L, L.rlppo_dbg_set(40, 1))
            assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any(), (epi, N, K)


# ------------------------------------------------------------------------------------------------ 2. one pass against float64
BINS = (3, 2, 4, 1, 5)   # a multi-discrete nvec that is not the reference's: 15 logits, a one-bin head


def make_case(head, seed, n=420, d=13, pol_hidden=(64, 128), val_hidden=(32, 64), pol_act="tanh", val_act=None):
    """Policy + critic + an n-row buffer whose stored log-probabilities are the float64 yardstick's, shifted as
    tests/test_gpu_diag_gaussian.py::make_case shifts them: a third of the rows inside the clip range, a third above, a third below."""
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    n_out = {"discrete": 6, "diag": 3, "gaussian": 6, "nvec": sum(BINS)}[head]
    pol, val = nets.init_mlp(d, pol_hidden, n_out), nets.init_mlp(d, val_hidden, 1)
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    hk, log_std, mask = {}, None, None
    if head == "discrete":
        act = rs.randint(0, n_out, n).astype(np.float32)
    elif head == "nvec":
        act = np.stack([rs.randint(0, b, n) for b in BINS], 1).astype(np.float32)
        mask = rs.rand(n, n_out) < 0.7
        for h, (s, b) in enumerate(zip(A.starts(BINS), BINS)):
            mask[np.arange(n), s + act[:, h].astype(int)] = True   # stored actions are valid
        mask[3::5] = True
        hk = dict(bins=BINS, mask=mask)
    elif head == "gaussian":
        act = np.clip(0.5 * rs.randn(n, 3), -1, 1).astype(np.float32)
    else:
        log_std = rs.uniform(-1.0, 0.5, n_out).astype(np.float32)
        mean = A.forward64(pol, obs, pol_act)
        act = (mean + np.exp(log_std.astype(np.float64)) * rs.randn(n, n_out)).astype(np.float32)
    c = dict(head=head, pol=pol, val=val, obs=obs, act=act, log_std=log_std, mask=mask, hk=hk, pol_act=pol_act, val_act=val_act or pol_act)
    z = torch.as_tensor(A.forward64(pol, obs, pol_act, out_tanh=head == "gaussian"))
    ls64 = None if log_std is None else torch.as_tensor(log_std, dtype=torch.float64)
    logp = A.head_terms(head, z, torch.as_tensor(act, dtype=torch.float64), log_std=ls64, **hk)[0].numpy()
    cls = np.arange(n) % 3
    off = 0.05 * rs.randn(n) + np.where(cls == 1, -0.5, 0.0) + np.where(cls == 2, 0.5, 0.0)
    c.update(old=(logp + off).astype(np.float32), adv=rs.randn(n).astype(np.float32), tgt=rs.randn(n).astype(np.float32), rs=rs)
    return c


def yard(c, idx, mb_ratio):
    m = c["mask"]
    hk = dict(c["hk"], mask=m[idx]) if m is not None else c["hk"]
    args = (c["head"], c["pol"], c["val"], c["obs"][idx], c["act"][idx], c["old"][idx], c["adv"][idx], c["tgt"][idx], CLIP, ENT, mb_ratio)
    hk = dict(hk, pol_act=c["pol_act"], val_act=c["val_act"], log_std=c["log_std"])
    r64 = A.minibatch(torch.float64, *args, **hk)
    assert_clear_of_clip_edges(r64["ratio"], CLIP)
    return r64, A.minibatch(torch.float32, *args, **hk)


def hip(L, c, idx, mb_ratio, entry="ex", precision="fp32", **kw):
    return run_pass(L, c["pol"], c["val"], c["obs"], c["act"], c["old"], c["tgt"], c["adv"], idx, head=c["head"], entry=entry, precision=precision,
                    pol_act=c["pol_act"], val_act=c["val_act"], clip=CLIP, ent=ENT, mb_ratio=mb_ratio, log_std=c["log_std"],
                    bins=c["hk"].get("bins"), mask=c["mask"], raise_rc=False, **kw)


def pass_idx(c, mb=300):
    return c["rs"].permutation(len(c["obs"]))[:mb]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", ["discrete_gemv_head", "diag_gemm_head"])
def test_pass_against_float64(L, shape, act):
    """mb = 300 (a row tail), obs 13.  discrete (13, 64, 128, 6) + critic (13, 32, 64, 1): the one-output head on a power-of-two width
    takes the matrix-vector dX; diagonal-Gaussian (13, 96, 96, 3) + critic (13, 96, 96, 1): a width that is no power of two takes the
    GEMM dX for the head.  Witnesses: one pass, not paired, not gather-fused."""
    if shape == "discrete_gemv_head":
        c = make_case("discrete", 31, pol_act=act)
    else:
        c = make_case("diag", 37, pol_hidden=(96, 96), val_hidden=(96, 96), pol_act=act)
    idx = pass_idx(c)
    r64, r32 = yard(c, idx, 0.5)
    before = counters(L, 2, 3, 4)
    got = hip(L, c, idx, 0.5)
    after = counters(L, 2, 3, 4)
    assert got["rc"] == 0, got["msg"]
    assert [b - a for a, b in zip(before, after)] == [1, 0, 0]
    A.gate(got, r64, r32, f"[act fp64 gate] {shape} {act}")
    # the paired / gather-fused forms forced "always" (switches 29 = 2, 26 = 2) still do not apply to a tanh / ELU pass
    check(L, L.rlppo_dbg_set(29, 2))
    check(L, L.rlppo_dbg_set(26, 2))
    try:
        before = counters(L, 2, 3, 4)
        again = hip(L, c, idx, 0.5)
        assert [b - a for a, b in zip(before, counters(L, 2, 3, 4))] == [1, 0, 0]
    finally:
        check(L, L.rlppo_dbg_set(29, 1))
        check(L, L.rlppo_dbg_set(26, 1))
    assert torch.equal(again["gp"], got["gp"]) and torch.equal(again["gv"], got["gv"])   # the same launches: bit-reproducible


def test_pass_mixed_activations_ring_empty_buffer_rows_and_accumulation(L):
    """A tanh policy beside an ELU critic; the same pass from a ring-mapped buffer and with n_rows == 0 is bit-identical; a pass into
    gradient arenas that already hold values ADDS to them."""
    c = make_case("discrete", 41, pol_act="tanh", val_act="elu")
    idx = pass_idx(c)
    r64, r32 = yard(c, idx, 1.0)
    got = hip(L, c, idx, 1.0)
    assert got["rc"] == 0, got["msg"]
    A.gate(got, r64, r32, "[act fp64 gate] tanh policy, ELU critic")
    for kw in (dict(ring=137), dict(n_rows=0)):
        other = hip(L, c, idx, 1.0, **kw)
        assert other["rc"] == 0 and torch.equal(other["gp"], got["gp"]) and torch.equal(other["gv"], got["gv"]), kw
        assert np.array_equal(other["stats"], got["stats"]), kw
    gp0, gv0 = torch.randn_like(got["gp"]), torch.randn_like(got["gv"])
    acc = hip(L, c, idx, 1.0, grads=(gp0.clone(), gv0.clone()))
    for new, base, g in ((acc["gp"], gp0, got["gp"]), (acc["gv"], gv0, got["gv"])):
        assert torch.equal(new, base + g)   # one add per element and launch


@pytest.mark.parametrize("head", ["nvec", "gaussian"])
def test_pass_other_heads(L, head):
    """The multi-discrete head for an nvec of its own WITH a mask, and the reference's Gaussian head, ELU hidden layers."""
    c = make_case(head, {"nvec": 43, "gaussian": 47}[head], pol_act="elu")
    idx = pass_idx(c)
    r64, r32 = yard(c, idx, 1.0)
    c6 = counters(L, 6)[0]
    got = hip(L, c, idx, 1.0)
    assert got["rc"] == 0, got["msg"]
    if head == "nvec":
        assert counters(L, 6)[0] == c6 + 1   # the general (any nvec) loss kernel ran
    A.gate(got, r64, r32, f"[act fp64 gate] {head} elu")


def test_zero_extension_is_the_plain_entry_point(L):
    """rlppo_ppo_minibatch_ex with an all-zero extension, with a NULL one, and rlppo_ppo_minibatch: bit-identical gradients and
    statistics on a ReLU pass whose shape takes the bitmask forms (hidden widths 128)."""
    c = make_case("discrete", 53, pol_hidden=(128, 128), val_hidden=(128, 128), pol_act="relu")
    idx = pass_idx(c)
    outs = [hip(L, c, idx, 1.0, entry=e) for e in ("plain", "ex_zero", "ex_null", "ex")]   # ("ex": both activation codes 0)
    assert all(o["rc"] == 0 for o in outs)
    for o in outs[1:]:
        assert torch.equal(o["gp"], outs[0]["gp"]) and torch.equal(o["gv"], outs[0]["gv"]) and np.array_equal(o["stats"], outs[0]["stats"])
    assert float(outs[0]["gp"].abs().max()) > 0
    # switch 19 = 0: the same ReLU pass in the plain form (dX by the saved activation): the same gradients up to summation order
    check(L, L.rlppo_dbg_set(19, 0))
    try:
        plain = hip(L, c, idx, 1.0, entry="plain")
    finally:
        check(L, L.rlppo_dbg_set(19, 1))
    assert A.err(A.tensors(plain), A.tensors(outs[0])) < 1e-5
    # update precisions bf16 / x3 refuse a tanh / ELU network by name (before any launch)
    c["pol_act"] = "tanh"
    for prec in ("bf16", "x3"):
        r = hip(L, c, idx, 1.0, precision=prec)
        assert r["rc"] == 1001 and "hidden activation tanh" in r["msg"] and prec in r["msg"], r["msg"]


# ------------------------------------------------------------------------------------------------ 3. rollout
OBS = 13
MD_BINS = (3, 2, 4)


REFERENCE_BINS = (3, 3, 3, 3, 3, 2, 2, 2)


def build_policy(kind, act, seed=7, hidden=(32, 32), bins=MD_BINS):
    from rlgym_ppo_amd.ppo import ContinuousPolicy, DiagGaussianPolicy, DiscreteFF, LayerSizes, MultiDiscreteFF
    torch.manual_seed(seed)
    sizes = LayerSizes(hidden, act) if act != "plain" else tuple(hidden)
    if kind == "discrete":
        return DiscreteFF(OBS, 6, sizes, "cuda:0")
    if kind == "multidiscrete":
        return MultiDiscreteFF(OBS, sizes, "cuda:0", bins=bins)   # (bins=None: the reference's eight heads on the fixed-bin kernels)
    if kind == "gaussian":
        return ContinuousPolicy(OBS, 6, sizes, "cuda:0")
    pol = DiagGaussianPolicy(OBS, 3, sizes, "cuda:0")
    pol.fill_log_std(-0.3)
    return pol


def params_cpu(module):
    return [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in module.arena.linears]


def head_of_output(kind, pol, y, noise, bins=None, mask=None):
    """torch, any dtype: the head's (choice or action, log p, margin) on network outputs y [n, n_out] with the call's noise.
    margin: for the discrete heads, the relative gap of the two best p / q per row (and head) -- +inf elsewhere.
    bins: the multi-discrete head's nvec (default MD_BINS); mask (bool [n, n_out], the discrete heads): invalid logits are -inf and
    the arg-max runs over the valid entries (include/rlppo.h, "[ABI 8]" / "[nvec, masked]")."""
    dt = y.dtype
    q = torch.as_tensor(np.asarray(noise), dtype=dt)
    n = y.shape[0]
    if kind in ("discrete", "multidiscrete"):
        bins = (y.shape[1],) if kind == "discrete" else tuple(bins or MD_BINS)
        B = max(bins)
        q = q.view(n, len(bins), B)
        m = torch.ones(y.shape, dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask, bool))
        acts, logp, margin = [], 0.0, []
        for h, (s, b) in enumerate(zip(A.starts(bins), bins)):
            mh = m[:, s:s + b]
            lsm = torch.log_softmax(y[:, s:s + b].masked_fill(~mh, float("-inf")), -1)
            p = torch.exp(lsm)
            if kind == "discrete":   # the reference's clamp (on valid actions; an invalid one is never selectable)
                p = torch.clamp(p, min=nets.PROB_MIN, max=1)
                lsm = torch.log(p)
            score = torch.where(mh, p / q[:, h, :b], torch.full_like(p, float("-inf")))
            a = score.argmax(-1)
            top = torch.sort(score, -1).values
            margin.append((top[:, -1] - top[:, -2]) / top[:, -1] if b > 1 else torch.full((n,), float("inf"), dtype=dt))
            acts.append(a)
            logp = logp + lsm.gather(1, a[:, None]).view(-1)
        return torch.stack(acts, 1), logp, torch.stack(margin, 1)
    if kind == "gaussian":
        k = y.shape[1] // 2
        m, b = nets.var_map(0.1, 1.0)
        mean, std = y[:, :k], y[:, k:] * m + b
        act = (q * std + mean).clamp(-1, 1)
        return act, nets.gauss_logpdf(act, mean, std).sum(1), None
    ls = pol.log_std.detach().cpu().to(dt)
    act = y + torch.exp(ls) * q
    return act, logp_terms(act, y, ls).sum(-1), None


def check_rollout(kind, pol, act_name, obs, noise, got_act, got_logp, label, bins=None, mask=None):
    """The seeded actions of the discrete heads equal the float32 torch restatement's choice wherever its two best p / q are further
    apart than the forward allowance; continuous actions and log-probabilities lie within the forward allowance
    (|dy| <= 1e-5 |y| + 2e-6 on the network outputs) carried through the head by its float64 derivative, or within 1.5 x what the
    float32 restatement itself misses float64 by."""
    params = params_cpu(pol)
    out_tanh = kind == "gaussian"
    y64 = torch.as_tensor(A.forward64(params, obs, act_name, out_tanh)).requires_grad_(True)
    y32 = torch.as_tensor(A.forward32(params, obs, act_name, out_tanh))
    a64, lp64, _ = head_of_output(kind, pol, y64, noise, bins, mask)
    a32, lp32, margin = head_of_output(kind, pol, y32, noise, bins, mask)
    dy = A.FWD_RTOL * y64.detach().abs() + A.FWD_ATOL            # the forward allowance, elementwise
    got_act, got_logp = np.asarray(got_act), np.asarray(got_logp, np.float64)
    (g,) = torch.autograd.grad(lp64.sum(), y64, retain_graph=True)
    lp_allow = ((g.abs() * dy).sum(1) + 1e-5 * lp64.detach().abs() + 2e-6).numpy()
    e32 = np.abs(lp32.double().numpy() - lp64.detach().numpy())
    if kind in ("discrete", "multidiscrete"):
        # a relative error of 2 max|dz| on every p (softmax of logits that are off by dz): twice that on a ratio of two scores
        clear = (margin.double() > 4 * float(dy.max()) + 4 * U32).numpy()
        mine = got_act.reshape(clear.shape)
        assert np.array_equal(mine[clear], a32.numpy()[clear]), label
        if mask is not None:   # no sampled action is invalid, near-tie or not
            for h, (s, b) in enumerate(zip(A.starts(bins or (mask.shape[1],)), bins or (mask.shape[1],))):
                assert np.asarray(mask, bool)[np.arange(len(mine)), s + mine[:, h]].all(), (label, "an invalid action was sampled", h)
        assert clear.mean() > 0.9, (label, "the inputs hold too many near-ties")
        same = (mine == a64.numpy()).all(1)
        err = np.abs(got_logp - lp64.detach().numpy())[same]
        assert (err <= np.maximum(lp_allow[same], 1.5 * e32.max())).all(), (label, float(err.max()))
    else:
        amp = 1.0 + np.abs(np.asarray(noise, np.float64)).reshape(got_act.shape)
        allow = amp * float(dy.max()) + 4 * U32 * np.abs(a64.detach().numpy())
        e_a32 = np.abs(a32.double().numpy() - a64.detach().numpy()).max()
        assert (np.abs(got_act.astype(np.float64) - a64.detach().numpy()) <= np.maximum(allow, 1.5 * e_a32)).all(), label
        err = np.abs(got_logp - lp64.detach().numpy())
        assert (err <= np.maximum(lp_allow, 1.5 * e32.max())).all(), (label, float(err.max()), float(lp_allow.min()))


@pytest.mark.parametrize("n", [5, 80])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("kind", ["discrete", "multidiscrete", "gaussian", "diag"])
def test_rollout_paths(L, kind, act, n):
    """get_action (a graph replay for a small host batch), act_padded (eager, device) and -- the discrete head -- step(): the same
    results bit for bit, right against the restatement, through the layer chain and never the one-launch kernel."""
    from rlgym_ppo_amd import _native as N
    pol = build_policy(kind, act)
    want_mod = {"tanh": torch.nn.Tanh, "elu": torch.nn.ELU}[act]
    assert pol.hidden_activation == act and pol.arena.hidden_act == N.HIDDEN_ACTIVATIONS[act]
    assert [type(m) for m in list(pol.model)[1:4:2]] == [want_mod, want_mod]
    rs = np.random.RandomState(100 * n + len(kind))
    obs = np.clip(rs.randn(n, OBS), -5, 5).astype(np.float32)
    shape = tuple(pol._noise_shape(n))
    noise = torch.as_tensor((rs.exponential(1.0, shape) if kind in ("discrete", "multidiscrete") else rs.randn(*shape)).astype(np.float32))
    c0 = counters(L, 0, 1)
    act_g, logp_g = pol.get_action(obs, noise=noise)                      # the captured graph (bucket of n)
    assert len(pol._graphs) == 1
    g = next(iter(pol._graphs.values()))
    assert g.late is False                                               # the noise is staged before the launch
    rows = pol.arena.stage_obs(obs)
    act_e, logp_e = pol.act_padded(rows, noise)                          # eager
    assert torch.equal(act_g, act_e.cpu()) and torch.equal(logp_g, logp_e.cpu())
    if kind == "discrete":
        act_s, logp_s = pol.step(obs, noise)
        assert torch.equal(act_s, act_g) and torch.equal(logp_s, logp_g)
        c1 = counters(L, 0, 1)
        assert c1[0] == c0[0] and c1[1] > c0[1]                          # the layer chain, never the one-launch kernel
        o = N.ActOpts()
        assert L.rlppo_discrete_step_one_launch(pol.arena.dims_c, pol.arena.n_layers, n, ctypes.byref(pol.arena.act_opts(o))) == 0
        probs = pol.get_output(obs).cpu().double()
        want = torch.softmax(torch.as_tensor(A.forward64(params_cpu(pol), obs, act)), -1)
        A.assert_forward_close(probs, want, f"get_output {act} n={n}")
    if kind in ("gaussian", "diag"):
        y = pol.arena.forward(rows, out_tanh=kind == "gaussian")[:, :pol.arena.d_out].cpu()
        A.assert_forward_close(y, A.forward64(params_cpu(pol), obs, act, kind == "gaussian"), f"{kind} {act} n={n}")
    check_rollout(kind, pol, act, obs, noise.numpy(), act_g.numpy(), logp_g.numpy(), f"{kind} {act} n={n}")


def random_mask(rs, n, bins):
    """bool [n, sum(bins)]: every entry valid with probability 0.6, one forced valid per head, every 4th row all valid."""
    m = rs.rand(n, sum(bins)) < 0.6
    for s, b in zip(A.starts(bins), bins):
        m[np.arange(n), s + rs.randint(0, b, n)] = True
    m[3::4] = True
    return m


@pytest.mark.parametrize("act", ACTS)
def test_rollout_masked_calls_and_reference_bins(L, act):
    """The rollout entry points test_rollout_paths does not reach, with tanh / ELU hidden layers: the fixed-bin multi-discrete step
    (rlppo_multidiscrete_act: the reference's eight heads), the masked multi-discrete step (rlppo_multidiscrete_act_nvec_masked) and
    the masked discrete step (rlppo_discrete_step / _act with rlppo_act_opts.action_mask) -- graph replay, eager call and (discrete)
    step() bit for bit alike, right against the restatement, no invalid action sampled, an all-valid mask = the unmasked call."""
    n = 37
    rs = np.random.RandomState(11)
    obs = np.clip(rs.randn(n, OBS), -5, 5).astype(np.float32)
    # the reference's bins: the fixed kernels
    ref = build_policy("multidiscrete", act, bins=None)
    assert ref.md_nvec is None and tuple(ref.splits) == REFERENCE_BINS
    noise = torch.as_tensor(rs.exponential(1.0, tuple(ref._noise_shape(n))).astype(np.float32))
    c6 = counters(L, 6)[0]
    a_g, l_g = ref.get_action(obs, noise=noise)
    a_e, l_e = ref.act_padded(ref.arena.stage_obs(obs), noise)
    assert counters(L, 6)[0] == c6   # never the general kernel
    assert torch.equal(a_g, a_e.cpu()) and torch.equal(l_g, l_e.cpu())
    check_rollout("multidiscrete", ref, act, obs, noise.numpy(), a_g.numpy(), l_g.numpy(), f"reference bins {act}", bins=REFERENCE_BINS)
    # the masked multi-discrete step (graph: host mask; eager: the same mask)
    md = build_policy("multidiscrete", act)
    mask = random_mask(rs, n, MD_BINS)
    noise = torch.as_tensor(rs.exponential(1.0, tuple(md._noise_shape(n))).astype(np.float32))
    a_g, l_g = md.get_action(obs, noise=noise, action_mask=mask)
    assert (_bucket_of(n), True) in md._graphs
    a_e, l_e = md.act_padded(md.arena.stage_obs(obs), noise, mask)
    assert torch.equal(a_g, a_e.cpu()) and torch.equal(l_g, l_e.cpu())
    check_rollout("multidiscrete", md, act, obs, noise.numpy(), a_g.numpy(), l_g.numpy(), f"masked nvec {act}", bins=MD_BINS, mask=mask)
    # the masked discrete step
    dis = build_policy("discrete", act)
    mask = random_mask(rs, n, (6,))
    noise = torch.as_tensor(rs.exponential(1.0, (n, 6)).astype(np.float32))
    a_g, l_g = dis.get_action(obs, noise=noise, action_mask=mask)
    a_s, l_s = dis.step(obs, noise, action_mask=mask)
    a_e, l_e = dis.act_padded(dis.arena.stage_obs(obs), noise, mask)
    assert torch.equal(a_g, a_s) and torch.equal(l_g, l_s) and torch.equal(a_g, a_e.cpu()) and torch.equal(l_g, l_e.cpu())
    check_rollout("discrete", dis, act, obs, noise.numpy(), a_g.numpy(), l_g.numpy(), f"masked discrete {act}", mask=mask)
    a_u, l_u = dis.step(obs, noise)
    a_v, l_v = dis.step(obs, noise, action_mask=np.ones((n, 6), bool))
    assert torch.equal(a_u, a_v) and torch.equal(l_u, l_v)
    probs = dis.get_output(obs, action_mask=mask).cpu().numpy()
    assert (probs[~mask] == 0).all() and np.abs(probs.sum(1) - 1).max() < 1e-5


def _bucket_of(n):
    from rlgym_ppo_amd.ppo._mlp import _bucket
    return _bucket(n)


def test_relu_policy_still_takes_the_one_launch_kernel(L):
    """In the same process as tanh / ELU policies: a ReLU policy built from a plain tuple and one built from LayerSizes(..., "relu")
    pass no options of their own (None where they passed None), take the one-launch kernel and agree bit for bit.  (64, 64): a
    shape the one-launch kernel covers -- the tanh policy of the SAME shape is refused it and takes the layer chain.)"""
    from rlgym_ppo_amd.ppo import LayerSizes
    tanh = build_policy("discrete", "tanh", hidden=(64, 64))
    plain, wrapped = build_policy("discrete", "plain", hidden=(64, 64)), build_policy("discrete", "relu", hidden=(64, 64))
    assert type(wrapped.model[1]) is torch.nn.ReLU and plain.arena.hidden_act == wrapped.arena.hidden_act == 0
    assert plain.arena.act_opts() is None and tanh.arena.act_opts().hidden_act == 1
    assert L.rlppo_discrete_step_one_launch(plain.arena.dims_c, plain.arena.n_layers, 80, None) == 1
    assert L.rlppo_discrete_step_one_launch(tanh.arena.dims_c, tanh.arena.n_layers, 80, ctypes.byref(tanh.arena.act_opts())) == 0
    rs = np.random.RandomState(5)
    obs = np.clip(rs.randn(80, OBS), -5, 5).astype(np.float32)
    noise = torch.as_tensor(rs.exponential(1.0, (80, 6)).astype(np.float32))
    c0 = counters(L, 0, 1)
    tanh.step(obs, noise)
    assert counters(L, 0, 1) == [c0[0], c0[1] + 1]
    tanh.get_action(obs[:5], noise=noise[:5])                            # its graph: the chain form, noise before the launch
    assert next(iter(tanh._graphs.values())).late is False
    c0 = counters(L, 0, 1)
    a0, l0 = plain.step(obs, noise)
    a1, l1 = wrapped.step(obs, noise)
    assert counters(L, 0, 1) == [c0[0] + 2, c0[1]]
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
    assert isinstance(LayerSizes((32, 32), "relu"), tuple)


# ------------------------------------------------------------------------------------------------ 4. PPOLearner.learn
LEARN_SEED = 19
K, N_ROWS, B, MB, EPOCHS, LR = 3, 1024, 512, 128, 2, 3e-4


def build_learner(head, act, seed=LEARN_SEED, wrap=True, **kw):
    from rlgym_ppo_amd.ppo import LayerSizes, PPOLearner
    torch.manual_seed(seed)
    np.random.seed(seed)
    sizes = LayerSizes((32, 32), act) if wrap else (32, 32)
    ptype, space = (3, K) if head == "diag" else (0, 6)
    learner = PPOLearner(OBS, space, ptype, sizes, sizes, (0.1, 1.0), B, EPOCHS, LR, LR, CLIP, ENT, MB, "cuda:0", **kw)
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(N_ROWS, OBS), -5, 5).astype(np.float32)
    if head == "diag":
        noise = torch.as_tensor(rs.randn(N_ROWS, K).astype(np.float32))
    else:
        noise = torch.as_tensor(rs.exponential(1.0, (N_ROWS, 6)).astype(np.float32))
    act_, logp = learner.policy.get_action(obs, noise=noise)
    exp = dict(states=obs, actions=act_.numpy().astype(np.float32), log_probs=logp.numpy() + 0.1 * rs.randn(N_ROWS).astype(np.float32),
               values=rs.randn(N_ROWS).astype(np.float32), advantages=rs.randn(N_ROWS).astype(np.float32))
    return learner, exp


def buffer_of(exp, seed=LEARN_SEED):
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    buf = ExperienceBuffer(N_ROWS, seed, "cpu")
    z = np.zeros(N_ROWS, np.float32)
    buf.submit_experience(exp["states"], exp["actions"], exp["log_probs"], z, exp["states"], z, z, exp["values"], exp["advantages"])
    return buf


def learner_params(learner):
    ls = learner.policy.log_std.detach().cpu().clone() if learner.policy_type == 3 else None
    return params_cpu(learner.policy), ls, params_cpu(learner.value_net)


_YARD = {}


def learn_yardstick(head, act, pol, ls, val, exp):
    """The float64 and float32 yardsticks of one (head, activation) learn(): computed once, shared, left unchanged."""
    key = (head, act)
    if key not in _YARD:
        weakest = {}
        run = lambda dt, **kw: A.learn(dt, head, act, pol, val, exp, B, MB, EPOCHS, CLIP, ENT, LR, LR, np.random.RandomState(LEARN_SEED), log_std=ls, **kw)
        t = run(torch.float64, weakest=weakest)
        _YARD[key] = (t[0], t[1], *run(torch.float32), weakest)
    return _YARD[key]


def learn_errs(p_, v_, yard_):
    """tests/test_gpu_diag_gaussian.py::learn_errs: (err over the well-conditioned parameters, worst ill-conditioned one as a fraction
    of its derived bound steps x lr x min(1, 1e-5 / w_i))."""
    t_pol, t_val, _, _, weakest = yard_
    steps = EPOCHS * (N_ROWS // B)
    good = frac = 0.0
    for x, tr, weak in ((p_, t_pol, weakest["pol"]), (v_, t_val, weakest["val"])):
        dlt, bad = np.abs(np.asarray(x, np.float64) - tr), weak < 1e-4
        good = max(good, float(dlt[~bad].max() / np.abs(tr).max()))
        if bad.any():
            bound = steps * LR * np.minimum(1.0, 1e-5 / np.maximum(weak[bad], 1e-300))
            frac = max(frac, float((dlt[bad] / bound).max()))
    return good, frac


def flats(learner):
    return learner.policy.arena.flat.cpu().numpy().astype(np.float64), learner.value_net.arena.flat.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("head,act", [("diag", "tanh"), ("diag", "elu"), ("discrete", "tanh")])
def test_learn_against_the_float64_yardstick(L, head, act):
    """obs 13, (32, 32) networks, 1024 rows, B 512, MB 128, 2 epochs, lr 3e-4.  Well-conditioned parameters (|g_i| >= 1e-4 max|g| in
    every step) fall under the tolerance rule, the ill-conditioned ones under steps x lr x min(1, 1e-5 / w_i); at most 5 % may be
    ill-conditioned -- asserted from float64 before the GPU result is looked at.  (On the CPU, from the float64 yardstick alone at these
    sizes: 1.2 - 2.4 % for tanh and ELU; the float32 yardstick misses float64 by 1.2 - 1.7e-7 on the parameters: the 1e-5 floor governs.)"""
    learner, exp = build_learner(head, act)
    pol, ls, val = learner_params(learner)
    yard_ = learn_yardstick(head, act, pol, ls, val, exp)
    t_pol, t_val, f_pol, f_val, weakest = yard_
    n_ill = int((weakest["pol"] < 1e-4).sum() + (weakest["val"] < 1e-4).sum())
    assert n_ill <= 0.05 * (t_pol.size + t_val.size), n_ill
    c0 = counters(L, 2, 3, 4)
    report = learner.learn(buffer_of(exp))
    steps = EPOCHS * (N_ROWS // B)
    c1 = counters(L, 2, 3, 4)
    assert report["Cumulative Model Updates"] == steps and c1[0] > c0[0] and c1[1:] == c0[1:]
    assert all(np.isfinite(float(v)) for v in report.values())
    got = flats(learner)
    assert got[0].size == t_pol.size and got[1].size == t_val.size
    e_hip, e_32 = learn_errs(*got, yard_), learn_errs(f_pol, f_val, yard_)
    print(f"[act fp64 gate] learn() {head} {act}: err(HIP, fp64)={e_hip[0]:.2e}  err(float32 yardstick, fp64)={e_32[0]:.2e}; {n_ill} ill-conditioned "
          f"parameters of {t_pol.size + t_val.size}: HIP at {e_hip[1]:.3f} of the derived bound, float32 yardstick {e_32[1]:.3f}")
    assert e_hip[0] <= max(1e-5, 1.5 * e_32[0]) and e_hip[1] <= 1.0, (e_hip, e_32)
    # the same learn() from the same state: bit-identical
    twin, exp2 = build_learner(head, act)
    assert all(np.array_equal(exp[k], exp2[k]) for k in exp)
    twin.learn(buffer_of(exp2))
    assert torch.equal(twin.policy.arena.flat, learner.policy.arena.flat) and torch.equal(twin.value_net.arena.flat, learner.value_net.arena.flat)


def test_learn_refuses_bf16_and_x3_and_relu_is_unchanged(L):
    learner, exp = build_learner("diag", "tanh")
    flat0 = learner.policy.arena.flat.clone()
    for prec in ("bf16", "x3"):
        learner.update_precision = prec
        with pytest.raises(ValueError, match=f"hidden activation 'tanh'.*'{prec}'"):
            learner.learn(buffer_of(exp))
    assert torch.equal(learner.policy.arena.flat, flat0)
    # ReLU through LayerSizes(..., "relu") is the learner a plain tuple builds: the same entry point, the same parameters bit for bit
    a, exp_a = build_learner("discrete", "relu")
    b, exp_b = build_learner("discrete", "relu", wrap=False)
    assert all(np.array_equal(exp_a[k], exp_b[k]) for k in exp_a) and a.policy.arena.hidden_act == b.policy.arena.hidden_act == 0
    a.learn(buffer_of(exp_a))
    b.learn(buffer_of(exp_b))
    assert torch.equal(a.policy.arena.flat, b.policy.arena.flat) and torch.equal(a.value_net.arena.flat, b.value_net.arena.flat)


def test_two_virtual_ranks_sum_the_same_gradient():
    """Two data-parallel ranks with tanh networks (dp.run_virtual_ranks): the replicas end bit-identical to each other and, like one
    rank on the union, within the rule of the float64 yardstick of the same learn()."""
    from rlgym_ppo_amd import dp
    one, exp = build_learner("diag", "tanh")
    pol, ls, val = learner_params(one)
    one.learn(buffer_of(exp))
    reps = [build_learner("diag", "tanh")[0] for _ in range(2)]
    dp.run_virtual_ranks(reps, [buffer_of(exp) for _ in range(2)])
    assert torch.equal(reps[0].policy.arena.flat, reps[1].policy.arena.flat) and torch.equal(reps[0].value_net.arena.flat, reps[1].value_net.arena.flat)
    yard_ = learn_yardstick("diag", "tanh", pol, ls, val, exp)
    e_32, _ = learn_errs(yard_[2], yard_[3], yard_)
    for who, l_ in (("one rank", one), ("two ranks", reps[0])):
        good, frac = learn_errs(*flats(l_), yard_)
        print(f"[act fp64 gate] learn(), {who}: err(HIP, fp64)={good:.2e}  err(float32 yardstick, fp64)={e_32:.2e}; ill-conditioned at {frac:.3f} of the bound")
        assert good <= max(1e-5, 1.5 * e_32) and frac <= 1.0, (who, good, e_32, frac)


# ------------------------------------------------------------------------------------------------ 5. Learner end to end
LOOP = dict(n_proc=1, min_inference_size=2, exp_buffer_size=1024, ts_per_iteration=384, ppo_epochs=1, ppo_batch_size=384, ppo_minibatch_size=192,
            policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32), add_unix_timestamp=False, continuous_head="diag")
MODULE = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "elu": torch.nn.ELU}


def learner_state(l_):
    p_ = l_.ppo_learner
    return dict(pol=p_.policy.arena.flat.clone(), val=p_.value_net.arena.flat.clone(), m=p_.policy_optimizer.exp_avg.clone(),
                v=p_.policy_optimizer.exp_avg_sq.clone(), vm=p_.value_optimizer.exp_avg.clone(), vv=p_.value_optimizer.exp_avg_sq.clone(),
                steps=(p_.policy_optimizer.step_count, p_.value_optimizer.step_count, p_.cumulative_model_updates),
                book=l_.agent.cumulative_timesteps, acts=l_.experience_buffer.actions.clone(), logp=l_.experience_buffer.log_probs.clone())


def same_state(got, want, keys, what):
    for key in keys:
        same = torch.equal(got[key], want[key]) if isinstance(want[key], torch.Tensor) else got[key] == want[key]
        assert same, (what, key)


def assert_networks(learner, act):
    for net in (learner.ppo_learner.policy, learner.ppo_learner.value_net):
        assert [type(m) for m in list(net.model)[1:4:2]] == [MODULE[act]] * 2 and net.arena.hidden_act == {"relu": 0, "tanh": 1, "elu": 2}[act]
    assert learner.hidden_activation == act and learner.hidden_activations == {"policy": act, "critic": act}
    assert learner.config["hidden_activation"] == act and learner.config["policy_layer_sizes"] == (32, 32)


def run_reports(learner):
    """learner._learn() with every learn() report kept."""
    reports = []
    plain = learner.ppo_learner.learn
    learner.ppo_learner.learn = lambda exp: reports.append(plain(exp)) or reports[-1]
    learner._learn()
    assert reports and all(np.isfinite(float(v)) for r in reports for v in r.values())
    return reports


def test_learner_loop_vector_mode_elu(tmp_path):
    """One iteration through the vector manager's step() path with ELU networks: a finite report, the chosen modules."""
    from rlgym_ppo_amd import Learner
    learner = Learner(E.make_echo_vector_env, timestep_limit=300, save_every_ts=10_000_000, checkpoint_load_folder=None, random_seed=3,
                      vector_env=True, hidden_activation="elu", checkpoints_save_folder=str(tmp_path / "ckpt"), **LOOP)
    try:
        run_reports(learner)
        assert learner.epoch >= 1
        assert_networks(learner, "elu")
    finally:
        learner.agent.cleanup()


def test_learner_loop_process_mode_tanh_and_its_checkpoint(tmp_path):
    """Process mode with tanh networks: one iteration (finite report, the chosen modules), which checkpoints; a SECOND Learner -- another
    seed, so other initial weights -- loads "latest": policy, critic, both Adam moments, the step counts and the book-keeping come
    back bit for bit INTO Tanh networks, and a further iteration from there stays finite.
    This is narrower than "continue equals the uninterrupted run", which the vector-mode test below shows for tanh and ELU alike:
    in process mode the environments live in worker processes, and neither their state nor the workers' generators are checkpoint
    state or reachable from here, so the second iteration of a resumed run cannot be given the inputs the uninterrupted run had
    (every continuation test of this repository is vector-mode for that reason).  What a checkpoint DOES hold is compared exactly."""
    from rlgym_ppo_amd import Learner
    kw = dict(LOOP, vector_env=False, save_every_ts=300, standardize_obs=False, standardize_returns=False, hidden_activation="tanh",
              checkpoints_save_folder=str(tmp_path / "ck"))
    first = Learner(E.make_echo_env, timestep_limit=300, checkpoint_load_folder=None, random_seed=3, **kw)
    try:
        run_reports(first)
        assert_networks(first, "tanh")
        saved = learner_state(first)
    finally:
        first.agent.cleanup()
    assert saved["steps"][0] >= 1 and saved["book"] >= 384
    second = Learner(E.make_echo_env, timestep_limit=saved["book"] + 300, checkpoint_load_folder="latest", random_seed=9, **kw)
    try:
        assert_networks(second, "tanh")
        same_state(learner_state(second), saved, ("pol", "val", "m", "v", "vm", "vv", "steps", "book"), "restored")
        assert second.ppo_learner.policy.arena.is_bound()
        run_reports(second)
        after = learner_state(second)
        assert after["book"] > saved["book"] and after["steps"][0] > saved["steps"][0] and not torch.equal(after["pol"], saved["pol"])
        assert torch.isfinite(after["pol"]).all() and torch.isfinite(after["val"]).all()
    finally:
        second.agent.cleanup()


def run_counter_env(learner):
    try:
        learner._learn()
        return learner_state(learner), int(learner.agent.env.t), torch.get_rng_state(), np.random.get_state(), learner.experience_buffer.rng.get_state()
    finally:
        learner.agent.cleanup()


@pytest.mark.parametrize("act", ["elu", "tanh"])
def test_learner_save_load_continue_equals_the_uninterrupted_run(tmp_path, act):
    """tests/test_gpu_diag_gaussian.py's test of the same name with ELU / tanh networks (vector mode: the environment is in this
    process, so its state and the host generators can be carried over): one Learner that runs two iterations against a Learner that
    checkpoints after one and a second one that loads "latest" and continues -- bit for bit.  The activation is a hyper-parameter,
    not checkpoint state: the second Learner is given it again."""
    from rlgym_ppo_amd import Learner
    kw = dict(LOOP, vector_env=True, exp_buffer_size=384, save_every_ts=300, standardize_obs=False, standardize_returns=False, hidden_activation=act)
    whole, t_end, _, _, _ = run_counter_env(Learner(functools.partial(E.CounterVectorEnv, 0), timestep_limit=700, checkpoint_load_folder=None,
                                                    random_seed=3, checkpoints_save_folder=str(tmp_path / "whole"), **kw))
    first, t_mid, rng_torch, rng_numpy, rng_buffer = run_counter_env(Learner(functools.partial(E.CounterVectorEnv, 0), timestep_limit=300,
                                                                             checkpoint_load_folder=None, random_seed=3,
                                                                             checkpoints_save_folder=str(tmp_path / "ck"), **kw))
    assert first["book"] == 384 and whole["book"] == 768 and first["steps"] == (1, 1, 1) and not torch.equal(first["pol"], whole["pol"])
    second = Learner(functools.partial(E.CounterVectorEnv, t_mid), timestep_limit=700, checkpoint_load_folder="latest", random_seed=9,
                     checkpoints_save_folder=str(tmp_path / "ck"), **kw)
    try:
        assert_networks(second, act)
        same_state(learner_state(second), first, ("pol", "val", "m", "v", "vm", "vv", "steps", "book"), "restored")
        torch.set_rng_state(rng_torch)
        np.random.set_state(rng_numpy)
        second.experience_buffer.rng.set_state(rng_buffer)
    except BaseException:
        second.agent.cleanup()
        raise
    resumed, t_res, _, _, _ = run_counter_env(second)
    assert t_res == t_end
    same_state(resumed, whole, tuple(whole), "continued")


def test_relu_through_the_learner_keyword_is_the_learner_without_it(L, tmp_path):
    """Learner(hidden_activation="relu") against Learner() without the keyword (what every caller of the parent commit wrote): the
    same ReLU modules, a ReLU arena that passes no options of its own, the same pass forms (the pass counters move alike: the plain
    rlppo_ppo_minibatch_diag entry point, never the extended one's plain form) and, after one iteration from the same seed on the
    same environment, the same parameters, Adam moments and buffer bit for bit.  Both runs take this tree's code; that this tree's
    ReLU path computes what the parent computed is held by the existing suite, unchanged, against the recorded fixtures."""
    from rlgym_ppo_amd import Learner
    kw = dict(LOOP, vector_env=True, exp_buffer_size=384, save_every_ts=10_000_000, standardize_obs=False, standardize_returns=False,
              timestep_limit=300, checkpoint_load_folder=None, random_seed=3)
    states, moved = [], []
    for name, extra in (("keyword", {"hidden_activation": "relu"}), ("omitted", {})):
        learner = Learner(functools.partial(E.CounterVectorEnv, 0), checkpoints_save_folder=str(tmp_path / name), **kw, **extra)
        assert_networks(learner, "relu")
        assert learner.ppo_learner.policy.arena.act_opts() is None and type(learner.ppo_learner.policy.model[1]) is torch.nn.ReLU
        c0 = counters(L, 2, 3, 4, 5)
        states.append(run_counter_env(learner)[0])
        moved.append([b - a for a, b in zip(c0, counters(L, 2, 3, 4, 5))])
    assert moved[0] == moved[1] and moved[0][0] >= 1
    same_state(states[0], states[1], tuple(states[1]), "keyword against omitted")
