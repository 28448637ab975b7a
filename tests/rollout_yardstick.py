"""The yardstick of the rollout steps (csrc/fused_act.hip, the sampling kernels of csrc/heads.hip behind act_chain of csrc/api.hip):
float64 truth of every head from GIVEN logits, a PER-ELEMENT allowance without a floor, a choice rule that leaves no row out, a
propagated bound for the network in front of the head, input makers with fixed seeds, and float32 restatements with deliberately
wrong variants (MUTANTS).  Plain numpy / torch on the CPU: tests/test_rollout_yardstick_host.py shows the rules are reachable and
separate right from wrong, tests/test_gpu_rollout_truth.py holds every rollout entry point to them.

Two tiers
---------
(i)  The sampling kernels consume exactly the buffer rlppo_mlp_forward returns, so the head is held on the kernel's OWN logits: these
     are float32 numbers, the truth is the float64 head of those numbers, and the allowance counts the head's roundings alone.
(ii) From the observations: the float64 network gives z64, the kernel's logits miss it by at most e_z (logit_bound), and a log-
     probability moves by at most  e_a + sum_j p_j e_j  under a logit perturbation bounded by e (d log p_a / dz_j = [a = j] - p_j
     and sum_j |[a = j] - p_j| e_j <= e_a + sum_j p_j e_j; the mean-value point's p differs from p64 by a factor exp(2 max e) that
     multiplies the second term -- it is applied).  This is added ON TOP of the head allowance of tier (i).

The discrete head (softmax -> clamp(1e-11, 1) -> log, include/rlppo.h)
----------------------------------------------------------------------
u = 2^-24.  V = the row's valid columns, A_v = |V|, d_c = z_c - max_V z.  The kernel's roundings, in its order:
  1  d_c = fl(z_c - max): the maximum is exact, the difference rounds once                                   |d_c| u   (in the exponent)
  2  e_c = expf(d_c): a transcendental, the project's convention of a few ulp (as + 4 u |f| for tanh)        4 u       relative
  3  s = the sum of the A_v positive e_c in ANY order and grouping: A_v - 1 additions, each rounding a partial sum <= s;
     on top, every term carries (|d_c| + 4) u, which weighs in with p_c:                                     (A_v - 1 + 4 + E_p|d|) u
  4  p_c = fl(e_c / s)                                                                                        1 u
  5  pc_c = min(max(p_c, 1e-11f), 1): exact, and 1-Lipschitz
  6  log pc: logf, a transcendental                                                                           4 u |log pc|
so with R_c = A_v + 8 + |d_c| + E_p|d|  (E_p|d| = sum_V p_c |d_c|) a probability is allowed the RELATIVE error g_c = R_c u / (1 - R_c u)
(Higham's gamma: the product of R factors 1 +- u, quotients included, taken without dropping the second order) plus SUB = 2^-126 for
float32 subnormals (an e_c or p_c below the smallest normal may lose all its bits or be flushed).  Columns outside V hold exactly 0.
The clamp's floor is the float32 number 1e-11f (FLOOR; torch.clamp on a float32 tensor compares with the same number); a clamped
probability is allowed g_c p_c (the clamp is 1-Lipschitz), and an element whose truth is below FLOOR by MORE than its allowance must
equal FLOOR bit for bit.  log pc is allowed g_c + 4 u |log pc| (log is 1 / pc-Lipschitz: a relative error g is an absolute one of
-log(1 - g) ~ g), and 4 u |log FLOOR| alone where the clamp is firm.  Nothing is raised to a floor: a probability of 1e-6 is held
to ~1e-6 x 1e-5.

The choice rule
---------------
The kernel takes the first arg-max over V of fl(pc_c / q_c).  Its score misses the float64 score by at most m = g + 2 u relative (g the
row's largest g_c, one rounding for the quotient, one spare for the second order), so whatever it chose satisfies
score64[a] >= max score64 x (1 - m)^2 -- asserted on EVERY row -- and where the float64 runner-up is below that the choice must be
the float64 arg-max.  The chosen index must be valid.  Among columns whose float64 scores are EXACTLY equal (identical inputs:
duplicated logits with equal noise, firmly clamped columns with equal noise -- the kernel's scores are then bit-equal too) the first
must be chosen.  A row whose float64 top two are within the margin without being equal is `undecided`: the makers keep those at or
under 1 % of a case's rows (asserted from float64 alone before any GPU call).  log p is checked on every row at the index the kernel
chose.

Multi-discrete (fixed bins and any nvec, masked or not)
-------------------------------------------------------
Per head with b valid bins: mx exact; s = sum of b terms expf(d_c): (b - 1 + 4 + E_p|d|) u relative; logf(s): that plus 4 u |log s|;
lse = fl(mx + log s): u |lse|; the head's term fl(z_a - lse): u |z_a - lse|.  The row's log p adds H terms: in float, serially
(the fixed kernel; (H - 1) u sum_h |term|) or in double, rounded once (the general kernel; u |log p|, the serial bound covers it).
Scores are (expf(d_c) / s) / q: R = b + 9 + |d_c| + E_p|d| units, the choice rule as above per head.

The reference's Gaussian head (4-term formula on the tanh outputs y, std = y var_m + var_b, the action clamped to +-1)
---------------------------------------------------------------------------------------------------------------------------
sd: two roundings or one fused, r_sd = (|y var_m| / sd + 1) u relative.  action = clamp(fl(eps sd + mean)): (r_sd + 1 u) |eps sd| + u |a|, the
clamp 1-Lipschitz and |a| <= 1 exact.  log p is taken at the kernel's OWN stored action (what the update will recompute): with
q = 2 r_sd + 3 u the three quotients t1, t2, t3 carry q |t_i| each, t4 = logf(1 / sqrtf(2 pi ssq)) carries r_sd + 3.5 u + 4 u |t4|, the three
additions 3 u sum|t_i|; over the k dimensions (k - 1) u sum_j |term_j| (float up to 32; double rounded once above: covered).
Diagonal Gaussian: diag_gaussian_yardstick.logp_terms in float64 at the stored action; sigma = expf(log_std) 4 u, the quotient 13 u,
two subtractions, then the same sum over k.

The network (tier ii)
---------------------
e_out = |W| e_in + gemm_yardstick.nt_allow(S, K) with S = sum |w| (|h64| + e_in) + |b| (the kernel multiplies ITS inputs); ReLU and
ELU (alpha = 1) are 1-Lipschitz, tanh too; tanhf / expm1f add 4 u |f|.  e_0 = 0: the padded rows are the observations, exactly.
"""
import numpy as np
import torch

from gemm_yardstick import U32, nt_allow

U = U32
FLOOR = float(np.float32(1e-11))
SUB = 2.0 ** -126
T_ULP = 4.0                                   # units of u per transcendental (expf, logf, tanhf, expm1f)
UNDECIDED_CAP = 0.01
F32 = np.float32


def gamma(R):
    return R * U / (1.0 - R * U)


# ------------------------------------------------------------------------------------------------------------ discrete: truth
def discrete_truth(z, q=None, mask=None):
    """Float64 head of the logits z [n, A] (any float dtype: the VALUES are the operands).  mask: bool [n, A] (a row without a valid
    action counts as all-valid).  -> dict: valid, d, p, pc, logpc, g (relative allowance per element), firm (truth below FLOOR by more
    than the allowance), score (pc / q, -inf outside V; with q), m (the row's score margin)."""
    z = np.asarray(z, np.float64)
    n, A = z.shape
    valid = np.ones((n, A), bool) if mask is None else np.asarray(mask, bool).copy()
    valid[~valid.any(1)] = True
    zz = np.where(valid, z, -np.inf)
    d = zz - zz.max(1, keepdims=True)
    e = np.exp(d)
    p = e / e.sum(1, keepdims=True)
    absd = np.where(valid, -d, 0.0)
    R = valid.sum(1, keepdims=True) + 8.0 + absd + (p * absd).sum(1, keepdims=True)
    g = np.where(valid, gamma(R), 0.0)
    firm = valid & (p * (1 + g) + SUB < FLOOR)
    pc = np.where(valid, np.clip(p, FLOOR, 1.0), 0.0)
    with np.errstate(divide="ignore"):
        logpc = np.where(valid, np.log(np.where(valid, pc, 1.0)), 0.0)
    out = dict(valid=valid, d=d, p=p, pc=pc, logpc=logpc, g=g, firm=firm, n=n, A=A)
    out["allow_logp"] = np.where(firm, 0.0, -np.log1p(-g)) + T_ULP * U * np.abs(logpc)
    out["allow_logp_soft"] = -np.log1p(-g) + T_ULP * U * np.abs(logpc)   # (tier ii: the clamp as a 1-Lipschitz map, no firm region)
    return out if q is None else with_noise(out, q)


def with_noise(T, q):
    """The truth with the scores pc / q (-inf outside V) and the row's score margin m added."""
    T = dict(T)
    T["score"] = np.where(T["valid"], T["pc"] / np.asarray(q, np.float64), -np.inf)
    T["m"] = T["g"].max(1) + 2 * U
    return T


def _ratio(err, allow):
    """err / allow elementwise; allow == 0 asks for exactness (0 or inf); NaN in err is inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(err), np.inf, r)


def probs_worst(got, T, clamped):
    """Worst ratio over EVERY element of a probability matrix against the truth: invalid columns exactly 0, firmly clamped ones
    exactly FLOOR (clamped), everything else within g p (+ SUB where nothing is clamped)."""
    got = np.asarray(got, np.float64)
    want = T["pc"] if clamped else T["p"]
    allow = T["g"] * T["p"] + (0.0 if clamped else SUB)
    allow = np.where(T["valid"], allow, 0.0)
    if clamped:
        want = np.where(T["firm"], FLOOR, want)
        allow = np.where(T["firm"], 0.0, allow)
    return float(_ratio(np.abs(got - want), allow).max())


def choice_check(act, score, m, valid):
    """The choice rule on every row of score [n, C] (float64, -inf outside `valid`) with relative margins m [n].  -> dict(bad: the
    rows that break it, undecided: the rows whose top two are within the margin without being equal)."""
    act = np.asarray(act).astype(np.int64).reshape(-1)
    n, C = score.shape
    rows = np.arange(n)
    in_range = (act >= 0) & (act < C)
    a = np.where(in_range, act, 0)
    ok_valid = in_range & valid[rows, a]
    top = score.max(1)
    first = score.argmax(1)                                                  # first index of the float64 maximum
    keep = (1.0 - m) ** 2
    chosen = score[rows, a]
    ok_margin = chosen >= top * keep
    runner = np.where(np.arange(C)[None, :] == first[:, None], -np.inf, score).max(1)
    decided = runner < top * keep
    ok_decided = ~decided | (a == first)
    tied = score == chosen[:, None]                                          # exact float64 ties with the chosen column
    ok_tie = tied.argmax(1) == a
    bad = ~(ok_valid & ok_margin & ok_decided & ok_tie)
    undecided = ~decided & (runner != top)
    return dict(bad=np.flatnonzero(bad), undecided=int(undecided.sum()), invalid=int((~ok_valid).sum()))


def undecided_rows(T):
    return choice_check(T["score"].argmax(1), T["score"], T["m"], T["valid"])["undecided"]


def logp_worst(logp, act, T, extra=None):
    """Worst ratio over EVERY row of log p at the index the kernel chose (an index out of range counts as inf)."""
    act = np.asarray(act).astype(np.int64).reshape(-1)
    rows = np.arange(T["n"])
    ok = (act >= 0) & (act < T["A"])
    a = np.where(ok, act, 0)
    allow = T["allow_logp"][rows, a] if extra is None else T["allow_logp_soft"][rows, a] + extra
    r = _ratio(np.abs(np.asarray(logp, np.float64).reshape(-1) - T["logpc"][rows, a]), allow)
    return float(np.where(ok, r, np.inf).max())


def discrete_hold(name, act, logp, T, probs=None, extra=None):
    """Every check of a sampled discrete step; prints and returns the worst ratio (choice violations count as inf)."""
    c = choice_check(act, T["score"], T["m"], T["valid"])
    w = logp_worst(logp, act, T, extra)
    wp = probs_worst(probs, T, True) if probs is not None else 0.0
    worst = max(w, wp, np.inf if len(c["bad"]) else 0.0)
    print(f"[rollout truth] {name}: n={T['n']} A={T['A']} worst log p ratio {w:.3g}" + (f", probabilities {wp:.3g}" if probs is not None else "")
          + f"; rows breaking the choice rule {len(c['bad'])} (invalid {c['invalid']}), undecided {c['undecided']}")
    return worst


def tier2_extra(T64, e_z):
    """|delta log p_a| <= e_a + sum_j p_j e_j for every column [n, A]; the second term with p taken anywhere between the two logit
    vectors (a factor exp(2 max e) on p64)."""
    e = np.where(T64["valid"], e_z, 0.0)
    return e + (T64["p"] * e).sum(1, keepdims=True) * np.exp(2 * e.max(1, keepdims=True))


def extra_at(extra, act):
    act = np.asarray(act).astype(np.int64).reshape(-1)
    return extra[np.arange(len(act)), np.clip(act, 0, extra.shape[1] - 1)]


# ------------------------------------------------------------------------------------------------------ multi-discrete: truth
def starts(bins):
    return [int(s) for s in np.cumsum((0,) + tuple(bins))[:-1]]


def md_truth(z, bins, q, mask=None):
    """Float64 multi-discrete head of logits z [n, >= S]: per head log-softmax over its valid bins.  q: noise [n H, B].
    -> dict(ls [n, H, B] (-inf outside), valid3, score, m [n, H], allow [n, H, B]: the allowance of the head's TERM at bin c)."""
    z = np.asarray(z, np.float64)
    n, H, B = z.shape[0], len(bins), max(bins)
    q = np.asarray(q, np.float64).reshape(n, H, B)
    ls = np.full((n, H, B), -np.inf)
    valid3 = np.zeros((n, H, B), bool)
    allow = np.zeros((n, H, B))
    m = np.zeros((n, H))
    score = np.full((n, H, B), -np.inf)
    for h, (s, b) in enumerate(zip(starts(bins), bins)):
        v = np.ones((n, b), bool) if mask is None else np.asarray(mask, bool)[:, s:s + b].copy()
        v[~v.any(1)] = True
        zz = np.where(v, z[:, s:s + b], -np.inf)
        mx = zz.max(1, keepdims=True)
        d = zz - mx
        e = np.exp(d)
        ssum = e.sum(1, keepdims=True)
        p = e / ssum
        absd = np.where(v, -d, 0.0)
        Ep = (p * absd).sum(1, keepdims=True)
        nb = v.sum(1, keepdims=True)
        lse = mx + np.log(ssum)
        term = np.where(v, zz - lse, -np.inf)
        ls[:, h, :b], valid3[:, h, :b] = term, v
        one = nb == 1                                                        # one valid bin: expf(0) = 1, log 1 = 0, z - (mx + 0) = 0: exact
        a_h = gamma(nb - 1 + T_ULP + Ep) + T_ULP * U * np.abs(np.log(ssum)) + U * np.abs(lse) + U * np.abs(np.where(v, term, 0.0))
        allow[:, h, :b] = np.where(one, 0.0, np.where(v, a_h, 0.0))
        score[:, h, :b] = np.where(v, p / q[:, h, :b], -np.inf)
        m[:, h] = gamma(nb[:, 0] + 9 + absd.max(1) + Ep[:, 0]) + 2 * U
    return dict(ls=ls, valid3=valid3, score=score, m=m, allow=allow, n=n, H=H, B=B, bins=tuple(bins))


def md_logp_at(T, act, extra=None):
    """(log p [n], allowance [n]) of a row at the chosen bins act [n, H]: the heads' terms added up; the heads' allowances (+ extra
    [n, H, B], tier ii) + (H - 1) u sum |term| for the additions + u |log p| for the rounding of the sum."""
    n, H, B = T["n"], T["H"], T["B"]
    a = np.clip(np.asarray(act).astype(np.int64).reshape(n, H), 0, B - 1)[..., None]
    term = np.take_along_axis(T["ls"], a, -1)[..., 0]
    allow = np.take_along_axis(T["allow"] if extra is None else T["allow"] + extra, a, -1)[..., 0]
    term = np.where(np.isfinite(term), term, np.nan)                         # (an invalid bin: NaN, which every ratio reads as inf)
    return term.sum(1), allow.sum(1) + (H - 1) * U * np.abs(term).sum(1) + U * np.abs(term.sum(1))


def md_hold(name, act, logp, T, extra=None, choice=True):
    """Choice rule per head on every row (choice=False, tier ii: it was held on the kernel's own logits), log p on every row at
    the chosen bins (md_logp_at).  Prints and returns the worst ratio."""
    act = np.asarray(act).astype(np.int64).reshape(T["n"], T["H"])
    n, H, B = T["n"], T["H"], T["B"]
    want, total = md_logp_at(T, act, extra)
    w = float(_ratio(np.abs(np.asarray(logp, np.float64).reshape(-1) - want), total).max())
    if not choice:
        print(f"[rollout truth] {name}: n={n} heads={H} worst log p ratio {w:.3g}")
        return w
    c = choice_check(act.reshape(-1), T["score"].reshape(n * H, B), T["m"].reshape(-1), T["valid3"].reshape(n * H, B))
    print(f"[rollout truth] {name}: n={n} heads={H} worst log p ratio {w:.3g}; heads breaking the choice rule {len(c['bad'])} "
          f"(invalid {c['invalid']}), undecided {c['undecided']}")
    return max(w, np.inf if len(c["bad"]) else 0.0)


def md_undecided(T):
    n, H, B = T["n"], T["H"], T["B"]
    s = T["score"].reshape(n * H, B)
    return choice_check(s.argmax(1), s, T["m"].reshape(-1), T["valid3"].reshape(n * H, B))["undecided"]


def md_tier2_extra(T64, e_z, bins):
    """Per head: e_a + sum over the head's valid bins of p_j e_j (x exp(2 max e)), as [n, H, B]."""
    out = np.zeros_like(T64["allow"])
    for h, (s, b) in enumerate(zip(starts(bins), bins)):
        v = T64["valid3"][:, h, :b]
        e = np.where(v, e_z[:, s:s + b], 0.0)
        p = np.where(v, np.exp(np.where(v, T64["ls"][:, h, :b], 0.0)), 0.0)
        out[:, h, :b] = e + (p * e).sum(1, keepdims=True) * np.exp(2 * e.max(1, keepdims=True))
    return out


# ------------------------------------------------------------------------------------------------------------ Gaussian heads
def gauss_terms64(x, mean, sd):
    msq, ssq, xsq = mean * mean, sd * sd, x * x
    return -(msq / (2 * ssq)), (mean * x) / ssq, -(xsq / (2 * ssq)), np.log(1 / np.sqrt(2 * np.pi * ssq))


def gauss_truth(y, eps, var_m, var_b):
    """The reference's Gaussian head on tanh outputs y [n, 2k] (float32 values) with var_m / var_b as the float32 numbers the kernel
    gets.  -> dict(mean, sd, r_sd, act: clamp(eps sd + mean, -1, 1), allow_act)."""
    y = np.asarray(y, np.float64)
    k = y.shape[1] // 2
    vm, vb = float(F32(var_m)), float(F32(var_b))
    mean, ys = y[:, :k], y[:, k:2 * k]
    sd = ys * vm + vb
    r_sd = (np.abs(ys * vm) / np.abs(sd) + 1) * U
    raw = np.asarray(eps, np.float64) * sd + mean
    allow = (r_sd + U) * np.abs(np.asarray(eps, np.float64) * sd) + U * np.abs(raw)
    return dict(mean=mean, sd=sd, r_sd=r_sd, act=np.clip(raw, -1, 1), allow_act=allow, k=k, eps=np.asarray(eps, np.float64), vm=vm)


def gauss_logp64(T, act):
    """(log p [n], allowance [n]) of the 4-term formula at the actions `act` (the kernel's own, float32 values)."""
    x = np.asarray(act, np.float64).reshape(T["mean"].shape)
    t = gauss_terms64(x, T["mean"], T["sd"])
    qr = 2 * T["r_sd"] + 3 * U
    a = qr * (np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2])) + T["r_sd"] + 3.5 * U + T_ULP * U * np.abs(t[3])
    sabs = sum(np.abs(ti) for ti in t)
    a = a + 3 * U * sabs
    term = t[0] + t[1] + t[2] + t[3]
    k = T["k"]
    return term.sum(1), a.sum(1) + (k - 1) * U * np.abs(term).sum(1) + U * np.abs(term.sum(1))


def gauss_tier2_extra(T, act, e_y):
    """What log p at a STORED action moves by when the tanh outputs move by at most e_y [n, 2k]: |d lp / d mean| = |x - mean| / sd^2 and
    |d lp / d sd| = |(x - mean)^2 / sd^3 - 1 / sd|, taken at the worst point of the box (|x - mean| + e, sd - e)."""
    k = T["k"]
    x = np.asarray(act, np.float64).reshape(T["mean"].shape)
    e_m, e_s = e_y[:, :k], np.abs(T["vm"]) * e_y[:, k:2 * k]
    dist, sd = np.abs(x - T["mean"]) + e_m, T["sd"] - e_s
    return (dist / sd ** 2 * e_m + np.maximum(dist ** 2 / sd ** 3, 1.0 / sd) * e_s).sum(1)


def diag_tier2_extra(T, act, e_mu):
    x = np.asarray(act, np.float64).reshape(T["mu"].shape)
    return ((np.abs(x - T["mu"]) + e_mu) / T["sd"][None, :] ** 2 * e_mu).sum(1)


def gauss_hold(name, act, logp, T, e_y=None):
    """Actions within their allowance of clamp(eps sd + mean) and inside [-1, 1]; log p of every row at the stored action.  e_y (tier
    ii): a bound on the tanh outputs [n, 2k], carried into the action (e_mean + |eps var_m| e_sd) and into log p (gauss_tier2_extra)."""
    act = np.asarray(act, np.float64).reshape(T["mean"].shape)
    allow_a = T["allow_act"]
    if e_y is not None:
        k = T["k"]
        allow_a = allow_a + e_y[:, :k] + np.abs(T["eps"] * T["vm"]) * e_y[:, k:2 * k]
    ra = float(_ratio(np.abs(act - T["act"]), allow_a).max())
    inside = bool((np.abs(act) <= 1.0).all())
    lp, allow = gauss_logp64(T, act)
    if e_y is not None:
        allow = allow + gauss_tier2_extra(T, act, e_y)
    rl = float(_ratio(np.abs(np.asarray(logp, np.float64).reshape(-1) - lp), allow).max())
    print(f"[rollout truth] {name}: n={act.shape[0]} k={T['k']} worst action ratio {ra:.3g}, log p ratio {rl:.3g}, clamped "
          f"{int((np.abs(T['act']) == 1).sum())}, inside [-1, 1] {inside}")
    return max(ra, rl, 0.0 if inside else np.inf)


def diag_truth(mu, log_std, eps):
    mu, ls = np.asarray(mu, np.float64), np.asarray(log_std, np.float64)
    sd = np.exp(ls)
    raw = np.asarray(eps, np.float64) * sd[None, :] + mu
    return dict(mu=mu, ls=ls, sd=sd, act=raw, allow_act=(T_ULP + 1) * U * np.abs(np.asarray(eps, np.float64) * sd[None, :]) + U * np.abs(raw),
                k=mu.shape[1])


def diag_logp64(T, act):
    from diag_gaussian_yardstick import logp_terms
    x = torch.as_tensor(np.asarray(act, np.float64).reshape(T["mu"].shape))
    term = logp_terms(x, torch.as_tensor(T["mu"]), torch.as_tensor(T["ls"])).numpy()
    dd = (x.numpy() - T["mu"]) ** 2 / (2 * T["sd"][None, :] ** 2)
    a = 13 * U * dd + U * (dd + np.abs(T["ls"])[None, :]) + U * np.abs(term) + U * 0.92
    k = T["k"]
    return term.sum(1), a.sum(1) + (k - 1) * U * np.abs(term).sum(1) + U * np.abs(term.sum(1))


def diag_hold(name, act, logp, T, e_mu=None):
    act = np.asarray(act, np.float64).reshape(T["mu"].shape)
    ra = float(_ratio(np.abs(act - T["act"]), T["allow_act"] + (0.0 if e_mu is None else e_mu)).max())
    lp, allow = diag_logp64(T, act)
    if e_mu is not None:
        allow = allow + diag_tier2_extra(T, act, e_mu)
    rl = float(_ratio(np.abs(np.asarray(logp, np.float64).reshape(-1) - lp), allow).max())
    print(f"[rollout truth] {name}: n={act.shape[0]} k={T['k']} worst action ratio {ra:.3g}, log p ratio {rl:.3g}")
    return max(ra, rl)


# ---------------------------------------------------------------------------------------------------------------- the network
ACT64 = {"relu": lambda x: np.maximum(x, 0.0), "tanh": np.tanh, "elu": lambda x: np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))}


def logit_bound(params, obs, act="relu", out_tanh=False, dup=False):
    """(z64 [n, out], e_z [n, out]): the float64 network on the float32 observations and the bound a float32 layer chain is allowed
    to miss it by, carried through the layers (module docstring, "The network").  dup: output units 1 and out - 2 are duplicates
    (peaked_policy): their exact values are equal, and column out - 2 is given column 1's float64 value -- a blocked float64 product
    may round the two apart by 1e-16, which would turn the exact tie the makers build there into a near-tie on some hosts."""
    h = np.asarray(obs, np.float64)
    e = np.zeros_like(h)
    for i, (w, b) in enumerate(params):
        w64, b64 = np.asarray(w, np.float64), np.asarray(b, np.float64)
        K = w64.shape[1]
        pre = h @ w64.T + b64
        S = (np.abs(h) + e) @ np.abs(w64).T + np.abs(b64)
        e = e @ np.abs(w64).T + nt_allow(torch.as_tensor(S), K).numpy()
        last = i == len(params) - 1
        if not last:
            h = ACT64[act](pre)
            if act != "relu":
                e = e + T_ULP * U * np.abs(h)
        else:
            h = np.tanh(pre) if out_tanh else pre
            if out_tanh:
                e = e + T_ULP * U * np.abs(h)
    if dup and h.shape[1] >= 4:
        h[:, -2], e[:, -2] = h[:, 1], np.maximum(e[:, 1], e[:, -2])
    return h, e


# ------------------------------------------------------------------------------------------------------------------- makers
def rand_mask(rs, n, A, p=0.66):
    """tests/test_gpu_action_mask.py::rand_mask (imported on use: that module pulls in the whole GPU test kit)."""
    from test_gpu_action_mask import rand_mask as rm
    return rm(rs, n, A, p)


ROW_SCALE_UNIFORM, ROW_SCALE_LOW = 1e-3, 0.15


def row_scales(n):
    """Every fifth row nearly uniform (x 1e-3), every fourth (from 1) at 0.15 of its neighbours' scale: with maxima near the span
    next to it the row maxima differ by more than 0.6 x span inside one row tile."""
    s = np.ones(n)
    s[1::4] = ROW_SCALE_LOW
    s[4::5] = ROW_SCALE_UNIFORM
    return s


def logit_case(n, A, span, seed, masked=False, ties=True):
    """Logits given directly (tier i on the host): randn rows scaled so that max|z| = span, row_scales applied, then every fourth row
    (from 2) shifted by -65 as a whole (softmax does not see it, the max-subtraction does: neighbouring maxima differ by > 60).
    Columns 1 and A - 2 are duplicates of each other (exact ties once their noise is equal).  -> (z float32, mask or None, rs)."""
    rs = np.random.RandomState(1009 * seed + 31 * A + n)
    z = rs.randn(n, A)
    z *= span / np.abs(z).max()
    z *= row_scales(n)[:, None]
    z[2::4] -= 65.0
    if ties and A >= 4:
        z[:, A - 2] = z[:, 1]
    mask = rand_mask(rs, n, A) if masked else None
    return z.astype(F32), mask, rs


def noise_case(z64, mask, rs, ties=True, T=None):
    """Exp(1) noise [n, A] as float32 for logits z64, with the special rows the checks need (chosen from the float64 head alone):
      r % 11 == 2   1e-30 at the valid column whose p is the largest below FLOOR / 2  -> a clamped probability is chosen
      r % 11 == 5   1e-30 at the valid column whose p is the smallest above 2 FLOOR   -> a probability just above the clamp is chosen
      r % 11 == 7   the duplicated columns 1 and A - 2 get EQUAL noise small enough to win together -> an exact tie, first index wins
      odd rows      1e-30 on every INVALID column (where the clamp's floor would win if an invalid action were a candidate)."""
    n, A = z64.shape
    q = rs.exponential(1.0, (n, A)).astype(F32)
    q = np.maximum(q, F32(1e-6))
    T = discrete_truth(z64, None, mask) if T is None else T
    p, valid = T["p"], T["valid"]
    rows = np.arange(n)
    below = np.where(valid & (p < FLOOR / 2), p, -1.0)
    above = np.where(valid & (p > 2 * FLOOR), p, 2.0)
    for r in rows[rows % 11 == 2]:
        if below[r].max() > 0:
            q[r, below[r].argmax()] = F32(1e-30)
    for r in rows[rows % 11 == 5]:
        if above[r].min() < 1e-6:
            q[r, above[r].argmin()] = F32(1e-30)
    if ties and A >= 4:
        for r in rows[rows % 11 == 7]:
            if valid[r, 1] and valid[r, A - 2]:
                q[r, 1] = q[r, A - 2] = F32(1e-25)
    if mask is not None:
        odd = np.zeros((n, 1), bool)
        odd[1::2] = True
        q = np.where(odd & ~valid, F32(1e-30), q)
    return q


def assert_inputs(T, label):
    """The condition on a case's inputs, from float64 alone: the undecided rows at or under 1 % of its rows."""
    und = undecided_rows(T)
    assert und <= UNDECIDED_CAP * T["n"], (label, "undecided rows", und, T["n"])
    return und


def peaked_policy(d, hidden, A, span, obs, seed, act="relu", dup=True):
    """A policy whose logits reach +-span on `obs` (the last layer scaled, as update_case(saturate=True) does).  The hidden biases are
    zero, so a ReLU network is positively homogeneous in its input and a ROW's scale sets its peakedness (row_scales); the last
    layer keeps its bias (unscaled: the nearly uniform rows see it).  dup: output units 1 and A - 2 are duplicates."""
    from oracle import nets
    torch.manual_seed(seed)
    pol = nets.init_mlp(d, hidden, A)
    pol = [(w, torch.zeros_like(b)) for w, b in pol[:-1]] + [pol[-1]]
    z, _ = logit_bound([(w.numpy(), np.zeros_like(b.numpy())) for w, b in pol], obs, act)
    w, b = pol[-1]
    w = w * float(span / np.abs(z).max())
    if dup and A >= 4:
        w, b = w.clone(), b.clone()
        w[A - 2], b[A - 2] = w[1], b[1]
    return pol[:-1] + [(w.contiguous(), b.contiguous())]


def obs_case(n, d, seed):
    rs = np.random.RandomState(7919 * seed + n)
    obs = np.clip(rs.randn(n, d), -5, 5) * row_scales(n)[:, None]
    return obs.astype(F32), rs


# ------------------------------------------------------------------------------------- float32 restatements and their mutants
MUTANTS = ("no_max_subtraction", "clamp_floor_1e-10", "clamp_before_normalising", "padded_in_normaliser", "log_of_unclamped_p",
           "exp_2^-12", "last_index_on_ties", "neighbour_noise_row", "invalid_through_floor", "nvec_padding_candidate",
           "gauss_logp_unclamped", "gauss_no_var_b")
DISCRETE_MUTANTS = MUTANTS[:9]


def discrete32(z, q, mask=None, mutant=None, n_pad=0):
    """softmax -> clamp -> log -> first arg-max of pc / q in float32 numpy, op by op as the kernels have it.  n_pad: padded columns
    behind A (their logits are 0: zero weights and bias), which only the mutant counts.  -> (act, logp, pc, p)."""
    z, q = np.asarray(z, F32), np.asarray(q, F32)
    n, A = z.shape
    valid = np.ones((n, A), bool) if mask is None else np.asarray(mask, bool).copy()
    valid[~valid.any(1)] = True
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        zz = np.where(valid, z, F32(-np.inf))
        mx = np.zeros((n, 1), F32) if mutant == "no_max_subtraction" else zz.max(1, keepdims=True)
        e = np.where(valid, np.exp(zz - mx), F32(0)).astype(F32)
        if mutant == "exp_2^-12":
            e = (e * (F32(1) + F32(2.0 ** -12) * ((np.arange(A) % 3) - 1).astype(F32))).astype(F32)
        s = e.sum(1, keepdims=True, dtype=F32)
        if mutant == "padded_in_normaliser":
            s = (s + np.where(valid, F32(0), np.exp(z - mx)).sum(1, keepdims=True, dtype=F32) + F32(n_pad) * np.exp(-mx)).astype(F32)
        floor = F32(1e-10) if mutant == "clamp_floor_1e-10" else F32(1e-11)
        if mutant == "clamp_before_normalising":
            p = (e / s).astype(F32)
            pc = np.minimum(np.maximum(e, floor) / s, F32(1)).astype(F32)
        else:
            p = (e / s).astype(F32)
            pc = np.minimum(np.maximum(p, floor), F32(1))
        cand = np.ones((n, A), bool) if mutant == "invalid_through_floor" else valid
        qq = np.roll(q, -1, axis=0) if mutant == "neighbour_noise_row" else q
        v = np.where(cand, (pc / qq).astype(F32), F32(-np.inf))
        if mutant == "last_index_on_ties":
            act = A - 1 - v[:, ::-1].argmax(1)
        else:
            act = v.argmax(1)
        chosen = (p if mutant == "log_of_unclamped_p" else pc)[np.arange(n), act]
        logp = np.log(chosen).astype(F32)
    pc = np.where(valid, pc, F32(0))
    p = np.where(valid, p, F32(0))
    return act, logp, pc, p


def md32(z, bins, q, mask=None, mutant=None, float_sum=False):
    """The multi-discrete sampling step in float32 numpy (csrc/heads.hip: lse = mx + logf(sum), term = z_a - lse; the row's sum in
    double rounded once, or serially in float).  -> (act [n, H], logp [n])."""
    z = np.asarray(z, F32)
    n, H, B, S = z.shape[0], len(bins), max(bins), sum(bins)
    q = np.asarray(q, F32).reshape(n, H, B)
    act = np.zeros((n, H), np.int64)
    lp64, lp32 = np.zeros(n), np.zeros(n, F32)
    zp = np.concatenate([z[:, :S], np.zeros((n, B), F32)], 1)
    for h, (s, b) in enumerate(zip(starts(bins), bins)):
        w = B if mutant == "nvec_padding_candidate" else b
        v = np.ones((n, w), bool)
        if mask is not None and mutant != "nvec_padding_candidate":
            v = np.asarray(mask, bool)[:, s:s + b].copy()
            v[~v.any(1)] = True
        zz = np.where(v, zp[:, s:s + w], F32(-np.inf))
        mx = zz.max(1, keepdims=True)
        e = np.where(v, np.exp(zz - mx), F32(0)).astype(F32)
        ssum = e.sum(1, keepdims=True, dtype=F32)
        lse = (mx + np.log(ssum)).astype(F32)
        sc = np.where(v, ((e / ssum).astype(F32) / q[:, h, :w]).astype(F32), F32(-np.inf))
        act[:, h] = sc.argmax(1)
        term = (zz[np.arange(n), act[:, h]] - lse[:, 0]).astype(F32)
        lp64 += term.astype(np.float64)
        lp32 = (lp32 + term).astype(F32)
    return act, lp32 if float_sum else lp64.astype(F32)


def gauss32(y, eps, var_m, var_b, mutant=None):
    """The Gaussian sampling step in float32 numpy (gauss_logpdf of csrc/heads.hip).  -> (act [n, k], logp [n])."""
    y, eps = np.asarray(y, F32), np.asarray(eps, F32)
    k = y.shape[1] // 2
    vm, vb = F32(var_m), F32(0.0 if mutant == "gauss_no_var_b" else var_b)
    mean = y[:, :k]
    sd = (y[:, k:2 * k] * vm + vb).astype(F32)
    raw = (eps * sd + mean).astype(F32)
    a = np.clip(raw, F32(-1), F32(1))
    x = raw if mutant == "gauss_logp_unclamped" else a
    with np.errstate(divide="ignore", invalid="ignore"):
        msq, ssq, xsq = mean * mean, sd * sd, x * x
        t1 = -(msq / (F32(2) * ssq))
        t2 = (mean * x) / ssq
        t3 = -(xsq / (F32(2) * ssq))
        t4 = np.log(F32(1) / np.sqrt(F32(2 * np.pi) * ssq))
        term = (((t1 + t2).astype(F32) + t3).astype(F32) + t4).astype(F32)
    lp = np.zeros(y.shape[0], F32)
    for j in range(k):
        lp = (lp + term[:, j]).astype(F32)
    return a, lp if k <= 32 else term.astype(np.float64).sum(1).astype(F32)


def diag32(mu, log_std, eps):
    mu, ls, eps = np.asarray(mu, F32), np.asarray(log_std, F32), np.asarray(eps, F32)
    sd = np.exp(ls).astype(F32)
    a = (eps * sd[None, :] + mu).astype(F32)
    d = (a - mu).astype(F32)
    term = ((-(d * d) / (F32(2) * (sd * sd))[None, :]).astype(F32) - ls[None, :]).astype(F32) - F32(0.9189385332046727)
    k = mu.shape[1]
    lp = np.zeros(mu.shape[0], F32)
    for j in range(k):
        lp = (lp + term[:, j]).astype(F32)
    return a, lp if k <= 32 else term.astype(np.float64).sum(1).astype(F32)


# ------------------------------------------------------------------------------------------------------ on-policy consistency
def ploss_bound(allow_rollout, allow_update, mean_ratio=1.0, gap=0.0):
    """RLPPO_STAT_PLOSS + 1 = -mean(ratio - 1) at unchanged weights with advantages 1 is allowed the mean of the two sides'
    log-probability allowances (|exp(x) - 1| <= |x| exp|x|, the factor is applied) plus the float32 rounding of the mean: per row
    expf (4 u), the products with the advantage and 1 / mb (2 u), one addition into the thread's accumulator and the six levels of
    the wave's shuffle tree (7 u); the waves' sums are added in double.  gap [n]: where each side's allowance is taken around its OWN
    truth (the sharp form: head-only allowances on each side's own network output), the distance of the two truths."""
    x = np.asarray(allow_rollout, np.float64) + np.asarray(allow_update, np.float64) + gap
    return float((x * np.exp(x)).mean()) + (T_ULP + 2 + 7) * U * mean_ratio
