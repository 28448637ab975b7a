"""Float64 truth, element for element, for what happens to a gradient AFTER the minibatch pass: gradient-norm clip + Adam
(rlppo_clip_adam and every fused form of it), the batch statistics of advantage normalisation (rlppo_adv_stats), the target-KL
gate's batch sum (rlppo_kl_gate / rlppo_kl_gate_lr) and the packed image (rlppo_net_pack).  Plain numpy, importable without a GPU.

Every bound here is DERIVED (the precedent of fp64_gate.gauss_logp_check), never fitted to what a device returns: a first-order
forward error analysis of the kernel's own operation list, in which every float32 rounding contributes SLACK * u * |rounded value|
(u = 2^-24, SLACK = 2: the factor fp64_gate._check_flips allows) and is carried through the operations behind it by their partial
derivatives.  Per element that is c * u * (sum of the |terms| that meet in each addition) with c = 2 x (roundings on the path).

The operation list of adam_kernel (csrc/optim.hip; -ffp-contract=off, so no product is fused into an addition), 25 roundings:
    coef  (5)  (float)max_norm [host] | (float)sqrt(gnorm2) | the constant 1e-6f | total + 1e-6f | max_norm / (...)
    g'    (1)  g * coef                                                       -> 6 roundings behind g': c = 12 when clipped
    m'    (4)  (float)(1 - beta1) [host] | g' - m | omb1 * (...) | m + (...)
    v'    (6)  (float)beta2 [host] | v * beta2 | (float)(1 - beta2) [host] | omb2 * g' | (...) * g' | the sum
    denom (5)  sqrtf(v') | (float)sqrt(bc2) [host] | ... / bc2_sqrt | (float)eps [host] | ... + eps
    p'    (4)  (float)(lr / bc1) [host] | step_size * m' | ... / denom | p + (...)
A coefficient that the clamp sets to 1 is exact: when max_norm / (sqrt(norm2) + 1e-6) exceeds 1 by more than the five roundings
can move it, coef carries no error and g' is the gradient bit for bit."""
import math

import numpy as np

U32 = 2.0 ** -24   # float32 unit roundoff
SLACK = 2.0        # fp64_gate._check_flips' factor
W = SLACK * U32    # what one float32 rounding contributes, relative to the value it rounds
COEF_ROUNDINGS = 5
ADAM_ROUNDINGS = 25   # the list above: c = 2 x 25 = 50 bounds every path through it


def _f64(x):
    return np.asarray(x, np.float64)


def clip_adam64(p, g, m, v, norm2, max_norm, lr, beta1, beta2, eps, step, lr_device=None, mutant=None):
    """clip_grad_norm_ + torch.optim.Adam (single-tensor math) in float64 from the float32 state handed in:
        coef = min(1, max_norm / (sqrt(norm2) + 1e-6));  g' = g coef
        m'   = m + (1 - beta1)(g' - m);                  v' = beta2 v + (1 - beta2) g'^2
        p'   = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),   bc_k = 1 - beta_k^step
    norm2: the squared norm the implementation under test itself clipped with, as a double (the device's gnorm2 word, held to
    exact_sum_squares on its own; the CPU oracle's float32 total, squared): the chain behind it is what this function bounds, so a
    float32 accumulation of the norm -- which torch's CPU path has and the kernels, summing in double, have not -- is not charged
    to the step.  lr_device: the rate when it lives in a device double (it replaces lr:
    the kernel then forms (float)(lr_device / bc1), the same single rounding).  -> (truth, bound), dicts over "g", "m", "v", "p".
    mutant: one of MUTANTS -- a deliberately wrong restatement, for the host test that shows the bound separates right from wrong."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    rate = float(lr if lr_device is None else lr_device)
    raw = max_norm / (math.sqrt(norm2) + 1e-6)
    coef = raw if mutant == "coef_not_clamped" else min(1.0, raw)
    r_coef = COEF_ROUNDINGS * W
    if raw > 1.0 + 2.0 * r_coef:
        r_coef = 0.0   # every float32 evaluation of the quotient is above 1 too: the clamp returns exactly 1
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** (step + 1 if mutant == "step_plus_one_in_bc2" else step)
    if mutant == "bc1_omitted":
        bc1 = 1.0
    b1 = beta2 if mutant == "beta2_for_beta1" else beta1
    omb1, omb2, ss, bc2s = 1.0 - b1, 1.0 - beta2, rate / bc1, math.sqrt(bc2)

    g1 = g * coef
    e_g = np.abs(g1) * ((r_coef + W) if r_coef else 0.0)          # coef == 1 exactly: g * 1.0f is g
    # m' = m + omb1 * (g' - m)
    d = g1 - m
    e_d = e_g + W * np.abs(d)
    prod = omb1 * d
    e_prod = omb1 * e_d + 2 * W * np.abs(prod)                    # (float)(1 - beta1), the product
    m1 = m + prod
    e_m = e_prod + W * np.abs(m1)
    # v' = v * beta2 + (omb2 * g') * g'
    a = v * beta2
    e_a = 2 * W * np.abs(a)                                       # (float)beta2, the product
    b = omb2 * g1
    e_b = omb2 * e_g + 2 * W * np.abs(b)                          # (float)(1 - beta2), the product
    c = b * g1
    e_c = np.abs(g1) * e_b + np.abs(b) * e_g + W * np.abs(c)
    v1 = a + c
    e_v = e_a + e_c + W * np.abs(v1)
    # denom = sqrt(v') / bc2_sqrt + eps
    s = np.sqrt(v1)
    lower = np.sqrt(np.maximum(v1 - e_v, 0.0))
    e_s = np.where(e_v > 0, e_v / np.maximum(s + lower, 1e-300), 0.0) + W * s
    if mutant == "eps_before_division":
        den = (s + eps) / bc2s
    elif mutant == "eps_under_root":
        den = np.sqrt(v1 / bc2 + eps)
    else:
        den = s / bc2s + eps
    q = s / bc2s
    e_q = e_s / bc2s + 2 * W * q                                  # (float)sqrt(bc2), the division
    e_den = e_q + W * eps + W * np.abs(den)                       # (float)eps, the sum
    # p' = p + (-step_size * m') / denom
    num = ss * m1
    e_num = ss * e_m + 2 * W * np.abs(num)                        # (float)(lr / bc1), the product
    upd = num / den
    e_upd = e_num / den + np.abs(upd) * e_den / den + W * np.abs(upd)
    p1 = p - upd
    e_p = e_upd + W * np.abs(p1)
    return dict(g=g1, m=m1, v=v1, p=p1), dict(g=e_g, m=e_m, v=e_v, p=e_p)


MUTANTS = ("eps_before_division", "eps_under_root", "step_plus_one_in_bc2", "bc1_omitted", "beta2_for_beta1", "coef_not_clamped")


def exact_sum_squares(g):
    """sum g_i^2 of float32 values: every square is exact in float64 (24 x 24 bits), math.fsum adds them exactly."""
    x = _f64(g).ravel()
    return math.fsum((x * x).tolist())


def worst(got, truth, bound):
    """max over the elements of |got - truth| / bound, with 0 / 0 = 0 and anything / 0 = inf: no element is left out."""
    err = np.abs(_f64(got) - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


# ------------------------------------------------------------------------------------------------ the table of section a
# (id, n, step, gradient kind, max_norm, (beta1, beta2)).  Sizes: 1 / 255 / 256 / 257 = one workgroup and its edges; 262144 = the
# 1024-workgroup cap of launch_clip_adam; 262145 = the first grid-stride element; 1100003 = several stride rounds.  Kinds: "wide" =
# magnitudes log-uniform over 1e-9 .. 1e3 per element, "small" = all about 1e-4 (never clipped at max_norm 0.5 below 2.5e7
# elements), "big" = all about 30 (clipped at 0.5 and 1e-3, not at 1e9).  Small step counts with small-gradient elements are where
# a misplaced eps or a bias correction that is off shows; the row at step 100000 is "big" and unclipped ON PURPOSE: there bc2 == 1
# in double and v' ~ 900 >> eps, so the two eps mutants are invisible by construction (test_optim_yardstick_host asserts both).
ADAM_CASES = [
    ("n1_step1_wide", 1, 1, "wide", 0.5, (0.9, 0.999)),
    ("n255_step2_wide_tightclip", 255, 2, "wide", 1e-3, (0.9, 0.999)),
    ("n256_step7_small", 256, 7, "small", 0.5, (0.9, 0.999)),
    ("n257_step1_big", 257, 1, "big", 0.5, (0.9, 0.999)),
    ("n256_step1_small_noclip", 256, 1, "small", 1e9, (0.9, 0.999)),
    ("n257_step1000_wide_betas", 257, 1000, "wide", 1e-3, (0.8, 0.99)),
    ("n255_step100000_big_noclip", 255, 100000, "big", 1e9, (0.9, 0.999)),
    ("n262144_step1_wide", 262144, 1, "wide", 0.5, (0.9, 0.999)),
    ("n262145_step2_wide_noclip_betas", 262145, 2, "wide", 1e9, (0.8, 0.99)),
    ("n262145_step1000_small_tightclip", 262145, 1000, "small", 1e-3, (0.9, 0.999)),
    ("n1100003_step7_wide", 1100003, 7, "wide", 0.5, (0.9, 0.999)),
]
LR, EPS = 3e-4, 1e-8


def gradient(kind, n, rs):
    sign = np.where(rs.rand(n) < 0.5, -1.0, 1.0)
    if kind == "wide":
        mag = 10.0 ** rs.uniform(-9.0, 3.0, n)
    elif kind == "small":
        mag = 1e-4 * rs.uniform(0.5, 1.5, n)
    elif kind == "big":
        mag = 30.0 * rs.uniform(0.5, 1.5, n)
    else:
        raise ValueError(kind)
    return (sign * mag).astype(np.float32)


def adam_state(case, seed=0):
    """-> float32 (p, g, m, v) of a table row: m = v = 0 at step 1, else moments of the gradient's own scale, element by element
    (so that a small-gradient element has a small second moment: the elements on which eps matters)."""
    _, n, step, kind, _, _ = case
    rs = np.random.RandomState(1000 + seed + n % 9973 + step)
    p = (rs.randn(n) * 0.2).astype(np.float32)
    g = gradient(kind, n, rs)
    if step == 1:
        return p, g, np.zeros(n, np.float32), np.zeros(n, np.float32)
    g64 = np.abs(g.astype(np.float64))
    m = (g64 * rs.uniform(-1.0, 1.0, n)).astype(np.float32)
    v = (g64 * g64 * rs.uniform(0.5, 1.5, n)).astype(np.float32)
    return p, g, m, v


def torch_adam32(p, g, m, v, max_norm, lr, beta1, beta2, eps, step):
    """The CPU float32 oracle: oracle.ppo.clip_coef and the operations of oracle.ppo.adam_step (torch.optim.Adam's single-tensor
    math) with the hyper-parameters as arguments.  -> float32 arrays dict(g, m, v, p) and norm2 = its float32 total norm, squared."""
    import torch
    from oracle import ppo
    t = lambda x: torch.as_tensor(np.array(x, np.float32))
    p, g, m, v = t(p), t(g), t(m), t(v)
    k = g.numel() // 2
    coef, total = ppo.clip_coef([(g[:k], g[k:])], max_norm)
    g = g * coef
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))
    return dict(g=g.numpy(), m=m.numpy(), v=v.numpy(), p=p.numpy()), float(total) ** 2


# ------------------------------------------------------------------------------------------------ advantage statistics
def ring_rows(idx, ring_base, ring_cap):
    idx = np.asarray(idx, np.int64)
    return (idx + ring_base) % ring_cap if ring_cap > 0 else idx


def _ulp32(x):
    """Spacing of float32 in the binade that holds |x| (round-to-nearest errs by at most half of it)."""
    x = abs(float(x))
    if x < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.floor(math.log2(x)) - 23)


def adv_stats64(adv, idx, ring_base=0, ring_cap=0):
    """(mean, 1 / (std + 1e-8)) of adv[rows(idx)] with the unbiased (n - 1) deviation and exact summation (math.fsum; the deviation
    by the corrected two-pass formula), n == 1: (0, 1) as rlppo_adv_stats defines it.  -> (mean, scale, bound_mean, bound_scale).
    The bounds are those of adv_stats_kernel's arithmetic: shifted double sums t0 = sum d, t1 = sum d^2 over d = A - A_first (n
    additions in any order: n 2^-53 sum|terms| each, doubled), m = t0 / n, var = (t1 - t0 m) / (n - 1), one float32 rounding of each
    result:
        |mean err|  <= ulp32(mean) / 2 + n 2^-52 mean|A - A_first|
        |var err|   <= [ n 2^-52 t1  +  2 |m| n 2^-52 sum|d|  +  2^-52 (|t0 m| + |t1 - t0 m|) ] / (n - 1)
                       (the sum of squares; t0 m = t0^2 / n through t0's error; the product, the division and the CANCELLING
                       subtraction)
        |scale err| <= ulp32(scale) / 2 + scale^2 |var err| / (2 std)."""
    a = _f64(np.asarray(adv, np.float32)[ring_rows(idx, ring_base, ring_cap)])
    n = a.size
    if n == 1:
        return 0.0, 1.0, 0.0, 0.0
    mean = math.fsum(a.tolist()) / n
    dev = a - mean
    ss = math.fsum((dev * dev).tolist()) - math.fsum(dev.tolist()) ** 2 / n
    var = max(ss, 0.0) / (n - 1)
    std = math.sqrt(var)
    scale = 1.0 / (std + 1e-8)
    d = a - a[0]
    sum_abs_d = math.fsum(np.abs(d).tolist())
    t0, t1 = math.fsum(d.tolist()), math.fsum((d * d).tolist())
    m = t0 / n
    u = 2.0 ** -52
    b_mean = 0.5 * _ulp32(mean) + n * u * (sum_abs_d / n)
    e_var = (n * u * t1 + 2.0 * abs(m) * n * u * sum_abs_d + u * (abs(t0 * m) + abs(t1 - t0 * m))) / (n - 1)
    e_std = 0.0 if e_var == 0.0 else e_var / (std + math.sqrt(max(var - e_var, 0.0)) + 1e-300)
    b_scale = 0.5 * _ulp32(scale) + scale * scale * e_std
    return mean, scale, b_mean, b_scale


# (n, advantages, idx, ring) of section c.  Sizes: 1 / 2 / 3 = the smallest batches; 511 / 512 / 513 = the grid is cdiv(n, 512);
# 65536 = exactly 128 workgroups; 65537 = the first grid-stride row; 200003 = several stride rounds.  Advantages: "normal" N(0, 1),
# "offset" N(1e4, 1e-2) (cancellation), "constant", "two" (two values), "outlier" (the FIRST row -- the kernel's pivot -- 1e3 sigma
# out).  idx: a permutation or rows drawn with repetition; plain arrays or a ring whose base makes the rows wrap.
ADV_CASES = [
    (1, "normal", "perm", False), (2, "offset", "perm", True), (2, "constant", "perm", False), (3, "two", "repeat", False),
    (3, "outlier", "perm", True), (511, "normal", "repeat", True), (512, "offset", "perm", False), (513, "outlier", "perm", True),
    (513, "constant", "perm", False), (65536, "normal", "perm", True), (65537, "offset", "repeat", False),
    (65537, "constant", "repeat", True), (200003, "outlier", "repeat", True), (200003, "two", "perm", False),
]


def adv_case(n, kind, idx_kind, ring, seed=0):
    """-> (adv float32 [cap] as it lies in memory, idx int64 [n] logical rows, ring_base, ring_cap)."""
    rs = np.random.RandomState(77 + seed + n)
    cap = n + 7
    if kind == "normal":
        adv = rs.randn(cap)
    elif kind == "offset":
        adv = 1e4 + 1e-2 * rs.randn(cap)
    elif kind == "constant":
        adv = np.full(cap, 0.3712)
    elif kind == "two":
        adv = np.where(rs.rand(cap) < 0.3, -1.25, 0.7)
    elif kind == "outlier":
        adv = 0.5 + 0.1 * rs.randn(cap)
    else:
        raise ValueError(kind)
    idx = rs.permutation(cap)[:n] if idx_kind == "perm" else rs.randint(0, cap, n)
    idx = idx.astype(np.int64)
    base, rcap = (cap - max(1, n // 3), cap) if ring else (0, 0)
    if kind == "outlier":
        adv[ring_rows(idx[:1], base, rcap)] = 0.5 + 1e3 * 0.1
    return adv.astype(np.float32), idx, base, rcap


# ------------------------------------------------------------------------------------------------ the KL gate's batch sum
def kl_batch64(regions):
    """regions: [(mb_ratio, slots)] per pass.  KL_b = sum_pass mb_ratio * fsum(slots), with the bound of ANY summation order of the
    kernel's shape (per pass at most `slots` double additions, then one product and one addition per pass):
    (slots per pass + passes) 2^-53 sum|terms|, the terms being mb_ratio * slot."""
    kl, abs_terms, widest = 0.0, 0.0, 0
    parts = []
    for ratio, slots in regions:
        s = _f64(slots).ravel()
        parts.append(float(ratio) * math.fsum(s.tolist()))
        abs_terms += abs(float(ratio)) * math.fsum(np.abs(s).tolist())
        widest = max(widest, s.size)
    kl = math.fsum(parts)
    return kl, (widest + len(regions)) * 2.0 ** -53 * abs_terms


def exchange_bound(kl):
    """What KL_b loses on its way through the two exchange floats hi = fl32(KL_b), lo = fl32(KL_b - hi): the difference is exact in
    double and |KL_b - hi| <= 2^-24 |KL_b|, so the one rounding of lo costs at most 2^-24 * 2^-24 |KL_b| -- two floats carry 48 bits."""
    return 2.0 ** -48 * abs(kl)


# ------------------------------------------------------------------------------------------------ the packed image
def packed_layout(dims, L=None):
    """[(in, out, pin, pout, off_w, off_wt, off_b, off_flat_w, off_flat_b)] per layer and the two totals, by the rule of
    include/rlppo.h: Pin_0 = rlppo_padded_width(dims[0]), Pin_l = Pout_(l-1), Pout_l = rlppo_padded_out(dims[l + 1]); per layer
    W[Pout][Pin], W^T[Pin][Pout], b[Pout] one behind the other (the offsets fp64_gate.hip_masks walks).  The two width functions are
    host code of the library: no GPU is needed."""
    if L is None:
        from rlgym_ppo_amd import _native as N
        L = N.lib()
    pin, off, flat, out = int(L.rlppo_padded_width(dims[0])), 0, 0, []
    for l in range(len(dims) - 1):
        i, o = int(dims[l]), int(dims[l + 1])
        pout = int(L.rlppo_padded_out(o))
        out.append((i, o, pin, pout, off, off + pout * pin, off + 2 * pout * pin, flat, flat + o * i))
        off += 2 * pout * pin + pout
        flat += o * i + o
        pin = pout
    return out, off, flat


def packed_image(dims, flat, L=None):
    """The image rlppo_net_pack is documented to build from the flat arena (float32, zero wherever no parameter lands)."""
    flat = np.asarray(flat, np.float32)
    layers, total, n_flat = packed_layout(dims, L)
    assert flat.size >= n_flat   # (a parameter tail behind the layers is never packed)
    img = np.zeros(total, np.float32)
    for i, o, pin, pout, off_w, off_wt, off_b, fw, fb in layers:
        w = flat[fw:fw + o * i].reshape(o, i)
        img[off_w:off_w + pout * pin].reshape(pout, pin)[:o, :i] = w
        img[off_wt:off_wt + pin * pout].reshape(pin, pout)[:i, :o] = w.T
        img[off_b:off_b + o] = flat[fb:fb + o]
    return img
