"""Every rollout step held to float64 truth, element by element and row by row (tests/rollout_yardstick.py has the derivation):
tier (i) on the kernel's own logits (what rlppo_mlp_forward returns on the same rows, packed weights and options), tier (ii) from
the observations with the propagated logit bound e_z; the choice rule on every row; the one-launch kernel and the chain bit for bit
at peaked inputs; the bf16 inference precision; and the on-policy consistency of the rollout's log p with the update's.

No fixed log p or probability tolerance, no norm-wise comparison, no count of rows that may differ: every assertion is
`worst ratio <= 1` against a derived per-element allowance, or an exact statement."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rollout_yardstick as R  # noqa: E402
from hip_pass import L, Net, P, check, dev, run_pass, stream  # noqa: E402,F401
from oracle import nets  # noqa: E402

D = 107
ROWS = (1, 17, 250, 4099)
WORST = {}


def hold(entry, ratio):
    """Books the worst ratio of an entry point (printed: the figures of DESIGN.md, "What the rollout steps are held to") and asserts."""
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    print(f"[rollout truth] worst ratio so far, {entry}: {WORST[entry]:.3g}")
    assert ratio <= 1.0, (entry, ratio)


def act_opts(hidden_act="relu", bf16=False, words=None):
    from rlgym_ppo_amd import _native as N
    if hidden_act == "relu" and not bf16 and words is None:
        return None, None
    o = N.ActOpts()
    o.hidden_act = N.HIDDEN_ACTIVATIONS[hidden_act]
    if bf16:
        o.precision = N.PRECISION_BF16
    if words is not None:
        o.action_mask, o.mask_words = words.data_ptr(), words.shape[1]
    return o, ctypes.byref(o)


def pack_mask(mask, A):
    from rlgym_ppo_amd.util import action_mask as AM
    return None if mask is None else AM.pack(np.asarray(mask, bool), A, "cuda")


def counters(L):
    return int(L.rlppo_dbg_counter(0)), int(L.rlppo_dbg_counter(1))


def forward(L, net, rows, n, out_tanh=0, hidden_act="relu", bf16=False):
    """The chain's own output on the rows: [n, outputs] float32 (no mask: the layers know none)."""
    out = torch.full((n, net.ld_out), float("nan"), device="cuda")
    w = net.ws(n)
    _, ref = act_opts(hidden_act, bf16)
    check(L, L.rlppo_mlp_forward(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, out_tanh, P(out), net.ld_out, P(w), w.numel(), ref))
    torch.cuda.synchronize()
    return out[:, :net.dims[-1]].cpu().numpy()


def discrete_act(L, net, rows, n, q, mask=None, hidden_act="relu", bf16=False):
    """rlppo_discrete_act with probs_out -> (act, logp, probs, (one-launch runs, chain runs))."""
    A = net.dims[-1]
    act = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((n,), float("nan"), device="cuda")
    pr = torch.full((n, A), float("nan"), device="cuda")
    w = net.ws(n)
    words = pack_mask(mask, A)
    o, ref = act_opts(hidden_act, bf16, words)
    qd = dev(q)
    c = counters(L)
    check(L, L.rlppo_discrete_act(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, P(qd), P(act), P(lp), P(pr), P(w), w.numel(), ref))
    torch.cuda.synchronize()
    c1 = counters(L)
    return act.cpu().numpy(), lp.cpu().numpy(), pr.cpu().numpy(), (c1[0] - c[0], c1[1] - c[1])


class Case:
    """A peaked discrete policy on ROWS[-1] (or n_max) observation rows, its float64 side and its noise, made once per test."""

    def __init__(self, L, hidden, A, span, masked, act="relu", n_max=ROWS[-1], seed=None, d=D, label=""):
        seed = A + 7 * len(hidden) + span if seed is None else seed
        self.A, self.n_max = A, n_max
        self.obs, rs = R.obs_case(n_max, d, seed)
        self.pol = R.peaked_policy(d, hidden, A, span, self.obs, seed, act=act)
        self.z64, self.e_z = R.logit_bound(self.pol, self.obs, act, dup=True)
        self.mask = R.rand_mask(rs, n_max, A) if masked else None
        T = R.discrete_truth(self.z64, None, self.mask)
        self.q = R.noise_case(self.z64, self.mask, rs, T=T)
        self.T64 = R.with_noise(T, self.q)
        self.extra = R.tier2_extra(self.T64, self.e_z)
        self.assert_inputs((label, hidden, A, span, masked))                               # float64 alone; nothing is on the GPU yet
        if L is not None:
            self.net = Net(L, self.pol)
            self.rows = self.net.pad(self.obs)

    def head(self, T, n):
        """The first n rows of a truth."""
        return {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in dict(T, n=n).items()}

    def assert_inputs(self, label):
        """From float64 alone, before any GPU call: the undecided rows at or under 1 % for every row count the test runs."""
        for n in sorted({n for n in ROWS if n < self.n_max} | {self.n_max}):
            R.assert_inputs(self.head(self.T64, n), (label, n))

    def m(self, n):
        return None if self.mask is None else self.mask[:n]


def hold_discrete(L, c, n, entry, label, fused, hidden_act="relu", bf16=False, tier2=True):
    act, lp, pr, ran = discrete_act(L, c.net, c.rows, n, c.q[:n], c.m(n), hidden_act, bf16)
    assert ran == ((1, 0) if fused else (0, 1)), (label, "one-launch / chain launches", ran)
    z = forward(L, c.net, c.rows, n, 0, hidden_act, bf16)
    T = R.discrete_truth(z, c.q[:n], c.m(n))                                               # tier (i): the kernel's own logits
    hold(entry, R.discrete_hold(f"{label} n={n} tier (i)", act, lp, T, probs=pr))
    if tier2:
        lw = float(R._ratio(np.abs(z - c.z64[:n]), c.e_z[:n]).max())                         # tier (ii): the network, then log p
        T64 = c.head(c.T64, n)
        w = R.logp_worst(lp, act, T64, R.extra_at(c.extra[:n], act))
        print(f"[rollout truth] {label} n={n} tier (ii): logits {lw:.3g}, log p {w:.3g}")
        hold(entry + ", tier (ii)", max(lw, w))
    return act, lp, pr


# ------------------------------------------------------------------------------------------- rlppo_discrete_act, one launch
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [5, 64, 90, 128])
@pytest.mark.parametrize("hidden", [(64, 64), (128, 128), (256, 256, 256)])
def test_discrete_act_one_launch(L, hidden, A, masked):
    """The shapes of the one-launch kernel.  It keeps the padded observation row and the padded head inside the hidden width
    (fused_act_ok of csrc/fused_act.hip): 45 features (padded 64) in front of 64 units, and 64 units take the one launch up to 64
    actions -- at 90 and 128 they run the chain, which is held all the same; which of the two ran is read off the counters and
    must be what rlppo_discrete_step_one_launch announces."""
    d = 45 if hidden[0] == 64 else D
    fused = int(L.rlppo_padded_out(A)) <= hidden[0]
    assert fused or hidden[0] == 64
    for span in (30, 100):
        c = Case(L, hidden, A, span, masked, d=d)
        for n in ROWS:
            assert int(L.rlppo_discrete_step_one_launch(c.net.dims_c, c.net.nl, n, None)) == int(fused)
            hold_discrete(L, c, n, "rlppo_discrete_act, " + ("one launch" if fused else "chain") + (", masked" if masked else ""),
                          f"one launch {hidden} A={A} span={span}", fused)


# ----------------------------------------------------------------------------------------------- rlppo_discrete_act, chain
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("span", [30, 100])
@pytest.mark.parametrize("A", [64, 65, 128, 129, 512, 513, 2048])
def test_discrete_act_chain(L, A, span, masked):
    """(128, 96) is a network the one-launch kernel does not cover; the widths are both sides of the three regimes of dispatch_discrete."""
    c = Case(L, (128, 96), A, span, masked)
    for n in ROWS:
        hold_discrete(L, c, n, "rlppo_discrete_act, chain" + (", masked" if masked else ""), f"chain A={A} span={span}", False)


def test_discrete_act_chain_beyond_the_one_launch_limit(L):
    c = Case(L, (128, 128), 90, 30, True, n_max=8200)
    hold_discrete(L, c, 8200, "rlppo_discrete_act, chain, masked", "chain past 8192 rows (128, 128) A=90", False)
    hold_discrete(L, c, 8192, "rlppo_discrete_act, one launch, masked", "one launch at 8192 rows (128, 128) A=90", True)


@pytest.mark.parametrize("act", ["tanh", "elu"])
def test_discrete_act_tanh_elu_chain(L, act):
    for hidden, A, masked in (((128, 96), 90, False), ((128, 128), 129, True)):
        c = Case(L, hidden, A, 30, masked, act=act)
        for n in ROWS:
            hold_discrete(L, c, n, f"rlppo_discrete_act, {act}", f"{act} {hidden} A={A}", False, hidden_act=act)


# ------------------------------------------------------------------------------------- one launch and chain, bit for bit
def test_one_launch_and_chain_agree_bit_for_bit_at_peaked_inputs(L):
    for span, masked in ((30, False), (100, True)):
        c = Case(L, (128, 128), 90, span, masked)
        for n in (17, 4099):
            a = hold_discrete(L, c, n, "rlppo_discrete_act, one launch" + (", masked" if masked else ""), f"both forms, one launch span={span}", True)
            assert L.rlppo_dbg_set(27, 0) == 0
            try:
                b = hold_discrete(L, c, n, "rlppo_discrete_act, chain" + (", masked" if masked else ""), f"both forms, chain span={span}", False)
            finally:
                assert L.rlppo_dbg_set(27, 1) == 0
            assert all(np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)
                       for x, y in zip(a, b)), (span, n)


# ----------------------------------------------------------------------------------------------------- rlppo_discrete_step
def standardise64(x, mode, mean0, std0, mean_v, std_v):
    """(rows [n, d] float64, allowance): the contract of rlppo_discrete_step on (float)x: clip((x - mean) / std, -5, 5); the cast of a
    float64 observation, the subtraction and the quotient round once each."""
    x64 = np.asarray(x, np.float64)
    if mode == 0:
        return x64, R.U * np.abs(x64) * (x.dtype == np.float64)
    mean, std = (np.float64(np.float32(mean0)), np.float64(np.float32(std0))) if mode == 1 else (mean_v.astype(np.float64), std_v.astype(np.float64))
    v = (x64 - mean) / std
    allow = 2 * R.U * np.abs(v) + R.U * np.abs(x64 - mean) / np.abs(std) + R.U * np.abs(x64) / np.abs(std) * (x.dtype == np.float64)
    return np.clip(v, -5, 5), allow


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_discrete_step_raw_observation_modes(L, mode, f64):
    for hidden, fused in (((128, 128), True), ((128, 96), False)):
        A, n_max = 90, ROWS[-1]
        rs = np.random.RandomState(40 + mode)
        raw = (rs.randn(n_max, D) * 2.0 + 0.7) * R.row_scales(n_max)[:, None]
        raw = raw.astype(np.float64 if f64 else np.float32)
        mean_v = (0.7 + 0.2 * rs.randn(D)).astype(np.float32)
        std_v = (2.0 + 0.5 * rs.rand(D)).astype(np.float32)
        want_rows, allow_rows = standardise64(raw, mode, mean_v[0], std_v[0], mean_v, std_v)
        obs32 = want_rows.astype(np.float32)
        pol = R.peaked_policy(D, hidden, A, 30, obs32, seed=mode + 3)
        z64, _ = R.logit_bound(pol, obs32, dup=True)
        mask = R.rand_mask(rs, n_max, A)
        T = R.discrete_truth(z64, None, mask)
        q = R.noise_case(z64, mask, rs, T=T)
        T = R.with_noise(T, q)
        for n in ROWS + (1030,):                                                           # (1030: 1024 + 6, a second tail)
            R.assert_inputs(Case.head(None, T, n), ("step", mode, f64, n))
        net = Net(L, pol)
        for n in ROWS + (1030,):
            src = dev(raw[:n], torch.float64 if f64 else torch.float32)
            act = torch.full((n,), -7, dtype=torch.int64, device="cuda")
            act_f = torch.full((n,), float("nan"), device="cuda")
            lp = torch.full((n,), float("nan"), device="cuda")
            rows_out = torch.full((n, net.ld_in), float("nan"), device="cuda")
            ws = torch.empty(int(L.rlppo_discrete_step_workspace_bytes(net.dims_c, net.nl, n)), dtype=torch.uint8, device="cuda")
            words = pack_mask(mask[:n], A)
            o, ref = act_opts(words=words)
            mv, sv, qd = dev(mean_v), dev(std_v), dev(q[:n])
            c0 = counters(L)
            check(L, L.rlppo_discrete_step(stream(), net.dims_c, net.nl, P(net.packed), P(src), int(f64), D, n, mode, float(mean_v[0]), float(std_v[0]),
                                           P(mv) if mode == 2 else None, P(sv) if mode == 2 else None, P(qd), P(act), P(act_f), P(lp),
                                           P(rows_out), net.ld_in, P(ws), ws.numel(), ref))
            torch.cuda.synchronize()
            c1 = counters(L)
            assert (c1[0] - c0[0], c1[1] - c0[1]) == ((1, 0) if fused else (0, 1)), (hidden, mode, f64)
            got_rows = rows_out.cpu().numpy()
            assert (got_rows[:, D:] == 0).all()
            hold("rlppo_discrete_step, rows_out", float(R._ratio(np.abs(got_rows[:, :D] - want_rows[:n]), allow_rows[:n]).max()))
            z = forward(L, net, rows_out, n)                                               # the logits of ITS rows
            Tn = R.discrete_truth(z, q[:n], mask[:n])
            a, l = act.cpu().numpy(), lp.cpu().numpy()
            assert np.array_equal(act_f.cpu().numpy(), a.astype(np.float32))
            hold("rlppo_discrete_step, " + ("one launch" if fused else "chain"), R.discrete_hold(f"step mode={mode} f64={f64} {hidden} n={n}", a, l, Tn))


# ------------------------------------------------------------------------------ rlppo_discrete_probs, rlppo_categorical_select
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("A", [90, 129, 600, 2048])
def test_discrete_probs_every_element(L, A, masked):
    c = Case(L, (128, 96), A, 100 if A < 600 else 30, masked)
    for n in ROWS:
        z = forward(L, c.net, c.rows, n)
        T = R.discrete_truth(z, None, c.m(n))
        words = pack_mask(c.m(n), A)
        o, ref = act_opts(words=words)
        w = c.net.ws(n)
        for clamp in (0, 1):
            pr = torch.full((n, A + 3), float("nan"), device="cuda")
            check(L, L.rlppo_discrete_probs(stream(), c.net.dims_c, c.net.nl, P(c.net.packed), P(c.rows), c.net.ld_in, n, clamp, P(pr), A + 3, None, P(w),
                                            w.numel(), ref))
            torch.cuda.synchronize()
            got = pr.cpu().numpy()
            assert np.isnan(got[:, A:]).all()
            r = R.probs_worst(got[:, :A], T, bool(clamp))
            print(f"[rollout truth] rlppo_discrete_probs A={A} n={n} clamp={clamp} masked={masked}: worst ratio over every element {r:.3g}; "
                  f"smallest probability held {T['p'][T['valid']].min():.3g}")
            hold("rlppo_discrete_probs, " + ("clamped" if clamp else "unclamped"), r)


@pytest.mark.parametrize("A", [5, 90, 600])
def test_categorical_select_on_float64_rounded_probabilities(L, A):
    """The probabilities are the float64 head's, rounded once: the score is ONE correctly rounded quotient, so the margin is 2 u, and
    log p is logf of the given number."""
    n_max = ROWS[-1]
    z, _, rs = R.logit_case(n_max, A, 30, seed=A)
    T0 = R.discrete_truth(z)
    q = R.noise_case(z.astype(np.float64), None, rs, T=T0)
    p32 = T0["pc"].astype(np.float32)
    p = p32.astype(np.float64)
    T = dict(T0, pc=p, logpc=np.log(p), score=p / q.astype(np.float64), m=np.full(n_max, 2 * R.U), allow_logp=R.T_ULP * R.U * np.abs(np.log(p)))
    for n in ROWS:
        R.assert_inputs(Case.head(None, T, n), ("select", A, n))
    for n in ROWS:
        act = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        lp = torch.full((n,), float("nan"), device="cuda")
        pd, qd = dev(p32[:n]), dev(q[:n])
        check(L, L.rlppo_categorical_select(stream(), P(pd), A, n, A, P(qd), P(act), P(lp)))
        torch.cuda.synchronize()
        hold("rlppo_categorical_select", R.discrete_hold(f"select A={A} n={n}", act.cpu().numpy(), lp.cpu().numpy(), Case.head(None, T, n)))


# ----------------------------------------------------------------------------------------------------------- multi-discrete
NVEC_CASES = {"S_past_64": ((33, 2, 31), 64, (64, 64)), "H_at_cap": ((2,) * 64, 107, (128, 128)), "one_bin_head": ((1, 4), 33, (64, 64))}


def md_setup(L, bins, d, hidden, seed, masked, n_max=ROWS[-1], span=30):
    obs, rs = R.obs_case(n_max, d, seed)
    pol = R.peaked_policy(d, hidden, sum(bins), span, obs, seed, dup=False)
    z64, e_z = R.logit_bound(pol, obs)
    q = np.maximum(rs.exponential(1.0, (n_max * len(bins), max(bins))), 1e-6).astype(np.float32)
    mask = None
    if masked:
        from masked_multidiscrete_yardstick import rand_mask
        mask = rand_mask(rs, n_max, bins)
    T64 = R.md_truth(z64, bins, q, mask)
    assert R.md_undecided(T64) <= R.UNDECIDED_CAP * n_max * len(bins)
    net = Net(L, pol)
    return dict(obs=obs, pol=pol, z64=z64, e_z=e_z, q=q, mask=mask, T64=T64, net=net, rows=net.pad(obs), bins=bins, H=len(bins), B=max(bins))


def md_call(L, s, n, entry, bf16=False):
    from rlgym_ppo_amd.util import action_mask as AM
    import multidiscrete_nvec_yardstick as Y
    net, bins, H = s["net"], s["bins"], s["H"]
    act = torch.full((n, H), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((n,), float("nan"), device="cuda")
    w = net.ws(n)
    qd = dev(s["q"][:n * H])
    o, ref = act_opts(bf16=bf16)
    args = (stream(), net.dims_c, net.nl, P(net.packed), P(s["rows"]), net.ld_in, n, P(qd), P(act), P(lp), P(w), w.numel(), ref)
    if entry == "rlppo_multidiscrete_act":
        check(L, L.rlppo_multidiscrete_act(*args))
    elif s["mask"] is None:
        check(L, L.rlppo_multidiscrete_act_nvec(*args, Y.nvec_array(bins), H))
    else:
        words = AM.pack(s["mask"][:n], sum(bins), "cuda", heads=bins)
        check(L, L.rlppo_multidiscrete_act_nvec_masked(*args, Y.nvec_array(bins), H, P(words), words.shape[1]))
    torch.cuda.synchronize()
    return act.cpu().numpy(), lp.cpu().numpy()


def hold_md(L, s, n, entry, label, bf16=False):
    bins, H = s["bins"], s["H"]
    act, lp = md_call(L, s, n, entry, bf16)
    m = None if s["mask"] is None else s["mask"][:n]
    z = forward(L, s["net"], s["rows"], n, bf16=bf16)
    hold(("bf16 inference, " if bf16 else "") + entry, R.md_hold(f"{label} n={n} tier (i)", act, lp, R.md_truth(z, bins, s["q"][:n * H], m)))
    if not bf16:
        T64 = R.md_truth(s["z64"][:n], bins, s["q"][:n * H], m)
        lw = float(R._ratio(np.abs(z - s["z64"][:n]), s["e_z"][:n]).max())
        w = R.md_hold(f"{label} n={n} tier (ii), log p", act, lp, T64, extra=R.md_tier2_extra(T64, s["e_z"][:n], bins), choice=False)
        print(f"[rollout truth] {label} n={n} tier (ii): logits {lw:.3g}, log p {w:.3g}")
        hold(entry + ", tier (ii)", max(lw, w))
    return act, lp


def test_multidiscrete_act_fixed_bins(L):
    s = md_setup(L, nets.MD_BINS, D, (64, 64), 21, False)
    for n in ROWS:
        hold_md(L, s, n, "rlppo_multidiscrete_act", "fixed bins")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", list(NVEC_CASES))
def test_multidiscrete_act_nvec(L, name, masked):
    bins, d, hidden = NVEC_CASES[name]
    s = md_setup(L, bins, d, hidden, 30 + len(bins), masked)
    for n in ROWS:
        hold_md(L, s, n, "rlppo_multidiscrete_act_nvec" + ("_masked" if masked else ""), f"nvec {name}")


# ------------------------------------------------------------------------------------------------------------ Gaussian heads
def gauss_setup(L, k, n_max=ROWS[-1]):
    from test_gpu_heads import saturate_sd
    torch.manual_seed(50 + k)
    rs = np.random.RandomState(50 + k)
    pol = saturate_sd(nets.init_mlp(D, (128, 64), 2 * k), k)
    obs = np.clip(rs.randn(n_max, D), -5, 5).astype(np.float32)
    eps = rs.randn(n_max, k).astype(np.float32)
    eps[: n_max // 4] *= 4.0
    net = Net(L, pol)
    y64, e_y = R.logit_bound(pol, obs, out_tanh=True)
    return dict(pol=pol, obs=obs, eps=eps, net=net, rows=net.pad(obs), y64=y64, e_y=e_y, k=k)


def gauss_call(L, s, n, bf16=False):
    net, k = s["net"], s["k"]
    vm, vb = nets.var_map(0.1, 1.0)
    act = torch.full((n, k), float("nan"), device="cuda")
    lp = torch.full((n,), float("nan"), device="cuda")
    w = net.ws(n)
    _, ref = act_opts(bf16=bf16)
    eps = dev(s["eps"][:n])
    check(L, L.rlppo_gaussian_act(stream(), net.dims_c, net.nl, P(net.packed), P(s["rows"]), net.ld_in, n, P(eps), vm, vb, P(act), P(lp),
                                  P(w), w.numel(), ref))
    torch.cuda.synchronize()
    return act.cpu().numpy(), lp.cpu().numpy(), vm, vb


@pytest.mark.parametrize("k", [1, 17, 33])
def test_gaussian_act(L, k):
    s = gauss_setup(L, k)
    for n in ROWS:
        act, lp, vm, vb = gauss_call(L, s, n)
        y = forward(L, s["net"], s["rows"], n, out_tanh=1)
        assert (y[:, k] == -1.0).all() and (k == 1 or (y[:, k + 1] == 1.0).all())          # the saturated sd units
        T = R.gauss_truth(y, s["eps"][:n], vm, vb)
        if n == ROWS[-1]:
            assert (np.abs(T["act"]) == 1).sum() > 10
        hold("rlppo_gaussian_act", R.gauss_hold(f"gaussian k={k} n={n} tier (i)", act, lp, T))
        lw = float(R._ratio(np.abs(y - s["y64"][:n]), s["e_y"][:n]).max())
        T64 = R.gauss_truth(s["y64"][:n], s["eps"][:n], vm, vb)
        hold("rlppo_gaussian_act, tier (ii)", max(lw, R.gauss_hold(f"gaussian k={k} n={n} tier (ii), tanh outputs {lw:.3g}", act, lp, T64, e_y=s["e_y"][:n])))


def diag_setup(L, k, n_max=ROWS[-1]):
    torch.manual_seed(60 + k)
    rs = np.random.RandomState(60 + k)
    pol = nets.init_mlp(D, (128, 64), k)
    obs = np.clip(rs.randn(n_max, D), -5, 5).astype(np.float32)
    net = Net(L, pol)
    mu64, e_mu = R.logit_bound(pol, obs)
    return dict(pol=pol, obs=obs, eps=rs.randn(n_max, k).astype(np.float32), log_std=rs.uniform(-2.5, 0.7, k).astype(np.float32), net=net,
                rows=net.pad(obs), mu64=mu64, e_mu=e_mu, k=k)


def diag_call(L, s, n, bf16=False):
    net, k = s["net"], s["k"]
    act = torch.full((n, k), float("nan"), device="cuda")
    lp = torch.full((n,), float("nan"), device="cuda")
    w = net.ws(n)
    _, ref = act_opts(bf16=bf16)
    eps, ls = dev(s["eps"][:n]), dev(s["log_std"])
    check(L, L.rlppo_diag_gaussian_act(stream(), net.dims_c, net.nl, P(net.packed), P(s["rows"]), net.ld_in, n, P(eps), P(ls), P(act), P(lp), P(w),
                                       w.numel(), ref))
    torch.cuda.synchronize()
    return act.cpu().numpy(), lp.cpu().numpy()


@pytest.mark.parametrize("k", [1, 33])
def test_diag_gaussian_act(L, k):
    s = diag_setup(L, k)
    for n in ROWS:
        act, lp = diag_call(L, s, n)
        mu = forward(L, s["net"], s["rows"], n)
        hold("rlppo_diag_gaussian_act", R.diag_hold(f"diag k={k} n={n} tier (i)", act, lp, R.diag_truth(mu, s["log_std"], s["eps"][:n])))
        lw = float(R._ratio(np.abs(mu - s["mu64"][:n]), s["e_mu"][:n]).max())
        T64 = R.diag_truth(s["mu64"][:n], s["log_std"], s["eps"][:n])
        hold("rlppo_diag_gaussian_act, tier (ii)", max(lw, R.diag_hold(f"diag k={k} n={n} tier (ii), means {lw:.3g}", act, lp, T64, e_mu=s["e_mu"][:n])))


# ------------------------------------------------------------------------------------------------- bf16 inference precision
def test_bf16_inference_precision_every_head(L):
    """Tier (i) unchanged: the logits come from the same bf16 chain (rlppo_mlp_forward with the call's precision)."""
    n = 1030
    c = Case(L, (128, 128), 90, 30, True, n_max=n)
    hold_discrete(L, c, n, "bf16 inference, rlppo_discrete_act", "bf16 discrete", False, bf16=True, tier2=False)
    hold_md(L, md_setup(L, nets.MD_BINS, D, (64, 64), 21, False, n_max=n), n, "rlppo_multidiscrete_act", "bf16 fixed bins", bf16=True)
    hold_md(L, md_setup(L, (33, 2, 31), 64, (64, 64), 33, True, n_max=n), n, "rlppo_multidiscrete_act_nvec_masked", "bf16 nvec S_past_64", bf16=True)
    s = gauss_setup(L, 17, n_max=n)
    act, lp, vm, vb = gauss_call(L, s, n, bf16=True)
    y = forward(L, s["net"], s["rows"], n, out_tanh=1, bf16=True)
    hold("bf16 inference, rlppo_gaussian_act", R.gauss_hold("bf16 gaussian k=17", act, lp, R.gauss_truth(y, s["eps"][:n], vm, vb)))
    s = diag_setup(L, 33, n_max=n)
    act, lp = diag_call(L, s, n, bf16=True)
    mu = forward(L, s["net"], s["rows"], n, bf16=True)
    hold("bf16 inference, rlppo_diag_gaussian_act", R.diag_hold("bf16 diag k=33", act, lp, R.diag_truth(mu, s["log_std"], s["eps"][:n])))


# ----------------------------------------------------------------------------------------------------- on-policy consistency
N_ON = 1024


def update_output(L, net, rows, n, out_tanh=False):
    """The network output as the UPDATE's forward forms it at n rows: the pass runs the product's own gemm_nt launcher layer by layer
    (bias + ReLU, then bias or bias + tanh), which rlppo_dbg_gemm_nt reaches on the packed weights -- the premise tests/fp64_gate.py::
    hip_masks reads the pass's ReLU decisions by.  [n, outputs] float32."""
    h, pin, off = rows, net.ld_in, 0
    for l in range(net.nl):
        pout = int(L.rlppo_padded_out(net.dims[l + 1]))
        w_ptr = ctypes.c_void_p(net.packed.data_ptr() + 4 * off)
        b_ptr = ctypes.c_void_p(net.packed.data_ptr() + 4 * (off + 2 * pout * pin))
        out = torch.full((n, pout), float("nan"), device="cuda")
        epi = 1 if l < net.nl - 1 else (2 if out_tanh else 0)
        check(L, L.rlppo_dbg_gemm_nt(stream(), P(h), pin, w_ptr, pin, b_ptr, None, 0, P(out), pout, n, pout, pin, epi))
        off += 2 * pout * pin + pout
        h, pin = out, pout
    torch.cuda.synchronize()
    return h[:, :net.dims[-1]].cpu().numpy()


def on_policy(L, label, pol, obs, acts, logp, allow, sharp=None, **kw):
    """One pass at UNCHANGED weights with the rollout's own log p as old_logp and advantages 1: RLPPO_STAT_PLOSS + 1 = -mean(ratio - 1)
    within the mean of the two sides' allowances + the float32 rounding of the mean; RLPPO_STAT_CLIPFRAC exactly 0.
    allow: the tier-(ii) allowance of a row, for both sides (the propagated worst case: wide on peaked policies).
    sharp = ((log p64, allowance) on the rollout's own network output, the same on the update's): the head-only tier-(i) allowance
    of each side around its own truth, and the float64 distance of the two truths in between -- a bound of ~1e-5 that a systematic
    rollout-update bias of 1e-4 breaks."""
    torch.manual_seed(5)
    val = nets.init_mlp(obs.shape[1], (64, 64), 1)
    ones, zeros = np.ones(N_ON, np.float32), np.zeros(N_ON, np.float32)
    r = run_pass(L, pol, val, obs, acts, logp, zeros, ones, np.arange(N_ON), clip=0.2, ent=0.0, mb_ratio=1.0, **kw)
    bias = float(r["stats"][4]) + 1.0
    bound = None if allow is None else R.ploss_bound(allow, allow)
    print(f"[rollout truth] on-policy {label}: PLOSS + 1 = -mean(ratio - 1) = {bias:.3e}" + ("" if bound is None else f", allowed {bound:.3e}, ratio "
          f"{abs(bias) / bound:.3g}") + f"; clip fraction {float(r['stats'][3])}")
    if bound is not None:
        hold("on-policy consistency, " + label, abs(bias) / bound)
        assert float(r["stats"][3]) == 0.0
    if sharp is not None:
        (lp_r, a_r), (lp_u, a_u) = sharp
        gap = np.abs(lp_u - lp_r)
        b2 = R.ploss_bound(a_r, a_u, gap=gap)
        print(f"[rollout truth] on-policy {label}, sharp: allowed {b2:.3e} (largest distance of the two sides' truths {gap.max():.3e}, rows whose "
              f"network outputs differ {int((gap > 0).sum())}), ratio {abs(bias) / b2:.3g}")
        hold("on-policy consistency, sharp, " + label, abs(bias) / b2)
    return bias


def discrete_at(z, mask, act):
    T = R.discrete_truth(z, None, mask)
    rows = np.arange(len(act))
    return T["logpc"][rows, act], T["allow_logp"][rows, act]


def test_on_policy_consistency_discrete(L):
    """Logits within +-1 (a fresh policy) and within +-30 (peaked)."""
    for span, masked in ((1, False), (1, True), (30, False), (30, True)):
        c = Case(L, (128, 128), 90, span, masked, n_max=N_ON, label="on-policy")
        act, lp, _, _ = discrete_act(L, c.net, c.rows, N_ON, c.q, c.mask)
        allow = c.T64["allow_logp_soft"][np.arange(N_ON), act] + R.extra_at(c.extra, act)
        sharp = (discrete_at(forward(L, c.net, c.rows, N_ON), c.mask, act), discrete_at(update_output(L, c.net, c.rows, N_ON), c.mask, act))
        on_policy(L, f"discrete, span {span}" + (", masked" if masked else ""), c.pol, c.obs, act.astype(np.float32), lp, allow, sharp=sharp,
                  head="discrete", mask=c.mask)
    # a bf16-precision rollout against the fp32 update: printed only (the reference has no such mode)
    act, lp, _, _ = discrete_act(L, c.net, c.rows, N_ON, c.q, c.mask, bf16=True)
    on_policy(L, "discrete, masked, bf16 rollout (printed only)", c.pol, c.obs, act.astype(np.float32), lp, None, head="discrete", mask=c.mask)


def md_allow(T64, e_z, bins, act):
    return R.md_logp_at(T64, act, R.md_tier2_extra(T64, e_z, bins))[1]


def md_sharp(L, s, act):
    n, H = N_ON, s["H"]
    at = lambda z: R.md_logp_at(R.md_truth(z, s["bins"], s["q"][:n * H], s["mask"]), act)
    return at(forward(L, s["net"], s["rows"], n)), at(update_output(L, s["net"], s["rows"], n))


def test_on_policy_consistency_multidiscrete(L):
    for span in (1, 30):
        s = md_setup(L, nets.MD_BINS, D, (64, 64), 21, False, n_max=N_ON, span=span)
        act, lp = md_call(L, s, N_ON, "rlppo_multidiscrete_act")
        on_policy(L, f"multi-discrete, fixed bins, span {span}", s["pol"], s["obs"], act.astype(np.float32), lp,
                  md_allow(s["T64"], s["e_z"], s["bins"], act), sharp=md_sharp(L, s, act), head="multidiscrete")
        for masked in (False, True):
            s = md_setup(L, (33, 2, 31), 64, (64, 64), 33, masked, n_max=N_ON, span=span)
            act, lp = md_call(L, s, N_ON, "nvec")
            on_policy(L, f"multi-discrete, nvec, span {span}" + (", masked" if masked else ""), s["pol"], s["obs"], act.astype(np.float32), lp,
                      md_allow(s["T64"], s["e_z"], s["bins"], act), sharp=md_sharp(L, s, act), head="nvec", entry="nvec", bins=s["bins"],
                      mask=s["mask"], mask_heads=masked)


def test_on_policy_consistency_gaussian_heads(L):
    s = gauss_setup(L, 17, n_max=N_ON)
    act, lp, vm, vb = gauss_call(L, s, N_ON)
    T64 = R.gauss_truth(s["y64"], s["eps"], vm, vb)
    allow = R.gauss_logp64(T64, act)[1] + R.gauss_tier2_extra(T64, act, s["e_y"])
    at = lambda y: R.gauss_logp64(R.gauss_truth(y, s["eps"], vm, vb), act)
    sharp = (at(forward(L, s["net"], s["rows"], N_ON, out_tanh=1)), at(update_output(L, s["net"], s["rows"], N_ON, out_tanh=True)))
    on_policy(L, "gaussian", s["pol"], s["obs"], act, lp, allow, sharp=sharp, head="gaussian", var=(0.1, 1.0))
    s = diag_setup(L, 33, n_max=N_ON)
    act, lp = diag_call(L, s, N_ON)
    T64 = R.diag_truth(s["mu64"], s["log_std"], s["eps"])
    allow = R.diag_logp64(T64, act)[1] + R.diag_tier2_extra(T64, act, s["e_mu"])
    at = lambda mu: R.diag_logp64(R.diag_truth(mu, s["log_std"], s["eps"]), act)
    sharp = (at(forward(L, s["net"], s["rows"], N_ON)), at(update_output(L, s["net"], s["rows"], N_ON)))
    on_policy(L, "diagonal Gaussian", s["pol"], s["obs"], act, lp, allow, sharp=sharp, head="diag", entry="diag", log_std=s["log_std"])
