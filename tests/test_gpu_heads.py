"""Every policy head on every update path: the Gaussian (ContinuousPolicy) and multi-discrete (MultiDiscreteFF) heads through the
launch forms of rlppo_ppo_minibatch that the discrete head's tests pin (fused row-table gather, paired policy + critic launches,
folded value head, stacked pairs, per-layer dW), across action widths and the edges of their loss kernels (csrc/heads.hip),
with ring-resident experience, at the paired pass's default size, and through PPOLearner at an action width above 32; and the
discrete kernels' instantiations for more than 128 actions that the discrete head's own tests do not launch (section 7).
Reference: float64 truth (tests/fp64_gate.py over oracle/ppo.py::minibatch_analytic)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets, ppo  # noqa: E402
import fp64_gate  # noqa: E402
import ppo_yardstick as PY  # noqa: E402
from hip_pass import L, Net, P, check, dev, relerr, run_minibatch, run_pass, stream, triple  # noqa: E402,F401

D = 107


def make_case(head, seed, n, k=8, hidden=(256, 256, 256), var=(0.1, 1.0), noise=0.2):
    """Policy + critic and an n-row experience buffer whose actions / old log-probabilities the float32 oracle drew from the
    policy itself (ratios exp(+-noise * randn): both clip edges crossed)."""
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    n_out = {"discrete": 90, "gaussian": 2 * k, "multidiscrete": 21}[head]
    pol, val = nets.init_mlp(D, hidden, n_out), nets.init_mlp(D, hidden, 1)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    with torch.no_grad():
        if head == "discrete":
            act, logp = nets.discrete_sample(nets.discrete_probs(pol, obs), nets.draw_exp_noise(n, 90))
        elif head == "gaussian":
            mean, std = nets.gauss_out(pol, obs, *var)
            act, logp = nets.gauss_sample(mean, std, torch.as_tensor(rs.randn(n, k).astype(np.float32)))
        else:
            lsm, probs = nets.md_dist(pol, obs)
            act, logp = nets.md_sample(lsm, probs, nets.draw_exp_noise(n * 8, 3))
    acts = act.numpy().astype(np.float32)
    old = (logp.numpy() + noise * rs.randn(n)).astype(np.float32)
    tgt, adv = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    return pol, val, obs, acts, old, tgt, adv, rs


def gate_rows(L, head, pol, val, obs, acts, old, tgt, adv, idx, mb_ratio, got, var=(0.1, 1.0), label=""):
    return fp64_gate.gate(L, head, pol, val, obs[idx], acts[idx], old[idx], adv[idx], tgt[idx], 0.2, 0.005, mb_ratio, got, var=var,
                          label=label)


def bit_equal(a, b, what):
    for (x, y), (u, v) in zip(a, b):
        assert torch.equal(x, u) and torch.equal(y, v), what


def within(a, b, tol, what):
    for (x, y), (u, v) in zip(a, b):
        assert relerr(u, x) < tol and relerr(v, y) < tol, what


# ------------------------------------------------------------------------------- 1. head x launch-form matrix
@pytest.mark.parametrize("head,k", [("gaussian", 8), ("gaussian", 3), ("multidiscrete", 8)])
def test_launch_forms_for_every_head(L, head, k):
    """tests/test_gpu_kernels.py::test_fused_gather_and_paired_launches_are_bitwise_neutral for the other heads: the paired pass has a
    head dispatch of its own (the Gaussian tanh forward, the three loss launches), the fused gather strides the actions by act_dim.
    A ragged 1500-row minibatch (a partial row tile, five partial 256-row loss blocks) drawn with repeats from 5000 rows, 256x3 nets
    (twin_ok).  The multi-discrete head's 21 outputs go through the GEMM, not the matrix-vector head."""
    pol, val, obs, acts, old, tgt, adv, rs = make_case(head, 31 + k, 5000, k)
    idx = rs.randint(0, 5000, 1500)
    idx[:3] = [4999, 0, 4999]
    forms = dict(fused=(2, 2, 0, 1), separate_gather=(0, 2, 0, 1), two_chains=(2, 0, 0, 1), round2=(0, 0, 0, 1), stacked_pairs=(2, 2, 0, 0),
                 folded_value_head=(2, 2, 1, 1))
    runs, paired = {}, {}
    for key, (k26, k29, k32, k33) in forms.items():
        for knob, v in ((26, k26), (29, k29), (32, k32), (33, k33)):
            check(L, L.rlppo_dbg_set(knob, v))
        try:
            c3 = L.rlppo_dbg_counter(3)
            runs[key] = run_minibatch(L, head, pol, val, obs, acts, old, tgt, adv, idx, 0.2, 0.005, 0.25)
            paired[key] = L.rlppo_dbg_counter(3) - c3
        finally:
            for knob in (26, 29, 32, 33):
                check(L, L.rlppo_dbg_set(knob, 1))
    # the forms ran the paths they name
    assert paired["fused"] == 1 and paired["two_chains"] == 0 and paired["round2"] == 0 and paired["folded_value_head"] == 1
    gp0, gv0, st0 = runs["fused"]
    for key, (gp, gv, st) in runs.items():
        if key == "folded_value_head":
            continue
        bit_equal(gp0 + gv0, gp + gv, key)
        np.testing.assert_allclose(st0, st, rtol=1e-12, atol=0, err_msg=key)  # (double atomics of two chains: order of the last bit)
    gp1, gv1, st1 = runs["folded_value_head"]
    bit_equal(gp0, gp1, "folded_value_head: policy")
    within(gv0, gv1, 2e-6, "folded_value_head: critic")
    check(L, L.rlppo_dbg_set(37, 0))
    try:
        gp3, gv3, st3 = run_minibatch(L, head, pol, val, obs, acts, old, tgt, adv, idx, 0.2, 0.005, 0.25)
    finally:
        check(L, L.rlppo_dbg_set(37, 1))
    within(gp0 + gv0, gp3 + gv3, 2e-6, "per_layer_dw")
    runs["per_layer_dw"] = (gp3, gv3, st3)
    for key in ("fused", "two_chains", "folded_value_head", "per_layer_dw"):
        gate_rows(L, head, pol, val, obs, acts, old, tgt, adv, idx, 0.25, runs[key], label=f"{head} k={k} {key}, ragged 1500-row minibatch")


# ------------------------------------------------------------------------------- 2. shapes and edges of the non-discrete heads
def saturate_sd(pol, k):
    """Output-layer biases of +-30 on sd units: tanh == -1 exactly (sd == var_min, 1 - y^2 == 0) on unit k, +1 (sd == var_max) on unit
    k + 1 when there is one -- for every row."""
    w, b = pol[-1]
    b = b.clone()
    b[k] = -30.0
    if k > 1:
        b[k + 1] = 30.0
    return pol[:-1] + [(w, b)]


@pytest.mark.parametrize("k,var,mb", [(1, (0.1, 1.0), 1000), (3, (0.2, 1.5), 2100), (8, (0.1, 1.0), 1500), (17, (0.2, 1.5), 1300),
                                      (32, (0.1, 1.0), 2999), (40, (0.2, 1.5), 1700), (64, (0.2, 1.5), 1100)])
def test_gaussian_widths_and_edges(L, k, var, mb):
    """gaussian_loss_kernel (one thread per row, 256 rows per block) at action widths 1 ... 64 (above 32 its log-probability is summed in double) and row counts above one block and not a
    multiple of 256.  Every row set has: actions clamped to exactly +-1 (noise x 4 on a quarter of the rows), sd units with tanh
    saturated at both ends, ratios beyond both clip edges; a non-default var range goes to the kernel and to the gate alike.  (With
    sd pinned at a var_min of 0.05 on every row, the four-term log-density loses ~1e-4 of the policy loss in ANY float32 evaluation,
    the CPU oracle's included: the float64 statistics gate would measure the data, not the kernel.  The CPU test of the float64
    formulas, tests/test_oracle_nets_ppo.py, covers that range.)"""
    torch.manual_seed(k)
    rs = np.random.RandomState(100 + k)
    n = mb + 500
    pol = saturate_sd(nets.init_mlp(D, (128, 64), 2 * k), k)
    val = nets.init_mlp(D, (128, 64), 1)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    eps = rs.randn(n, k).astype(np.float32)
    eps[: n // 4] *= 4.0
    with torch.no_grad():
        mean, std = nets.gauss_out(pol, obs, *var)
        act, logp = nets.gauss_sample(mean, std, torch.as_tensor(eps))
    acts = act.numpy()
    old = (logp.numpy() + 0.3 * rs.randn(n)).astype(np.float32)
    tgt, adv = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    idx = rs.permutation(n)[:mb]
    # the edges are really there
    assert (np.abs(acts[idx]) == 1.0).any()
    y = nets.mlp(pol, obs, out_act="tanh").detach().numpy()
    assert (y[:, k] == -1.0).all() and (k == 1 or (y[:, k + 1] == 1.0).all())
    ratio = np.exp(logp.numpy()[idx].astype(np.float64) - old[idx])
    assert (ratio < 0.8).sum() > 10 and (ratio > 1.2).sum() > 10
    got = run_minibatch(L, "gaussian", pol, val, obs, acts, old, tgt, adv, idx, 0.2, 0.005, 0.5, var=var)
    gate_rows(L, "gaussian", pol, val, obs, acts, old, tgt, adv, idx, 0.5, got, var=var, label=f"gaussian k={k} var={var} mb={mb}")


def test_multidiscrete_saturated_logits(L):
    """multidiscrete_loss_kernel over ~3000 rows (12 blocks, the last partial) with logits scaled to +-30 (near one-hot 3-bin and
    2-bin heads).  A third of the rows carry uniformly drawn actions -- log-probabilities down to hundreds below zero -- with old
    log-probabilities 0.5 off either way (ratio clipped); every bin of every head occurs."""
    torch.manual_seed(5)
    rs = np.random.RandomState(5)
    n, mb = 3500, 2999
    pol = nets.init_mlp(D, (128, 128), 21)
    val = nets.init_mlp(D, (128, 128), 1)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    with torch.no_grad():
        s = 30.0 / nets.mlp(pol, obs).abs().max().item()
        pol = pol[:-1] + [(pol[-1][0] * s, pol[-1][1] * s)]
        lsm, probs = nets.md_dist(pol, obs)
        act, _ = nets.md_sample(lsm, probs, nets.draw_exp_noise(n * 8, 3))
        third = n // 3
        bins = torch.as_tensor(nets.MD_BINS)
        act[:third] = (torch.as_tensor(rs.rand(third, 8)) * bins).long()
        logp = lsm.gather(-1, act[..., None]).squeeze(-1).sum(-1)
    logits = nets.mlp(pol, obs).detach()
    assert 25 < logits.abs().max().item() <= 30.001
    acts = act.numpy().astype(np.float32)
    off = 0.3 * rs.randn(n)
    off[:third] = np.where(rs.rand(third) < 0.5, -0.5, 0.5)
    old = (logp.numpy() + off).astype(np.float32)
    tgt, adv = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    idx = rs.permutation(n)[:mb]
    for h, b in enumerate(nets.MD_BINS):
        assert set(np.unique(acts[idx, h]).astype(int)) == set(range(b)), h
    assert logp.numpy()[idx].min() < -50
    got = run_minibatch(L, "multidiscrete", pol, val, obs, acts, old, tgt, adv, idx, 0.2, 0.005, 0.5)
    gate_rows(L, "multidiscrete", pol, val, obs, acts, old, tgt, adv, idx, 0.5, got, label="multi-discrete, +-30 logits, 2999 rows")


@pytest.mark.parametrize("k,n", [(1, 700), (17, 513), (32, 300), (40, 611), (64, 333)])
def test_gaussian_act_widths(L, k, n):
    """rlppo_gaussian_act at several hundred ragged rows: actions == clamp(mean + sd * eps, -1, 1) of the float32 oracle, log-probs
    against float64 with the derived bound of fp64_gate.gauss_logp_check."""
    torch.manual_seed(200 + k)
    rs = np.random.RandomState(200 + k)
    pol = nets.init_mlp(D, (256, 256, 256), 2 * k)
    net = Net(L, pol)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    eps = rs.randn(n, k).astype(np.float32) * 2.0
    rows = net.pad(obs)
    act = torch.empty(n, k, device="cuda")
    logp = torch.empty(n, device="cuda")
    w = net.ws(n)
    m, b = nets.var_map(0.1, 1.0)
    epsd = dev(eps)
    check(L, L.rlppo_gaussian_act(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, P(epsd), m, b, P(act), P(logp),
                                  P(w), w.numel(), None))
    with torch.no_grad():
        mean, std = nets.gauss_out(pol, obs)
        oact, _ = nets.gauss_sample(mean, std, torch.as_tensor(eps))
    np.testing.assert_allclose(act.cpu().numpy(), oact.numpy(), rtol=1e-5, atol=2e-6)
    assert (np.abs(oact.numpy()) == 1.0).any()
    y = torch.empty(n, net.ld_out, device="cuda")
    check(L, L.rlppo_mlp_forward(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, 1, P(y), net.ld_out, P(w), w.numel(),
                                 None))
    fp64_gate.gauss_logp_check(pol, obs, eps, y, act, logp, label=f"k={k} n={n}")


def test_multidiscrete_act_at_scale(L):
    """rlppo_multidiscrete_act at 1000 rows against oracle/nets.py::md_sample with the same noise: indices exact except on near-ties
    (margin: the two candidates' p / q within 1e-4 relative, as test_seeded_rollout_draws_the_reference_noise_stream states it);
    log-probs within 1e-5."""
    torch.manual_seed(9)
    rs = np.random.RandomState(9)
    n = 1000
    pol = nets.init_mlp(D, (256, 256, 256), 21)
    net = Net(L, pol)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    q = nets.draw_exp_noise(n * 8, 3)
    rows = net.pad(obs)
    act = torch.empty(n, 8, dtype=torch.int64, device="cuda")
    logp = torch.empty(n, device="cuda")
    w = net.ws(n)
    qd = dev(q)
    check(L, L.rlppo_multidiscrete_act(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, P(qd), P(act), P(logp), P(w),
                                       w.numel(), None))
    with torch.no_grad():
        lsm, probs = nets.md_dist(pol, obs)
        oact, ologp = nets.md_sample(lsm, probs, q)
    a = act.cpu()
    score = (probs.reshape(n * 8, 3) / q).reshape(n, 8, 3)
    diff = (a != oact).nonzero()
    for r, h in diff.tolist():
        s = score[r, h]
        assert abs(s[a[r, h]] - s[oact[r, h]]) <= 1e-4 * s[oact[r, h]], "index mismatch that is not a near-tie"
    assert len(diff) <= 2
    same = (a == oact).all(1)
    assert same.sum() >= n - 2
    assert np.abs(logp.cpu().numpy()[same] - ologp.numpy()[same]).max() < 1e-5


# ------------------------------------------------------------------------------- 3. ring-resident minibatches
@pytest.mark.parametrize("head,k", [("discrete", 1), ("gaussian", 5), ("multidiscrete", 8)])
@pytest.mark.parametrize("k26", [0, 2], ids=["gather_pass", "fused_gather"])
def test_ring_resident_minibatch_is_bitwise_the_plain_one(L, head, k, k26):
    """The experience arrays as a ring (rlppo_minibatch_args.ring_base / ring_cap: logical row i at physical (i + base) mod cap):
    the same minibatch over the rotated arrays must give bit for bit the gradients of the plain arrays -- rows on both sides of the
    wrap, both gather forms (the separate gather pass, the row table fused into the first layer's launches)."""
    n, base = 5000, 3777
    pol, val, obs, acts, old, tgt, adv, rs = make_case(head, 40 + k, n, k)
    idx = rs.randint(0, n, 1300)
    idx[:4] = [n - base - 1, n - base, 0, n - 1]   # the last logical row before the wrap, the first after it
    wrapped = (idx + base) >= n
    assert 0.3 < wrapped.mean() < 0.9
    check(L, L.rlppo_dbg_set(26, k26))
    try:
        plain = run_minibatch(L, head, pol, val, obs, acts, old, tgt, adv, idx, 0.2, 0.005, 0.5)
        ring = run_minibatch(L, head, pol, val, obs, acts, old, tgt, adv, idx, 0.2, 0.005, 0.5, ring=base)
    finally:
        check(L, L.rlppo_dbg_set(26, 1))
    bit_equal(plain[0] + plain[1], ring[0] + ring[1], f"ring {head} 26={k26}")
    np.testing.assert_allclose(plain[2], ring[2], rtol=1e-12, atol=0)
    if k26 == 2:  # (one gate per head: the bit-equality above carries it to the other form)
        gate_rows(L, head, pol, val, obs, acts, old, tgt, adv, idx, 0.5, ring, label=f"{head} k={k}, ring-resident")


# ------------------------------------------------------------------------------- 6. the paired pass at its default size
@pytest.mark.parametrize("head", ["gaussian", "multidiscrete"])
def test_paired_pass_default_size_other_heads(L, head):
    """262,144 rows in one minibatch: the paired policy + critic launches and the fused gather engage by default (nothing forced).
    float64 truth on ALL rows, and additivity against four 65,536-row minibatches (mb_ratio 1/4 each), which run the unpaired forms
    -- the tolerances of test_fused_pass_full_size_cfg2."""
    n = 262144
    pol, val, obs, acts, old, tgt, adv, rs = make_case(head, 77, n, 8)
    idx = rs.permutation(n)
    c3, c4 = L.rlppo_dbg_counter(3), L.rlppo_dbg_counter(4)
    gp, gv, st = run_minibatch(L, head, pol, val, obs, acts, old, tgt, adv, idx, 0.2, 0.005, 1.0)
    assert L.rlppo_dbg_counter(3) == c3 + 1 and L.rlppo_dbg_counter(4) == c4 + 1
    acc = [[torch.zeros_like(w, dtype=torch.float64), torch.zeros_like(b, dtype=torch.float64)] for w, b in gp + gv]
    st_sum = np.zeros(5)
    for j in range(4):
        gpj, gvj, stj = run_minibatch(L, head, pol, val, obs, acts, old, tgt, adv, idx[j * 65536:(j + 1) * 65536], 0.2, 0.005, 0.25)
        for a, g in zip(acc, gpj + gvj):
            a[0] += g[0].double()
            a[1] += g[1].double()
        st_sum += stj[:5]
    assert L.rlppo_dbg_counter(3) == c3 + 1   # the quarters ran unpaired
    for whole, parts in zip(gp + gv, acc):
        for i in (0, 1):
            assert relerr(whole[i], parts[i]) < 1e-5
    np.testing.assert_allclose(st[:5], st_sum / 4, rtol=1e-5, atol=1e-8)
    gate_rows(L, head, pol, val, obs, acts, old, tgt, adv, idx, 1.0, (gp, gv, st), label=f"{head}, paired pass, 262,144 rows")


# ------------------------------------------------------------------------------- 4. learn() with 40 action dimensions
def test_learn_continuous_40_actions_matches_float64(L):
    """PPOLearner with a 40-dimensional ContinuousPolicy (80 outputs: above the 32 action dimensions the Gaussian loss kernel once
    capped) collects through its own sampler and learns; after every optimiser step its parameters are held against
    oracle/ppo.py::learn64 with the allowance of tests/test_gpu_learner.py::test_learn_matches_reference_fixture, the CPU float32
    oracle (oracle/ppo.py::learn, the reference's op sequence) standing in for the reference's own fixture."""
    from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner
    cfg = dict(d=64, k=40, layers=(48, 48), n=512, B=256, MB=128, epochs=2, seed=13, lr=3e-4, clip=0.2, ent=0.005)
    torch.manual_seed(cfg["seed"])
    np.random.seed(cfg["seed"])
    learner = PPOLearner(cfg["d"], cfg["k"], 2, cfg["layers"], cfg["layers"], (0.1, 1.0), cfg["B"], 1, cfg["lr"], cfg["lr"], cfg["clip"],
                         cfg["ent"], cfg["MB"], "cuda:0")
    pol0 = [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in learner.policy.arena.linears]
    val0 = [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in learner.value_net.arena.linears]
    rs = np.random.RandomState(cfg["seed"])
    n = cfg["n"]
    obs = np.clip(rs.randn(n, cfg["d"]), -5, 5).astype(np.float32)
    eps = rs.randn(n, cfg["k"]).astype(np.float32)
    act, logp = learner.policy.get_action(obs, noise=eps)
    act, logp = torch.as_tensor(act).reshape(n, cfg["k"]), torch.as_tensor(logp).reshape(n)
    with torch.no_grad():
        oact, ologp = nets.gauss_sample(*nets.gauss_out(pol0, obs), torch.as_tensor(eps))
    np.testing.assert_allclose(act.numpy(), oact.numpy(), rtol=1e-5, atol=2e-6)
    rews = rs.randn(n).astype(np.float32)
    dones = (rs.rand(n) < 0.02).astype(np.float32)
    trunc = np.zeros(n, np.float32)
    vals = rs.randn(n).astype(np.float32)
    adv = rs.randn(n).astype(np.float32)
    buf = ExperienceBuffer(n, cfg["seed"], "cpu")
    buf.submit_experience(obs, act.numpy(), logp.numpy(), rews, obs, dones, trunc, vals, adv)
    exp = dict(states=obs, actions=act.numpy(), log_probs=logp.numpy(), values=vals, advantages=adv)
    args = (cfg["B"], cfg["MB"], cfg["epochs"], cfg["clip"], cfg["ent"], cfg["lr"], cfg["lr"], np.random.RandomState(cfg["seed"]))
    truth, weakest, ref = {}, {}, {}
    flat = lambda p: np.concatenate([np.asarray(t, np.float64).ravel() for wb in p for t in wb])
    ppo.learn64("gaussian", pol0, val0, exp, *args, weakest=weakest,
                on_step=lambda i, p, v: truth.__setitem__(i, (flat(p), flat(v), weakest["pol"].copy(), weakest["val"].copy())))
    pol32 = [(w.clone(), b.clone()) for w, b in pol0]
    val32 = [(w.clone(), b.clone()) for w, b in val0]
    ppo.learn("gaussian", pol32, val32, {k: torch.as_tensor(v) for k, v in exp.items()}, *args[:7], np.random.RandomState(cfg["seed"]),
              on_step=lambda i, p, v: ref.__setitem__(i, (flat([(w.detach(), b.detach()) for w, b in p]),
                                                         flat([(w.detach(), b.detach()) for w, b in v]))))
    steps_per_epoch = n // cfg["B"]
    for e in range(cfg["epochs"]):
        learner.learn(buf)
        s = (e + 1) * steps_per_epoch - 1
        pv = torch.nn.utils.parameters_to_vector(learner.policy.parameters()).detach().cpu().numpy().astype(np.float64)
        vv = torch.nn.utils.parameters_to_vector(learner.value_net.parameters()).detach().cpu().numpy().astype(np.float64)
        tp, tv, wp, wv = truth[s]
        errs = {}
        for who, p_, v_ in (("hip", pv, vv), ("ref", *ref[s])):
            worst_good = frac_ill = 0.0
            for got, tr, weak in ((p_, tp, wp), (v_, tv, wv)):
                d = np.abs(got - tr)
                ill = weak < 1e-4
                worst_good = max(worst_good, float(d[~ill].max() / np.abs(tr).max()))
                if ill.any():
                    bound = (s + 1) * cfg["lr"] * np.minimum(1.0, 1e-5 / np.maximum(weak[ill], 1e-300))
                    frac_ill = max(frac_ill, float((d[ill] / bound).max()))
            errs[who] = (worst_good, frac_ill)
        print(f"[fp64 gate] learn() k=40 after optimiser step {s}: err(HIP, fp64)={errs['hip'][0]:.2e}  err(CPU fp32 oracle, fp64)="
              f"{errs['ref'][0]:.2e}  ill-conditioned: HIP {errs['hip'][1]:.3f} / oracle {errs['ref'][1]:.3f} of the derived bound")
        assert errs["hip"][0] <= max(1e-5, 1.5 * errs["ref"][0]), (s, errs)
        assert int((wp < 1e-4).sum() + (wv < 1e-4).sum()) <= 0.05 * (wp.size + wv.size)
        assert errs["hip"][1] <= 1.0 and errs["ref"][1] <= 1.0, (s, errs)


# ------------------------------------------------------------------------------- 7. wide discrete rows, masked and from probabilities
# The wave-per-row discrete kernels (csrc/heads.hip) hold 2 / 8 / 32 elements per lane for up to 128 / 512 / 2048 actions.  The widths
# here are both ends of the 8 and of the 32 class, for the three forms no other test launches above 128 actions: sampling from given
# probabilities, masked probabilities and the masked loss of the widest class.  5 rows = one block of 4 rows and a block with one.
WIDE = [129, 512, 513, 2048]


@pytest.mark.parametrize("A", WIDE)
def test_categorical_select_wide_rows(L, A):
    """tests/test_gpu_kernels.py::test_categorical_select_exact_at_scale above 128 categories: identical probabilities + identical
    noise => identical indices, log-probability = log of the chosen one."""
    torch.manual_seed(A)
    n = 5
    probs = torch.softmax(torch.randn(n, A) * 3, -1).clamp(1e-11, 1)
    q = torch.empty(n, A).exponential_(1)
    q[1, A - 1] = 1e-30   # the last column of a row wins: the row's last lane / element is a candidate
    ref = torch.argmax(probs / q, -1)
    act, lp = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, device="cuda")
    pd, qd = dev(probs), dev(q)
    check(L, L.rlppo_categorical_select(stream(), P(pd), A, n, A, P(qd), P(act), P(lp)))
    assert torch.equal(act.cpu(), ref) and int(act[1]) == A - 1
    assert torch.equal(lp, torch.log(pd.gather(1, act.view(-1, 1))).view(-1))


@pytest.mark.parametrize("A", WIDE)
def test_masked_discrete_probs_wide_rows(L, A):
    """rlppo_discrete_probs with an action mask above 128 actions, against the float64 masked softmax with the allowance of
    tests/test_gpu_action_mask.py::check_sampling: invalid actions read exactly 0 with and without the clamp, a row without a valid
    action is all-valid, and the flat arg-max is exact given the library's own probabilities (never an invalid action)."""
    import test_gpu_action_mask as M
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.util import action_mask as AM
    rs = np.random.RandomState(A)
    n, d = 5, 40
    params = [(torch.as_tensor(rs.randn(A, d).astype(np.float32)), torch.as_tensor(rs.randn(A).astype(np.float32) * 3))]
    net = Net(L, params)
    obs = rs.randn(n, d).astype(np.float32)
    m = M.rand_mask(rs, n, A)
    z = M.logits64(params, obs)
    m[np.arange(n), z.argmax(1)] = False   # every row's largest logit is masked out: the arg-max must not take it
    m[2] = False                           # no valid action: all-valid
    eff = m.copy()
    eff[~m.any(1)] = True
    rows, w = net.pad(obs), net.ws(n)
    words = AM.pack(torch.from_numpy(m).cuda(), A, "cuda")
    opts = N.ActOpts()
    opts.action_mask, opts.mask_words = words.data_ptr(), words.shape[1]
    soft, clamped = torch.full((n, A), float("nan"), device="cuda"), torch.full((n, A), float("nan"), device="cuda")
    best = torch.empty(1, dtype=torch.int64, device="cuda")
    check(L, L.rlppo_discrete_probs(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, 0, P(soft), A, None, P(w), w.numel(),
                                    ctypes.byref(opts)))
    check(L, L.rlppo_discrete_probs(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, 1, P(clamped), A, P(best), P(w),
                                    w.numel(), ctypes.byref(opts)))
    want = M.softmax64(z, eff)
    got = soft.cpu().numpy()
    assert np.isfinite(got).all() and (got[~eff] == 0.0).all() and (clamped.cpu().numpy()[~eff] == 0.0).all()
    err = np.abs(got - want)[eff].max() / want.max()
    print(f"[masked probs] A={A}: max|p - p64|/max p64 = {err:.2e}")
    assert err <= 1e-5, err
    valid = torch.from_numpy(eff).cuda()
    assert torch.equal(clamped, torch.where(valid, soft.clamp(min=1e-11, max=1), torch.zeros_like(soft)))
    assert int(best) == int(clamped.cpu().numpy().argmax()) and eff.reshape(-1)[int(best)]


@pytest.mark.parametrize("A", [513, 2048])
def test_masked_loss_widest_rows(L, A):
    """The masked discrete loss above 512 padded columns (32 elements per lane), which tests/test_gpu_action_mask.py reaches at 90 and
    200 actions only: 5 rows through rlppo_ppo_minibatch against that module's float64 gate.  Row 1 has no valid action (all-valid);
    row 3's stored action is masked out (the literal chain: pc = 1e-11, no gradient through the clamp); ratios on both sides of the
    clip interval and inside it."""
    import test_gpu_action_mask as M
    torch.manual_seed(A)
    rs = np.random.RandomState(A)
    n = 5
    pol, val = nets.init_mlp(D, (64,), A), nets.init_mlp(D, (64,), 1)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    m = M.rand_mask(rs, n, A)
    m[1] = False
    eff = m.copy()
    eff[1] = True
    acts = np.array([rs.choice(np.flatnonzero(r)) for r in eff], np.float32)
    m[3, int(acts[3])] = eff[3, int(acts[3])] = False
    p = np.clip(M.softmax64(M.logits64(pol, obs), eff), 1e-11, 1.0)
    logp = np.log(p[np.arange(n), acts.astype(int)])
    assert p[3, int(acts[3])] == 1e-11
    old = (logp - np.array([0.05, -0.3, 0.3, -0.05, 0.1])).astype(np.float32)
    pr = dict(obs=obs, mask=m, acts=acts, old=old, adv=rs.randn(n).astype(np.float32), tgt=rs.randn(n).astype(np.float32), redrawn=0,
              outside=0.4)
    rows, kw = M.rows_of(dict(pr, mask=torch.from_numpy(m).cuda()))
    got = triple(run_pass(L, pol, val, *rows, np.array([4, 0, 3, 1, 2]), **kw))
    PY.masked_gate(L, "discrete", pol, val, dict(pr, mask=eff), got, f"[masked fp64 gate] {D} -> (64,) -> {A}, 5 rows")


# ------------------------------------------------------------------ 5. one act_padded: the eager call, its launcher, the graph
@pytest.mark.parametrize("head", ["discrete", "multidiscrete", "gaussian"])
def test_act_padded_is_the_heads_act_launch_and_the_graph_replays_it(head):
    """ArenaModule.act_padded is the head's _act_launch on buffers of its own: the same call made by hand on the same rows, noise and
    mask words gives the same bits, and so does get_action on the same host batch through ActGraph.  17 rows (one ragged
    bucket of the graph), a 2 x 64 body; the masking heads also under a mask with rows whose heads keep exactly one bin."""
    from rlgym_ppo_amd.ppo.continuous_policy import ContinuousPolicy
    from rlgym_ppo_amd.ppo.discrete_policy import DiscreteFF
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF
    torch.manual_seed(31)
    rs = np.random.RandomState(31)
    n, d, bins = 17, 23, (2, 7, 3, 11, 2)
    pol = {"discrete": lambda: DiscreteFF(d, 33, (64, 64), "cuda:0"),
           "multidiscrete": lambda: MultiDiscreteFF(d, (64, 64), "cuda:0", bins=bins),
           "gaussian": lambda: ContinuousPolicy(d, 6, (64, 64), "cuda:0")}[head]()
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    rows = pol.arena.stage_obs(obs)
    q = pol._draw_noise(n).clone()
    assert tuple(q.shape) == tuple(pol._noise_shape(n))
    masks, lay = [None], pol.mask_layout
    assert (lay is None) == (head == "gaussian")
    single = [3, 11]
    if lay is not None:
        segs = [(0, lay.width)] if lay.heads is None else [(int(s), int(s) + b) for s, b in zip(lay.starts, lay.heads)]
        m = rs.rand(n, lay.width) < 0.5
        for lo, hi in segs:
            m[np.arange(n), rs.randint(lo, hi, n)] = True
        m[single] = False
        only = [hi - 1 for _, hi in segs]
        m[np.ix_(single, only)] = True        # exactly one valid bin (the last) in every head of these rows
        masks.append(m)
    bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t
    for m in masks:
        a0, l0 = pol.act_padded(rows, noise=q, action_mask=m)
        a1, l1 = pol._action_buffer(n, "cuda:0").fill_(-7), torch.full((n,), -7.0, device="cuda:0")
        assert a1.dtype == a0.dtype and a1.shape == a0.shape
        words = None if m is None else lay.pack(m, "cuda:0")
        pol._act_launch(rows, n, q.cuda(), a1, l1, pol.arena.forward_ws(n), None, words)
        assert torch.equal(bits(a0), bits(a1)) and torch.equal(bits(l0), bits(l1)), (head, m is not None)
        calls = sum(g.calls for g in pol._graphs.values())
        a2, l2 = pol.get_action(obs, noise=q, action_mask=m) if m is not None else pol.get_action(obs, noise=q)
        key = 32 if m is None else (32, True)
        assert key in pol._graphs and sum(g.calls for g in pol._graphs.values()) == calls + 1   # the graph served it
        assert torch.equal(bits(a0.cpu()), bits(a2)) and torch.equal(bits(l0.cpu()), bits(l2)), (head, m is not None)
        assert torch.isfinite(l0).all()
        if m is not None:
            a = a0.cpu().numpy().reshape(n, -1)
            off = np.array([lo for lo, _ in segs])
            assert m[np.arange(n)[:, None], a + off].all()                                       # valid actions only
            assert np.array_equal((a + off)[single], np.tile(only, (2, 1))) and (l0.cpu().numpy()[single] == 0).all()
