"""Pins oracle/nets.py and oracle/ppo.py to the reference through fixtures G1, G2, G4, G5, G9 (all produced by
importing the reference, tests/golden/make_golden.py).  On CPU the fp32 autograd form runs the same ATen ops
in the same order as the reference, so these checks are tight; the float64 analytic form (the gradient
formulas the HIP kernels implement) is held to 1e-5 relative."""
import json

import numpy as np
import pytest
import torch

from oracle import nets, ppo

torch.set_num_threads(1)


def T(x):
    return torch.as_tensor(np.asarray(x))


_HOST = {}


def fixture_host():
    """True when this CPU's ATen kernels reproduce the fixtures bit for bit (the build container, where they were generated)."""
    if "same" not in _HOST:
        from conftest import load_golden
        g = load_golden("g1_discrete_forward")
        ok = torch.equal(nets.discrete_probs(nets.params_from_state(g, "p."), g["obs"]), T(g["probs"]))
        for name, head, acts_key in (("g4_discrete_loss", "discrete", "acts"), ("g9_continuous", "gaussian", "act")):
            g = load_golden(name)
            acts = T(g[acts_key]).view(-1) if head == "discrete" else T(g[acts_key])
            r = ppo.minibatch_autograd(head, nets.params_from_state(g, "p."), nets.params_from_state(g, "v."), T(g["obs"]), acts,
                                       T(g["old_logp"]), T(g["adv"]), T(g["targets"]), float(g["clip"]), float(g["ent_coef"]),
                                       float(g["mb_ratio"]))
            ok = ok and torch.equal(r["logp"], T(g["out.logp"])) and r["kl"] == float(g["out.kl"])
        _HOST["same"] = bool(ok)
    return _HOST["same"]


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def same(a, b, tol=3e-6):
    """Bit-exact on the CPU family that produced the fixtures (the build container: the restatement runs the same ATen ops in
    the same order as the reference); ATen picks CPU-specific GEMM / vector-math kernels, so on another host (e.g. the GPU box's
    EPYC) the same ops round differently in the last bit: there float32 rounding accuracy is required instead.  Integer outputs
    (action indices) are always compared exactly by the callers."""
    a, b = torch.as_tensor(np.asarray(a)), torch.as_tensor(np.asarray(b))
    if a.shape != b.shape:
        return False
    if torch.equal(a, b):
        return True
    if not a.is_floating_point():
        return False
    d = (a.double() - b.double()).abs()
    return bool((d <= tol * b.double().abs().max().clamp_min(1e-30) + tol * b.double().abs()).all())


def test_g1_discrete_forward_and_sampling(golden):
    g = golden("g1_discrete_forward")
    pol = nets.params_from_state(g, "p.")
    probs = nets.discrete_probs(pol, g["obs"])
    assert same(probs, g["probs"])
    act, logp = nets.discrete_sample(probs, T(g["q"]))
    assert torch.equal(act, T(g["actions"]))          # bit-exact action indices
    assert same(logp, g["logp"])
    assert int(probs.numpy().argmax()) == int(g["det_action"])  # quirk Q11: flat argmax


def test_g2_value_forward(golden):
    g = golden("g2_value_forward")
    val = nets.params_from_state(g, "v.")
    assert same(nets.value_forward(val, g["obs"]), g["values"])
    assert same(nets.value_forward(val, g["obs"].astype(np.float64)), g["values_from_f64"])


def _check_minibatch(g, head, acts):
    pol, val = nets.params_from_state(g, "p."), nets.params_from_state(g, "v.")
    args = (head, pol, val, T(g["obs"]), acts, T(g["old_logp"]), T(g["adv"]), T(g["targets"]),
            float(g["clip"]), float(g["ent_coef"]), float(g["mb_ratio"]))
    r = ppo.minibatch_autograd(*args)
    assert same(r["logp"], g["out.logp"])
    assert same(r["vals"], g["out.vals"])
    if fixture_host():
        for key in ("entropy", "kl", "clip_fraction", "policy_loss", "value_loss"):
            assert r[key] == float(g["out." + key]), key
    else:  # another CPU: last-bit differences, and the fixture's rows ENGINEERED onto a clip edge may fall the other way
        for key in ("entropy", "value_loss"):
            assert abs(r[key] - float(g["out." + key])) <= 3e-6 * max(abs(float(g["out." + key])), 1e-3), key
    for i, (gw, gb) in enumerate(r["grad_policy"]):
        if not fixture_host() and head == "discrete":
            break  # (edge rows: see above; tests/test_gpu_kernels.py::test_g4... resolves them against float64)
        assert same(gw, g[f"gp.model.{2 * i}.weight"], 1e-5) and same(gb, g[f"gp.model.{2 * i}.bias"], 1e-5)
    for i, (gw, gb) in enumerate(r["grad_value"]):
        assert same(gw, g[f"gv.model.{2 * i}.weight"], 1e-5) and same(gb, g[f"gv.model.{2 * i}.bias"], 1e-5)
    # float64 analytic form vs fp32 autograd.  Rows whose ratio sits exactly on a clip edge are decided by the
    # last fp32 bit, so for THIS comparison they are moved off the edge (both forms see the same moved input).
    old = T(g["old_logp"]).clone()
    edge = np.isclose(np.abs(np.asarray(g["out.ratio"]) - 1.0), float(g["clip"]), rtol=0, atol=1e-4)
    old[torch.as_tensor(edge)] += 0.05
    args = args[:5] + (old,) + args[6:]
    r2 = ppo.minibatch_autograd(*args)
    a = ppo.minibatch_analytic(*args)
    for key in ("entropy", "kl", "clip_fraction", "policy_loss", "value_loss"):
        assert abs(a[key] - r2[key]) <= 1e-5 * max(abs(r2[key]), 1e-3), (key, a[key], r2[key])
    assert relerr(a["logp"], r2["logp"]) < 1e-5
    for (aw, ab), (gw, gb) in zip(a["grad_policy"] + a["grad_value"], r2["grad_policy"] + r2["grad_value"]):
        assert relerr(aw, gw) < 2e-5 and relerr(ab, gb) < 2e-5, (relerr(aw, gw), relerr(ab, gb))
    return r


def test_g4_discrete_loss_and_grads(golden):
    g = golden("g4_discrete_loss")
    # the fixture really exercises the special regions
    assert (g["probs"] == np.float32(1e-11)).sum() > 50
    chosen = g["probs"][np.arange(96), g["acts"].astype(np.int64).ravel()]
    assert (chosen[:8] == np.float32(1e-11)).all()
    ratio = g["out.ratio"]
    assert (ratio[72:] == 1.0).all() and (ratio[8:24] < 0.79).all() and (ratio[24:40] > 1.21).all()
    _check_minibatch(g, "discrete", T(g["acts"]))


def test_g9_gaussian_head(golden):
    g = golden("g9_continuous")
    pol = nets.params_from_state(g, "p.")
    mean, std = nets.gauss_out(pol, g["obs"])
    assert same(mean, g["mean"]) and same(std, g["std"])
    act, logp = nets.gauss_sample(mean, std, T(g["eps"]))
    assert same(act, g["act"]) and same(logp, g["logp"], 2e-5)
    assert (np.abs(g["act"]) == 1.0).any()  # quirk Q9 exercised: some samples were clamped
    assert same(mean, g["det"])
    _check_minibatch(g, "gaussian", T(g["act"]))


def test_g9_multidiscrete_head(golden):
    g = golden("g9_multidiscrete")
    pol = nets.params_from_state(g, "p.")
    assert same(nets.mlp(pol, g["obs"]), g["logits"])
    lsm, probs = nets.md_dist(pol, g["obs"])
    act, logp = nets.md_sample(lsm, probs, T(g["q"]))
    assert torch.equal(act, T(g["act"]))
    np.testing.assert_allclose(logp.numpy(), g["logp"], rtol=1e-6, atol=1e-6)
    assert torch.equal(nets.md_deterministic(pol, g["obs"]), T(g["det"]))
    pol_, val_ = pol, nets.params_from_state(g, "v.")
    r = ppo.minibatch_autograd("multidiscrete", pol_, val_, T(g["obs"]), T(g["act"]), T(g["old_logp"]), T(g["adv"]),
                               T(g["targets"]), float(g["clip"]), float(g["ent_coef"]), float(g["mb_ratio"]))
    # torch.distributions normalises with logsumexp internally; the restatement matches to rounding, not bitwise
    np.testing.assert_allclose(r["logp"].numpy(), g["out.logp"], rtol=1e-6, atol=1e-6)
    for key in ("entropy", "kl", "policy_loss", "value_loss"):
        assert abs(r[key] - float(g["out." + key])) <= 2e-6 * max(1.0, abs(float(g["out." + key]))), key
    for i, (gw, gb) in enumerate(r["grad_policy"]):
        assert relerr(gw, g[f"gp.model.{2 * i}.weight"]) < 1e-5 and relerr(gb, g[f"gp.model.{2 * i}.bias"]) < 1e-5
    a = ppo.minibatch_analytic("multidiscrete", pol_, val_, T(g["obs"]), T(g["act"]), T(g["old_logp"]), T(g["adv"]),
                               T(g["targets"]), float(g["clip"]), float(g["ent_coef"]), float(g["mb_ratio"]))
    for (aw, ab), (gw, gb) in zip(a["grad_policy"], r["grad_policy"]):
        assert relerr(aw, gw) < 2e-5 and relerr(ab, gb) < 2e-5


@pytest.mark.parametrize("name", ["g5_learn_discrete", "g9_learn_continuous", "g9_learn_multidiscrete"])
def test_full_learn_matches_reference(golden, name):
    g = golden(name)
    cfg = json.loads(str(g["cfg"]))
    head = nets.HEADS[cfg["policy_type"]]
    pol, val = nets.params_from_state(g, "p0."), nets.params_from_state(g, "v0.")
    buf = {k: T(g["exp." + k]) for k in ("states", "actions", "log_probs", "values", "advantages")}
    snaps = {}

    def on_step(i, p, v):
        snaps[i] = (nets.flatten(p).clone(), nets.flatten(v).clone())

    rng = np.random.RandomState(cfg["seed"])
    report, ap, av = ppo.learn(head, pol, val, buf, cfg["B"], cfg["MB"], cfg["epochs"], cfg["clip"], cfg["ent"],
                               cfg["lr"], cfg["lr"], rng, on_step=on_step)
    n_steps = int(g["n_steps"])
    assert len(snaps) == n_steps == cfg["epochs"] * (cfg["n"] // cfg["B"])
    # (2e-6 on the fixture host; Adam's lr * m / (sqrt(v) + 1e-8) turns last-bit gradient differences of another CPU's kernels into
    # up to ~1e-5 at the few parameters whose gradient is ~0: tests/test_gpu_learner.py measures that against float64)
    for i in range(n_steps):
        assert relerr(snaps[i][0], g[f"step{i}.policy"]) < 2e-5, i
        assert relerr(snaps[i][1], g[f"step{i}.value"]) < 2e-5, i
    for k, v in report.items():
        ref = float(g["report." + k])
        assert abs(v - ref) <= 1e-5 * max(abs(ref), 1e-6) + 1e-9, (k, v, ref)
    assert ap.step == float(g["adam_step"])
    assert relerr(ap.m[0][0], g["adam_exp_avg0"]) < 1e-5 and relerr(ap.v[0][0], g["adam_exp_avg_sq0"]) < 1e-5


def test_init_consumes_rng_like_the_reference(golden):
    # PPOLearner.__init__ builds policy then critic with nn.Linear defaults (ppo_learner.py:34-53); G5 used seed 123
    g = golden("g5_learn_discrete")
    torch.manual_seed(123)
    pol = nets.init_mlp(107, (32, 32), 90)
    val = nets.init_mlp(107, (32, 32), 1)
    for (w, b), (rw, rb) in zip(pol, nets.params_from_state(g, "p0.")):
        assert torch.equal(w, rw) and torch.equal(b, rb)
    for (w, b), (rw, rb) in zip(val, nets.params_from_state(g, "v0.")):
        assert torch.equal(w, rw) and torch.equal(b, rb)


def _analytic_vs_autograd(head, pol, val, obs, acts, old, adv, tgt, var_range):
    """minibatch_analytic against minibatch_autograd run on float64 tensors: the same ATen op sequence, differentiated by autograd, at
    the precision of the hand-derived formulas -- so a wrong term shows at its own size, not hidden under float32 rounding (the
    four-term Gaussian log-density at sd = 0.05 loses ~1e-5 of its ratio in float32 alone).  Tolerance 1e-9, far inside the 2e-5 of
    the fixture checks."""
    D64 = lambda t: torch.as_tensor(np.asarray(t), dtype=torch.float64)
    p64 = lambda ps: [(w.double(), b.double()) for w, b in ps]
    args = (head, p64(pol), p64(val), D64(obs), D64(acts), D64(old), D64(adv), D64(tgt), 0.2, 0.005, 0.5, var_range)
    r = ppo.minibatch_autograd(*args)
    a = ppo.minibatch_analytic(*args)
    for key in ("entropy", "kl", "policy_loss", "value_loss"):
        assert abs(a[key] - r[key]) <= 1e-9 * max(abs(r[key]), 1e-3), (key, a[key], r[key])
    assert abs(a["clip_fraction"] - r["clip_fraction"]) < 1e-7  # (the reference's mean of a .float() mask: a float32 number)
    assert relerr(a["logp"], r["logp"]) < 1e-9
    for (aw, ab), (gw, gb) in zip(a["grad_policy"] + a["grad_value"], r["grad_policy"] + r["grad_value"]):
        assert relerr(aw, gw) < 1e-9 and relerr(ab, gb) < 1e-9, (relerr(aw, gw), relerr(ab, gb))
    return r


@pytest.mark.parametrize("k", [1, 3, 40])
def test_analytic_gaussian_widths_var_range_and_saturated_sd(k):
    """The float64 hand-derived Gaussian gradients (the GPU gates' yardstick) against autograd at widths the fixtures never had, a
    non-default var range, sd units whose tanh is saturated (sd == var_min exactly, 1 - y^2 == 0) on every row, clamped actions
    and ratios beyond both clip edges."""
    torch.manual_seed(k)
    rs = np.random.RandomState(k)
    n, d, var = 300, 24, (0.05, 2.0)
    pol, val = nets.init_mlp(d, (32, 32), 2 * k), nets.init_mlp(d, (32,), 1)
    w, b = pol[-1]
    b = b.clone()
    b[k] = -30.0
    pol = pol[:-1] + [(w, b)]
    obs = rs.randn(n, d).astype(np.float32)
    with torch.no_grad():
        assert (nets.mlp(pol, obs, out_act="tanh")[:, k] == -1.0).all()
        mean, std = nets.gauss_out(pol, obs, *var)
        eps = rs.randn(n, k).astype(np.float32) * 3
        eps[: n // 10] *= 10
        act, logp = nets.gauss_sample(mean, std, T(eps))
    assert (act.abs() == 1.0).any()
    old = (logp.numpy() + 0.3 * rs.randn(n)).astype(np.float32)
    r = _analytic_vs_autograd("gaussian", pol, val, obs, act.numpy(), old, rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32),
                              var)
    ratio = np.exp(r["logp"].numpy().astype(np.float64) - old)
    assert (ratio < 0.8).any() and (ratio > 1.2).any()


def test_analytic_multidiscrete_saturated_logits():
    """... and the multi-discrete gradients with logits scaled to +-30 (near one-hot heads) and actions of tiny probability."""
    torch.manual_seed(2)
    rs = np.random.RandomState(2)
    n, d = 300, 24
    pol, val = nets.init_mlp(d, (32, 32), 21), nets.init_mlp(d, (32,), 1)
    obs = rs.randn(n, d).astype(np.float32)
    with torch.no_grad():
        s = 30.0 / nets.mlp(pol, obs).abs().max().item()
        pol = pol[:-1] + [(pol[-1][0] * s, pol[-1][1] * s)]
        lsm, _ = nets.md_dist(pol, obs)
        act = (T(rs.rand(n, 8)) * T(np.array(nets.MD_BINS))).long()
        logp = lsm.gather(-1, act[..., None]).squeeze(-1).sum(-1)
    assert logp.min() < -50
    old = (logp.numpy() + np.where(rs.rand(n) < 0.5, -0.5, 0.5)).astype(np.float32)
    _analytic_vs_autograd("multidiscrete", pol, val, obs, act.numpy().astype(np.float32), old, rs.randn(n).astype(np.float32),
                          rs.randn(n).astype(np.float32), (0.1, 1.0))
