"""The options beyond the reference (PPOLearner: normalize_advantages, value_clip_range, target_kl, max_grad_norm) on the device:
off is off bit for bit, the normalised surrogate and the clipped value loss against float64 truth (tests/fp64_gate.py: the HIP's
own ReLU decisions, no row excluded), the target-KL stop (never, always, after s steps; one and several virtual ranks), every
update precision, and the Learner loop with all options on."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_gate  # noqa: E402
import synthetic_env  # noqa: E402

D, HID = 107, (128, 128)
TYPE = {"discrete": 0, "multidiscrete": 1, "gaussian": 2}


@pytest.fixture(scope="module")
def L():
    from rlgym_ppo_amd import _native as N
    return N.lib()


def knob(L, key, value):
    assert L.rlppo_dbg_set(key, value) == 0


def build(head="discrete", B=2048, MB=1024, epochs=2, seed=5, lr=3e-4, k=8, **opts):
    from rlgym_ppo_amd.ppo import PPOLearner
    torch.manual_seed(seed)
    act = {"discrete": 90, "gaussian": k, "multidiscrete": 8}[head]
    return PPOLearner(D, act, TYPE[head], HID, HID, (0.1, 1.0), B, epochs, lr, lr, 0.2, 0.005, MB, "cuda:0", **opts)


def make_exp(learner, head, n, seed, adv=None, tgt=None):
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    act, logp = learner.policy.get_action(obs)
    act = np.asarray(torch.as_tensor(act).cpu(), np.float32)
    act = act.reshape(n) if head == "discrete" else act.reshape(n, -1)
    old = (np.asarray(torch.as_tensor(logp).cpu(), np.float32).reshape(n) + 0.1 * rs.randn(n)).astype(np.float32)
    tgt = rs.randn(n).astype(np.float32) if tgt is None else tgt
    adv = rs.randn(n).astype(np.float32) if adv is None else adv
    z = np.zeros(n, np.float32)
    return (obs, act, old, z, obs, z, z, tgt, adv)


def buffer(exp, seed=9):
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    buf = ExperienceBuffer(exp[0].shape[0], seed, "cpu")
    buf.submit_experience(*exp)
    return buf


def params(net):
    return [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in net.arena.linears]


def split(flat, ps):
    out, o = [], 0
    for w, b in ps:
        gw = flat[o:o + w.numel()].view(w.shape)
        o += w.numel()
        out.append((gw, flat[o:o + b.numel()]))
        o += b.numel()
    return out, o


def state(learner):
    torch.cuda.synchronize()
    po, vo = learner.policy_optimizer, learner.value_optimizer
    return [t.detach().clone() for t in (learner.policy.arena.flat, learner.value_net.arena.flat, po.exp_avg, po.exp_avg_sq, vo.exp_avg,
                                         vo.exp_avg_sq)] + [po.step_count, vo.step_count, learner.cumulative_model_updates]


def same_state(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), (what, i)


def same_report(a, b, what, skip=()):
    keys = set(a) - {"PPO Batch Consumption Time"} - set(skip)
    assert keys == set(b) - {"PPO Batch Consumption Time"} - set(skip), what
    for k in keys:
        assert a[k] == b[k], (what, k, a[k], b[k])


def first_gradient(learner, buf):
    got = []
    learner.grad_probe = lambda g: got.append(g.detach().clone()) if not got else None
    report = learner.learn(buf)
    learner.grad_probe = None
    return got[0].cpu(), report


# ------------------------------------------------------------------------------------------------------- off is off
@pytest.mark.parametrize("paired", [1, 2])
def test_options_off_is_off(L, paired):
    """The four arguments at their off values give, bit for bit, the learner built without them: parameters, Adam moments and step
    counts, report -- at a fused size (default launch selection) and in the paired pass (rlppo_dbg_set(29, 2))."""
    knob(L, 29, paired)
    try:
        out = []
        for opts in ({}, dict(normalize_advantages=False, value_clip_range=None, target_kl=None, max_grad_norm=0.5)):
            learner = build(**opts)
            exp = make_exp(learner, "discrete", 4096, 1)
            report = learner.learn(buffer(exp))
            out.append((state(learner), report))
    finally:
        knob(L, 29, 1)
    same_state(out[0][0], out[1][0], "off is off")
    same_report(out[0][1], out[1][1], "off is off")
    assert out[0][0][6] == 4 and "PPO Optimizer Steps" not in out[1][1]


def test_invalid_options_raise(L):
    learner = build(epochs=1)
    buf = buffer(make_exp(learner, "discrete", 2048, 2))
    for attr, bad in (("value_clip_range", 0.0), ("target_kl", -1.0), ("max_grad_norm", 0.0), ("max_grad_norm", float("nan"))):
        good = getattr(learner, attr)
        setattr(learner, attr, bad)
        with pytest.raises(ValueError):
            learner.learn(buf)
        setattr(learner, attr, good)
    learner.target_kl, learner.fused_optimizer_step = 0.01, False
    with pytest.raises(ValueError, match="target_kl"):
        learner.learn(buf)
    learner.target_kl = None
    learner.learn(buf)       # the FusedAdam.step form still takes every other option
    assert learner.cumulative_model_updates == 1


# ---------------------------------------------------------------------------------------------------- normalisation
def norm_adv64(adv):
    a = np.asarray(adv, np.float64)
    return (a - a.mean()) / (a.std(ddof=1) + 1e-8)


CASES = [(h, f, p) for h in ("discrete", "gaussian", "multidiscrete") for f, p in ((1, 0), (8, 2))] + [("discrete", 8, 0), ("discrete", 1, 2)]


@pytest.mark.parametrize("head,fuse,paired", CASES)
def test_normalised_surrogate_gradient_matches_float64(L, head, fuse, paired):
    """The first optimiser step's gradient with normalize_advantages: the surrogate of (A - mean) / (std + 1e-8) over the step's
    batch (all 4,096 rows: the permutation only orders the sum), the value loss on the raw data; float64 truth under the HIP's own
    ReLU decisions, err <= max(1e-5, 1.5 x err(CPU float32))."""
    n = 4096
    knob(L, 29, paired)
    try:
        learner = build(head, B=n, MB=1024, epochs=1, normalize_advantages=True)
        learner.max_fused_minibatches = fuse
        pol, val = params(learner.policy), params(learner.value_net)
        obs, act, old, _, _, _, _, tgt, adv = exp = make_exp(learner, head, n, 3, adv=(2.0 + 3.0 * np.random.RandomState(4).randn(n)).astype(np.float32))
        c0 = int(L.rlppo_dbg_counter(3))
        g, report = first_gradient(learner, buffer(exp))
        assert (int(L.rlppo_dbg_counter(3)) > c0) == (paired == 2)   # paired policy + critic launches ran / did not
    finally:
        knob(L, 29, 1)
    gp, o = split(g, pol)
    gv, _ = split(g[o:], val)
    fp64_gate.gate(L, head, pol, val, obs, act, old, norm_adv64(adv), tgt, 0.2, 0.005, 1.0, (gp, gv, None),
                   label=f"normalised advantages, {head}, RLPPO_FUSE={fuse}, dbg29={paired}")
    assert np.isfinite(report["Mean KL Divergence"])


def test_constant_batch_normalises_to_zero_and_ranks_agree(L):
    """A batch of equal advantages normalises to exactly 0: its policy gradient is, bit for bit, that of an all-zero batch with
    normalisation off.  2 and 4 virtual ranks (each computing the batch statistics locally) give the one-rank gradient up to
    summation order, and their replicas stay bit-identical."""
    from rlgym_ppo_amd import dp
    n = 4096
    grads = []
    for norm, a in ((True, 0.7), (False, 0.0)):
        learner = build(B=n, MB=1024, epochs=1, normalize_advantages=norm)
        exp = make_exp(learner, "discrete", n, 6, adv=np.full(n, a, np.float32))
        grads.append(first_gradient(learner, buffer(exp))[0])
    n_pol = learner.policy.arena.n_flat
    assert torch.equal(grads[0][:n_pol], grads[1][:n_pol])

    one = build(B=n, MB=512, epochs=1, normalize_advantages=True)
    exp = make_exp(one, "discrete", n, 7)
    g1, _ = first_gradient(one, buffer(exp))
    for world in (2, 4):
        reps = [build(B=n, MB=512, epochs=1, normalize_advantages=True) for _ in range(world)]
        got = []
        reps[0].grad_probe = lambda g: got.append(g.detach().cpu().clone())
        dp.run_virtual_ranks(reps, [buffer(exp) for _ in range(world)])
        assert fp64_gate._rel(got[0][:n_pol], g1[:n_pol]) < 1e-5 and fp64_gate._rel(got[0][n_pol:], g1[n_pol:]) < 1e-5, world
        for r in reps[1:]:
            same_state(state(r)[:6], state(reps[0])[:6], f"{world} replicas")


# ----------------------------------------------------------------------------------------------------- value clipping
def critic_grad64(val, obs, v_old, tgt, c, masks):
    """float64 gradient and loss of mean((v_old + clamp(v - v_old, -c, c) - tgt)^2) under imposed ReLU masks."""
    f = lambda t: np.asarray(t, np.float64)
    h, acts = f(obs), []
    for l, (w, b) in enumerate(val):
        acts.append(h)
        h = h @ f(w).T + f(b)
        if l + 1 < len(val):
            h = h * masks[l]
    v = h[:, 0]
    dv = v - v_old
    d = v_old + np.clip(dv, -c, c) - tgt
    n = len(v)
    gout = (2.0 * d / n * (np.abs(dv) <= c))[:, None]
    grads = [None] * len(val)
    for l in range(len(val) - 1, -1, -1):
        grads[l] = (gout.T @ acts[l], gout.sum(0))
        if l:
            gout = (gout @ f(val[l][0])) * masks[l - 1]
    return grads, float((d * d).mean()), float((np.abs(dv) > c).mean())


def critic_grad32(val, obs, v_old, tgt, c):
    ps = [(w.clone().requires_grad_(True), b.clone().requires_grad_(True)) for w, b in val]
    h = torch.as_tensor(obs)
    for l, (w, b) in enumerate(ps):
        h = torch.nn.functional.linear(h, w, b)
        if l + 1 < len(ps):
            h = torch.relu(h)
    vo = torch.as_tensor(v_old)
    v_pred = vo + torch.clamp(h.view(-1) - vo, -c, c)
    torch.nn.functional.mse_loss(v_pred, torch.as_tensor(tgt)).backward()
    return [(w.grad, b.grad) for w, b in ps]


@pytest.mark.parametrize("paired", [0, 2])
def test_clipped_value_loss_matches_float64(L, paired):
    """value_clip_range: v_old = fl32(target - A), about half of the rows outside the band; the critic's gradient and the reported
    "Value Function Loss" against float64 truth (the HIP's ReLU decisions), in both pass forms."""
    n, c = 4096, 0.05
    knob(L, 29, paired)
    try:
        learner = build(B=n, MB=1024, epochs=1, value_clip_range=c)
        val = params(learner.value_net)
        rs = np.random.RandomState(8)
        obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
        with torch.no_grad():
            h = torch.as_tensor(obs)
            for l, (w, b) in enumerate(val):
                h = torch.nn.functional.linear(h, w, b)
                h = torch.relu(h) if l + 1 < len(val) else h
        v0 = h.view(-1).numpy()
        tgt = rs.randn(n).astype(np.float32)
        adv = (tgt - (v0 + 0.07 * rs.randn(n))).astype(np.float32)      # v_old = v + N(0, 0.07): |v - v_old| > 0.05 for ~48 %
        exp = list(make_exp(learner, "discrete", n, 8, adv=adv, tgt=tgt))
        exp[0] = exp[4] = obs
        c0 = int(L.rlppo_dbg_counter(3))
        g, report = first_gradient(learner, buffer(tuple(exp)))
        assert (int(L.rlppo_dbg_counter(3)) > c0) == (paired == 2)
    finally:
        knob(L, 29, 1)
    v_old = (tgt - adv).astype(np.float32).astype(np.float64)
    masks = fp64_gate.hip_masks(L, val, obs)
    truth, loss64, outside = critic_grad64(val, obs, v_old, tgt, c, masks)
    assert 0.3 <= outside <= 0.7, outside
    gv, _ = split(g[learner.policy.arena.n_flat:], val)
    cpu = critic_grad32(val, obs, v_old.astype(np.float32), tgt, c)
    cpu_truth, _, _ = critic_grad64(val, obs, v_old, tgt, c, fp64_gate.cpu_masks(val, obs))
    e_hip, e_cpu = fp64_gate.grads_err(gv, truth), fp64_gate.grads_err(cpu, cpu_truth)
    print(f"[fp64 gate] clipped value loss, dbg29={paired}: err(HIP)={e_hip:.2e} err(CPU fp32)={e_cpu:.2e}, {outside:.0%} outside")
    assert e_hip <= max(1e-5, 1.5 * e_cpu), (e_hip, e_cpu)
    assert abs(report["Value Function Loss"] - loss64) <= 1e-5 * abs(loss64), (report["Value Function Loss"], loss64)


# ---------------------------------------------------------------------------------------------------------- target KL
def batch_kl(learner, slots):
    from rlgym_ppo_amd import _native as N
    stride = int(N.lib().rlppo_kl_slots_doubles(learner._fused_rows))
    tot = 0.0
    for p in range(len(slots) // stride):
        r = slots[p * stride:(p + 1) * stride]
        if r[0] > 0:
            tot += r[1] * r[2:2 + int(r[0])].sum()
    return tot


def test_target_kl_never_triggered_is_off(L):
    out = []
    for opts in ({}, dict(target_kl=1e9)):
        learner = build(**opts)
        report = learner.learn(buffer(make_exp(learner, "discrete", 4096, 11)))
        out.append((state(learner), report))
    same_state(out[0][0], out[1][0], "target_kl that never triggers")
    same_report(out[0][1], out[1][1], "target_kl that never triggers", skip=("PPO Optimizer Steps", "KL Early Stopped"))
    assert out[1][1]["PPO Optimizer Steps"] == 4 and out[1][1]["KL Early Stopped"] == 0.0


@pytest.mark.parametrize("one_launch", [True, False])
def test_target_kl_always_triggered_applies_nothing(L, one_launch):
    """A tiny target_kl stops at the first batch: nothing applied (parameters, moments, step counts, "Cumulative Model Updates"), the
    report's KL is the first batch's, the shuffle generator is where a full learn() leaves it.  Both optimiser forms."""
    n = 4096
    ref = build(B=n, MB=1024, epochs=1)
    exp = make_exp(ref, "discrete", n, 12)
    ref_buf = buffer(exp)
    ref_report = ref.learn(ref_buf)                     # one batch of all rows: the KL of the first batch
    full = build(B=n, MB=1024, epochs=3)
    full_buf = buffer(exp)
    full.learn(full_buf)
    learner = build(B=n, MB=1024, epochs=3, target_kl=1e-9)
    learner.one_launch_optimizer = one_launch
    before = state(learner)
    buf = buffer(exp)
    c0 = int(L.rlppo_dbg_counter(2))
    report = learner.learn(buf)
    passes = int(L.rlppo_dbg_counter(2)) - c0
    same_state(state(learner), before, "nothing applied")
    assert report["PPO Optimizer Steps"] == 0 and report["KL Early Stopped"] == 1.0 and report["Cumulative Model Updates"] == 0
    kl, want = report["Mean KL Divergence"], ref_report["Mean KL Divergence"]
    assert want > 0 and abs(kl - want) <= 1e-5 * want, (kl, want)
    assert passes <= 2 * 1, passes                     # (s + 2) x passes per batch, s = 0, one fused pass per batch
    s1, s2 = buf.rng.get_state(), full_buf.rng.get_state()
    assert np.array_equal(s1[1], s2[1]) and s1[2] == s2[2]
    assert float(learner._grad_all.abs().max()) == 0.0
    report = learner.learn(buf)                        # a stopped learn() leaves a learner that can go on
    assert report["KL Early Stopped"] == 1.0


def kl_trace(lr, n, MB, epochs, seed):
    """(KL of every optimiser step, learner) of a run whose target_kl never triggers."""
    learner = build(B=n, MB=MB, epochs=epochs, lr=lr, target_kl=1e9)
    exp = make_exp(learner, "discrete", n, seed)
    kls = []
    learner.grad_probe = lambda _: kls.append(batch_kl(learner, learner._opt["kl"].cpu().numpy()))
    learner.learn(buffer(exp))
    return np.array(kls), exp


def test_target_kl_stops_after_s_steps(L):
    """A threshold between the KL of steps < s and that of step s (with margin): the result is bit-identical to the same learner
    limited to s steps, at most one batch beyond the trigger was evaluated, two runs stop alike, and 2 and 4 virtual ranks stop at
    the same step with bit-identical replicas."""
    from rlgym_ppo_amd import dp
    n, MB, epochs, lr, seed = 4096, 512, 8, 3e-3, 13
    kls, exp = kl_trace(lr, n, MB, epochs, seed)
    s = next((b for b in range(2, epochs) if kls[b] > 1.2 * kls[:b].max()), None)
    assert s is not None, kls
    target = np.sqrt(kls[:s].max() * kls[s]) / 1.5
    runs = []
    for _ in range(2):
        learner = build(B=n, MB=MB, epochs=epochs, lr=lr, target_kl=target)
        c0 = int(L.rlppo_dbg_counter(2))
        report = learner.learn(buffer(exp))
        passes = int(L.rlppo_dbg_counter(2)) - c0
        assert report["PPO Optimizer Steps"] == s and report["KL Early Stopped"] == 1.0, (report, kls)
        assert report["Cumulative Model Updates"] == s and passes <= (s + 2) * 1, passes   # one fused pass per batch
        runs.append(state(learner))
    same_state(runs[0], runs[1], "two identical runs")
    limited = build(B=n, MB=MB, epochs=s, lr=lr)        # one batch per epoch: s epochs = the first s steps
    limited.learn(buffer(exp))
    same_state(runs[0], state(limited), "stopped after s steps == limited to s steps")
    for world in (2, 4):
        reps = [build(B=n, MB=MB, epochs=epochs, lr=lr, target_kl=target) for _ in range(world)]
        reports = dp.run_virtual_ranks(reps, [buffer(exp) for _ in range(world)])
        assert all(r["PPO Optimizer Steps"] == s for r in reports), (world, [r["PPO Optimizer Steps"] for r in reports])
        for r in reps[1:]:
            same_state(state(r), state(reps[0]), f"{world} replicas")


# --------------------------------------------------------------------------------------------------------- precisions
@pytest.mark.parametrize("precision", ["bf16", "x3"])
def test_every_option_in_the_reduced_precisions(L, precision):
    out = []
    for _ in range(2):
        learner = build(normalize_advantages=True, value_clip_range=0.2, target_kl=0.5, max_grad_norm=1.0)
        learner.update_precision = precision
        report = learner.learn(buffer(make_exp(learner, "discrete", 4096, 14)))
        st = state(learner)
        assert all(torch.isfinite(t).all() for t in st[:6]) and all(np.isfinite(v) for v in report.values())
        out.append((st, report))
    same_state(out[0][0], out[1][0], f"{precision}: run to run")
    same_report(out[0][1], out[1][1], f"{precision}: run to run")


# ------------------------------------------------------------------------------------------------------- Learner loop
def test_learner_loop_with_every_option(tmp_path, capsys):
    from rlgym_ppo_amd import Learner
    learner = Learner(synthetic_env.make_vector_env, vector_env=True, n_proc=1, timestep_limit=1500, exp_buffer_size=1024,
                      ts_per_iteration=512, ppo_epochs=2, ppo_batch_size=512, ppo_minibatch_size=256,
                      policy_layer_sizes=(64, 64), critic_layer_sizes=(64, 64), checkpoints_save_folder=str(tmp_path / "ck"),
                      add_unix_timestamp=False, save_every_ts=1000, checkpoint_load_folder=None, random_seed=3,
                      ppo_normalize_advantages=True, ppo_value_clip_range=0.2, ppo_target_kl=0.02, ppo_max_grad_norm=1.0)
    p = learner.ppo_learner
    assert (p.normalize_advantages, p.value_clip_range, p.target_kl, p.max_grad_norm) == (True, 0.2, 0.02, 1.0)
    try:
        learner._learn()
    finally:
        learner.agent.cleanup()
    out = capsys.readouterr().out
    assert out.count("BEGIN ITERATION REPORT") == 3 and out.count("KL Early Stopped") == 3
    assert learner.epoch == 3 and 0 < p.cumulative_model_updates <= 2 * (1 + 2 + 2)
    assert torch.isfinite(p.policy.arena.flat).all() and torch.isfinite(p.value_net.arena.flat).all()
