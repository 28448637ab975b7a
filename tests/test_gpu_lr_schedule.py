"""The learning-rate schedules on the device (include/rlppo.h, "[lr]"): the gate's rate rule against
lr_schedule.adapt_lr bit for bit, the optimiser tail reading its rate from device memory against the same rate in the descriptor,
PPOLearner.learn(lr_schedule="adaptive") against a replay that uses none of the new code (a constant-schedule learner handed the
recorded rates), one and two virtual ranks, together with target_kl, and the Learner loop ("adaptive": save / load / continue,
update_learning_rate; "linear")."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diag_gaussian_env as E  # noqa: E402
from rlgym_ppo_amd.ppo.lr_schedule import adapt_lr, linear_lr  # noqa: E402
from hip_pass import L, P, check, stream  # noqa: E402,F401

D_KL, LO, HI = 0.01, 1e-5, 1e-2
OBS, HID, ROWS, B, MB, EPOCHS = 24, (64, 64), 1024, 1024, 256, 6
HEADS = {"discrete": (0, 6), "diag": (3, 3)}


def f64(values):
    return torch.tensor(values, dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. the gate's rule
STRIDE = 8   # doubles per pass region: {workgroup count, mb_ratio, up to 6 slots}


def one_pass(kl):
    """One pass, one workgroup slot, mb_ratio 1: KL_b is the slot, exactly."""
    return [[1.0, 1.0, kl, 0, 0, 0, 0, 0]], float(kl)


def three_passes(scale=1.0):
    """Three passes with unequal mb_ratio and three slots each; KL_b in the kernel's order: thread t holds slot t, the xor tree adds
    lane 2 to lane 0 before lane 1 joins, the passes are weighted and added in pass order."""
    rs = np.random.RandomState(2)
    regions, kl = [], 0.0
    for ratio in (0.5, 0.25, 0.125):
        a = (rs.rand(3) * 0.02 * scale).tolist()
        regions.append([3.0, ratio] + a + [0, 0, 0])
        kl += ratio * ((a[0] + a[2]) + a[1])
    return regions, kl


class Gate:
    def __init__(self, L, regions, rates, desired_kl=D_KL, bounds=(LO, HI), stop=None, threshold=1e30, host=False, kl_out=True):
        from rlgym_ppo_amd import _native as N
        self.L = L
        self.slots = f64(np.asarray(regions, np.float64).reshape(-1))
        self.rates = f64(rates)
        self.kl = f64([-7.0]) if kl_out else None
        self.exchange = torch.full((2,), -3.0, dtype=torch.float32, device="cuda")
        self.stop = None if stop is None else torch.tensor([stop], dtype=torch.int32, device="cuda")
        self.host = torch.zeros(2, dtype=torch.int32).pin_memory() if host else None
        g, a = N.KlGateArgs(), N.LrAdaptArgs()
        g.kl_slots, g.slot_stride, g.n_passes, g.threshold = self.slots.data_ptr(), STRIDE, len(regions), threshold
        g.exchange, g.batch, g.done_value = self.exchange.data_ptr(), 4, 77
        g.stop_word = None if self.stop is None else self.stop.data_ptr()
        g.host_words = None if self.host is None else self.host.data_ptr()
        a.lr, a.n_lr, a.desired_kl, a.factor = self.rates.data_ptr(), len(rates), desired_kl, 1.5
        a.lr_min, a.lr_max = bounds
        a.kl_out = None if self.kl is None else self.kl.data_ptr()
        self.g, self.a = g, a

    def run(self, phase=0):
        self.g.phase = phase
        check(self.L, self.L.rlppo_kl_gate_lr(stream(), ctypes.byref(self.g), ctypes.byref(self.a)))
        torch.cuda.synchronize()
        return self.rates.cpu().tolist()


RULE_CASES = [
    ("decrease", 0.05), ("increase", 0.001), ("unchanged", 0.01), ("exactly 2d", 2.0 * D_KL), ("exactly d/2", D_KL / 2.0),
    ("just above 2d", float(np.nextafter(2.0 * D_KL, 1.0))), ("just below d/2", float(np.nextafter(D_KL / 2.0, 0.0))),
    ("zero", 0.0), ("nan", float("nan")), ("negative", -1e-3), ("huge", 1e300),
]


@pytest.mark.parametrize("name,kl", RULE_CASES, ids=[c[0].replace(" ", "_") for c in RULE_CASES])
def test_gate_rule_equals_adapt_lr(L, name, kl):
    """Two rates that move and clamp on their own: (1.2e-5, 3e-4, 8e-3) -- the first clamps at lr_min on a decrease (1e-5, not
    8e-6), the last at lr_max on an increase (1e-2, not 1.2e-2), the middle one moves freely.  No stop word, no host words."""
    rates = [1.2e-5, 3e-4, 8e-3]
    regions, kl_b = one_pass(kl)
    gate = Gate(L, regions, rates)
    got = gate.run()
    want = [adapt_lr(r, kl_b, D_KL, LO, HI) for r in rates]
    assert got == want, (name, got, want)
    back = gate.kl.item()
    assert back == kl_b or (np.isnan(back) and np.isnan(kl_b))
    if name in ("decrease", "just above 2d", "huge"):
        assert got == [1e-5, 3e-4 / 1.5, 8e-3 / 1.5]
    elif name in ("increase", "just below d/2"):
        assert got == [1.2e-5 * 1.5, 3e-4 * 1.5, 1e-2]
    else:
        assert got == rates


def test_gate_three_passes_phases_and_stop_word(L):
    from rlgym_ppo_amd import _native as N
    rates = [3e-4, 1e-3]
    for scale, moved in ((1.0, "unchanged"), (5.0, "decrease"), (0.2, "increase")):
        regions, kl_b = three_passes(scale)
        gate = Gate(L, regions, rates)
        got = gate.run()
        assert gate.kl.item() == kl_b and got == [adapt_lr(r, kl_b, D_KL, LO, HI) for r in rates], scale
        assert {"unchanged": got == rates, "decrease": got[0] < rates[0], "increase": got[0] > rates[0]}[moved], (scale, kl_b)
    regions, kl_b = three_passes(5.0)   # (a decrease)
    # a set stop word: the rates stay, the host words carry it as rlppo_kl_gate's do
    gate = Gate(L, regions, rates, stop=3, host=True)
    assert gate.run() == rates and gate.stop.item() == 3 and gate.host.tolist() == [3, 77] and gate.kl.item() == kl_b
    # the gate that sets the stop word itself moves nothing either
    gate = Gate(L, regions, rates, stop=0, threshold=kl_b / 2, host=True)
    assert gate.run() == rates and gate.stop.item() == 5 and gate.host.tolist() == [5, 77]
    # a stop word that stays clear: the rule runs, the host words say "running"
    gate = Gate(L, regions, rates, stop=0, threshold=kl_b * 2, host=True)
    assert gate.run() == [r / 1.5 for r in rates] and gate.stop.item() == 0 and gate.host.tolist() == [0, 77]
    # phase 1 writes the two exchange floats and nothing else; phase 2 decides from their sum over the ranks (here: two equal ranks)
    gate = Gate(L, regions, rates)
    assert gate.run(1) == rates and gate.kl.item() == -7.0
    hi = np.float32(kl_b)
    lo = np.float32(kl_b - np.float64(hi))
    assert gate.exchange.cpu().numpy().tolist() == [hi, lo]
    gate.exchange *= 2
    kl2 = float(np.float64(np.float32(2) * hi) + np.float64(np.float32(2) * lo))
    assert gate.run(2) == [adapt_lr(r, kl2, D_KL, LO, HI) for r in rates] and gate.kl.item() == kl2
    # without the optional KL output
    gate = Gate(L, regions, rates, kl_out=False)
    assert gate.run() == [r / 1.5 for r in rates]
    # refusals, before any launch
    bad = Gate(L, regions, rates)
    bad.a.n_lr = 0
    assert L.rlppo_kl_gate_lr(stream(), ctypes.byref(bad.g), ctypes.byref(bad.a)) != 0
    bad.a.n_lr, bad.a.lr_min = 2, 1.0
    assert L.rlppo_kl_gate_lr(stream(), ctypes.byref(bad.g), ctypes.byref(bad.a)) != 0
    assert L.rlppo_kl_gate_lr(stream(), ctypes.byref(bad.g), None) != 0
    assert bad.rates.cpu().tolist() == rates


# ------------------------------------------------------------------------------------------- 2. the optimiser's device rate
def opt_state(L, dims, tail, seed):
    from rlgym_ppo_amd import _native as N
    g = torch.Generator(device="cuda").manual_seed(seed)
    dc, nl = N.dims_array(dims), len(dims) - 1
    n = int(L.rlppo_flat_floats(dc, nl)) + tail
    flat = torch.randn(n, device="cuda", generator=g) * 0.1
    st = dict(dc=dc, nl=nl, n=n, tail=tail, gen=g)
    for tag in ("ref", "dev"):
        st[tag] = dict(p=flat.clone(), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"),
                       packed=torch.zeros(int(L.rlppo_packed_floats(dc, nl)), device="cuda"), gn=torch.zeros(1, dtype=torch.float64, device="cuda"))
        check(L, L.rlppo_net_pack(stream(), dc, nl, P(st[tag]["p"]), P(st[tag]["packed"])))
    return st


def descriptor(st, tag, grad, lr, step):
    from rlgym_ppo_amd import _native as N
    b, d = st[tag], N.OptNet()
    d.dims, d.n_layers = ctypes.cast(st["dc"], ctypes.POINTER(ctypes.c_int32)), st["nl"]
    d.params, d.grads, d.exp_avg, d.exp_avg_sq = b["p"].data_ptr(), grad.data_ptr(), b["m"].data_ptr(), b["v"].data_ptr()
    d.packed, d.gnorm2 = b["packed"].data_ptr(), b["gn"].data_ptr()
    d.max_norm, d.lr, d.beta1, d.beta2, d.eps, d.step = 0.5, lr, 0.9, 0.999, 1e-8, step
    return d


SIZES = {"below_the_prefetch": (24, 64), "above_the_prefetch": (64, 512)}   # FUSED_EPT x 256 x grid = 196,608 elements at most


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "three_operations"])
@pytest.mark.parametrize("tail", [0, 3], ids=["no_tail", "tail"])
@pytest.mark.parametrize("size", list(SIZES))
def test_device_rate_equals_the_rate_in_the_descriptor(L, size, tail, one_launch):
    """rlppo_clip_adam_pack2_lr with the rates in device doubles (the descriptors' own lr set to a value that would show) against
    rlppo_clip_adam_pack2_tail with the same rates in the descriptors: parameters, both moments, the packed images, the squared
    norms bit for bit, gradients zeroed.  Rates that no float holds (3e-4 / 1.5 and 1e-3 / 1.5 / 1.5); then one pointer NULL; then
    both NULL (the parent's entry point).  The gradients of step 2 are large enough for the clip to bite."""
    from rlgym_ppo_amd import _native as N
    obs, h = SIZES[size]
    nets = [opt_state(L, [obs, h, h, 1], 0, 1), opt_state(L, [obs, h, h, 3], tail, 2)]   # critic, policy (+ log_std)
    assert (max(st["n"] for st in nets) > 6 * 256 * 128) == (size == "above_the_prefetch")
    syncs = [torch.zeros(N.OPT_SYNC_BYTES // 4, dtype=torch.int32, device="cuda") if one_launch else None for _ in range(2)]
    rates = f64([0.0, 0.0])
    plans = [((3e-4 / 1.5, 1e-3 / 1.5 / 1.5), (True, True)), ((3e-4 / 1.5 / 1.5, 1e-3 * 1.5), (True, True)),
             ((1.2e-5, 2e-4 / 1.5), (False, True)), ((3e-4, 1e-3 / 1.5), (True, False)), ((3e-4 / 1.5, 1e-3), (False, False))]
    for step, (lrs, on_device) in enumerate(plans, start=1):
        assert any(float(np.float32(lr)) != lr for lr in lrs)
        grads = [torch.randn(st["n"], device="cuda", generator=st["gen"]) * (3.0 if step == 2 else 0.01) for st in nets]
        g_ref, g_dev = [g.clone() for g in grads], [g.clone() for g in grads]
        d_ref = [descriptor(st, "ref", g, lr, step) for st, g, lr in zip(nets, g_ref, lrs)]
        d_dev = [descriptor(st, "dev", g, 0.5 if dev_ else lr, step) for st, g, lr, dev_ in zip(nets, g_dev, lrs, on_device)]
        rates.copy_(f64(list(lrs)))
        ptrs = [ctypes.c_void_p(rates.data_ptr() + 8 * k) if dev_ else None for k, dev_ in enumerate(on_device)]
        check(L, L.rlppo_clip_adam_pack2_tail(stream(), ctypes.byref(d_ref[0]), ctypes.byref(d_ref[1]), P(syncs[0]), nets[0]["tail"], nets[1]["tail"]))
        check(L, L.rlppo_clip_adam_pack2_lr(stream(), ctypes.byref(d_dev[0]), ctypes.byref(d_dev[1]), P(syncs[1]), nets[0]["tail"], nets[1]["tail"],
                                            ptrs[0], ptrs[1]))
        torch.cuda.synchronize()
        assert rates.cpu().tolist() == list(lrs)   # the call never writes a rate
        for k, st in enumerate(nets):
            for key in ("p", "m", "v", "packed"):
                assert torch.equal(st["ref"][key], st["dev"][key]), (step, k, key)
            assert (g_dev[k] == 0).all() and (g_ref[k] == 0).all()
            # (the three-operation form accumulates its norm with atomics: equal up to the order of the additions)
            assert abs(st["ref"]["gn"].item() - st["dev"]["gn"].item()) <= (0 if one_launch else 1e-12) * st["ref"]["gn"].item()
    if one_launch:
        assert syncs[0].cpu().numpy()[2] == 0 and syncs[1].cpu().numpy()[2] == 0   # no barrier wait gave up


# ------------------------------------------------------------------------------------------------ 3. learn(), end to end
def build(head, lr=(3e-4, 1e-3), epochs=EPOCHS, seed=5, **opts):
    from rlgym_ppo_amd.ppo import PPOLearner
    torch.manual_seed(seed)
    ptype, act = HEADS[head]
    schedule = {k: opts.pop(k) for k in ("lr_schedule", "desired_kl", "lr_bounds") if k in opts}
    learner = PPOLearner(OBS, act, ptype, HID, HID, (0.1, 1.0), B, epochs, lr[0], lr[1], 0.2, 0.005, MB, "cuda:0", **opts)
    if schedule:
        learner.set_lr_schedule(**schedule)
    return learner


_EXP = {}


def experience(head):
    """The 1024-row buffer content of a head, sampled ONCE by a learner of the standard construction (every learner of this file
    starts from the same parameters) and shared; old log-probabilities perturbed as tests/test_gpu_ppo_options.py::make_exp does."""
    if head not in _EXP:
        learner = build(head)
        rs = np.random.RandomState(31)
        obs = np.clip(rs.randn(ROWS, OBS), -5, 5).astype(np.float32)
        torch.manual_seed(77)
        act, logp = learner.policy.get_action(obs)
        act = np.asarray(torch.as_tensor(act).cpu(), np.float32)
        act = act.reshape(ROWS) if head == "discrete" else act.reshape(ROWS, -1)
        old = (np.asarray(torch.as_tensor(logp).cpu(), np.float32).reshape(ROWS) + 0.1 * rs.randn(ROWS)).astype(np.float32)
        z = np.zeros(ROWS, np.float32)
        _EXP[head] = (obs, act, old, z, obs, z, z, rs.randn(ROWS).astype(np.float32), rs.randn(ROWS).astype(np.float32))
    return _EXP[head]


def buffer(exp, seed=9):
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    buf = ExperienceBuffer(exp[0].shape[0], seed, "cpu")
    buf.submit_experience(*exp)
    return buf


def state(learner):
    torch.cuda.synchronize()
    po, vo = learner.policy_optimizer, learner.value_optimizer
    return [t.detach().clone() for t in (learner.policy.arena.flat, learner.value_net.arena.flat, po.exp_avg, po.exp_avg_sq, vo.exp_avg,
                                         vo.exp_avg_sq)] + [po.step_count, vo.step_count, learner.cumulative_model_updates]


def same_state(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), (what, i)


def rates_of(learner):
    return [learner.policy_optimizer.param_groups[0]["lr"], learner.value_optimizer.param_groups[0]["lr"]]


def probe_into(learner, trace):
    learner.lr_probe = lambda rates, kl: trace.append((rates.cpu().tolist(), float(kl.item())))


def check_trace(trace, lr0, desired_kl, bounds=(LO, HI), label=""):
    """The probed rates are adapt_lr applied to the probed KLs, and no KL lies within 1e-6 (relative) of a threshold.
    -> the set of outcomes per step."""
    lr, outcomes = list(lr0), []
    for step, (rates, kl) in enumerate(trace):
        for thr in (2.0 * desired_kl, desired_kl / 2.0):
            assert abs(kl - thr) > 1e-6 * thr, (label, step, kl, thr)
        want = [adapt_lr(r, kl, desired_kl, *bounds) for r in lr]
        assert rates == want, (label, step, kl, rates, want)
        outcomes.append("decrease" if want[0] < lr[0] else "increase" if want[0] > lr[0] else "unchanged")
        lr = want
    print(f"[lr trace] {label}: KL {[f'{kl:.3e}' for _, kl in trace]} policy rate {[f'{r[0]:.3e}' for r, _ in trace]} {outcomes}")
    return outcomes


def adaptive_run(head, lr0, desired_kl, precision=None, **opts):
    learner, trace = build(head, lr0, lr_schedule="adaptive", desired_kl=desired_kl, **opts), []
    learner.update_precision = precision
    probe_into(learner, trace)
    report = learner.learn(buffer(experience(head)))
    return learner, trace, report


def replay(head, lr0, trace, precision=None):
    """A constant-schedule learner driven one epoch (= one optimiser step) per learn() on ONE buffer, its optimisers handed the
    recorded rates before each call: rlppo_clip_adam_pack2(_tail) with the rate in the descriptor, no gate, no device rate."""
    learner = build(head, lr0, epochs=1)
    learner.update_precision = precision
    buf = buffer(experience(head))
    for rates, _ in trace:
        learner.policy_optimizer.param_groups[0]["lr"], learner.value_optimizer.param_groups[0]["lr"] = rates
        report = learner.learn(buf)
        assert "Policy Learning Rate" not in report
    return learner


# (initial rates {policy, critic}, desired_kl): the buffer's old log-probabilities are off by N(0, 0.1), a KL of ~5e-3 at the first
# step whatever the rate -- far above 2 x 1e-4 (decreases), far below 0.5 / 2 (increases), inside (2.5e-3, 1e-2) for 5e-3 (unchanged)
PAIRS = [((3e-4, 1e-3), 1e-4), ((3e-4, 1e-3), 0.5), ((1e-4, 2e-4), 5e-3)]
_SEEN = {}


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("pair", range(len(PAIRS)))
def test_adaptive_learn_equals_the_replay_of_its_rates(L, head, pair):
    lr0, desired_kl = PAIRS[pair]
    learner, trace, report = adaptive_run(head, lr0, desired_kl)
    assert len(trace) == EPOCHS
    _SEEN.setdefault(head, set()).update(check_trace(trace, lr0, desired_kl, label=f"{head}, pair {pair}"))
    assert rates_of(learner) == trace[-1][0] == [report["Policy Learning Rate"], report["Critic Learning Rate"]]
    assert learner.policy_optimizer.state_dict()["param_groups"][0]["lr"] == trace[-1][0][0]   # the stock state_dict carries it
    same_state(state(replay(head, lr0, trace)), state(learner), f"{head}, pair {pair}: replay")


@pytest.mark.parametrize("head", list(HEADS))
def test_the_three_pairs_cover_every_outcome(L, head):
    """Not vacuous: over the three pairs the traces above decreased, increased and left the rate alone at least once each."""
    for pair, (lr0, desired_kl) in enumerate(PAIRS):   # (run alone, this test records the traces itself)
        if len(_SEEN.get(head, ())) < 3:
            _SEEN.setdefault(head, set()).update(check_trace(adaptive_run(head, lr0, desired_kl)[1], lr0, desired_kl, label=f"{head}, pair {pair}"))
    assert _SEEN[head] == {"decrease", "increase", "unchanged"}, _SEEN[head]


def test_adaptive_learn_equals_its_replay_in_bf16(L):
    lr0, desired_kl = PAIRS[1]
    learner, trace, _ = adaptive_run("discrete", lr0, desired_kl, precision="bf16")
    assert "increase" in check_trace(trace, lr0, desired_kl, label="bf16")
    same_state(state(replay("discrete", lr0, trace, precision="bf16")), state(learner), "bf16: replay")


# ------------------------------------------------------------------------------------------------ 4. a rule that cannot move
@pytest.mark.parametrize("desired_kl", [1e-9, 1e9], ids=["always_above", "always_below"])
def test_bounds_that_pin_the_rate_give_the_constant_run(L, desired_kl):
    """lr_min = lr_max = the initial rates: the rule fires at every step and is clamped back every time; parameters, moments, step
    counts and the report are the constant schedule's, apart from the two added keys."""
    lr = (3e-4, 3e-4)
    const = build("discrete", lr)
    r_const = const.learn(buffer(experience("discrete")))
    pinned, trace, r_pinned = adaptive_run("discrete", lr, desired_kl, lr_bounds=(3e-4, 3e-4))
    assert all(rates == [3e-4, 3e-4] for rates, _ in trace) and all((kl > 2 * desired_kl) or (0 < kl < desired_kl / 2) for _, kl in trace)
    same_state(state(pinned), state(const), "pinned")
    assert set(r_pinned) - set(r_const) == {"Policy Learning Rate", "Critic Learning Rate"} and set(r_const) <= set(r_pinned)
    for k in set(r_const) - {"PPO Batch Consumption Time"}:
        assert r_const[k] == r_pinned[k], k
    assert r_pinned["Policy Learning Rate"] == 3e-4 == r_pinned["Critic Learning Rate"]


# ------------------------------------------------------------------------------------------------ 5. two virtual ranks
def test_two_virtual_ranks_follow_the_one_rank_trace(L):
    from rlgym_ppo_amd import dp
    lr0, desired_kl = PAIRS[1]
    _, one, _ = adaptive_run("discrete", lr0, desired_kl)
    check_trace(one, lr0, desired_kl, label="one rank")
    reps, traces = [build("discrete", lr0, lr_schedule="adaptive", desired_kl=desired_kl) for _ in range(2)], [[], []]
    for r, t in zip(reps, traces):
        probe_into(r, t)
    reports = dp.run_virtual_ranks(reps, [buffer(experience("discrete")) for _ in range(2)])
    check_trace(traces[0], lr0, desired_kl, label="two ranks")
    assert traces[0] == traces[1] and [r for r, _ in traces[0]] == [r for r, _ in one]
    same_state(state(reps[0]), state(reps[1]), "replicas")
    assert rates_of(reps[0]) == rates_of(reps[1]) == one[-1][0]
    assert reports[0]["Policy Learning Rate"] == reports[1]["Policy Learning Rate"] == one[-1][0][0]


# ------------------------------------------------------------------------------------------------ 6. with target_kl
def test_adaptive_with_target_kl_stops_like_the_limited_run(L):
    """The pattern of test_target_kl_stops_after_s_steps: a threshold between the KL of the steps before s and that of step s; the
    stopped learner equals the adaptive learner limited to s steps, rates included -- those its last applied step used."""
    lr0, desired_kl = (3e-3, 3e-3), 0.5       # increases from a high rate: the KL climbs step by step
    _, trace, _ = adaptive_run("discrete", lr0, desired_kl, target_kl=1e9)
    kls = np.array([kl for _, kl in trace])
    check_trace(trace, lr0, desired_kl, label="target_kl never reached")
    s = next((b for b in range(2, EPOCHS) if kls[b] > 1.2 * kls[:b].max()), None)
    assert s is not None, kls
    target = np.sqrt(kls[:s].max() * kls[s]) / 1.5
    stopped, t2, report = adaptive_run("discrete", lr0, desired_kl, target_kl=target)
    assert report["PPO Optimizer Steps"] == s and report["KL Early Stopped"] == 1.0, (report, kls)
    assert [r for r, _ in t2[:s]] == [r for r, _ in trace[:s]] and all(r == trace[s - 1][0] for r, _ in t2[s:]) and len(t2) <= s + 2
    assert rates_of(stopped) == trace[s - 1][0] == [report["Policy Learning Rate"], report["Critic Learning Rate"]]
    limited, t3, _ = adaptive_run("discrete", lr0, desired_kl, epochs=s)
    assert t3 == trace[:s] and rates_of(limited) == rates_of(stopped)
    same_state(state(stopped), state(limited), "stopped after s steps == limited to s steps")


# ------------------------------------------------------------------------------------------------ 7. / 8. the Learner loop
LOOP = dict(vector_env=True, n_proc=1, min_inference_size=2, exp_buffer_size=384, ts_per_iteration=384, ppo_epochs=3, ppo_batch_size=384,
            ppo_minibatch_size=192, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32), add_unix_timestamp=False, save_every_ts=300,
            standardize_obs=False, standardize_returns=False, continuous_head="diag", policy_lr=3e-4, critic_lr=1e-3)
ADAPTIVE = dict(ppo_lr_schedule="adaptive", ppo_desired_kl=1.0)   # every KL above 0 is below 1 / 2: the rates climb


def loop_state(l_):
    p_ = l_.ppo_learner
    return dict(pol=p_.policy.arena.flat.clone(), val=p_.value_net.arena.flat.clone(), m=p_.policy_optimizer.exp_avg.clone(),
                v=p_.policy_optimizer.exp_avg_sq.clone(), vm=p_.value_optimizer.exp_avg.clone(), vv=p_.value_optimizer.exp_avg_sq.clone(),
                steps=(p_.policy_optimizer.step_count, p_.value_optimizer.step_count, p_.cumulative_model_updates),
                book=l_.agent.cumulative_timesteps, rates=tuple(rates_of(p_)), logp=l_.experience_buffer.log_probs.clone())


def run_loop(l_, before_learn=None):
    """Runs the loop -> (state, reports of PPOLearner.learn, environment step, host generators)."""
    reports, plain = [], l_.ppo_learner.learn

    def learn(exp):
        if before_learn is not None:
            before_learn(l_, len(reports))
        reports.append(plain(exp))
        return reports[-1]
    l_.ppo_learner.learn = learn
    try:
        l_._learn()
        return loop_state(l_), reports, int(l_.agent.env.t), (torch.get_rng_state(), np.random.get_state(), l_.experience_buffer.rng.get_state())
    finally:
        l_.agent.cleanup()


def test_learner_adaptive_save_load_continue_equals_the_uninterrupted_run(tmp_path):
    """The pattern of tests/test_gpu_diag_gaussian.py::test_learner_save_load_continue_equals_the_uninterrupted_run with the adaptive
    schedule: the second Learner is built with OTHER rates and must go on from the checkpoint's (its optimisers' param_groups)."""
    from rlgym_ppo_amd import Learner
    env = functools.partial(E.CounterVectorEnv, 0)
    whole, reports, t_end, _ = run_loop(Learner(env, timestep_limit=700, checkpoint_load_folder=None, random_seed=3,
                                                checkpoints_save_folder=str(tmp_path / "whole"), **LOOP, **ADAPTIVE))
    assert len(reports) == 2 and all("Policy Learning Rate" in r and "Critic Learning Rate" in r for r in reports)
    assert (reports[1]["Policy Learning Rate"], reports[1]["Critic Learning Rate"]) == whole["rates"]
    first, r1, t_mid, rng = run_loop(Learner(env, timestep_limit=300, checkpoint_load_folder=None, random_seed=3,
                                             checkpoints_save_folder=str(tmp_path / "ck"), **LOOP, **ADAPTIVE))
    assert first["book"] == 384 and whole["book"] == 768 and first["steps"] == (3, 3, 3)
    assert first["rates"][0] > 3e-4 and first["rates"][1] > 1e-3 and whole["rates"][0] > first["rates"][0]   # the schedule moved them, twice
    assert r1[0]["Policy Learning Rate"] == reports[0]["Policy Learning Rate"] == first["rates"][0]
    second = Learner(functools.partial(E.CounterVectorEnv, t_mid), timestep_limit=700, checkpoint_load_folder="latest", random_seed=9,
                     checkpoints_save_folder=str(tmp_path / "ck"), **dict(LOOP, policy_lr=5e-4, critic_lr=5e-4), **ADAPTIVE)
    try:
        restored = loop_state(second)
        for key in ("pol", "val", "m", "v", "vm", "vv", "steps", "book", "rates"):
            same = torch.equal(restored[key], first[key]) if isinstance(first[key], torch.Tensor) else restored[key] == first[key]
            assert same, ("restored", key, restored[key], first[key])
        torch.set_rng_state(rng[0])
        np.random.set_state(rng[1])
        second.experience_buffer.rng.set_state(rng[2])
    except BaseException:
        second.agent.cleanup()
        raise
    resumed, _, t_res, _ = run_loop(second)
    assert t_res == t_end
    for key, want in whole.items():
        same = torch.equal(resumed[key], want) if isinstance(want, torch.Tensor) else resumed[key] == want
        assert same, ("continued", key)


def test_learner_adaptive_honours_update_learning_rate(tmp_path):
    """Learner.update_learning_rate between two iterations: the next learn() refreshes the device rates from the host copies, so its
    first gate starts from the new rates."""
    from rlgym_ppo_amd import Learner
    traces = []

    def before(l_, iteration):
        traces.append([])
        probe_into(l_.ppo_learner, traces[-1])
        if iteration == 1:
            l_.update_learning_rate(new_policy_lr=2e-3, new_critic_lr=4e-5)
    learner = Learner(functools.partial(E.CounterVectorEnv, 0), timestep_limit=700, checkpoint_load_folder=None, random_seed=3,
                      checkpoints_save_folder=str(tmp_path / "ck"), **LOOP, **ADAPTIVE)
    final, reports, _, _ = run_loop(learner, before)
    assert len(traces) == 2 and len(traces[1]) == 3
    check_trace(traces[0], (3e-4, 1e-3), 1.0, label="first iteration")
    check_trace(traces[1], (2e-3, 4e-5), 1.0, label="after update_learning_rate")
    # (the first KL of an iteration is that of rows the policy has just sampled: 0 up to rounding, either side of it -- the two
    # steps behind it see a policy that has moved, and climb)
    assert traces[1][0][0] in ([2e-3, 4e-5], [2e-3 * 1.5, 4e-5 * 1.5]) and final["rates"] == tuple(traces[1][-1][0])
    assert final["rates"][0] >= 2e-3 * 1.5 * 1.5 and final["rates"][1] >= 4e-5 * 1.5 * 1.5
    assert reports[1]["Policy Learning Rate"] == final["rates"][0] and reports[1]["Critic Learning Rate"] == final["rates"][1]


def test_learner_linear_schedule_anneals_over_the_timestep_limit(tmp_path):
    from rlgym_ppo_amd import Learner
    seen = []
    learner = Learner(functools.partial(E.CounterVectorEnv, 0), timestep_limit=1000, checkpoint_load_folder=None, random_seed=3,
                      checkpoints_save_folder=str(tmp_path / "ck"), ppo_lr_schedule="linear", **LOOP)
    final, reports, _, _ = run_loop(learner, lambda l_, i: seen.append((l_.agent.cumulative_timesteps - 384, rates_of(l_.ppo_learner))))
    assert [t for t, _ in seen] == [0, 384, 768] and len(reports) == 3
    for (t, rates), report in zip(seen, reports):
        want = [linear_lr(3e-4, t, 1000), linear_lr(1e-3, t, 1000)]
        assert rates == want == [report["Policy Learning Rate"], report["Critic Learning Rate"]], (t, rates, want)
    assert reports[0]["Policy Learning Rate"] == 3e-4 and 0 < reports[2]["Policy Learning Rate"] < reports[1]["Policy Learning Rate"] < 3e-4
    assert learner.ppo_learner.lr_schedule == "constant"   # the annealing is the loop's: the update runs the constant schedule's launches
