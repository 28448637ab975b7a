"""The learning-rate schedules' host side (rlgym_ppo_amd/ppo/lr_schedule.py): adapt_lr -- the float64 restatement of the device rule
and the GPU tests' yardstick --, linear_lr, and every refusal of the options, none of which needs a GPU."""
import math

import pytest

from rlgym_ppo_amd.ppo import lr_schedule as S

D, LO, HI = 0.01, 1e-5, 1e-2


def test_adapt_lr_decreases_increases_and_holds():
    assert S.adapt_lr(3e-4, 0.05, D, LO, HI) == 3e-4 / 1.5
    assert S.adapt_lr(3e-4, 0.001, D, LO, HI) == 3e-4 * 1.5
    assert S.adapt_lr(3e-4, 0.01, D, LO, HI) == 3e-4
    assert S.adapt_lr(3e-4, 0.05, D, LO, HI, factor=2.0) == 1.5e-4


def test_adapt_lr_thresholds_are_strict():
    for kl in (2.0 * D, D / 2.0, 0.0, -0.0, float("nan"), -1e-3):
        assert S.adapt_lr(3e-4, kl, D, LO, HI) == 3e-4, kl
    assert S.adapt_lr(3e-4, math.nextafter(2.0 * D, 1.0), D, LO, HI) == 3e-4 / 1.5
    assert S.adapt_lr(3e-4, math.nextafter(D / 2.0, 0.0), D, LO, HI) == 3e-4 * 1.5
    assert S.adapt_lr(3e-4, 5e-324, D, LO, HI) == 3e-4 * 1.5          # any KL above 0 counts
    assert S.adapt_lr(3e-4, float("inf"), D, LO, HI) == 3e-4 / 1.5


def test_adapt_lr_clamps_at_both_bounds():
    assert S.adapt_lr(1.2e-5, 1.0, D, LO, HI) == 1e-5                  # not 8e-6
    assert S.adapt_lr(8e-3, 1e-4, D, LO, HI) == 1e-2                   # not 1.2e-2
    assert S.adapt_lr(1e-5, 1.0, D, LO, HI) == 1e-5 and S.adapt_lr(1e-2, 1e-4, D, LO, HI) == 1e-2
    assert S.adapt_lr(3e-4, 1.0, D, 3e-4, 3e-4) == 3e-4 and S.adapt_lr(3e-4, 1e-4, D, 3e-4, 3e-4) == 3e-4


def test_linear_lr():
    assert S.linear_lr(3e-4, 0, 1000) == 3e-4
    assert S.linear_lr(3e-4, 500, 1000) == 1.5e-4
    assert S.linear_lr(3e-4, 1000, 1000) == 0.0 and S.linear_lr(3e-4, 1512, 1000) == 0.0
    assert S.linear_lr(3e-4, 250, 1000) == 3e-4 * 0.75


def test_check_schedule_returns_floats():
    assert S.check_schedule("adaptive", 1, (1e-5, 1), policy_lr=3e-4, critic_lr=1e-3) == ("adaptive", 1.0, (1e-5, 1.0))
    assert S.check_schedule("linear", 0.01, [1e-5, 1e-2])[0] == "linear"
    assert S.check_schedule("constant", 0.01, (1e-5, 1e-2), policy_lr=1.0, critic_lr=1.0)[0] == "constant"   # bounds bind "adaptive" only


@pytest.mark.parametrize("kw", [
    dict(lr_schedule="cosine"), dict(lr_schedule=None),
    dict(desired_kl=0.0), dict(desired_kl=-0.01), dict(desired_kl=float("nan")), dict(desired_kl=float("inf")), dict(desired_kl=None),
    dict(lr_bounds=(0.0, 1e-2)), dict(lr_bounds=(1e-2, 1e-5)), dict(lr_bounds=(1e-5, float("inf"))), dict(lr_bounds=(float("nan"), 1e-2)),
    dict(lr_bounds=(1e-5,)), dict(lr_bounds=None),
])
def test_check_schedule_refuses(kw):
    args = dict(lr_schedule="adaptive", desired_kl=0.01, lr_bounds=(1e-5, 1e-2), policy_lr=3e-4, critic_lr=3e-4)
    args.update(kw)
    with pytest.raises(ValueError):
        S.check_schedule(**args)


def test_adaptive_refuses_initial_rates_outside_the_bounds():
    with pytest.raises(ValueError, match=r"policy_lr=0\.1.*1e-05.*0\.01"):
        S.check_schedule("adaptive", 0.01, (1e-5, 1e-2), policy_lr=0.1, critic_lr=3e-4)
    with pytest.raises(ValueError, match=r"critic_lr=1e-06.*1e-05.*0\.01"):
        S.check_schedule("adaptive", 0.01, (1e-5, 1e-2), policy_lr=3e-4, critic_lr=1e-6)


def bare_ppo_learner(policy_lr=3e-4, critic_lr=3e-4, fused=True):
    """A PPOLearner with nothing but what set_lr_schedule reads (the two optimisers' rates, the optimiser form): its constructor
    needs a GPU, the method is host code."""
    from types import SimpleNamespace
    from rlgym_ppo_amd.ppo import PPOLearner
    learner = object.__new__(PPOLearner)
    learner.policy_optimizer = SimpleNamespace(param_groups=[{"lr": policy_lr}])
    learner.value_optimizer = SimpleNamespace(param_groups=[{"lr": critic_lr}])
    learner.fused_optimizer_step = fused
    learner.lr_schedule, learner.desired_kl, learner.lr_bounds, learner.report_learning_rates = "constant", 0.01, (1e-5, 1e-2), False
    return learner


def test_set_lr_schedule_sets_the_checked_options():
    learner = bare_ppo_learner()
    learner.set_lr_schedule("adaptive", desired_kl=1, lr_bounds=[1e-4, 1e-3])
    assert (learner.lr_schedule, learner.desired_kl, learner.lr_bounds, learner.report_learning_rates) == ("adaptive", 1.0, (1e-4, 1e-3), True)
    learner.set_lr_schedule()
    assert (learner.lr_schedule, learner.desired_kl, learner.lr_bounds, learner.report_learning_rates) == ("constant", 0.01, (1e-5, 1e-2), False)


@pytest.mark.parametrize("kw,match", [
    (dict(lr_schedule="cosine"), "lr_schedule"),
    (dict(lr_schedule="linear"), "Learner"),                       # a bare PPOLearner has no horizon
    (dict(lr_schedule="adaptive", desired_kl=0.0), "desired_kl"),
    (dict(lr_schedule="adaptive", lr_bounds=(1e-2, 1e-5)), "lr_bounds"),
    (dict(lr_schedule="adaptive", policy_lr=0.5), "policy_lr"),
    (dict(lr_schedule="adaptive", critic_lr=1e-7), "critic_lr"),
    (dict(desired_kl=float("nan")), "desired_kl"),
])
def test_set_lr_schedule_refuses_and_leaves_the_learner_as_it_was(kw, match):
    learner = bare_ppo_learner(**{k: kw.pop(k) for k in ("policy_lr", "critic_lr") if k in kw})
    with pytest.raises(ValueError, match=match):
        learner.set_lr_schedule(**kw)
    assert (learner.lr_schedule, learner.desired_kl, learner.lr_bounds, learner.report_learning_rates) == ("constant", 0.01, (1e-5, 1e-2), False)


def test_adaptive_refuses_the_unfused_optimiser_step(monkeypatch):
    with pytest.raises(ValueError, match="RLPPO_FUSED_OPT=1"):
        bare_ppo_learner(fused=False).set_lr_schedule("adaptive")
    bare_ppo_learner(fused=False).set_lr_schedule("constant")
    from rlgym_ppo_amd import Learner
    monkeypatch.setenv("RLPPO_FUSED_OPT", "0")

    def no_env():
        raise AssertionError("the options are checked before an environment is built")
    with pytest.raises(ValueError, match="RLPPO_FUSED_OPT=1"):
        Learner(no_env, checkpoint_load_folder=None, ppo_lr_schedule="adaptive")


def test_the_constructors_keep_their_parameter_lists():
    """The schedule is PPOLearner.set_lr_schedule's, not three more constructor parameters: PPOLearner's list stays the reference's
    plus the four options; Learner's three stand in front of per_feature_obs_standardization, off by default."""
    import inspect
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd.ppo import PPOLearner
    assert list(inspect.signature(PPOLearner.__init__).parameters)[-1] == "max_grad_norm"
    sig = inspect.signature(PPOLearner.set_lr_schedule).parameters
    assert [(k, sig[k].default) for k in list(sig)[1:]] == [("lr_schedule", "constant"), ("desired_kl", 0.01), ("lr_bounds", (1e-5, 1e-2))]
    params = inspect.signature(Learner.__init__).parameters
    assert [params[k].default for k in ("ppo_lr_schedule", "ppo_desired_kl", "ppo_lr_bounds")] == ["constant", 0.01, (1e-5, 1e-2)]


@pytest.mark.parametrize("kw,match", [
    (dict(ppo_lr_schedule="exponential"), "lr_schedule"),
    (dict(ppo_lr_schedule="adaptive", ppo_desired_kl=-1.0), "desired_kl"),
    (dict(ppo_lr_schedule="adaptive", ppo_lr_bounds=(0.0, 1.0)), "lr_bounds"),
    (dict(ppo_lr_schedule="adaptive", policy_lr=1.0), "policy_lr"),
    (dict(ppo_lr_schedule="linear", timestep_limit=0), "timestep_limit"),
])
def test_learner_refuses_before_it_builds_anything(kw, match):
    from rlgym_ppo_amd import Learner

    def no_env():
        raise AssertionError("the options are checked before an environment is built")
    with pytest.raises(ValueError, match=match):
        Learner(no_env, checkpoint_load_folder=None, **kw)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The two added entry points check their arguments on the host (no GPU needed): nothing is launched."""
    import ctypes
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    assert L.rlppo_abi_version() == 8
    assert L.rlppo_kl_gate_lr(None, None, None) == 1001
    assert L.rlppo_clip_adam_pack2_lr(None, None, None, None, 0, 0, None, None) == 1001
    slots = (ctypes.c_double * 8)()
    rates = (ctypes.c_double * 2)(3e-4, 3e-4)
    g, a = N.KlGateArgs(), N.LrAdaptArgs()
    g.kl_slots, g.slot_stride, g.n_passes, g.phase = ctypes.addressof(slots), 8, 1, 0
    a.lr, a.n_lr, a.desired_kl, a.factor, a.lr_min, a.lr_max = ctypes.addressof(rates), 2, 0.01, 1.5, 1e-5, 1e-2
    for field, bad in (("n_lr", 0), ("n_lr", 9), ("desired_kl", 0.0), ("desired_kl", float("nan")), ("factor", 1.0), ("lr_min", 0.0),
                       ("lr_min", 1.0), ("lr_max", float("inf")), ("lr", None)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert L.rlppo_kl_gate_lr(None, ctypes.byref(g), ctypes.byref(a)) == 1001, (field, bad)
        setattr(a, field, good)
    g.phase = 2      # phases 1 and 2 need the exchange words
    assert L.rlppo_kl_gate_lr(None, ctypes.byref(g), ctypes.byref(a)) == 1001
    assert L.rlppo_kl_gate_lr(None, ctypes.byref(g), None) == 1001
    assert list(rates) == [3e-4, 3e-4]
