"""Mirror-symmetry augmentation, host side (no GPU): what ppo.Symmetry and rlppo_mirror_batch refuse, each by name; where the keyword
sits in Learner; and that PPOLearner's constructor is what it was."""
import ctypes
import inspect

import numpy as np
import pytest

from rlgym_ppo_amd import _native as N
from rlgym_ppo_amd.ppo import PPOLearner, Symmetry

ID5, ONE5 = np.arange(5), np.ones(5)
BINS = [3, 3, 2, 7, 7]
tables = lambda s, head, **kw: s.host_tables(head, 5, 16, **kw)


@pytest.mark.parametrize("build, match", [
    (lambda: Symmetry([0, 1, 1, 3, 4], ONE5, action=ID5), r"obs_perm is not a permutation of range\(5\): entry 1 at index 2"),
    (lambda: Symmetry(ID5, [1, 1, 0.5, 1, 1], action=ID5), r"obs_sign must hold -1 or \+1: entry 0.5 at index 2"),
    (lambda: Symmetry(ID5, ONE5, action=ID5, critic_obs_perm=[0, 2], critic_obs_sign=[1, 1]), r"critic_obs_perm is not a permutation.*index 1"),
    (lambda: Symmetry(ID5, ONE5, action=ID5, critic_obs_perm=[1, 0], critic_obs_sign=[1, -2]), r"critic_obs_sign must hold.*index 1"),
    (lambda: tables(Symmetry(ID5, ONE5, action=[0, 2, 2]), N.HEAD_DISCRETE, n_actions=3), r"action is not a permutation of range\(3\).*index 2"),
    (lambda: tables(Symmetry(ID5, ONE5, action=[1, 0]), N.HEAD_DISCRETE, n_actions=3), r"action has 2 entries, expected 3"),
    (lambda: tables(Symmetry(ID5, ONE5, action=([0, 1, 3, 2, 4], None)), N.HEAD_MULTIDISCRETE, bins=BINS), r"hperm maps component 3 \(7 bins\) onto component 2 \(2 bins\) at index 2"),
    (lambda: tables(Symmetry(ID5, ONE5, action=(None, [None, [0, 1, 1], None, None, None])), N.HEAD_MULTIDISCRETE, bins=BINS), r"binmaps\[1\] is not a permutation of range\(3\).*index 2"),
    (lambda: tables(Symmetry(ID5, ONE5, action=(None, [None, None, [1, 0, 2], None, None])), N.HEAD_MULTIDISCRETE, bins=BINS), r"binmaps\[2\] has 3 entries, expected 2"),
    (lambda: tables(Symmetry(ID5, ONE5, action=([1, 0, 2, 3], [1, 1, 1, 0])), N.HEAD_GAUSSIAN, act_dim=4), r"action asign must hold.*index 3"),
    (lambda: tables(Symmetry(ID5, ONE5, action=([1, 0, 2], [1, 1, 1])), N.HEAD_DIAG_GAUSSIAN, act_dim=4), r"action aperm has 3 entries, expected 4"),
    (lambda: Symmetry(ID5, ONE5, action=ID5).host_tables(N.HEAD_DISCRETE, 7, 16, n_actions=5), r"obs_perm has 5 entries, the policy observes 7"),
    (lambda: tables(Symmetry(ID5, ONE5, action=ID5), N.HEAD_DISCRETE, n_actions=5, critic_dim=3, critic_ld=16), r"critic_obs_perm / critic_obs_sign are required"),
    (lambda: tables(Symmetry(ID5, ONE5, action=ID5, critic_obs_perm=[1, 0], critic_obs_sign=[1, 1]), N.HEAD_DISCRETE, n_actions=5, critic_dim=3,
                    critic_ld=16), r"critic_obs_perm has 2 entries, the critic observes 3"),
])
def test_symmetry_refuses_by_field_and_index(build, match):
    with pytest.raises(ValueError, match=match):
        build()


def test_keyword_position_and_constructor_pins():
    from rlgym_ppo_amd.learner import Learner
    names = list(inspect.signature(Learner.__init__).parameters)
    assert names[names.index("gae_vtrace_c_bar") + 1] == "symmetry" and names.index("symmetry") < names.index("per_feature_obs_standardization")
    assert inspect.signature(Learner.__init__).parameters["symmetry"].default is None
    assert callable(PPOLearner.set_symmetry) and list(inspect.signature(PPOLearner.__init__).parameters)[-1] == "max_grad_norm"


@pytest.mark.parametrize("change, word", [(dict(s_obs_tab=None), "obs_tab is NULL"), (dict(s_act_tab=None), "act_tab is NULL"), (dict(states=0x10004), "16-byte aligned"),
                                          (dict(mb=0), "mb=0"), (dict(s_head=N.HEAD_GAUSSIAN), "describes head 2"), (dict(s_obs_ld=128), "obs_tab has 128 entries"),
                                          (dict(action_mask=0x800000, mask_words=3), "mask_tab is NULL")])
def test_mirror_batch_argument_errors_come_before_any_hip_call(change, word):
    """RLPPO_ERR_ARG naming the argument, found on the host: the device pointers are placeholders that are never dereferenced."""
    a, s = N.MinibatchArgs(), N.SymmetryArg()
    a.head, a.act_dim, a.mb, a.ld_states = N.HEAD_DISCRETE, 1, 64, 112
    a.states, a.actions, a.old_logp, a.targets, a.advantages, a.idx = (0x10000 * i for i in range(1, 7))
    s.head, s.act_dim, s.n_actions, s.obs_ld, s.obs_tab, s.act_tab = N.HEAD_DISCRETE, 1, 90, 112, 0x100000, 0x200000
    for k, v in change.items():
        setattr(s if k.startswith("s_") else a, k[2:] if k.startswith("s_") else k, v)
    rc = N.lib().rlppo_mirror_batch(None, ctypes.byref(a), None, ctypes.byref(s), ctypes.c_void_p(0x400000), 1 << 30)
    assert rc == 1001 and word in N.lib().rlppo_last_error().decode(), (change, rc, N.lib().rlppo_last_error())
