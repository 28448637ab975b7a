"""CPU checks of the diagonal-Gaussian head (include/rlppo.h, "[diag]"): every argument refusal at the C boundary before any HIP
call, the Learner's ValueErrors, the action-clip wrapper, the arena's parameter tail (layout arithmetic that needs no device
memory: an arena itself is device memory, so its state-dict round trip is in tests/test_gpu_diag_gaussian.py), and the yardstick's
closed forms against torch.distributions.Normal.  No GPU, no compute call."""
import ctypes
import inspect
import pickle

import numpy as np
import pytest
import torch

import diag_gaussian_yardstick as Y
import ppo_yardstick as PY
import synthetic_env

POL, VAL = [107, 256, 256, 8], [107, 256, 256, 1]


def _args(N, L, head=3, act_dim=8, mb=1500, pol=POL, val=VAL):
    """rlppo_minibatch_args with placeholders for every device pointer: the host never dereferences them."""
    pol_c, val_c = N.dims_array(pol), N.dims_array(val)
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.slot, a.precision = head, len(pol) - 1, len(val) - 1, act_dim, 0, N.PRECISION_FP32
    a.pol_dims = ctypes.cast(pol_c, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(val_c, ctypes.POINTER(ctypes.c_int32))
    fake = iter(range(0x10000, 0x1000000, 0x1000))  # distinct, never dereferenced
    for f in ("pol_packed", "val_packed", "pol_grad", "val_grad", "states", "actions", "old_logp", "targets", "advantages", "idx", "stats",
              "workspace"):
        setattr(a, f, next(fake))
    a.ld_states, a.n_rows, a.mb = 112, 5000, mb
    a.clip_range, a.ent_coef, a.mb_ratio = 0.2, 0.005, 1.0
    a.ws_bytes = L.rlppo_minibatch_workspace_bytes_for(pol_c, len(pol) - 1, val_c, len(val) - 1, mb, N.PRECISION_FP32)
    assert a.ws_bytes > 0
    a._keep = (pol_c, val_c)
    return a


def test_minibatch_refusals_come_before_any_hip_call():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    assert N.HEAD_DIAG_GAUSSIAN == 3 and N.DIAG_MAX_K >= 64
    sb = L.rlppo_diag_scratch_bytes(1500, 8)
    assert sb == 6 * 8 * 8   # ceil(1500 / 256) workgroups x k doubles
    LS, LG, SC = 0x2000000, 0x2001000, 0x2002000

    def diag(a, log_std=LS, grad=LG, scratch=SC, nbytes=sb):
        return L.rlppo_ppo_minibatch_diag(None, ctypes.byref(a), log_std, grad, scratch, nbytes), L.rlppo_last_error().decode()

    # head 3 through the plain entry points
    a = _args(N, L)
    for rc in (L.rlppo_ppo_minibatch(None, ctypes.byref(a)), L.rlppo_ppo_minibatch_nvec(None, ctypes.byref(a), None, 0)):
        msg = L.rlppo_last_error().decode()
        assert rc == 1001 and "head 3" in msg and "rlppo_ppo_minibatch_diag" in msg, (rc, msg)
    # ... and rlppo_ppo_minibatch_diag with another head
    for head in (0, 1, 2):
        rc, msg = diag(_args(N, L, head=head, act_dim=1))
        assert rc == 1001 and f"head {head}" in msg and "ppo_minibatch_diag" in msg, (rc, msg)
    rc, msg = diag(_args(N, L, head=99))
    assert rc == 1001 and "head 99" in msg, (rc, msg)
    # NULL log_std / log_std_grad
    for kw in ({"log_std": None}, {"grad": None}):
        rc, msg = diag(_args(N, L), **kw)
        assert rc == 1001 and "log_std" in msg and "NULL" in msg, (rc, msg)
    # act_dim != dims[last]
    rc, msg = diag(_args(N, L, act_dim=4))
    assert rc == 1001 and "act_dim=4" in msg and "8 outputs" in msg, (rc, msg)
    # scratch too small / missing / misaligned
    rc, msg = diag(_args(N, L), nbytes=sb - 1)
    assert rc == 1001 and "scratch" in msg and str(sb) in msg, (rc, msg)
    rc, msg = diag(_args(N, L), scratch=None)
    assert rc == 1001 and "scratch" in msg, (rc, msg)
    rc, msg = diag(_args(N, L), scratch=SC + 4)
    assert rc == 1001 and "scratch" in msg and "aligned" in msg, (rc, msg)
    # k beyond RLPPO_DIAG_MAX_K
    wide = N.DIAG_MAX_K + 1
    rc, msg = diag(_args(N, L, act_dim=wide, pol=[107, 256, 256, wide]), nbytes=L.rlppo_diag_scratch_bytes(1500, wide))
    assert rc == 1001 and "RLPPO_DIAG_MAX_K" in msg, (rc, msg)
    # a mask in the arguments: the Gaussian head's refusal text
    a = _args(N, L)
    a.action_mask, a.mask_words = 0x3000000, 1
    rc, msg = diag(a)
    assert rc == 1001 and "action_mask is an option of the discrete head" in msg and "diagonal-Gaussian" in msg, (rc, msg)
    # an empty pass is no error and no launch
    a = _args(N, L)
    a.mb = 0
    assert diag(a)[0] == 0


def test_act_refuses_a_mask_and_bad_arguments_before_any_hip_call():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    dims = N.dims_array(POL)

    def act(opts=None, d=dims, n=16, log_std=0x5000):
        rc = L.rlppo_diag_gaussian_act(None, d, 3, 0x1000, 0x2000, 112, n, 0x3000, log_std, 0x6000, 0x7000, 0x8000, 1 << 20,
                                       None if opts is None else ctypes.byref(opts))
        return rc, L.rlppo_last_error().decode()

    o = N.ActOpts(N.PRECISION_DEFAULT, 0, None)
    o.action_mask, o.mask_words = 0x9000, 1
    rc, msg = act(o)
    assert rc == 1001 and "action_mask is an option of the discrete head" in msg and "rlppo_diag_gaussian_act" in msg, (rc, msg)
    rc, msg = act(log_std=None)
    assert rc == 1001 and "diag_gaussian_act" in msg, (rc, msg)
    rc, msg = act(d=N.dims_array([107, 256, 256, N.DIAG_MAX_K + 1]))
    assert rc == 1001 and "RLPPO_DIAG_MAX_K" in msg, (rc, msg)
    assert act(n=0)[0] == 0


def test_optimiser_tail_refusals():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    d = N.OptNet()
    assert L.rlppo_clip_adam_pack2_tail(None, None, None, None, 0, 0) == 1001
    dims = N.dims_array([4, 4])
    d.dims, d.n_layers = ctypes.cast(dims, ctypes.POINTER(ctypes.c_int32)), 1
    assert L.rlppo_clip_adam_pack2_tail(None, ctypes.byref(d), ctypes.byref(d), None, -1, 0) == 1001
    assert b"tail" in L.rlppo_last_error()


class _Agent:
    """Stand-in for the collection manager: `code` is the action space type it reports."""
    code = 2

    def __init__(self, *a, **k):
        pass

    def init_processes(self, **k):
        _Agent.build_env_fn = k["build_env_fn"]
        return (20,), 3, _Agent.code

    def cleanup(self):
        pass


def _learner(monkeypatch, tmp_path, **kw):
    from rlgym_ppo_amd import learner as LM
    monkeypatch.setattr(LM, "BatchedAgentManager", _Agent)
    monkeypatch.setattr(LM, "ExperienceBuffer", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    return LM.Learner(synthetic_env.make_continuous_wire_env, device="cuda:0", checkpoints_save_folder=str(tmp_path / "c"),
                      add_unix_timestamp=False, checkpoint_load_folder=None, **kw)


def test_learner_value_errors(monkeypatch, tmp_path):
    """An unknown continuous_head, a non-finite continuous_log_std_init and a misplaced or malformed continuous_action_clip are
    refused at the top of the constructor, before the device is selected or a process is spawned.  "diag" on an action space that
    is not continuous can only be refused once the environment has reported its space -- after the manager has built it, before
    the PPOLearner is built (the place of the multi_discrete_bins check): the stand-ins below let the constructor get there
    without a GPU."""
    from rlgym_ppo_amd import Learner
    ps = inspect.signature(Learner.__init__).parameters
    assert ps["continuous_head"].default == "reference" and ps["continuous_log_std_init"].default == 0.0
    with pytest.raises(ValueError, match="continuous_head.*'tanh'"):
        _learner(monkeypatch, tmp_path, continuous_head="tanh")
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="log_std_init"):
            _learner(monkeypatch, tmp_path, continuous_head="diag", continuous_log_std_init=bad)
    for code in (0, 1):
        _Agent.code = code
        with pytest.raises(ValueError, match=f"'diag'.*type 2.*type {code}"):
            _learner(monkeypatch, tmp_path, continuous_head="diag")
    _Agent.code = 2
    # the clip belongs to the diag head: refused with the reference's, malformed ones refused too
    with pytest.raises(ValueError, match="continuous_action_clip"):
        _learner(monkeypatch, tmp_path, continuous_action_clip=(-1.0, 1.0))
    with pytest.raises(ValueError, match="continuous_action_clip is an option"):   # (a pair given as an array: the intended message)
        _learner(monkeypatch, tmp_path, continuous_action_clip=np.array([-1.0, 1.0]))
    for bad in ((1.0, -1.0), (0.0, float("inf")), (1.0,), "ab", np.array([1.0, -1.0])):
        with pytest.raises(ValueError, match="continuous_action_clip"):
            _learner(monkeypatch, tmp_path, continuous_head="diag", continuous_action_clip=bad)


def test_learner_wraps_the_environment_factory(monkeypatch, tmp_path):
    """With "diag" the manager is handed a ClippedEnvFactory ((-1, 1) by default, none with None); with the reference head the
    caller's own function.  (The PPOLearner, where the GPU begins, is replaced by a stand-in that ends the construction.)"""
    from rlgym_ppo_amd import learner as LM
    from rlgym_ppo_amd.util.action_clip import ClippedEnvFactory

    class Reached(Exception):
        pass

    def stand_in(*a, **k):
        raise Reached(k["policy_type"])
    monkeypatch.setattr(LM, "PPOLearner", stand_in)
    for kw, want in (({"continuous_head": "diag"}, (-1.0, 1.0)), ({"continuous_head": "diag", "continuous_action_clip": (-2, 0.5)}, (-2.0, 0.5)),
                     ({"continuous_head": "diag", "continuous_action_clip": np.array([-2.0, 0.5])}, (-2.0, 0.5)),
                     ({"continuous_head": "diag", "continuous_action_clip": None}, None), ({}, None)):
        _Agent.build_env_fn = None
        with pytest.raises(Reached) as reached:
            _learner(monkeypatch, tmp_path, **kw)
        assert reached.value.args[0] == (3 if kw else 2)   # PPOLearner's policy_type: 3 = the diagonal-Gaussian head
        fn = _Agent.build_env_fn
        if want is None:
            assert fn is synthetic_env.make_continuous_wire_env
        else:
            assert isinstance(fn, ClippedEnvFactory) and (fn.lo, fn.hi) == want and fn.build_env_fn is synthetic_env.make_continuous_wire_env


class _MaskedBox(synthetic_env.SyntheticEnv):
    def __init__(self):
        super().__init__(obs_dim=5, n_actions=3, n_agents=2, ep_len=4, seed=1, kind="continuous")
        self.seen = []

    def step(self, actions):
        self.seen.append(np.array(actions, copy=True))
        return super().step(actions)

    def action_masks(self):
        return np.ones((2, 3), bool)


def _make_masked_box():
    return _MaskedBox()


def test_clip_wrapper_clips_delegates_and_pickles():
    from rlgym_ppo_amd.util.action_clip import ActionClipEnv, ClippedEnvFactory, check_clip
    assert check_clip(None) is None and check_clip((-1, 2)) == (-1.0, 2.0) and check_clip(np.array([0.0, 1.0])) == (0.0, 1.0)
    factory = ClippedEnvFactory(_make_masked_box, -1.0, 0.5)
    env = factory()
    assert isinstance(env, ActionClipEnv)
    assert env.reset().shape == (2, 5)
    acts = np.array([[-3.0, 0.25, 7.0], [0.5, -1.0, 0.75]], np.float32)
    out = env.step(acts)
    assert len(out) == 5
    np.testing.assert_array_equal(env._env.seen[0], np.array([[-1.0, 0.25, 0.5], [0.5, -1.0, 0.5]], np.float32))
    np.testing.assert_array_equal(acts[0], [-3.0, 0.25, 7.0])   # the caller's array (what the buffer keeps) is untouched
    # everything else is the environment's
    assert env.action_space is env._env.action_space and env.observation_space is env._env.observation_space
    assert hasattr(env, "action_masks") and env.action_masks().shape == (2, 3) and env.n_agents == 2
    plain = ClippedEnvFactory(synthetic_env.make_continuous_wire_env, -1.0, 1.0)()
    assert not hasattr(plain, "action_masks")
    with pytest.raises(AttributeError):
        plain.no_such_attribute
    # the spawn path pickles the factory (and may pickle an environment)
    f2 = pickle.loads(pickle.dumps(factory))
    assert (f2.lo, f2.hi) == (-1.0, 0.5) and isinstance(f2(), ActionClipEnv)
    e2 = pickle.loads(pickle.dumps(env))
    e2.step(acts)
    assert float(np.max(e2._env.seen[-1])) == 0.5


def test_policy_refuses_bad_arguments_before_it_touches_the_gpu():
    from rlgym_ppo_amd.ppo import DiagGaussianPolicy
    from rlgym_ppo_amd.ppo.diag_gaussian_policy import check_log_std_init
    from rlgym_ppo_amd import _native as N
    assert check_log_std_init(-0.5) == -0.5
    with pytest.raises(ValueError, match="log_std_init"):
        DiagGaussianPolicy(20, 3, (32, 32), "cuda:0", log_std_init=float("nan"))
    for k in (0, N.DIAG_MAX_K + 1):
        with pytest.raises(ValueError, match="RLPPO_DIAG_MAX_K"):
            DiagGaussianPolicy(20, k, (32, 32), "cuda:0")
    ps = list(inspect.signature(DiagGaussianPolicy.get_action).parameters)
    assert ps == ["self", "obs", "deterministic", "noise", "standardize", "action_mask"]
    with pytest.raises(ValueError, match="Gaussian"):
        DiagGaussianPolicy.get_action(object.__new__(DiagGaussianPolicy), None, action_mask=np.ones((1, 3)))


def test_yardstick_closed_forms_equal_torch_distributions():
    rs = np.random.RandomState(0)
    for k in (1, 3, 33):
        mean, acts = rs.randn(50, k) * 3, rs.randn(50, k) * 4
        e_lp, e_ent = Y.check_closed_form(mean, rs.uniform(-2, 1, k), acts)
        assert e_lp <= 1e-12 and e_ent <= 1e-12
    # and its minibatch: float32 against float64 on a one-layer policy is pure rounding
    torch.manual_seed(0)
    from oracle import nets
    pol, val = nets.init_mlp(13, (), 3), nets.init_mlp(13, (), 1)
    ls = rs.uniform(-1, 0.5, 3)
    obs = rs.randn(64, 13)
    _, acts, logp = Y.sample64(pol, ls, obs, rs.randn(64, 3))
    args = ("diag", pol, val, obs, acts, logp + 0.3 * rs.randn(64), rs.randn(64), rs.randn(64), 0.2, 0.005, 0.5)
    r64, r32 = PY.minibatch(torch.float64, *args, log_std=ls), PY.minibatch(torch.float32, *args, log_std=ls)
    assert PY.err(PY.tensors(r32), PY.tensors(r64)) < 1e-5
    assert abs(r64["entropy"] - float((Y.ENT_C + ls).sum())) < 1e-12
    # the hand-derived log_std gradient of the header, in float64
    f = lambda t: np.asarray(t, np.float64)
    mean = obs @ f(pol[0][0]).T + f(pol[0][1])
    sd2 = np.exp(2 * ls)
    ratio, A = r64["ratio"], f(args[6])
    w = ppo_weight(ratio, A, 0.2)
    g_logp = 0.5 * (-(A * w * ratio) / 64)
    want = (g_logp[:, None] * ((acts - mean) ** 2 / sd2 - 1.0)).sum(0) - 0.5 * 0.005
    assert np.abs(r64["grad_log_std"] - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


def ppo_weight(ratio, adv, clip):
    from oracle import ppo
    return ppo.surrogate_weight(ratio, adv, clip)


def test_tail_layout_arithmetic():
    """What NetArena's tail relies on: rlppo_flat_floats counts the layers alone, so [n_net, n_net + k) is the tail."""
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.engine import NetArena
    L = N.lib()
    assert L.rlppo_flat_floats(N.dims_array([231, 512, 512, 512, 512, 8]), 5) == 231 * 512 + 512 + 3 * (512 * 512 + 512) + 512 * 8 + 8
    assert "tail" in inspect.signature(NetArena.__init__).parameters
