"""CPU checks of the critic's own observations (asymmetric actor-critic; include/rlppo.h "[critic rows]", ppo.ObsSizes,
ExperienceBuffer.critic_states, Learner(critic_observations=True)): the refusals, each before the GPU is needed where that is possible;
the added entry points at the C boundary (argument errors come before the first HIP call, so placeholders do); the vector manager's
first answer; the checkpoint book.  No GPU, no compute call."""
import ctypes
import inspect
import json
import warnings

import numpy as np
import pytest
import torch

import critic_obs_env as CE
import synthetic_env


# ------------------------------------------------------------------------------------------------ Learner
def test_learner_refusals_come_before_anything_is_built(monkeypatch, tmp_path):
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd import learner as LM
    p = inspect.signature(Learner.__init__).parameters["critic_observations"]
    assert p.default is False

    def never(*a, **k):
        raise AssertionError("the refusal must come before the collection manager is built")
    monkeypatch.setattr(LM, "BatchedAgentManager", never)
    monkeypatch.setattr(LM, "VectorAgentManager", never)
    monkeypatch.setattr(LM, "ExperienceBuffer", never)
    kw = dict(device="cuda:0", checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False, checkpoint_load_folder=None)
    with pytest.raises(ValueError, match="critic_observations=True needs vector_env=True.*[Pp]rocess-mode"):
        LM.Learner(synthetic_env.make_wire_env, critic_observations=True, **kw)
    with pytest.raises(ValueError, match="critic_observations=True together with gae_bootstrap_truncated=True"):
        LM.Learner(CE.make(False), critic_observations=True, vector_env=True, gae_bootstrap_truncated=True, **kw)


def test_learner_refuses_an_environment_without_the_method_and_hands_the_size_on(monkeypatch, tmp_path):
    """The environment is built by the manager, so this refusal is the manager's (init_processes, before the PPOLearner -- where the GPU
    begins -- is built); with the method, PPOLearner receives ObsSizes(policy, critic) taken from the first answer."""
    from rlgym_ppo_amd import learner as LM
    from rlgym_ppo_amd.ppo import ObsSizes
    monkeypatch.setattr(LM, "ExperienceBuffer", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)

    class Reached(Exception):
        pass

    def stand_in(obs_space_size, *a, **k):
        raise Reached(obs_space_size)
    monkeypatch.setattr(LM, "PPOLearner", stand_in)
    kw = dict(device="cuda:0", vector_env=True, checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False, checkpoint_load_folder=None)
    with pytest.raises(ValueError, match="critic_observations=True needs a vector environment with a critic_observations\\(\\) method"):
        LM.Learner(CE.NoCriticEnv, critic_observations=True, **kw)
    with pytest.raises(Reached) as reached:
        LM.Learner(CE.make(False), critic_observations=True, **kw)
    sizes = reached.value.args[0]
    assert isinstance(sizes, ObsSizes) and (sizes.policy, sizes.critic) == (CE.OBS, CE.CRITIC_OBS)
    with pytest.raises(Reached) as reached:   # the default: an integer, as it always was; the environment is never asked
        LM.Learner(CE.make(False), **kw)
    assert not isinstance(reached.value.args[0], ObsSizes) and int(reached.value.args[0]) == CE.OBS


def test_manager_first_answer():
    """init_processes asks once after reset(): the width, the statistics' first increment (the rows themselves stay RAW for the first
    collect), and a wrong shape by name."""
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    env = CE.CriticVectorEnv(alias=False, n_agents=8)
    mgr = VectorAgentManager(None, seed=5, standardize_obs=True)
    mgr.critic_observations = True
    mgr.init_processes(0, lambda: env)
    assert env.critic_calls == 1 and mgr.critic_obs_size == CE.CRITIC_OBS
    first = mgr._critic_initial
    assert first.shape == (8, CE.CRITIC_OBS) and first.dtype == np.float32 and np.array_equal(first[:, :CE.OBS], mgr._initial_obs)
    from rlgym_ppo_amd.util import WelfordRunningStat
    want = WelfordRunningStat(CE.CRITIC_OBS)
    want.increment(first, 8)
    assert mgr.critic_obs_stats.count == 8 and np.array_equal(mgr.critic_obs_stats.mean, want.mean) and np.array_equal(mgr.critic_obs_stats.std, want.std)
    env.critic_observations = lambda: np.zeros((8, CE.CRITIC_OBS + 1), np.float32)
    with pytest.raises(ValueError, match=r"critic_observations\(\) has shape \(8, 30\)"):
        mgr._critic_answer()
    off = VectorAgentManager(None, seed=5)
    env2 = CE.CriticVectorEnv(alias=False)
    off.init_processes(0, lambda: env2)
    assert env2.critic_calls == 0 and off.critic_obs_stats is None and off.critic_value_input_rows is None   # off: never asked


# ------------------------------------------------------------------------------------------------ PPOLearner / ExperienceBuffer
def test_obs_sizes_and_the_pinned_constructor():
    from rlgym_ppo_amd.ppo import ObsSizes, PPOLearner
    s = ObsSizes(13, 29)
    assert (s.policy, s.critic) == (13, 29) and "29" in repr(s)
    for bad in ((0, 29), (13, -1), (13, 2.5), (True, 3), (13, None)):
        with pytest.raises(ValueError, match="ObsSizes"):
            ObsSizes(*bad)
    assert list(inspect.signature(PPOLearner.__init__).parameters)[-1] == "max_grad_norm"   # the sizes travel in obs_space_size


def test_ppo_learner_refuses_bf16_with_critic_rows():
    """PPOLearner._check_options on a stand-in that holds only what the check reads (tests/test_hidden_activation_host.py)."""
    from rlgym_ppo_amd.ppo import PPOLearner

    class Net:
        hidden_activation = "relu"

    class Opt:
        param_groups = [{"lr": 3e-4}]

    class Buf:
        def __init__(self, width):
            self.critic_width = width

    def learner(critic, prec):
        s = object.__new__(PPOLearner)
        s.policy, s.value_net, s.update_precision, s.critic_obs_space_size = Net(), Net(), prec, critic
        s.lr_schedule, s.desired_kl, s.lr_bounds = "constant", 0.01, (1e-5, 1e-2)
        s.policy_optimizer = s.value_optimizer = Opt()
        s.fused_optimizer_step, s.value_clip_range, s.target_kl, s.max_grad_norm = True, None, None, 0.5
        return s
    with pytest.raises(ValueError, match="update_precision='bf16' with separate critic observations"):
        learner(29, "bf16")._check_options()
    with pytest.raises(ValueError, match="update_precision='bf16' with separate critic observations"):
        learner(None, "bf16")._check_options(Buf(13))   # a buffer with critic_states of the policy's width takes the same entry point
    learner(None, "bf16")._check_options(Buf(None))
    learner(None, "bf16")._check_options()
    for prec in ("fp32", "x3", None):
        learner(29, prec)._check_options(Buf(29))


def test_buffer_holds_critic_states_for_every_row_or_for_none():
    """The check comes before anything is copied: a stand-in that holds only the FIFO's counters needs no GPU."""
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    from rlgym_ppo_amd.ppo.experience_buffer import _FIELDS
    assert inspect.signature(ExperienceBuffer.submit_experience).parameters["critic_states"].default is None
    z = np.zeros(4, np.float32)
    rows = (np.zeros((4, 13), np.float32), z, z, z, np.zeros((4, 13), np.float32), z, z, z, z)
    buf = object.__new__(ExperienceBuffer)
    buf._cap, buf._count, buf._fields = 8, 4, _FIELDS
    with pytest.raises(ValueError, match="holds experience without critic_states and this submit comes with them"):
        buf.submit_experience(*rows, critic_states=np.zeros((4, 29), np.float32))
    buf._fields = _FIELDS + ("critic_states",)
    with pytest.raises(ValueError, match="holds experience with critic_states and this submit comes without them"):
        buf.submit_experience(*rows)
    assert buf.critic_width is None or buf.critic_width == buf._dc
    buf._fields = _FIELDS
    assert buf.critic_states is None and buf.critic_width is None and buf.action_masks is None


# ------------------------------------------------------------------------------------------------ the C boundary
def _args(N, pol, val, mb=300):
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.slot, a.precision = N.HEAD_DISCRETE, len(pol) - 1, len(val) - 1, 1, 0, N.PRECISION_FP32
    keep = (N.dims_array(pol), N.dims_array(val))
    a.pol_dims = ctypes.cast(keep[0], ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(keep[1], ctypes.POINTER(ctypes.c_int32))
    fake = iter(range(0x10000, 0x1000000, 0x1000))   # distinct, 16-byte aligned, never dereferenced
    for f in ("pol_packed", "val_packed", "pol_grad", "val_grad", "states", "actions", "old_logp", "targets", "advantages", "idx", "stats", "workspace"):
        setattr(a, f, next(fake))
    a.ld_states, a.n_rows, a.mb = 16, 420, mb
    a.clip_range, a.ent_coef, a.mb_ratio, a.var_m, a.var_b = 0.2, 0.005, 1.0, 1.0, 0.0
    return a, keep


def test_c_boundary_refusals_before_any_hip_call():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    pol, val = [13, 64, 128, 6], [29, 32, 64, 1]
    size = lambda fn, prec=N.PRECISION_FP32, mb=300: int(fn(N.dims_array(pol), 3, N.dims_array(val), 3, mb, prec))
    # the size: the old plan + [mb][padded critic width] floats, in every precision; the old functions' values do not move
    for prec in (N.PRECISION_FP32, N.PRECISION_BF16, N.PRECISION_X3):
        for mb in (1, 300, 65536):
            assert size(L.rlppo_minibatch_workspace_bytes_critic, prec, mb) == size(L.rlppo_minibatch_workspace_bytes_for, prec, mb) + 4 * mb * 32
    assert int(L.rlppo_padded_width(29)) == 32

    def call(a, ld=32, states=0x2000000):
        cr = N.CriticRows()
        cr.states, cr.ld_states = states, ld
        passes = L.rlppo_dbg_counter(2), L.rlppo_dbg_counter(N.COUNTER_CRITIC_ROWS_PASS)
        rc = L.rlppo_ppo_minibatch_critic(None, ctypes.byref(a), None, ctypes.byref(cr))
        assert (L.rlppo_dbg_counter(2), L.rlppo_dbg_counter(N.COUNTER_CRITIC_ROWS_PASS)) == passes   # refused before the pass was counted
        return rc, L.rlppo_last_error().decode()

    a, keep = _args(N, pol, val)
    a.ws_bytes = size(L.rlppo_minibatch_workspace_bytes_critic)
    rc, msg = call(a, ld=28)
    assert rc == 1001 and "critic ld_states=28" in msg and "32" in msg, (rc, msg)
    rc, msg = call(a, ld=34)
    assert rc == 1001 and "multiple of 4" in msg, (rc, msg)
    rc, msg = call(a, states=0x2000004)
    assert rc == 1001 and "16-byte aligned" in msg, (rc, msg)
    a.precision = N.PRECISION_BF16
    a.ws_bytes = size(L.rlppo_minibatch_workspace_bytes_critic, N.PRECISION_BF16)
    rc, msg = call(a)
    assert rc == 1001 and "bf16" in msg and "separate critic rows" in msg, (rc, msg)
    a.precision = N.PRECISION_FP32
    a.ws_bytes = size(L.rlppo_minibatch_workspace_bytes_for)                       # sized with the old function
    rc, msg = call(a)
    assert rc != 0 and rc != 1001 and "workspace" in msg and "rlppo_minibatch_workspace_bytes_critic" in msg, (rc, msg)
    # without a critic matrix the old rule stands: two widths are refused by the old message
    a.ws_bytes = size(L.rlppo_minibatch_workspace_bytes_critic)
    rc = L.rlppo_ppo_minibatch_critic(None, ctypes.byref(a), None, None)
    assert rc == 1001 and b"observe different sizes" in L.rlppo_last_error()
    rc, msg = call(a, states=0)
    assert rc == 1001 and "observe different sizes" in msg
    assert L.rlppo_dbg_counter(14) == -1 and L.rlppo_dbg_counter(N.COUNTER_CRITIC_ROWS_PASS) >= 0 and L.rlppo_dbg_counter(16) == -1


def test_gather_rows2_refusals():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    assert L.rlppo_gather_rows2(None, None) == 1001
    g = N.Gather2Args()
    assert L.rlppo_gather_rows2(None, ctypes.byref(g)) == 0          # n == 0: nothing to do
    g.n, g.src, g.critic_src, g.dst, g.critic_dst, g.idx = 5, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    g.width, g.ld_src, g.critic_width, g.critic_ld_src = 12, 16, 16, 12
    assert L.rlppo_gather_rows2(None, ctypes.byref(g)) == 1001 and b"critic width=16 ld=12" in L.rlppo_last_error()
    g.critic_ld_src, g.g_old = 16, 0x60000
    assert L.rlppo_gather_rows2(None, ctypes.byref(g)) == 1001 and b"come together" in L.rlppo_last_error()
    g.g_old, g.dst = None, 0x30004
    assert L.rlppo_gather_rows2(None, ctypes.byref(g)) == 1001 and b"16-byte aligned" in L.rlppo_last_error()
    g.dst, g.ring_cap, g.ring_base = 0x30000, 8, 8
    assert L.rlppo_gather_rows2(None, ctypes.byref(g)) == 1001 and b"ring_base" in L.rlppo_last_error()


# ------------------------------------------------------------------------------------------------ the checkpoint book
class _Ppo:
    cumulative_model_updates = 7

    def save_to(self, folder):
        pass

    def load_from(self, folder):
        pass


class _Mgr:
    standardize_obs, cumulative_timesteps, average_reward = True, 1234, 0.5


def _book_learner(tmp_path, critic=True):
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd.util import WelfordRunningStat
    s = object.__new__(Learner)
    s.checkpoints_save_folder, s.n_checkpoints_to_keep, s.add_unix_timestamp = str(tmp_path), 5, False
    s.ppo_learner, s.agent, s.epoch, s.ts_since_last_save, s.wandb_run = _Ppo(), _Mgr(), 3, 0, None
    s.return_stats, s.critic_observations = WelfordRunningStat(1), critic
    s.agent.obs_stats, s.agent.critic_obs_stats = WelfordRunningStat(CE.OBS), WelfordRunningStat(CE.CRITIC_OBS)
    return s


def test_checkpoint_book_round_trip(tmp_path):
    rs = np.random.RandomState(0)
    a = _book_learner(tmp_path)
    a.agent.obs_stats.increment(rs.randn(40, CE.OBS).astype(np.float32), 40)
    a.agent.critic_obs_stats.increment(rs.randn(40, CE.CRITIC_OBS).astype(np.float32) * 3 + 1, 40)
    a.save(1234)
    book = json.load(open(tmp_path / "1234" / "BOOK_KEEPING_VARS.json"))
    as_json = lambda st: json.loads(json.dumps(st.to_json()))
    assert book["critic_obs_running_stats"] == as_json(a.agent.critic_obs_stats) and book["critic_obs_running_stats"] != book["obs_running_stats"]
    b = _book_learner(tmp_path)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b.load(str(tmp_path / "1234"), False)
    assert as_json(b.agent.critic_obs_stats) == as_json(a.agent.critic_obs_stats) and b.agent.critic_obs_stats.count == 40
    assert np.allclose(b.agent.critic_obs_stats.mean, a.agent.critic_obs_stats.mean) and np.asarray(b.agent.critic_obs_stats.mean).size == CE.CRITIC_OBS
    assert as_json(b.agent.obs_stats) == as_json(a.agent.obs_stats)
    # off: the key is not written, and a book that has it is read as it always was
    c = _book_learner(tmp_path / "off", critic=False)
    c.save(1234)
    assert "critic_obs_running_stats" not in json.load(open(tmp_path / "off" / "1234" / "BOOK_KEEPING_VARS.json"))
    d = _book_learner(tmp_path, critic=False)
    fresh = d.agent.critic_obs_stats
    d.load(str(tmp_path / "1234"), False)
    assert d.agent.critic_obs_stats is fresh


def test_checkpoint_without_the_key_loads_with_a_warning(tmp_path):
    old = _book_learner(tmp_path, critic=False)
    old.save(1234)
    new = _book_learner(tmp_path)
    fresh = new.agent.critic_obs_stats
    with pytest.warns(RuntimeWarning, match="critic_obs_running_stats.*start fresh"):
        new.load(str(tmp_path / "1234"), False)
    assert new.agent.critic_obs_stats is fresh and fresh.count == 0 and new.epoch == 3
