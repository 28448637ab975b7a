"""Invalid-action masking of a MultiDiscrete environment in process-mode collection, the host side: the worker's trailer (S =
sum(nvec) floats per agent behind the observation, one per logit) and its four-float shapes reply, the manager's decision
(_configure_masking accepts action-space type 1; the masks' width is held against the policy's bins once the policy is known), the
per-head rule of both learner-side loops (the Python loop and rlppo_collector_ready_masks after rlppo_collector_set_mask_heads)
and the masks the loops return.  Real worker processes where a loop is driven; ONE worker, so that arrival order is fixed and the
two loops must agree value for value.  CPU only."""
import ctypes
import socket

import numpy as np
import pytest
import torch

import masked_multidiscrete_wire_env as W
import multidiscrete_env as E

NVEC = list(W.NVEC)
S, H = sum(NVEC), len(NVEC)
CALLS = (40, 17, 1, 33)


class _NvecPolicy:
    """The layout the manager reads (n_logits, splits) and a get_action that insists on one S-wide mask row per observation and picks
    the lowest valid bin of every head."""

    def __init__(self, nvec=NVEC):
        self.splits, self.n_logits, self.calls = list(nvec), sum(nvec), 0

    def get_action(self, obs, action_mask=None):
        obs = np.asarray(obs, np.float32)
        assert action_mask is not None, "a masked run hands every call its masks"
        m = np.asarray(action_mask) != 0
        assert m.shape == (obs.shape[0], self.n_logits)
        self.calls += 1
        act = np.stack([m[:, s:s + b].argmax(axis=1) for s, b in zip(W.starts(self.splits), self.splits)], axis=1)
        return torch.as_tensor(act.astype(np.int64)), torch.as_tensor(-np.abs(obs[:, 0]).astype(np.float32))


class _PlainPolicy:
    """The reference's signature: it would fail on an action_mask keyword."""

    def get_action(self, obs):
        obs = np.asarray(obs, np.float32)
        return torch.zeros((obs.shape[0], H), dtype=torch.int64), torch.as_tensor(-np.abs(obs[:, 0]).astype(np.float32))


def _layout(prev_n, done, trunc, rews, obs):
    """The slab of one step without metrics as comm_consts.py documents it, stated independently of StepSlab."""
    return np.concatenate([np.asarray([prev_n, done, trunc, obs.ndim, 0], np.float32), np.asarray(obs.shape, np.float32),
                           np.asarray(rews, np.float32), obs.ravel()])


# --------------------------------------------------------------------------------------------------- 1. the worker and the wire
@pytest.mark.parametrize("rank1", [False, True])
def test_trailer_is_one_float_per_logit_and_absent_without_the_method(rank1):
    from rlgym_ppo_amd.batched_agents import comm_consts as C
    from rlgym_ppo_amd.batched_agents.batched_agent import StepSlab, env_action_masks, reset_state_message
    from rlgym_ppo_amd.batched_agents.batched_agent_manager import parse_reset_state, parse_step_slab
    env = (W.MaskedNvecSingleEnv if rank1 else W.MaskedNvecEnv)()
    plain_env = E.NvecEnv()
    obs = np.asarray(env.reset(), np.float32)
    n_agents = 1 if rank1 else 2
    assert obs.shape == ((W.OBS_DIM,) if rank1 else (2, W.OBS_DIM)) and not hasattr(plain_env, "action_masks")
    mask = env_action_masks(env, n_agents)
    assert mask.dtype == np.float32 and mask.shape == (n_agents, S) and set(np.unique(mask)) <= {0.0, 1.0} and (mask == 0).any()
    assert np.array_equal(mask != 0, W.mask_of(obs).reshape(n_agents, S))
    for s, b in zip(W.starts(NVEC), NVEC):                       # every head of every row keeps a valid bin
        assert (mask[:, s:s + b].sum(1) >= 1).all()
    rews = [0.25] if rank1 else [0.25, -1.5]
    want = _layout(n_agents, 0.0, 1.0, rews, obs)
    plain, masked = StepSlab(bytearray(4 * 256), 0, 256), StepSlab(bytearray(4 * 256), 0, 256)
    n_plain = plain.write_step(n_agents, 0.0, 1.0, rews, np.empty((0,), np.float32), (), obs)
    n_masked = masked.write_step(n_agents, 0.0, 1.0, rews, np.empty((0,), np.float32), (), obs, mask)
    # without the method: exactly today's floats; with it: the same floats followed by n_agents x S floats of 0 / 1
    assert n_plain == want.size and plain.view[:n_plain].tobytes() == want.tobytes() and not np.any(plain.view[n_plain:])
    assert n_masked == n_plain + n_agents * S and masked.view[:n_plain].tobytes() == want.tobytes()
    assert masked.view[n_plain:n_masked].tobytes() == mask.tobytes() and not np.any(masked.view[n_masked:])
    if not rank1:
        assert n_masked == C.step_slab_floats(n_agents, n_agents, W.OBS_DIM, n_actions=S)
    pm = parse_step_slab(masked.view, S)
    assert len(pm) == 7 and pm[6].dtype == bool and np.array_equal(pm[6], mask != 0) and np.array_equal(pm[5], obs.reshape(n_agents, -1))
    assert len(parse_step_slab(plain.view)) == 6
    shape = [float(d) for d in obs.shape]
    today = C.pack_message(C.ENV_RESET_STATE_HEADER + [float(len(shape))] + shape) + obs.tobytes()
    assert reset_state_message(obs) == today and reset_state_message(obs, mask) == today + mask.tobytes()
    o, m = parse_reset_state(np.frombuffer(today + mask.tobytes(), np.float32))
    assert np.array_equal(o, obs.reshape(n_agents, -1)) and m.shape == (n_agents, S) and np.array_equal(m, mask != 0)


def test_size_checks_hold_at_the_widest_mask():
    """512 logits (RLPPO_MD_MAX_LOGITS) per agent: a reset datagram that fits PACKET_MAX_SIZE is sent and read back whole, an
    over-long one is reported by the worker -- not truncated -- and the slab has its own assertion."""
    from rlgym_ppo_amd.batched_agents import comm_consts as C
    from rlgym_ppo_amd.batched_agents.batched_agent import StepSlab, reset_state_message
    from rlgym_ppo_amd.batched_agents.batched_agent_manager import parse_reset_state
    rs = np.random.RandomState(0)
    width = 512
    obs, mask = rs.randn(3, 23).astype(np.float32), (rs.rand(3, width) < 0.5).astype(np.float32)
    msg = reset_state_message(obs, mask)
    assert len(msg) == 4 * (3 + 1 + 2 + 3 * 23 + 3 * width) <= C.PACKET_MAX_SIZE
    o, m = parse_reset_state(np.frombuffer(msg, np.float32))
    assert np.array_equal(o, obs) and m.shape == (3, width) and np.array_equal(m, mask != 0)
    obs4, mask4 = rs.randn(4, 23).astype(np.float32), np.ones((4, width), np.float32)
    assert 4 * (3 + 1 + 2 + 4 * 23 + 4 * width) > C.PACKET_MAX_SIZE
    with pytest.raises(AssertionError, match=r"LARGER THAN THE LARGEST DATAGRAM THE LEARNER READS \(8584 > 8192 BYTES\)"):
        reset_state_message(obs4, mask4)
    assert len(reset_state_message(obs4)) == 4 * (6 + 4 * 23)         # without a mask the datagram is whatever it was
    need = C.step_slab_floats(3, 3, 23, n_actions=width)
    assert StepSlab(bytearray(4 * need), 0, need).write_step(3, 0.0, 0.0, [0.0] * 3, np.empty((0,), np.float32), (), obs, mask) == need
    with pytest.raises(AssertionError, match="LARGER THAN MAXIMUM"):
        StepSlab(bytearray(4 * (need - 1)), 0, need - 1).write_step(3, 0.0, 0.0, [0.0] * 3, np.empty((0,), np.float32), (), obs, mask)


def _shapes_reply(env_fn):
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    from rlgym_ppo_amd.batched_agents.batched_agent_manager import ENV_SHAPES
    mgr = BatchedAgentManager(None, min_inference_size=1, seed=5, standardize_obs=False)
    try:
        shapes = mgr.init_processes(1, env_fn, shm_buffer_size=4096)
        w = mgr.processes[0]
        w.request_shapes()
        msg = w.recv()
        while msg is None or msg[0] != ENV_SHAPES:
            msg = w.recv()
        return shapes, msg, mgr.masked, mgr.n_actions, mgr.mask_space_type, mgr.current_mask[0], mgr.current_obs[0]
    finally:
        mgr.cleanup()


def test_shapes_reply_of_a_worker_process_has_type_1_and_a_fourth_float_when_masked():
    shapes, msg, masked, width, code, mask0, obs0 = _shapes_reply(W.make_masked_nvec_env)
    assert shapes == (W.OBS_DIM, H, 1) and msg[1:] == (float(W.OBS_DIM), float(H), 1.0, 1.0)
    assert masked and width == S and code == 1                        # the reply carries len(nvec): the width comes from the trailer
    assert mask0.shape == (2, S) and np.array_equal(mask0, W.mask_of(obs0))
    shapes, msg, masked, width, code, mask0, _ = _shapes_reply(E.make_env)
    assert shapes == (W.OBS_DIM, H, 1) and msg[1:] == (float(W.OBS_DIM), float(H), 1.0) and not masked and width == 0 and mask0 is None


# --------------------------------------------------------------------------------------- 2. the manager's decision, no worker
def _configured(masks, reply, policy=None):
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    from rlgym_ppo_amd.batched_agents.batched_agent_manager import ENV_SHAPES
    mgr = BatchedAgentManager(policy)
    mgr.current_mask = list(masks)
    mgr._configure_masking((ENV_SHAPES,) + tuple(reply))
    return mgr


def test_configure_masking_accepts_type_1_and_checks_the_width_against_the_policy():
    from rlgym_ppo_amd.ppo.continuous_policy import ContinuousPolicy
    from rlgym_ppo_amd.ppo.discrete_policy import DiscreteFF
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF
    ones = np.ones((2, S), bool)
    mgr = _configured([ones, ones], (23.0, float(H), 1.0, 1.0))
    assert mgr.masked and mgr.n_actions == S and mgr.mask_space_type == 1
    # the policy is known later: the layout is the policy's (util.action_mask.Layout.of), a duck-typed one's from (n_logits, splits)
    from rlgym_ppo_amd.util.action_mask import Layout
    mgr.policy = _NvecPolicy()
    lay = mgr._mask_layout()
    assert lay.width == S and lay.heads == tuple(NVEC) and lay.words == 1 and list(lay.starts) == W.starts(NVEC)
    pol = object.__new__(MultiDiscreteFF)                             # (no GPU: the attributes the check reads)
    pol.__dict__.update(n_logits=S, splits=list(NVEC), mask_layout=Layout(S, NVEC))
    mgr = _configured([ones], (23.0, float(H), 1.0, 1.0), pol)
    assert mgr._mask_layout() is pol.mask_layout and Layout.of(mgr.policy) is mgr.policy.mask_layout
    # a width other than sum(splits): both numbers are named, whichever side is wrong
    mgr = _configured([np.ones((2, H), bool)], (23.0, float(H), 1.0, 1.0), _NvecPolicy())
    with pytest.raises(ValueError, match=rf"\b{H} entries.*\b{S} logits"):
        mgr._mask_layout()
    mgr = _configured([ones], (23.0, float(H), 1.0, 1.0), _NvecPolicy([2, 7, 3, 11, 3]))
    with pytest.raises(ValueError, match=rf"\b{S} entries.*\b{S + 1} logits"):
        mgr._mask_layout()
    with pytest.raises(ValueError, match=rf"\b{S} entries.*\b{S + 1} logits"):          # (asked again: not cached as fine)
        mgr.collect_timesteps(1)
    with pytest.raises(ValueError, match="different widths"):
        _configured([ones, np.ones((2, S + 1), bool)], (23.0, float(H), 1.0, 1.0))
    with pytest.raises(ValueError, match="fewer than the 5 components"):
        _configured([np.ones((2, 3), bool)], (23.0, float(H), 1.0, 1.0))
    with pytest.raises(ValueError, match="n_logits, policy.splits"):                    # a policy without a layout
        mgr = _configured([ones], (23.0, float(H), 1.0, 1.0), _PlainPolicy())
        mgr._mask_layout()
    # type 2 (Box) keeps the refusal and its text, as does a policy class without masking
    with pytest.raises(ValueError, match="option of the discrete head.*an action space of type 2"):
        _configured([np.ones((2, 3), bool)], (23.0, 3.0, 2.0, 1.0))
    with pytest.raises(ValueError, match="option of the discrete head.*not of ContinuousPolicy"):
        _configured([ones], (23.0, float(H), 1.0, 1.0), object.__new__(ContinuousPolicy))
    # a masking head that is not the action space's own: the mismatch is named, not "not of" a head that does mask
    with pytest.raises(ValueError, match="type 1 is served by MultiDiscreteFF, the policy is a DiscreteFF"):
        _configured([ones], (23.0, float(H), 1.0, 1.0), object.__new__(DiscreteFF))
    with pytest.raises(ValueError, match="type 0 is served by DiscreteFF, the policy is a MultiDiscreteFF"):
        _configured([np.ones((2, 7), bool)], (13.0, 7.0, 0.0, 1.0), pol)
    # the discrete head is what it was: masks as wide as the action space
    mgr = _configured([np.ones((2, 7), bool)], (13.0, 7.0, 0.0, 1.0))
    assert mgr.masked and mgr.n_actions == 7 and mgr.mask_space_type == 0
    assert mgr._mask_layout().width == 7 and mgr._mask_layout().heads is None and mgr._mask_layout().words == 1
    with pytest.raises(ValueError, match="masks of 6 actions, the action space has 7"):
        _configured([np.ones((2, 6), bool)], (13.0, 7.0, 0.0, 1.0))


def test_python_loop_per_head_check_names_worker_agent_and_head():
    ones = np.ones((2, S), bool)
    bad = ones.copy()
    bad[1, 9:12] = False                                               # agent 1, head 2 (bins 9 .. 11)
    bad[1, 23:25] = False                                              # ... and head 4: the first one is named
    one_each = np.zeros((2, S), bool)
    one_each[:, [s + b - 1 for s, b in zip(W.starts(NVEC), NVEC)]] = True          # exactly the last bin of every head: fine
    mgr = _configured([ones, one_each, bad], (23.0, float(H), 1.0, 1.0), _NvecPolicy())
    rows = mgr._checked_masks([0, 1])
    assert rows.shape == (4, S) and np.array_equal(rows, np.concatenate([ones, one_each]))
    with pytest.raises(ValueError, match=r"worker 2, agent 1, head 2 \(bins 9 \.\. 11\) has no valid bin"):
        mgr._checked_masks([0, 1, 2])


# ------------------------------------------------------------------------------------------------------ 3. the C++ collector
def test_collector_head_layout_and_per_head_rule():
    """rlppo_collector_set_mask_heads after set_masked(S); ready_masks with the layout: RLPPO_ERR_MASK_ROW naming worker, agent and
    head; a row whose heads each keep exactly one bin passes and comes back byte for byte."""
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    sock, peer = socket.socket(socket.AF_INET, socket.SOCK_DGRAM), socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    slab = np.zeros(256, np.float32)
    h = ctypes.c_void_p()
    nvec = (ctypes.c_int32 * H)(*NVEC)
    try:
        sock.bind(("127.0.0.1", 0))
        peer.bind(("127.0.0.1", 0))                                    # the worker's end: this test plays the worker below
        peer.settimeout(10)
        fds, ports = (ctypes.c_int32 * 1)(sock.fileno()), (ctypes.c_int32 * 1)(peer.getsockname()[1])
        N.check(L.rlppo_collector_create(1, fds, ports, ctypes.c_void_p(slab.ctypes.data), slab.size, W.OBS_DIM, ctypes.byref(h)))
        assert L.rlppo_collector_set_mask_heads(h, nvec, H) == 1001 and b"set_masked comes first" in L.rlppo_last_error()
        N.check(L.rlppo_collector_set_masked(h, S))
        wrong = (ctypes.c_int32 * H)(2, 7, 3, 11, 3)
        assert L.rlppo_collector_set_mask_heads(h, wrong, H) == 1001
        err = L.rlppo_last_error().decode()
        assert "collector_set_mask_heads" in err and str(S + 1) in err and str(S) in err, err
        assert L.rlppo_collector_set_mask_heads(h, (ctypes.c_int32 * 2)(S, 0), 2) == 1001 and b"nvec[1] = 0" in L.rlppo_last_error()
        assert L.rlppo_collector_set_mask_heads(h, None, H) == 1001
        N.check(L.rlppo_collector_set_mask_heads(h, nvec, H))
        obs = np.random.RandomState(1).randn(2, W.OBS_DIM).astype(np.float32)
        N.check(L.rlppo_collector_set_obs(h, 0, obs.ctypes.data, 2, 1))
        rows, got = ctypes.c_int64(0), np.full((8, S), 7, np.uint8)
        out = np.zeros((8, W.OBS_DIM), np.float32)

        def ready_masks(mask):
            m8 = np.ascontiguousarray(mask, dtype=np.uint8)
            N.check(L.rlppo_collector_set_mask(h, 0, m8.ctypes.data, 2))
            N.check(L.rlppo_collector_ready(h, out.ctypes.data, 8, ctypes.byref(rows)))
            assert rows.value == 2
            return L.rlppo_collector_ready_masks(h, got.ctypes.data, 8)

        bad = np.ones((2, S), bool)
        bad[1, 2:9] = False                                            # agent 1: head 1 (bins 2 .. 8) is empty; the row is not
        assert ready_masks(bad) == 1005
        assert "worker 0, agent 1, head 1 (bins 2 .. 8) has no valid bin" in L.rlppo_last_error().decode()
        one_each = np.zeros((2, S), bool)
        one_each[0, [s for s in W.starts(NVEC)]] = True                # the first bin of every head
        one_each[1, [s + b - 1 for s, b in zip(W.starts(NVEC), NVEC)]] = True     # the last bin of every head
        assert ready_masks(one_each) == 0 and np.array_equal(got[:2], one_each.astype(np.uint8)) and (got[2:] == 7).all()

        # two steps with this test as the worker: emit_masks returns the masks the actions were sampled under, row for row with
        # _emit's states (agent by agent), S bytes per row next to action rows of width H
        from rlgym_ppo_amd.batched_agents import comm_consts as C
        from rlgym_ppo_amd.batched_agents.batched_agent import StepSlab
        writer = StepSlab(slab.data, 0, slab.size)
        rs = np.random.RandomState(2)
        sent_masks, sent_obs, sent_act = [one_each], [obs], []
        for step in range(2):
            if step:
                N.check(L.rlppo_collector_ready(h, out.ctypes.data, 8, ctypes.byref(rows)))
                assert rows.value == 2 and L.rlppo_collector_ready_masks(h, got.ctypes.data, 8) == 0
                assert np.array_equal(got[:2], sent_masks[-1].astype(np.uint8)) and np.array_equal(out[:2], sent_obs[-1])
            act = np.stack([sent_masks[-1][:, s:s + b].argmax(1) for s, b in zip(W.starts(NVEC), NVEC)], 1).astype(np.float32)
            sent_act.append(act)
            N.check(L.rlppo_collector_send(h, act.ctypes.data, H, np.zeros(2, np.float32).ctypes.data))
            msg = np.frombuffer(peer.recv(4096), np.float32)
            assert msg[:C.HEADER_LEN].tolist() == C.POLICY_ACTIONS_HEADER and np.array_equal(msg[C.HEADER_LEN:].reshape(2, H), act)
            nxt = rs.randn(2, W.OBS_DIM).astype(np.float32)
            m_next = W.mask_of(nxt)
            writer.write_step(2, 0.0, 0.0, [0.5, -0.5], np.empty((0,), np.float32), (), nxt, m_next.astype(np.float32))
            peer.sendto(C.pack_message(C.ENV_STEP_DATA_HEADER), sock.getsockname())
            n_got = ctypes.c_int64(0)
            one = np.ones(1, np.float32)
            N.check(L.rlppo_collector_collect(h, 1, 0, 0, one.ctypes.data, one.ctypes.data, None, None, None, 0, 5, None, ctypes.byref(n_got)))
            assert n_got.value == 2
            sent_masks.append(m_next)
            sent_obs.append(nxt)
        n_steps, aw, n_met, met_floats = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        N.check(L.rlppo_collector_finish(h, ctypes.byref(n_steps), ctypes.byref(aw), ctypes.byref(n_met), ctypes.byref(met_floats)))
        assert n_steps.value == 4 and aw.value == H
        m8 = np.full((4, S), 9, np.uint8)
        N.check(L.rlppo_collector_emit_masks(h, m8.ctypes.data))
        k, d = 4, W.OBS_DIM
        states, nxts, actions, logp = np.empty((k, d), np.float32), np.empty((k, d), np.float32), np.empty((k, H), np.float32), np.empty(k, np.float32)
        rew, dones, trunc = np.empty(k), np.empty(k), np.empty(k)
        mvals, mshapes = np.empty(int(met_floats.value), np.float32), np.zeros((int(n_met.value), 9), np.int32)
        N.check(L.rlppo_collector_emit(h, states.ctypes.data, actions.ctypes.data, logp.ctypes.data, rew.ctypes.data, nxts.ctypes.data,
                                       dones.ctypes.data, trunc.ctypes.data, mvals.ctypes.data, mshapes.ctypes.data))
        order = [(0, 0), (1, 0), (0, 1), (1, 1)]                       # (step, agent): agent by agent
        assert np.array_equal(states, np.stack([sent_obs[t][a] for t, a in order]))
        assert np.array_equal(actions, np.stack([sent_act[t][a] for t, a in order]))
        assert np.array_equal(m8, np.stack([sent_masks[t][a] for t, a in order]).astype(np.uint8))
        assert W.head_valid_actions(m8 != 0, actions).all()
    finally:
        if h:
            L.rlppo_collector_destroy(h)
        sock.close()
        peer.close()
    assert L.rlppo_collector_set_mask_heads(None, nvec, H) == 1001 and b"collector_set_mask_heads" in L.rlppo_last_error()


def test_ctypes_signature_of_the_new_symbols_matches_the_header():
    from rlgym_ppo_amd import _native as N
    header = open(N.HERE + "/../include/rlppo.h").read()
    assert "int rlppo_collector_set_mask_heads(void *handle, const int32_t *nvec, int32_t n_heads);" in header
    res, args = N.SIGNATURES["rlppo_collector_set_mask_heads"]
    assert res == ctypes.c_int32 and args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int32]
    assert "int rlppo_dbg_count(int32_t key, int64_t delta);" in header
    assert N.SIGNATURES["rlppo_dbg_count"] == (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int64])
    assert N.ABI_VERSION == 8 and "#define RLPPO_ABI_VERSION 8" in header
    L = N.lib()
    c6 = L.rlppo_dbg_counter(6)
    assert L.rlppo_dbg_count(6, 3) == 0 and L.rlppo_dbg_counter(6) == c6 + 3
    assert L.rlppo_dbg_count(6, -3) == 0 and L.rlppo_dbg_counter(6) == c6
    assert L.rlppo_dbg_count(2, 1) == 1001 and b"dbg_count" in L.rlppo_last_error()


# ------------------------------------------------------------------------------------------- 4. both loops with a real worker
def _run(native, env_fn, policy, calls=CALLS, n_proc=1):
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    mgr = BatchedAgentManager(policy, min_inference_size=1, seed=5, standardize_obs=False)
    mgr.native_collect = native
    try:
        shapes = mgr.init_processes(n_proc, env_fn, shm_buffer_size=4096)
        out = []
        for k in calls:
            exp, metrics, n, _ = mgr.collect_timesteps(k)
            out.append((exp, n, None if mgr.action_mask_rows is None else np.array(mgr.action_mask_rows, copy=True)))
        if n_proc > 0:
            assert (mgr._native is not None) == native, "the loop that ran is not the one the test asked for"
        return shapes, out, dict(avg=mgr.average_reward, total=mgr.cumulative_timesteps, masked=mgr.masked, width=mgr.n_actions)
    finally:
        mgr.cleanup()


def _check_masks(out):
    """Row-aligned with the states across the call boundaries: every mask is the environment's mask function of its stored state,
    action rows are len(nvec) wide, every stored action is the lowest valid bin of its head, and no step paid the out-of-range
    penalty."""
    n_rows = 0
    for (states, actions, _, rewards, *_), n, masks in out:
        assert masks is not None and masks.dtype == bool and masks.shape == (len(states), S)
        assert np.array_equal(masks, W.mask_of(states))
        a = np.asarray(actions)
        assert a.shape == (len(states), H) and W.head_valid_actions(masks, a).all()
        want = np.stack([masks[:, s:s + b].argmax(axis=1) for s, b in zip(W.starts(NVEC), NVEC)], axis=1)
        assert np.array_equal(a.astype(np.int64), want) and (np.asarray(rewards) < E.OUT_OF_RANGE_REWARD / 2).all()
        n_rows += len(states)
    assert n_rows > 0


@pytest.mark.parametrize("case", ["two_agents", "single_agent_rank1"])
def test_native_loop_equals_the_python_loop_masks_included(case):
    env_fn = {"two_agents": W.make_masked_nvec_env, "single_agent_rank1": W.make_masked_nvec_single_env}[case]
    (s0, o0, t0), (s1, o1, t1) = _run(False, env_fn, _NvecPolicy()), _run(True, env_fn, _NvecPolicy())
    assert s0 == s1 == (W.OBS_DIM, H, 1) and t0 == t1 and t0["masked"] and t0["width"] == S
    for (ea, na, ka), (eb, nb, kb) in zip(o0, o1):
        assert na == nb and len(ea) == len(eb) == 7                    # collect_timesteps keeps its 7-tuple
        for x, y, name in zip(ea, eb, ("states", "actions", "log_probs", "rewards", "next_states", "dones", "truncated")):
            assert x.shape == y.shape and np.array_equal(x, y), name
        assert ka.dtype == kb.dtype == bool and ka.shape == kb.shape and np.array_equal(ka, kb)
    _check_masks(o0)
    _check_masks(o1)


def test_local_worker_carries_the_masks_too():
    pol = _NvecPolicy()
    shapes, out, state = _run(False, W.make_masked_nvec_env, pol, calls=(40, 17), n_proc=0)
    assert shapes == (W.OBS_DIM, H, 1) and state["masked"] and state["width"] == S and pol.calls > 0
    _check_masks(out)


@pytest.mark.parametrize("native", [False, True])
def test_an_unmasked_multidiscrete_environment_is_never_handed_the_keyword(native):
    shapes, out, state = _run(native, E.make_env, _PlainPolicy())
    assert shapes == (W.OBS_DIM, H, 1) and not state["masked"] and all(masks is None for *_, masks in out)


@pytest.mark.parametrize("native", [False, True])
def test_an_empty_head_raises_on_the_learner_before_an_action_is_sent(native):
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    pol = _NvecPolicy()
    mgr = BatchedAgentManager(pol, min_inference_size=1, seed=5, standardize_obs=False)
    mgr.native_collect = native
    try:
        mgr.init_processes(1, W.make_empty_head_env, shm_buffer_size=4096)
        with pytest.raises(ValueError, match=r"worker 0, agent 1, head 1 \(bins 2 \.\. 8\) has no valid bin"):
            mgr.collect_timesteps(40)
        assert (mgr._native is not None) == native
        assert pol.calls == 3   # the three steps before it were served; no action was sent for the bad observation
    finally:
        mgr.cleanup()


@pytest.mark.parametrize("native", [False, True])
def test_masks_with_one_entry_per_component_are_refused_before_the_first_action(native):
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    pol = _NvecPolicy()
    mgr = BatchedAgentManager(pol, min_inference_size=1, seed=5, standardize_obs=False)
    mgr.native_collect = native
    try:
        assert mgr.init_processes(1, W.make_narrow_mask_env, shm_buffer_size=4096) == (W.OBS_DIM, H, 1)
        with pytest.raises(ValueError, match=rf"\b{H} entries.*\b{S} logits"):
            mgr.collect_timesteps(8)
        assert pol.calls == 0 and mgr._native is None
    finally:
        mgr.cleanup()
