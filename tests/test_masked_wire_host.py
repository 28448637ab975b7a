"""The opt-in mask trailer of the worker <-> learner wire format (comm_consts.py): what a worker whose environment has
action_masks() appends, what the manager's parsers make of it, and that without a mask every byte is what it was.  CPU only."""
import socket

import numpy as np
import pytest

import masked_wire_env
import synthetic_env


def _layout(prev_n, done, trunc, rews, metrics, metrics_shape, obs):
    """The slab of one step as comm_consts.py documents it, stated independently of StepSlab."""
    return np.concatenate([np.asarray([prev_n, done, trunc, obs.ndim, len(metrics_shape)], np.float32), np.asarray(metrics_shape, np.float32),
                           np.asarray(obs.shape, np.float32), np.asarray(rews, np.float32), np.asarray(metrics, np.float32).ravel(), obs.ravel()])


@pytest.mark.parametrize("rank1", [False, True])
def test_step_slab_and_reset_datagram_with_and_without_a_mask(rank1):
    from rlgym_ppo_amd.batched_agents import comm_consts as C
    from rlgym_ppo_amd.batched_agents.batched_agent import StepSlab, env_action_masks, reset_state_message
    from rlgym_ppo_amd.batched_agents.batched_agent_manager import parse_reset_state, parse_step_slab
    rs = np.random.RandomState(1)
    A = 7
    obs = (rs.randn(13) if rank1 else rs.randn(2, 13)).astype(np.float32)
    n_agents = 1 if rank1 else 2
    mask = masked_wire_env.mask_of(obs, A).reshape(n_agents, A).astype(np.float32)
    assert set(np.unique(mask)) <= {0.0, 1.0} and (mask.sum(1) >= 1).all() and (mask == 0).any()
    rews = [0.25] if rank1 else [0.25, -1.5]
    metrics = np.asarray([[1.0, 2.0, 3.0]], np.float32)
    want = _layout(n_agents, 1.0, 0.0, rews, metrics, metrics.shape, obs)

    buf_plain, buf_masked = bytearray(4 * 256), bytearray(4 * 256)
    plain, masked = StepSlab(buf_plain, 0, 256), StepSlab(buf_masked, 0, 256)
    n_plain = plain.write_step(n_agents, 1.0, 0.0, rews, metrics, metrics.shape, obs)
    n_masked = masked.write_step(n_agents, 1.0, 0.0, rews, metrics, metrics.shape, obs, mask)
    # without a mask: exactly today's floats; with one: the same floats followed by n_agents x A floats of 0 / 1
    assert n_plain == want.size
    if not rank1:   # (step_slab_floats counts a rank-2 observation's two shape floats)
        assert n_plain == C.step_slab_floats(n_agents, n_agents, 13, metrics.size, metrics.ndim)
        assert n_plain + n_agents * A == C.step_slab_floats(n_agents, n_agents, 13, metrics.size, metrics.ndim, n_actions=A)
    assert plain.view[:n_plain].tobytes() == want.tobytes() and not np.any(plain.view[n_plain:])
    assert n_masked == n_plain + n_agents * A
    assert masked.view[:n_plain].tobytes() == want.tobytes()
    assert masked.view[n_plain:n_masked].tobytes() == mask.tobytes() and not np.any(masked.view[n_masked:])
    # the longer slab falls under the same size assertion
    with pytest.raises(AssertionError, match="LARGER THAN MAXIMUM"):
        StepSlab(bytearray(4 * (n_masked - 1)), 0, n_masked - 1).write_step(n_agents, 1.0, 0.0, rews, metrics, metrics.shape, obs, mask)

    # the manager's parsers
    p = parse_step_slab(plain.view)
    assert len(p) == 6 and np.array_equal(p[5], obs.reshape(n_agents, 13))
    pm = parse_step_slab(masked.view, A)
    assert len(pm) == 7 and pm[6].dtype == bool and np.array_equal(pm[6], mask != 0)
    for x, y in zip(p, pm[:6]):
        assert np.array_equal(np.asarray(x), np.asarray(y))

    shape = [float(d) for d in obs.shape]
    today = C.pack_message(C.ENV_RESET_STATE_HEADER + [float(len(shape))] + shape) + obs.tobytes()
    assert reset_state_message(obs) == today
    assert reset_state_message(obs, mask) == today + mask.tobytes()
    o, m = parse_reset_state(np.frombuffer(today, np.float32))
    assert m is None and np.array_equal(o, obs.reshape(n_agents, 13))
    o, m = parse_reset_state(np.frombuffer(today + mask.tobytes(), np.float32))
    assert np.array_equal(o, obs.reshape(n_agents, 13)) and m.dtype == bool and np.array_equal(m, mask != 0)

    # a masked reset state that the learner could not read whole (it reads PACKET_MAX_SIZE bytes of a datagram) is refused by
    # the worker; without a mask the datagram is whatever it was
    big_obs, big_mask = np.zeros((6, 260), np.float32), np.ones((6, 90), np.float32)
    assert len(reset_state_message(big_obs)) == 4 * (3 + 3 + 6 * 260)
    with pytest.raises(AssertionError, match="LARGER THAN THE LARGEST DATAGRAM"):
        reset_state_message(big_obs, big_mask)

    class Env:
        def action_masks(self):
            return masked_wire_env.mask_of(obs, A)
    assert np.array_equal(env_action_masks(Env(), n_agents), mask) and env_action_masks(Env(), n_agents).dtype == np.float32


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
        return shapes, msg, mgr.masked, mgr.n_actions, mgr.current_mask[0], mgr.current_obs[0]
    finally:
        mgr.cleanup()


def test_shapes_reply_has_four_floats_when_masked_and_three_when_not():
    shapes, msg, masked, n_actions, mask0, obs0 = _shapes_reply(masked_wire_env.make_masked_wire_env)
    assert shapes == (13, 7, 0) and msg[1:] == (13.0, 7.0, 0.0, 1.0) and masked and n_actions == 7
    assert np.array_equal(mask0, masked_wire_env.mask_of(obs0, 7))      # the reset datagram's trailer
    shapes, msg, masked, n_actions, mask0, _ = _shapes_reply(synthetic_env.make_wire_env)
    assert shapes == (13, 7, 0) and msg[1:] == (13.0, 7.0, 0.0) and not masked and n_actions == 0 and mask0 is None


def test_a_three_float_reply_leaves_the_manager_unmasked():
    """What a worker built for the reference answers: three floats, reset states without a trailer."""
    from rlgym_ppo_amd.batched_agents import BatchedAgentManager
    from rlgym_ppo_amd.batched_agents import comm_consts as C
    from rlgym_ppo_amd.batched_agents.batched_agent_manager import ENV_SHAPES, _ProcessWorker
    w = object.__new__(_ProcessWorker)
    w.sock = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    peer = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        w.sock.bind(("127.0.0.1", 0))
        peer.bind(("127.0.0.1", 0))
        w.child, w.n_actions, w.shm_view = peer.getsockname(), 0, np.zeros(64, np.float32)
        peer.sendto(C.pack_message(C.ENV_SHAPES_HEADER + [13.0, 7.0, 0.0]), w.sock.getsockname())
        mgr = BatchedAgentManager(None)
        mgr.processes, mgr.current_mask = [w], [None]
        assert mgr._get_env_shapes() == (13, 7, 0)
        assert not mgr.masked and mgr.n_actions == 0 and w.n_actions == 0 and mgr.action_mask_rows is None
        assert peer.recv(64) == C.pack_message(C.ENV_SHAPES_HEADER)          # (the request the manager sent)
        peer.sendto(C.pack_message(C.ENV_SHAPES_HEADER + [13.0, 7.0, 0.0, 1.0]), w.sock.getsockname())
        assert w.recv() == (ENV_SHAPES, 13.0, 7.0, 0.0, 1.0)
        # a reply that says "masked" against reset states without a trailer (or the reverse) is refused, as is a masked
        # environment whose action space is not the discrete one
        peer.sendto(C.pack_message(C.ENV_SHAPES_HEADER + [13.0, 7.0, 0.0, 1.0]), w.sock.getsockname())
        with pytest.raises(ValueError, match="disagree"):
            mgr._get_env_shapes()
        mgr.current_mask = [np.ones((2, 3), bool)]
        peer.sendto(C.pack_message(C.ENV_SHAPES_HEADER + [13.0, 3.0, 2.0, 1.0]), w.sock.getsockname())
        with pytest.raises(ValueError, match="option of the discrete head"):
            mgr._get_env_shapes()
    finally:
        w.sock.close()
        peer.close()
