"""Device-resident vector environments (the _DeviceEnv side of VectorAgentManager's collect loop, csrc/rollout.hip): the three kernels through the C ABI
against numpy / torch restatements, bit for bit; a collect through the device interface against the same interaction through the
host interface, bit for bit; no host wait inside a collect; the Learner end to end on both interfaces."""
import contextlib
import ctypes
import io
import re
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import device_vector_env as E  # noqa: E402
import gae_bootstrap_yardstick as Y  # noqa: E402
import synthetic_env  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    from rlgym_ppo_amd import _native
    return _native.lib()


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(L, rc):
    assert rc == 0, (rc, L.rlppo_last_error())


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------ 1. the record kernel
def record_restated(r, d, tr, t, T, ep, avg, ended):
    """One step as the host side (_HostEnv) keeps it: float32 planes, double episode sums, the average over the ended agents in
    agent order as Python floats (two multiplications and one addition per episode, each rounded)."""
    r32 = np.asarray(r).astype(np.float32)
    dn, trn = np.asarray(d) != 0, np.asarray(tr) != 0
    ep = ep + r32.astype(np.float64)
    idx = np.flatnonzero(dn | trn)
    for x in ep[idx].tolist():
        avg = x if avg is None else avg * 0.9 + x * 0.1
    ep[idx] = 0.0
    stored_tr = np.where(dn, 0.0, 1.0) if t == T - 1 else trn.astype(np.float64)
    return r32, dn.astype(np.float32), stored_tr.astype(np.float32), (trn & ~dn).astype(np.float32), ep, avg, ended + idx.size


def _flags(rs, n, what):
    if what == "nobody":
        return np.zeros(n, bool), np.zeros(n, bool)
    if what == "everybody":   # every agent ends, by either flag (or both)
        d = rs.rand(n) < 0.5
        return d, ~d | (rs.rand(n) < 0.3)
    d, tr = rs.rand(n) < 0.2, rs.rand(n) < 0.2
    d[0], tr[n - 1] = True, True   # (flush step: a done agent and an environment-truncated one; n = 1: one agent with both)
    return d, tr


@pytest.mark.parametrize("patch", [False, True], ids=["nopatch", "patch"])
@pytest.mark.parametrize("flag_dtype", ["float32", "bool"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1030])
def test_record_kernel_bit_for_bit(L, n, flag_dtype, patch):
    T = 3
    # scenario = (average carried in, what happens at steps 0, 1, 2); step 2 is the flush step
    scenarios = [(None, ("nobody", "nobody", "nobody")), (None, ("nobody", "everybody", "some")), (None, ("some", "some", "some")),
                 (1.2345678901234567, ("some", "everybody", "some")), (-0.3, ("nobody", "some", "everybody"))]
    rs = np.random.RandomState(n)
    for avg0, plan in scenarios:
        state = torch.zeros(3, dtype=torch.int64, device=DEV)
        if avg0 is not None:
            state[:1].view(torch.float64)[0] = avg0
            state[1] = 1
        ep_dev = torch.zeros(n, dtype=torch.float64, device=DEV)
        rdt = torch.full((3, T, n), np.nan, dtype=torch.float32, device=DEV)
        P = torch.full((T, n), np.nan, dtype=torch.float32, device=DEV) if patch else None
        ep, avg, ended = np.zeros(n, np.float64), avg0, 0
        want = np.empty((4, T, n), np.float32)
        for t, what in enumerate(plan):
            # rewards with full mantissas (a contracted avg * 0.9 + x * 0.1 would round differently); float64 rewards with bool flags
            r = (rs.randn(n) * 3.7).astype(np.float64 if flag_dtype == "bool" else np.float32)
            d, tr = _flags(rs, n, what)
            want[0, t], want[1, t], want[2, t], want[3, t], ep, avg, ended = record_restated(r, d, tr, t, T, ep, avg, ended)
            conv = (lambda x: x) if flag_dtype == "bool" else (lambda x: x.astype(np.float32))
            r_d, d_d, tr_d = (torch.from_numpy(x).to(DEV) for x in (r, conv(d), conv(tr)))
            code = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(bool): 2}
            _check(L, L.rlppo_rollout_record(_stream(), _p(r_d), code[r.dtype], _p(d_d), code[conv(d).dtype], _p(tr_d), code[conv(tr).dtype],
                                             n, t, T, _p(rdt), _p(ep_dev), _p(state), _p(P[t]) if patch else _p(None)))
        got_state = state.cpu().numpy()
        assert np.array_equal(rdt.cpu().numpy().view(np.uint32), want[:3].view(np.uint32)), (n, plan)
        if patch:
            assert np.array_equal(P.cpu().numpy(), want[3])
        assert np.array_equal(bits(ep_dev.cpu().numpy()), bits(ep)), (n, plan)
        assert got_state[2] == ended
        assert bool(got_state[1]) == (avg is not None)
        if avg is not None:
            assert got_state[:1].view(np.uint64)[0] == bits([avg])[0], (n, plan, got_state[:1].view(np.float64)[0], avg)


def test_record_kernel_without_truncated_array(L):
    """The 4-tuple step: no truncated array at all."""
    n, T = 70, 2
    state, ep_dev = torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    rdt = torch.full((3, T, n), np.nan, dtype=torch.float32, device=DEV)
    rs, ep, avg, ended = np.random.RandomState(0), np.zeros(n), None, 0
    for t in range(T):
        r, d = rs.randn(n).astype(np.float32), rs.rand(n) < 0.3
        w = record_restated(r, d, np.zeros(n, bool), t, T, ep, avg, ended)
        ep, avg, ended = w[4], w[5], w[6]
        r_d, d_d = torch.from_numpy(r).to(DEV), torch.from_numpy(d).to(DEV)
        _check(L, L.rlppo_rollout_record(_stream(), _p(r_d), 0, _p(d_d), 2, _p(None), 0, n, t, T, _p(rdt), _p(ep_dev), _p(state), _p(None)))
        assert np.array_equal(rdt[2, t].cpu().numpy(), w[2])
    assert state.cpu().numpy()[:1].view(np.uint64)[0] == bits([avg])[0] and int(state[2]) == ended


# ------------------------------------------------------------------------------------------------ 2. the standardisation vectors
@pytest.mark.parametrize("d", [1, 107])
@pytest.mark.parametrize("per_feature", [False, True], ids=["scalar", "per_feature"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("count", [0, 1, 2, 7])
def test_obs_scalars_bit_for_bit(L, count, f64, per_feature, d):
    from rlgym_ppo_amd.util.running_stats import WelfordRunningStat
    for zero_feature in sorted({0, d - 1}):   # a zero-variance feature: feature 0 (the scalar mode's pair) and the last one
        st = WelfordRunningStat(shape=d)
        if f64:   # the state as a checkpoint load leaves it
            with contextlib.redirect_stdout(io.StringIO()):
                st.from_json(st.to_json())
        rs = np.random.RandomState(count * 7 + d)
        x = (rs.randn(max(count, 1), d) * 2 + 0.5).astype(np.float32)
        x[:, zero_feature] = 0.75
        for i in range(count):
            st.update(x[i])
        dt = np.float64 if f64 else np.float32
        assert np.asarray(st.running_mean).dtype == dt
        want_m, want_s = np.asarray(st.mean, np.float32).reshape(-1), np.asarray(st.std, np.float32).reshape(-1)
        if count >= 2:
            assert want_s[zero_feature] == 1.0
        if not per_feature:
            want_m, want_s = np.full(d, want_m[0], np.float32), np.full(d, want_s[0], np.float32)
        mean, m2 = (torch.from_numpy(np.asarray(a, dt).reshape(-1).copy()).to(DEV) for a in (st.running_mean, st.running_variance))
        mv, sv = (torch.full((d,), np.nan, dtype=torch.float32, device=DEV) for _ in range(2))
        _check(L, L.rlppo_obs_scalars(_stream(), _p(mean), _p(m2), int(f64), count, d, int(per_feature), _p(mv), _p(sv)))
        assert np.array_equal(mv.cpu().numpy().view(np.uint32), want_m.view(np.uint32))
        assert np.array_equal(sv.cpu().numpy().view(np.uint32), want_s.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. the transposition
@pytest.mark.parametrize("patched", [False, True], ids=["plain", "final_obs"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("ld", [32, 128])
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_to_trajectory_major_exact(L, n, T, ld, k, patched):
    g = torch.Generator(device=DEV).manual_seed(n * 100 + T)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    S, acts, logp, rdt = rnd(T + 1, n, ld), rnd(T, n, k), rnd(T, n), rnd(3, T, n)
    F = rnd(T, n, ld) if patched else None
    P = (torch.rand(T, n, device=DEV, generator=g) < 0.4).float() if patched else None
    N_ = n * T
    out = [torch.full(s, np.nan, device=DEV) for s in ((N_ + 1, ld), (N_, ld), (N_, k), (N_,), (N_,), (N_,), (N_,))]
    _check(L, L.rlppo_rollout_to_trajectory_major(_stream(), _p(S), _p(acts), _p(logp), _p(rdt), n, T, ld, k, _p(P), _p(F), *[_p(o) for o in out]))
    flat, nxt, a_o, lp_o, r_o, d_o, t_o = out
    assert torch.equal(flat[:N_].view(n, T, ld), S[:T].transpose(0, 1)) and torch.equal(flat[N_], S[T, n - 1])
    want_nxt = S[1:].transpose(0, 1)
    if patched:
        want_nxt = torch.where(P.t().unsqueeze(-1) != 0, F.transpose(0, 1), want_nxt)
    assert torch.equal(nxt.view(n, T, ld), want_nxt)
    assert torch.equal(a_o.view(n, T, k), acts.transpose(0, 1)) and torch.equal(lp_o.view(n, T), logp.t())
    for got, plane in zip((r_o, d_o, t_o), rdt):
        assert torch.equal(got.view(n, T), plane.t())


# ------------------------------------------------------------------------------------------------ 4. collect equivalence
def _policy(kind):
    from rlgym_ppo_amd.ppo import DiagGaussianPolicy, DiscreteFF
    torch.manual_seed(11)
    if kind == "gaussian":
        return DiagGaussianPolicy(107, 6, (32, 32), DEV, log_std_init=0.25)
    return DiscreteFF(107, 90, (32, 32), DEV)


def _host_env(kind):
    from rlgym_ppo_amd.util.action_clip import ActionClipEnv
    if kind == "gaussian":
        return synthetic_env.SyntheticVectorEnv(n_actions=6, seed=3, kind="continuous"), lambda e: ActionClipEnv(e, -1.0, 1.0)
    if kind == "masked":
        return E.MaskedSyntheticVectorEnv(seed=3), lambda e: e
    return synthetic_env.SyntheticVectorEnv(seed=3), lambda e: e


def _same(a, b, what):
    a, b = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.mark.parametrize("standardize", [True, False, "per_feature"])
@pytest.mark.parametrize("kind", ["discrete", "gaussian", "masked"])
def test_collect_equals_the_host_interface_bit_for_bit(L, kind, standardize):
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    mgrs = []
    for device_side in (False, True):
        pol = _policy(kind)
        mgr = VectorAgentManager(pol, seed=5, standardize_obs=bool(standardize))
        mgr.per_feature_obs_standardization = standardize == "per_feature"
        env, wrap = _host_env(kind)
        mgr.init_processes(0, lambda: wrap(E.DeviceTwin(env)) if device_side else wrap(env))
        mgrs.append(mgr)
    host_mgr, dev_mgr = mgrs
    assert dev_mgr._env_device is not None and host_mgr._env_device is None
    for n_req in (16 * 9, 16 * 5 - 3):
        T = -(-n_req // 16)
        got = []
        for mgr in mgrs:
            c0 = L.rlppo_dbg_counter(7)
            torch.manual_seed(100 + n_req)
            exp, _, n_col, _ = mgr.collect_timesteps(n_req)
            got.append((exp, n_col, torch.get_rng_state(), L.rlppo_dbg_counter(7) - c0))
        (exp_h, n_h, rng_h, rec_h), (exp_d, n_d, rng_d, rec_d) = got
        assert n_h == n_d == 16 * T and (rec_h, rec_d) == (0, T)
        for name, a, b in zip(("states", "actions", "log_probs", "rewards", "next_states", "dones", "truncated"), exp_h, exp_d):
            _same(a, b, name)
        _same(host_mgr.value_input_rows, dev_mgr.value_input_rows, "value_input_rows")
        _same(host_mgr._next_rows, dev_mgr._next_rows, "_next_rows")
        assert torch.equal(rng_h, rng_d)
        assert host_mgr.cumulative_timesteps == dev_mgr.cumulative_timesteps
        assert host_mgr.average_reward is not None and bits([host_mgr.average_reward])[0] == bits([dev_mgr.average_reward])[0]
        if standardize:
            hs, ds = host_mgr.obs_stats, dev_mgr.obs_stats
            assert hs.count == ds.count
            _same(hs.running_mean, ds.running_mean, "obs_stats mean")
            _same(hs.running_variance, ds.running_variance, "obs_stats variance")
            _same(hs.std, ds.std, "obs_stats std")
        if kind == "masked":
            _same(host_mgr.action_mask_rows.words, dev_mgr.action_mask_rows.words, "action masks")
            assert not host_mgr.action_masks.all()
        else:
            assert dev_mgr.action_mask_rows is None
    if kind == "gaussian":   # the environment saw clipped actions, the buffer holds the samples
        assert exp_d[1].abs().max() > 1.0 and exp_d[1].shape[1] == 6
    assert dev_mgr.episodes_ended > 0
    for mgr in mgrs:
        mgr.cleanup()


# ------------------------------------------------------------------------------------------------ 5. no host wait inside a collect
def _sync_warnings(mgr, n):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            mgr.collect_timesteps(n)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return [w for w in rec if "synchroniz" in str(w.message).lower()]


def test_no_host_wait_inside_a_device_collect():
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    na, T = 64, 8
    counts = {}
    for side in ("device", "host"):
        pol = _policy("discrete")
        pol.noise_mode = "device"
        mgr = VectorAgentManager(pol, seed=5, standardize_obs=True)
        mgr.init_processes(0, lambda: E.IntegerEnv(n_agents=na, device=torch.device(DEV) if side == "device" else None))
        mgr.collect_timesteps(na * T)   # warm-up: allocations, the first pack of the weights
        counts[side] = len(_sync_warnings(mgr, na * T))
        mgr.cleanup()
    print(f"synchronisation warnings in one collect of {T} steps: device interface {counts['device']}, host interface {counts['host']}")
    assert counts["device"] <= 1, counts      # the end-of-collect read
    assert counts["host"] >= T, counts        # the live control: torch's mode does flag a per-step wait


# ------------------------------------------------------------------------------------------------ 6. the Learner end to end
def _learner(make_env, tmp_path, **kw):
    from rlgym_ppo_amd import Learner
    na, T = 64, 8
    cfg = dict(vector_env=True, n_proc=1, timestep_limit=2 * na * T, exp_buffer_size=2 * na * T, ts_per_iteration=na * T, ppo_epochs=1,
               ppo_batch_size=na * T, ppo_minibatch_size=na * T // 2, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32),
               checkpoints_save_folder=str(tmp_path), add_unix_timestamp=False, checkpoint_load_folder=None, save_every_ts=10 ** 12,
               log_to_wandb=False, random_seed=5)
    cfg.update(kw)
    return Learner(make_env, **cfg)


def _flat_params(learner):
    return [torch.nn.utils.parameters_to_vector(m.parameters()).detach().cpu() for m in (learner.ppo_learner.policy, learner.ppo_learner.value_net)]


def test_learner_end_to_end_equals_the_numpy_twin(tmp_path, capsys):
    runs = {}
    for side, make in (("host", E.make_integer_host_env), ("device", E.make_integer_device_env)):
        capsys.readouterr()
        learner = _learner(make, tmp_path / side)
        try:
            learner._learn()
            rewards = re.findall(r"Policy Reward: (\S+)", capsys.readouterr().out)
            assert learner.epoch == 2 and len(rewards) == 2
            runs[side] = (_flat_params(learner), rewards, learner.agent.obs_stats.to_json(), learner.agent.average_reward)
            if side == "device":
                assert learner.agent._env_device is not None
                learner.save(learner.agent.cumulative_timesteps)
                learner.load("latest", False)                      # the statistics come back as float64 state
                assert np.asarray(learner.agent.obs_stats.running_mean).dtype == np.float64
                learner.timestep_limit += 64 * 8
                learner._learn()
                assert learner.epoch == 3 and learner.agent.cumulative_timesteps == 3 * 64 * 8
                assert all(torch.isfinite(p).all() for p in _flat_params(learner))
        finally:
            learner.agent.cleanup()
    (ph, rh, sh, ah), (pd, rd, sd, ad) = runs["host"], runs["device"]
    for a, b in zip(ph, pd):
        assert torch.equal(a, b)
    assert rh == rd and sh == sd and bits([ah])[0] == bits([ad])[0]


# ------------------------------------------------------------------------------------------------ 7. bootstrap, dense form
def test_bootstrap_truncated_on_the_device_interface(tmp_path):
    """Advantages and value targets of Learner(gae_bootstrap_truncated=True) through the device interface (one value pass over all N
    next-state rows, final observations patched in by the transposition) against the host interface (the m truncated rows)."""
    got = {}
    for side in ("host", "device"):
        dev = torch.device(DEV) if side == "device" else None
        with contextlib.redirect_stdout(io.StringIO()):
            learner = _learner(lambda: E.IntegerEnv(device=dev, final_obs=True), tmp_path / side, gae_bootstrap_truncated=True)
        try:
            out = []
            for _ in range(2):
                exp, _, n, _ = learner.agent.collect_timesteps(64 * 8)
                with contextlib.redirect_stdout(io.StringIO()):
                    learner.add_new_experience(exp)
                buf = learner.experience_buffer
                out.append((buf.values.detach().cpu().numpy()[-n:].copy(), buf.advantages.detach().cpu().numpy()[-n:].copy(),
                            exp[4].cpu().numpy().copy(), exp[6].cpu().numpy().copy(), exp[5].cpu().numpy().copy()))
            got[side] = out
            if side == "device":
                assert learner.agent.bootstrap_dense and learner.agent.bootstrap_rows.shape[0] == 64 * 8
        finally:
            learner.agent.cleanup()
    for it, (h, d) in enumerate(zip(got["host"], got["device"])):
        assert ((h[3] != 0) & (h[4] == 0)).reshape(64, 8)[:, :-1].any(), "the collect must hold environment-side truncations"
        _same(h[2], d[2], "next_states")   # (final observations in place)
        _same(h[3], d[3], "truncated")
        for name, a, b in (("value targets", h[0], d[0]), ("advantages", h[1], d[1])):
            print(f"bootstrap iteration {it}: max |{name} device - host| = {np.abs(a - b).max():.3e}")
            np.testing.assert_allclose(b, a, rtol=Y.RTOL, atol=Y.ATOL, err_msg=name)
            assert np.array_equal(a, b), name


def test_bootstrap_without_final_observation_warns_once():
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    mgr = VectorAgentManager(_policy("discrete"), seed=5)
    mgr.bootstrap_truncated = True
    mgr.init_processes(0, lambda: E.IntegerEnv(n_agents=16, device=torch.device(DEV)))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        mgr.collect_timesteps(16 * 4)
        mgr.collect_timesteps(16 * 4)
    assert sum("final_observation" in str(w.message) for w in rec) == 1
    assert mgr.bootstrap_dense and mgr.bootstrap_rows.shape[0] == 64
    mgr.cleanup()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals():
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    mgr = VectorAgentManager(_policy("discrete"), seed=5)
    mgr.init_processes(0, lambda: E.IntegerEnv(n_agents=16, device=torch.device(DEV)))
    mgr._env_device = torch.device("cuda", 7)   # (one GPU here: an environment that reported another device)
    with pytest.raises(ValueError, match=r"cuda:7.*cuda:0"):
        mgr.collect_timesteps(16)

    class CpuReset(E.IntegerEnv):
        def reset(self):
            return super().reset().cpu()

        def step(self, actions):
            return super().step(torch.as_tensor(np.asarray(actions, np.float32)).to(DEV))
    mgr = VectorAgentManager(_policy("discrete"), seed=5)
    mgr.init_processes(0, lambda: CpuReset(n_agents=16, device=torch.device(DEV)))
    assert mgr._env_device is None
    with pytest.raises(ValueError, match="reset\\(\\) returned a CPU tensor"):
        mgr.collect_timesteps(16)
