"""Learner(gae_bootstrap_truncated=True): the wiring from the rollout to the bootstrap form of the GAE scan.  The advantages and
value targets that reach the buffer are compared with the CPU oracle applied per trajectory (tests/gae_bootstrap_yardstick.py,
rtol 2e-6 / atol 2e-6), fed with the critic's own outputs on the same state and next-state rows, so that only the wiring is
under test: which steps bootstrap, from which rows, scattered to which entries."""
import contextlib
import io
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gae_bootstrap_yardstick as Y  # noqa: E402
import synthetic_env  # noqa: E402

NA, D, T = 8, 13, 16


class VecEnv(synthetic_env.SyntheticVectorEnv):
    """SyntheticVectorEnv at 8 agents x 13 features: episode lengths 5..15 and a time limit every 4 steps for every third agent,
    so a 16-step collect holds terminal and time-limit ends.  ends=False: no episode ends at all (only the flush truncates);
    final_obs=True: info["final_observation"] carries a fresh draw for every agent (meaningful where truncated and not done).
    Every step is logged."""

    def __init__(self, ends=True, final_obs=False, seed=0):
        super().__init__(obs_dim=D, n_actions=7, n_agents=NA, seed=seed)
        self.ends, self.final_obs, self.log = ends, final_obs, []

    def step(self, actions):
        if self.ends:
            obs, rew, done, trunc, info = super().step(actions)
        else:
            obs = self._obs()
            rew = self.rs.randn(NA).astype(np.float32)
            done = trunc = np.zeros(NA, np.float32)
            info = {"state": None}
        fo = None
        if self.final_obs:
            fo = (self.rs.randn(NA, D) * 3 - 1).astype(np.float32)
            info = dict(info, final_observation=fo)
        self.log.append(dict(obs=obs.copy(), done=np.asarray(done).copy(), trunc=np.asarray(trunc).copy(), fo=fo))
        return obs, rew, done, trunc, info


def make_learner(env_kw, fused=True, **kw):
    from rlgym_ppo_amd import Learner
    envs = []

    def mk():
        envs.append(VecEnv(**env_kw))
        return envs[-1]
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = Learner(mk, vector_env=True, n_proc=1, timestep_limit=10 ** 9, exp_buffer_size=NA * T, ts_per_iteration=NA * T,
                          ppo_epochs=1, ppo_batch_size=NA * T, ppo_minibatch_size=NA * T, policy_layer_sizes=(32, 32),
                          critic_layer_sizes=(32, 32), checkpoints_save_folder=None, checkpoint_load_folder=None,
                          save_every_ts=10 ** 12, log_to_wandb=False, random_seed=5, **kw)
    if not fused:
        learner.ppo_learner.policy.fused_step = False
    return learner, envs[0]


def host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def expected_from_oracle(learner, exp):
    """The per-trajectory oracle on the critic's outputs for the collect's own rows."""
    vn = learner.ppo_learner.value_net
    n = exp[0].shape[0]
    rews, dones, trunc = (host(exp[k]).reshape(n).astype(np.float32) for k in (3, 5, 6))
    values = host(vn.forward_padded(learner.agent.value_input_rows))
    idx = Y.boot_steps(dones, trunc)
    boot = np.full(n, np.nan, np.float32)
    if idx.size:
        rows = exp[4].index_select(0, torch.from_numpy(idx).cuda()).contiguous()
        boot[idx] = host(vn.forward_padded(rows))
    std = learner.return_stats.std[0] if learner.standardize_returns else None
    return Y.per_segment(rews, dones, trunc, values, boot, learner.gae_gamma, learner.gae_lambda, std), idx, dones, trunc


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
@pytest.mark.parametrize("env_kw", [dict(), dict(final_obs=True), dict(ends=False)], ids=["ends", "final_obs", "flush_only"])
def test_buffer_holds_the_per_trajectory_oracle(env_kw, fused):
    learner, env = make_learner(env_kw, fused, gae_bootstrap_truncated=True)
    assert learner.config["gae_bootstrap_truncated"] is True
    try:
        seen_done = seen_trunc = False
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for it in range(2):
                exp, _, n, _ = learner.agent.collect_timesteps(NA * T)
                want, idx, dones, trunc = expected_from_oracle(learner, exp)
                assert np.array_equal(learner.agent.bootstrap_steps, idx) and idx.size >= 1
                flush_only = env_kw.get("ends") is False
                assert (learner.agent.bootstrap_index is None) == flush_only        # the flush alone: no gather, S[T] as it stands
                seen_done |= bool(dones[np.arange(n) % T != T - 1].any())
                seen_trunc |= bool(trunc[np.arange(n) % T != T - 1].any())
                with contextlib.redirect_stdout(io.StringIO()):
                    learner.add_new_experience(exp)
                buf = learner.experience_buffer
                got = (host(buf.values), host(buf.advantages))
                for g, w, name in zip(got, want[:2], ("value_targets", "advantages")):
                    assert np.isfinite(g).all()
                    np.testing.assert_allclose(g, w, rtol=Y.RTOL, atol=Y.ATOL, err_msg=f"{name} iteration {it}")
                with contextlib.redirect_stdout(io.StringIO()):
                    learner.ppo_learner.learn(buf)                                   # the critic moves between the iterations
        if env_kw.get("ends", True):
            assert seen_done and seen_trunc, "the collects must hold terminal and time-limit ends"
    finally:
        learner.agent.cleanup()


def test_process_mode_experience_appends_the_next_states_to_the_value_pass():
    """Host arrays (what BatchedAgentManager hands over): the m next states ride in the one value pass behind the [N + 1, d] rows."""
    learner, _ = make_learner(dict(), gae_bootstrap_truncated=True, standardize_returns=False)
    try:
        n = 120                                                      # (fits the 128-row buffer)
        rs = np.random.RandomState(2)
        states, nxt = rs.randn(n, D).astype(np.float32), rs.randn(n, D).astype(np.float32)
        rews = rs.randn(n).astype(np.float32)
        dones = (rs.rand(n) < 0.05).astype(np.float32)
        trunc = (rs.rand(n) < 0.1).astype(np.float32)
        trunc[-1], dones[-1] = 1.0, 0.0
        vn = learner.ppo_learner.value_net
        idx = Y.boot_steps(dones, trunc)
        v_all = host(vn.forward_padded(vn.arena.stage_obs(np.concatenate([states, nxt[-1:], nxt[idx]], 0))))
        boot = np.full(n, np.nan, np.float32)
        boot[idx] = v_all[n + 1:]
        want = Y.per_segment(rews, dones, trunc, v_all[:n + 1], boot, learner.gae_gamma, learner.gae_lambda, None)
        exp = (states, rs.randint(0, 7, (n, 1)).astype(np.float32), rs.randn(n).astype(np.float32), rews, nxt, dones, trunc)
        learner.add_new_experience(exp)
        buf = learner.experience_buffer
        assert buf.states.shape[0] == n
        np.testing.assert_allclose(host(buf.values)[-n:], want[0], rtol=Y.RTOL, atol=Y.ATOL)
        np.testing.assert_allclose(host(buf.advantages)[-n:], want[1], rtol=Y.RTOL, atol=Y.ATOL)
    finally:
        learner.agent.cleanup()


def test_option_off_is_the_learner_without_the_keyword():
    fields = ("states", "actions", "log_probs", "rewards", "next_states", "dones", "truncated", "values", "advantages")
    runs = []
    for kw in (dict(), dict(gae_bootstrap_truncated=False)):
        learner, _ = make_learner(dict(final_obs=True), **kw)
        try:
            snaps = []
            for it in range(2):
                exp, _, _, _ = learner.agent.collect_timesteps(NA * T)
                assert learner.agent.bootstrap_steps is None and learner.agent.bootstrap_rows is None
                with contextlib.redirect_stdout(io.StringIO()):
                    learner.add_new_experience(exp)
                    snaps.append({k: getattr(learner.experience_buffer, k).clone() for k in fields})
                    learner.ppo_learner.learn(learner.experience_buffer)
            runs.append(snaps)
        finally:
            learner.agent.cleanup()
    for a, b in zip(*runs):
        for k in fields:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "chain"])
def test_final_observations_become_the_next_state_rows_of_the_truncated_steps(fused):
    results = {}
    for on in (True, False):
        learner, env = make_learner(dict(final_obs=True), fused, gae_bootstrap_truncated=on)
        try:
            agent, arena = learner.agent, learner.ppo_learner.policy.arena
            scal_log, orig = [], agent._standardize_scalars

            def logged():
                scal_log.append(orig())
                return scal_log[-1]
            agent._standardize_scalars = logged
            with warnings.catch_warnings():
                warnings.simplefilter("error")                       # the key is there: no warning
                exp, _, n, _ = agent.collect_timesteps(NA * T)
            assert len(scal_log) == T and len(env.log) == T
            nxt, rows = exp[4], agent.value_input_rows
            hits = 0
            for t, step in enumerate(env.log):
                sel = np.flatnonzero((step["trunc"] != 0) & (step["done"] == 0))
                for a in range(NA):
                    got = nxt[a * T + t]
                    if on and a in sel:
                        hits += 1
                        mean, std = scal_log[t]
                        want = arena.stage_obs(step["fo"][a:a + 1], scal_log[t])[0]
                        assert torch.equal(got, want), (a, t)
                        restated = np.clip((step["fo"][a] - np.float32(mean)) / np.float32(std), -5, 5)
                        np.testing.assert_allclose(host(got)[:D], restated, rtol=1e-5, atol=1e-6)
                        assert not torch.equal(got, rows[a * T + t + 1])     # not the post-reset observation
                    elif t < T - 1:
                        assert torch.equal(got, rows[a * T + t + 1]), (a, t)  # every other step: the state the agent saw next
            assert hits >= 3 or not on
            results[on] = (agent.obs_stats.to_json(), agent.steps_since_obs_stats_update, nxt.clone())
        finally:
            learner.agent.cleanup()
    # the staged final observations never enter the running observation statistics
    assert results[True][0] == results[False][0] and results[True][1] == results[False][1]
    assert not torch.equal(results[True][2], results[False][2])


def test_without_final_observation_the_warning_appears_once():
    learner, env = make_learner(dict(), gae_bootstrap_truncated=True)
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(2):
                learner.agent.collect_timesteps(NA * T)
        assert sum(bool(np.any((s["trunc"] != 0) & (s["done"] == 0))) for s in env.log) >= 2
        mine = [w for w in caught if "final_observation" in str(w.message)]
        assert len(mine) == 1 and "post-reset" in str(mine[0].message)
    finally:
        learner.agent.cleanup()
