"""Value normalisation at the PPOLearner and the Learner level: learn() under a preset statistic is the learner without the option
on host-normalised targets, bit for bit; the Learner's order of steps (scan under the old scale, statistic advanced, learn() under
the new one), its report, its checkpoint; one process-mode iteration with bootstrapped truncations."""
import contextlib
import io
import json
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gae_bootstrap_yardstick as GY  # noqa: E402
import synthetic_env  # noqa: E402
import value_norm_yardstick as VY  # noqa: E402


def host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


# ================================================================================================ PPOLearner
D, HID, ACTIONS, ROWS, MB = 21, (32, 32), 8, 3000, 1500


def build_ppo(seed=5, epochs=2):
    from rlgym_ppo_amd.ppo import PPOLearner
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return PPOLearner(D, ACTIONS, 0, HID, HID, (0.1, 1.0), ROWS, epochs, 3e-4, 3e-4, 0.2, 0.005, MB, "cuda:0")


def ppo_state(learner):
    torch.cuda.synchronize()
    po, vo = learner.policy_optimizer, learner.value_optimizer
    return [t.detach().clone() for t in (learner.policy.arena.flat, learner.value_net.arena.flat, po.exp_avg, po.exp_avg_sq, vo.exp_avg, vo.exp_avg_sq)]


def test_learn_under_a_preset_statistic_is_the_plain_learner_on_normalised_targets():
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    rs = np.random.RandomState(1)
    obs = np.clip(rs.randn(ROWS, D), -5, 5).astype(np.float32)
    tgt = (40.0 + 25.0 * rs.randn(ROWS)).astype(np.float32)
    adv, z = rs.randn(ROWS).astype(np.float32), np.zeros(ROWS, np.float32)
    out = []
    scale = None
    for on in (True, False):
        learner = build_ppo()
        assert learner.value_norm is None and learner.value_norm_state() is None
        act, logp = learner.policy.get_action(obs)
        act = np.asarray(torch.as_tensor(act).cpu(), np.float32).reshape(ROWS)
        logp = np.asarray(torch.as_tensor(logp).cpu(), np.float32).reshape(ROWS)
        if on:
            learner.set_value_normalization(True)
            assert host(learner.value_norm.scale).tolist() == [0.0, 1.0, 1.0, 0.0]            # fresh: raw
            learner.load_value_norm_state({"count": 1000.0, "mean": 38.7, "var": 24.3 ** 2})
            scale = host(learner.value_norm.scale)
            assert np.array_equal(scale, VY.scale32((1000.0, 38.7, 1000.0 * 24.3 ** 2)))
            st = learner.value_norm_state()
            assert st["count"] == 1000.0 and st["mean"] == 38.7 and abs(st["var"] - 24.3 ** 2) < 1e-9 and st["rejected"] == 0.0
            v = torch.randn(5, device="cuda")
            assert torch.equal(learner.value_norm.denormalize(v), v * learner.value_norm.scale[2] + learner.value_norm.scale[0])
            targets = tgt
        else:
            targets = VY.normalise_targets32(tgt, scale[0], scale[1])
        buf = ExperienceBuffer(ROWS, 9, "cpu")
        buf.submit_experience(obs, act, logp, z, obs, z, z, targets, adv)
        with contextlib.redirect_stdout(io.StringIO()):
            report = learner.learn(buf)
        out.append((ppo_state(learner), report, act))
        if on:
            assert np.array_equal(host(learner.value_norm.scale), scale)                      # learn() never moves the statistic
    assert np.array_equal(out[0][2], out[1][2])
    for k, (a, b) in enumerate(zip(out[0][0], out[1][0])):
        assert torch.equal(a, b), k
    for key in ("Value Function Loss", "Policy Entropy", "Mean KL Divergence", "Value Function Update Magnitude"):
        assert out[0][1][key] == out[1][1][key], key
    assert out[0][1]["Value Function Loss"] < 10.0                                            # normalised units (raw: ~ 40^2)


# ================================================================================================ Learner, vector mode
NA, T, ITERS = 64, 32, 3
OBS = 13


class StepEnv(synthetic_env.SyntheticVectorEnv):
    """SyntheticVectorEnv whose observations and reward noise are a function of the global step count, so that a second environment
    can start at the step a first one reached (the episode counters are replayed).  Rewards of size ~ 20 +- 50: value targets far
    from the unit scale."""

    def __init__(self, start=0):
        super().__init__(obs_dim=OBS, n_actions=7, n_agents=NA, seed=0)
        self.k = 0
        for _ in range(start):
            self._tick()

    def _tick(self):
        self.k += 1
        self.t += 1
        done = self.t >= self.ep_len
        trunc = (~done) & (self.t % 4 == 0) & (np.arange(self.n_agents) % 3 == 0)
        self.t[done | trunc] = 0
        return done, trunc

    def _draw(self):
        rs = np.random.RandomState(1000 + self.k)
        return (rs.randn(NA, OBS) * 2 + 0.5).astype(np.float32), rs.randn(NA)

    def reset(self):
        return self._draw()[0]

    def step(self, actions):
        actions = np.asarray(actions, np.float32).reshape(NA, -1)
        done, trunc = self._tick()
        obs, noise = self._draw()
        rew = (20.0 + 50.0 * np.tanh(actions.sum(1) * 0.3) + 5.0 * noise).astype(np.float32)
        return obs, rew, done.astype(np.float32), trunc.astype(np.float32), {"state": None}


def make_learner(tmp_path, start=0, iters=ITERS, **kw):
    from rlgym_ppo_amd import Learner
    cfg = dict(vector_env=True, n_proc=1, timestep_limit=iters * NA * T, exp_buffer_size=2 * NA * T, ts_per_iteration=NA * T, ppo_epochs=1,
               ppo_batch_size=NA * T, ppo_minibatch_size=NA * T // 2, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32),
               checkpoints_save_folder=str(tmp_path), add_unix_timestamp=False, checkpoint_load_folder=None, save_every_ts=10 ** 12,
               log_to_wandb=False, random_seed=5)
    cfg.update(kw)
    with contextlib.redirect_stdout(io.StringIO()):
        return Learner(lambda: StepEnv(start), **cfg)


def run_learner(learner):
    """_learn() with a spy behind add_new_experience (this iteration's value targets from the buffer, the statistic as the call left
    it) and one in front of the report printer."""
    import rlgym_ppo_amd.learner as LM
    snaps, reports = [], []
    plain, printer = learner.add_new_experience, LM.reporting.report_metrics

    def spy(experience):
        out = plain(experience)
        n = experience[0].shape[0]
        vn = learner.ppo_learner.value_norm
        snaps.append(dict(targets=host(learner.experience_buffer.values)[-n:].copy(), adv=host(learner.experience_buffer.advantages)[-n:].copy(),
                          state=None if vn is None else host(vn.state).copy(), scale=None if vn is None else host(vn.scale).copy()))
        return out

    def keep(loggable_metrics, debug_metrics, wandb_run=None):
        reports.append(dict(loggable_metrics))
        return printer(loggable_metrics, debug_metrics, wandb_run)
    learner.add_new_experience, LM.reporting.report_metrics = spy, keep
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            learner._learn()
        p_ = learner.ppo_learner
        torch.cuda.synchronize()
        state = dict(pol=p_.policy.arena.flat.clone(), val=p_.value_net.arena.flat.clone(), m=p_.policy_optimizer.exp_avg.clone(),
                     vm=p_.value_optimizer.exp_avg.clone(), book=learner.agent.cumulative_timesteps,
                     vnorm=None if p_.value_norm is None else host(p_.value_norm.state).tobytes() + host(p_.value_norm.scale).tobytes())
        return state, snaps, reports
    finally:
        LM.reporting.report_metrics = printer
        learner.agent.cleanup()


def same_state(a, b, keys):
    for k in keys:
        assert (torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k]), k


def test_learner_advances_the_statistic_reports_it_and_off_is_off(tmp_path):
    from test_gpu_value_norm import batch_bounds, check_scale, merged_bounds
    on, snaps, reports = run_learner(make_learner(tmp_path / "on", ppo_normalize_value=True))
    assert len(snaps) == len(reports) == ITERS
    truth, err = (0.0, 0.0, 0.0), (0.0, 0.0)
    for it, s in enumerate(snaps):
        bm = VY.batch_moments(s["targets"])
        new = VY.merge(truth, bm)
        err = merged_bounds(truth, err, bm, batch_bounds(s["targets"]), new)     # the statistic test's bound (tests/test_gpu_value_norm.py)
        truth = new
        got = s["state"]
        assert got[0] == truth[0] == (it + 1) * NA * T and got[3] == 0.0
        assert abs(got[1] - truth[1]) <= err[0] and abs(got[2] - truth[2]) <= err[1], (it, got, truth, err)
        check_scale(got, s["scale"])
        assert reports[it]["Value Norm Mean"] == float(s["scale"][0]) and reports[it]["Value Norm Std"] == float(s["scale"][2])
    assert abs(snaps[-1]["scale"][0]) > 5.0 and snaps[-1]["scale"][2] > 5.0             # targets far from the unit scale
    # off, with the keyword and without it: the same run, bit for bit; no statistic, no keys; and not the run with the option on
    off, off_snaps, off_reports = run_learner(make_learner(tmp_path / "off", ppo_normalize_value=False))
    bare, _, bare_reports = run_learner(make_learner(tmp_path / "bare"))
    same_state(off, bare, ("pol", "val", "m", "vm", "book", "vnorm"))
    assert off["vnorm"] is None and all("Value Norm Mean" not in r and "Value Norm Std" not in r for r in off_reports + bare_reports)
    for a, b in zip(off_reports, bare_reports):
        assert a["Value Function Loss"] == b["Value Function Loss"] or (np.isnan(a["Value Function Loss"]) and np.isnan(b["Value Function Loss"]))
    # the first iteration's scan ran raw (scale {0, 1, 1, 0}): the same targets; its learn() already ran under the new scale
    assert np.array_equal(snaps[0]["targets"], off_snaps[0]["targets"]) and not torch.equal(on["val"], off["val"])
    for it in range(1, ITERS):
        assert reports[it]["Value Function Loss"] != off_reports[it]["Value Function Loss"]
        assert reports[it]["Value Function Loss"] < 0.2 * off_reports[it]["Value Function Loss"]   # normalised units against ~ sigma^2 times as much


def test_save_load_continue_equals_the_uninterrupted_run(tmp_path):
    """Three iterations against two + a second Learner that loads "latest" and runs the third, bit for bit (the construction of the
    test of the same name in tests/test_gpu_critic_obs.py: the environment restarted at the step the first run reached, the host
    generators carried over, a buffer of one collect, no standardisation)."""
    kw = dict(standardize_obs=False, standardize_returns=False, exp_buffer_size=NA * T, ppo_normalize_value=True)
    whole, _, _ = run_learner(make_learner(tmp_path / "whole", **kw))
    first = make_learner(tmp_path / "ck", iters=2, save_every_ts=NA * T, **kw)
    s1, _, _ = run_learner(first)
    rng = torch.get_rng_state(), np.random.get_state(), first.experience_buffer.rng.get_state()
    assert s1["book"] == 2 * NA * T and whole["book"] == 3 * NA * T and s1["vnorm"] != whole["vnorm"]
    book = json.load(open(os.path.join(str(tmp_path / "ck"), str(2 * NA * T), "BOOK_KEEPING_VARS.json")))
    assert {"count", "mean", "var"} <= set(book["value_norm_running_stats"]) and book["value_norm_running_stats"]["count"] == 2 * NA * T
    second = make_learner(tmp_path / "ck", start=2 * T, checkpoint_load_folder="latest", random_seed=9, **kw)
    try:
        vn = second.ppo_learner.value_norm
        assert host(vn.state).tobytes() + host(vn.scale).tobytes() == s1["vnorm"]              # continues from its own statistic
        assert torch.equal(second.ppo_learner.value_net.arena.flat, s1["val"])
        torch.set_rng_state(rng[0])
        np.random.set_state(rng[1])
        second.experience_buffer.rng.set_state(rng[2])
    except BaseException:
        second.agent.cleanup()
        raise
    resumed, _, _ = run_learner(second)
    same_state(resumed, whole, ("pol", "val", "m", "vm", "book", "vnorm"))
    # a book with the key needs the option; a book without it loads with a warning and a fresh statistic
    with pytest.raises(ValueError, match="ppo_normalize_value"):
        make_learner(tmp_path / "ck", checkpoint_load_folder="latest", **dict(kw, ppo_normalize_value=False))
    run_learner(make_learner(tmp_path / "plain", iters=1, save_every_ts=NA * T, **dict(kw, ppo_normalize_value=False)))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fresh = make_learner(tmp_path / "plain", checkpoint_load_folder="latest", **kw)
    try:
        assert any("value_norm_running_stats" in str(w.message) for w in caught)
        assert host(fresh.ppo_learner.value_norm.state).tolist() == [0.0] * 4 and host(fresh.ppo_learner.value_norm.scale).tolist() == [0.0, 1.0, 1.0, 0.0]
    finally:
        fresh.agent.cleanup()


# ================================================================================================ Learner, process mode
def test_process_mode_bootstrap_values_are_denormalised():
    """One iteration, 2 workers, gae_bootstrap_truncated: the m next-state values ride in the one value pass as NORMALISED values and
    reach the scan through the scale; the buffer's advantages and targets against the yardstick on the collected arrays."""
    from rlgym_ppo_amd import Learner
    from test_gpu_value_norm import assert_close_norm
    ts = 256
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = Learner(synthetic_env.make_discrete_env, n_proc=2, min_inference_size=2, timestep_limit=10 ** 9, exp_buffer_size=4 * ts,
                          ts_per_iteration=ts, ppo_epochs=1, ppo_batch_size=ts, ppo_minibatch_size=ts // 2, policy_layer_sizes=(32, 32),
                          critic_layer_sizes=(32, 32), checkpoints_save_folder=None, checkpoint_load_folder=None, save_every_ts=10 ** 12,
                          log_to_wandb=False, random_seed=5, standardize_obs=False, standardize_returns=False, gae_bootstrap_truncated=True,
                          ppo_normalize_value=True)
    try:
        learner.ppo_learner.load_value_norm_state({"count": 500.0, "mean": 3.0, "var": 4.0})
        scale = host(learner.ppo_learner.value_norm.scale).astype(np.float64)
        exp, _, _, _ = learner.agent.collect_timesteps(ts)
        states, nxt = np.asarray(exp[0], np.float32), np.asarray(exp[4], np.float32)
        n = states.shape[0]
        states, nxt = states.reshape(n, -1), nxt.reshape(n, -1)
        rews, dones, trunc = (np.asarray(exp[k], np.float32).reshape(n) for k in (3, 5, 6))
        idx = GY.boot_steps(dones, trunc)
        assert idx.size >= 3, "the collect must hold truncated steps"
        vn = learner.ppo_learner.value_net
        v_all = host(vn.forward_padded(vn.arena.stage_obs(np.concatenate([states, nxt[-1:], nxt[idx]], 0))))
        boot = np.full(n, np.nan, np.float32)
        boot[idx] = v_all[n + 1:]
        want = VY.gae(rews, dones, trunc, v_all[:n + 1], boot, scale[0], scale[2], learner.gae_gamma, learner.gae_lambda, None)
        plain = VY.gae(rews, dones, trunc, v_all[:n + 1], None, scale[0], scale[2], learner.gae_gamma, learner.gae_lambda, None)
        assert np.abs(want[1] - plain[1]).max() > 1e-2                                        # the bootstrap values matter here
        with contextlib.redirect_stdout(io.StringIO()):
            learner.add_new_experience(exp)
        buf = learner.experience_buffer
        vmax = np.abs(v_all.astype(np.float64) * scale[2] + scale[0]).max()
        got = (host(buf.values)[-n:], host(buf.advantages)[-n:], want[2])
        assert_close_norm(got, want, vmax, "process mode")
        st = host(learner.ppo_learner.value_norm.state)
        assert st[0] == 500.0 + n and st[3] == 0.0
        with contextlib.redirect_stdout(io.StringIO()):
            report = learner.ppo_learner.learn(buf)
        assert np.isfinite(report["Value Function Loss"])
    finally:
        learner.agent.cleanup()
