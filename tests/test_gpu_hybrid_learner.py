"""The hybrid head end to end: Learner(vector_env=True, continuous_head="hybrid", multi_discrete_bins=[3, 2]) on a tiny vector
environment whose action rows are two analog axes and two buttons (defined here), two iterations."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import synthetic_env  # noqa: E402

OBS, K, NVEC, AGENTS = 11, 2, (3, 2), 8


class HybridVectorEnv:
    """Observations are a function of the step counter alone; step() keeps what it was handed."""

    def __init__(self):
        self.t, self.seen = 0, []
        self.observation_space = synthetic_env._Space(shape=(OBS,))
        self.action_space = synthetic_env.Box(shape=(K + len(NVEC),))

    def _obs(self):
        return (np.random.RandomState(500 + self.t).randn(AGENTS, OBS) * 1.5).astype(np.float32)

    def reset(self):
        return self._obs()

    def step(self, actions):
        a = np.array(actions, np.float32).reshape(AGENTS, -1)
        self.seen.append(a)
        self.t += 1
        done = ((self.t + np.arange(AGENTS)) % 7 == 0).astype(np.float32)
        return self._obs(), (a[:, 0] - 0.1 * a[:, K]).astype(np.float32), done, np.zeros(AGENTS, np.float32), {"state": None}

    def close(self):
        pass


def run(tmp_path, name, envs, **kw):
    from rlgym_ppo_amd import Learner

    def make():
        envs.append(HybridVectorEnv())
        return envs[-1]
    cfg = dict(n_proc=0, min_inference_size=2, timestep_limit=700, exp_buffer_size=1024, ts_per_iteration=384, ppo_epochs=1, ppo_batch_size=384,
               ppo_minibatch_size=192, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32), checkpoints_save_folder=str(tmp_path / name),
               add_unix_timestamp=False, save_every_ts=10_000_000, checkpoint_load_folder=None, random_seed=3, vector_env=True,
               continuous_head="hybrid", multi_discrete_bins=list(NVEC), continuous_log_std_init=0.25)
    cfg.update(kw)
    learner = Learner(make, **cfg)
    reports, plain = [], learner.ppo_learner.learn
    learner.ppo_learner.learn = lambda exp: reports.append(plain(exp)) or reports[-1]
    return learner, reports


def state(learner):
    p = learner.ppo_learner
    return [p.policy.arena.flat.clone(), p.value_net.arena.flat.clone(), p.policy_optimizer.exp_avg.clone(), p.policy_optimizer.exp_avg_sq.clone()]


def test_learner_loop_on_a_hybrid_vector_environment(tmp_path):
    from rlgym_ppo_amd.ppo import HybridPolicy
    envs = []
    learner, reports = run(tmp_path, "a", envs)
    try:
        pol = learner.ppo_learner.policy
        assert isinstance(pol, HybridPolicy) and learner.ppo_learner.policy_type == 4 and (pol.k, pol.splits) == (K, list(NVEC))
        before = pol.arena.flat.clone()
        learner._learn()
        assert learner.epoch == 2 and len(reports) == 2 and all(np.isfinite(float(v)) for r in reports for v in r.values())
        # one optimiser step per iteration: every pass of the first learn() ran at the weights the rollout sampled with, so its ratios are
        # 1 up to the float32 rounding of the two log-probabilities (|log ratio| ~ 1e-5 at most: KL ~ its square + 2^-24, no row clipped)
        assert reports[0]["SB3 Clip Fraction"] == 0 and abs(reports[0]["Mean KL Divergence"]) < 1e-6, reports[0]
        ent_gauss = K * (1.4189385332046727 + 0.25)   # the first pass saw log_std = 0.25; the heads add at most log 3 + log 2
        assert ent_gauss < reports[0]["Policy Entropy"] <= ent_gauss + np.log(6.0) + 1e-5
        after = pol.arena.flat
        assert not torch.equal(before, after) and bool(torch.isfinite(after).all())
        ls = pol.log_std.detach().cpu().numpy()
        assert 0 < np.abs(ls - 0.25).max() < 0.01   # log_std: started at the init, moved by the optimiser
        # the buffer holds the samples as drawn and float-encoded indices; the environment saw the axes clipped and integral indices
        acts, seen = learner.experience_buffer.actions.cpu().numpy(), np.concatenate(envs[0].seen)
        assert acts.shape[1] == K + len(NVEC) and np.abs(acts[:, :K]).max() > 1.5
        assert np.abs(seen[:, :K]).max() == 1.0
        for h, b in enumerate(NVEC):
            col = seen[:, K + h]
            assert (col == np.floor(col)).all() and col.min() == 0 and col.max() == b - 1
        # a checkpoint round trip restores log_std and its Adam moments (the tail of the policy's arena), bit for bit
        learner.save(learner.agent.cumulative_timesteps)
        other, _ = run(tmp_path, "a", envs, checkpoint_load_folder="latest", random_seed=9, continuous_log_std_init=-1.0)
        try:
            for x, y in zip(state(learner), state(other)):
                assert torch.equal(x, y)
            assert torch.equal(other.ppo_learner.policy.log_std.detach(), pol.log_std.detach())
        finally:
            other.agent.cleanup()
        # a second seeded run is bit-identical
        twin, _ = run(tmp_path, "b", envs)
        try:
            twin._learn()
            for x, y in zip(state(learner), state(twin)):
                assert torch.equal(x, y)
        finally:
            twin.agent.cleanup()
    finally:
        learner.agent.cleanup()
