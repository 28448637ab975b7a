"""The general multi-discrete head through the host classes: MultiDiscreteFF(bins=...) (seeded sampling, graph-replayed small call,
bins=None against the reference's bins given explicitly), PPOLearner on virtual ranks, and the Learner loop in vector and in
process mode on a MultiDiscrete((2, 7, 3, 11, 2)) environment (tests/multidiscrete_env.py)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import nets  # noqa: E402
import multidiscrete_env as E  # noqa: E402
import multidiscrete_nvec_yardstick as Y  # noqa: E402

BINS = (2, 7, 3, 11, 2)


def lib():
    from rlgym_ppo_amd import _native as N
    return N.lib()


def params(policy):
    return [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in policy.arena.linears]


# ------------------------------------------------------------------------------------------------ 4. the policy object
def test_seeded_get_action_is_the_cpu_categorical_sample():
    """A seeded get_action of MultiDiscreteFF(bins=(2, 7, 3, 11, 2)) == Categorical(logits=padded).sample() of the CPU under the same
    seed (near-tie rule of tests/multidiscrete_nvec_yardstick.py), and torch's generator ends where the CPU sampling leaves it."""
    from rlgym_ppo_amd.ppo import MultiDiscreteFF
    from rlgym_ppo_amd.util.torch_functions import MultiDiscreteRolv
    torch.manual_seed(4)
    pol = MultiDiscreteFF(E.OBS_DIM, (64, 64), "cuda:0", bins=BINS)
    assert pol.splits == list(BINS) and pol.arena.dims[-1] == sum(BINS)
    rs = np.random.RandomState(4)
    n = 300
    obs = np.clip(rs.randn(n, E.OBS_DIM), -5, 5).astype(np.float32)
    out = pol.get_output(obs)
    assert tuple(out.shape) == (n, sum(BINS))
    p = params(pol)
    z64 = Y.logits64(p, obs)
    np.testing.assert_allclose(out.cpu().numpy(), z64, rtol=1e-5, atol=2e-6)
    c6 = lib().rlppo_dbg_counter(6)
    torch.manual_seed(21)
    act, logp = pol.get_action(obs)
    state = torch.get_rng_state()
    assert lib().rlppo_dbg_counter(6) > c6   # the general sampling kernel
    assert act.dtype == torch.int64 and tuple(act.shape) == (n, len(BINS)) and tuple(logp.shape) == (n,)
    # the CPU sampling: the reference's construction on the float32 CPU logits of the same weights
    dist = MultiDiscreteRolv(list(BINS))
    with torch.no_grad():
        dist.make_distribution(nets.mlp(p, obs))
    torch.manual_seed(21)
    cpu_act = dist.sample()
    assert torch.equal(state, torch.get_rng_state())
    torch.manual_seed(21)
    q = torch.empty(n * len(BINS), max(BINS)).exponential_(1)
    oact, _ = Y.check_sampled(act.numpy(), logp.numpy(), z64, BINS, q.numpy())
    differ = (cpu_act.numpy() != oact).any(1).sum()   # the float32 CPU sample against float64: the same near-tie rule
    assert differ <= 2
    # the deterministic branch walks self.splits
    det, _ = pol.get_action(obs, deterministic=True)
    want = np.stack([z64[:, s:s + b].argmax(-1) for s, b in zip(np.cumsum((0,) + BINS[:-1]), BINS)])
    assert det.shape == (len(BINS), n) and (det != want).sum() <= 2


def test_graph_replayed_small_call_equals_the_eager_path():
    """ActGraph through the policy's hooks, 8 and 80 observations: bit-identical to the eager path, with given noise and with the
    default CPU-generator draw."""
    from rlgym_ppo_amd.ppo import MultiDiscreteFF
    torch.manual_seed(22)
    rs = np.random.RandomState(3)
    pol = MultiDiscreteFF(E.OBS_DIM, (64, 64), "cuda:0", bins=BINS)
    H, B = len(BINS), max(BINS)
    for n in (8, 80):
        obs = np.clip(rs.randn(n, E.OBS_DIM), -5, 5).astype(np.float32)
        q = torch.empty(n * H, B).exponential_(1)
        pol.act_graphs = True
        a1, l1 = pol.get_action(obs, noise=q)
        pol.act_graphs = False
        a0, l0 = pol.get_action(obs, noise=q)
        assert a1.shape == a0.shape == (n, H) and a1.dtype == a0.dtype and torch.equal(a0, a1) and torch.equal(l0, l1), n
        assert (a1 < torch.as_tensor(BINS)).all() and (a1 >= 0).all()
        pol.act_graphs = True
        torch.manual_seed(9)
        a1, l1 = pol.get_action(obs)
        s1 = torch.get_rng_state()
        pol.act_graphs = False
        torch.manual_seed(9)
        a0, l0 = pol.get_action(obs)
        assert torch.equal(a0, a1) and torch.equal(l0, l1) and torch.equal(s1, torch.get_rng_state())
    assert len(pol._graphs) >= 1   # the small calls really went through captured graphs


def build_learner(bins, seed=6, n=1024, B=512, MB=256, epochs=2):
    from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner
    torch.manual_seed(seed)
    np.random.seed(seed)
    space = 8 if bins is None else bins   # act_space_size: the number of components, or the nvec itself
    learner = PPOLearner(E.OBS_DIM, space, 1, (64, 64), (64, 64), (0.1, 1.0), B, epochs, 3e-4, 3e-4, 0.2, 0.005, MB, "cuda:0")
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(n, E.OBS_DIM), -5, 5).astype(np.float32)
    torch.manual_seed(seed + 1)
    act, logp = learner.policy.get_action(obs)
    buf = ExperienceBuffer(n, seed, "cpu")
    z = np.zeros(n, np.float32)
    buf.submit_experience(obs, act.numpy().astype(np.float32), logp.numpy() + 0.1 * rs.randn(n).astype(np.float32), z, obs, z, z,
                          rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32))
    return learner, buf, act, logp


def test_bins_none_and_the_reference_bins_are_the_same_policy():
    """bins=None and bins=[3, 3, 3, 3, 3, 2, 2, 2]: bit-identical actions, log-probabilities and, after one learn(), parameters; the
    library's counter of general-kernel launches does not move (the fixed kernels ran, through the plain entry points)."""
    c6 = lib().rlppo_dbg_counter(6)
    la, ba, act_a, logp_a = build_learner(None)
    lb, bb, act_b, logp_b = build_learner([3, 3, 3, 3, 3, 2, 2, 2])
    assert la.policy.md_nvec is None and lb.policy.md_nvec is None
    assert torch.equal(act_a, act_b) and torch.equal(logp_a, logp_b)
    ra, rb = la.learn(ba), lb.learn(bb)
    assert torch.equal(la.policy.arena.flat, lb.policy.arena.flat) and torch.equal(la.value_net.arena.flat, lb.value_net.arena.flat)
    for k in ("Policy Entropy", "Mean KL Divergence", "Value Function Loss", "SB3 Clip Fraction", "Policy Update Magnitude"):
        assert ra[k] == rb[k], k
    assert lib().rlppo_dbg_counter(6) == c6
    # ... and a policy forced onto the general kernels moves it (what tools/multidiscrete_bins_cost.py measures)
    lc, bc, act_c, logp_c = build_learner(None)
    lc.policy._force_general = True
    assert lc.policy.md_nvec is not None and lc.policy.n_heads == 8
    lc.learn(bc)
    assert lib().rlppo_dbg_counter(6) > c6


# ------------------------------------------------------------------------------------------------ 5. the learners
def test_two_virtual_ranks_end_one_learn_bit_identical():
    from rlgym_ppo_amd import dp
    reps, bufs = [], []
    for _ in range(2):
        learner, buf, act, _ = build_learner(BINS)
        reps.append(learner)
        bufs.append(buf)
    assert reps[0]._act_dim == len(BINS) and (act < torch.as_tensor(BINS)).all()
    before = reps[0].policy.arena.flat.clone()
    c6 = lib().rlppo_dbg_counter(6)
    reports = dp.run_virtual_ranks(reps, bufs)
    assert lib().rlppo_dbg_counter(6) > c6
    assert torch.equal(reps[0].policy.arena.flat, reps[1].policy.arena.flat)
    assert torch.equal(reps[0].value_net.arena.flat, reps[1].value_net.arena.flat)
    assert not torch.equal(before, reps[0].policy.arena.flat)
    assert all(np.isfinite(float(v)) for r in reports for v in r.values())


def run_loop(env_fn, tmp_path, n_proc, vector_env, **kw):
    from rlgym_ppo_amd import Learner
    cfg = dict(n_proc=n_proc, min_inference_size=2, timestep_limit=700, exp_buffer_size=1024, ts_per_iteration=384, ppo_epochs=1,
               ppo_batch_size=384, ppo_minibatch_size=192, policy_layer_sizes=(64, 64), critic_layer_sizes=(64, 64),
               checkpoints_save_folder=str(tmp_path / "ckpt"), add_unix_timestamp=False, save_every_ts=10_000_000,
               checkpoint_load_folder=None, random_seed=3, vector_env=vector_env, multi_discrete_bins=BINS)
    cfg.update(kw)
    learner = Learner(env_fn, **cfg)
    before = learner.ppo_learner.policy.arena.flat.clone()
    reports = []
    plain = learner.ppo_learner.learn
    learner.ppo_learner.learn = lambda exp: reports.append(plain(exp)) or reports[-1]
    try:
        learner._learn()
        assert learner.epoch == 2                      # two iterations
        buf = learner.experience_buffer
        acts = buf.actions.cpu().numpy()
        assert acts.shape[1] == len(BINS) and (acts >= 0).all() and (acts < np.asarray(BINS)).all() and (acts == np.floor(acts)).all()
        assert float(buf.rewards.max()) < E.OUT_OF_RANGE_REWARD / 2   # no step reached the environment with an action outside nvec
        for h, b in enumerate(BINS):                   # ... and the heads are really used up to their last bin
            assert acts[:, h].max() == b - 1
        assert all(np.isfinite(float(v)) for r in reports for v in r.values()) and len(reports) == 2
        assert not torch.equal(before, learner.ppo_learner.policy.arena.flat)
        assert np.isfinite(learner.ppo_learner.policy.arena.flat.cpu().numpy()).all()
        return learner
    finally:
        learner.agent.cleanup()


def test_learner_loop_vector_mode(tmp_path):
    c6 = lib().rlppo_dbg_counter(6)
    envs = []

    def make():
        envs.append(E.make_vector_env())
        return envs[-1]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        run_loop(make, tmp_path, 0, True)
    assert not [x for x in w if "multi_discrete_bins" in str(x.message)]   # bins == the environment's nvec: no warning
    env = envs[0]
    assert env.out_of_range_steps == 0 and (env.seen_max == np.asarray(BINS) - 1).all()
    assert lib().rlppo_dbg_counter(6) > c6


def test_learner_warns_once_when_the_bins_are_not_the_environments(tmp_path):
    """Vector mode, the environment's nvec visible and different from the bins in effect (here: the default, the reference's): one
    warning, no error -- the default behaviour stays what it was."""
    from rlgym_ppo_amd import Learner
    make = lambda: E.NvecVectorEnv(nvec=(3, 3, 3, 3, 3, 2, 2, 3))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        learner = Learner(make, n_proc=0, vector_env=True, policy_layer_sizes=(64, 64), critic_layer_sizes=(64, 64), ppo_batch_size=64,
                          exp_buffer_size=128, ts_per_iteration=64, checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False,
                          checkpoint_load_folder=None)
    try:
        hits = [x for x in w if "multi_discrete_bins" in str(x.message)]
        assert len(hits) == 1 and learner.ppo_learner.policy.splits == [3, 3, 3, 3, 3, 2, 2, 2]
    finally:
        learner.agent.cleanup()


def test_learner_loop_process_mode(tmp_path):
    run_loop(E.make_env, tmp_path, 2, False)
