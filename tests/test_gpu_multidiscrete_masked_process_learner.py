"""Invalid-action masking of a MultiDiscrete environment end to end in process-mode collection: worker processes whose environment has
action_masks() (one entry per logit), the mask trailer on the wire, both learner-side loops, the masked graph call of
MultiDiscreteFF.get_action, the masked experience buffer and the masked update."""
import contextlib
import io

import numpy as np
import pytest
import torch

import masked_multidiscrete_wire_env as W

pytestmark = pytest.mark.gpu

BINS = list(W.NVEC)
S, H, TS = sum(BINS), len(BINS), 256


def make_learner(env_fn, n_proc, native):
    from rlgym_ppo_amd import Learner
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = Learner(env_fn, n_proc=n_proc, min_inference_size=n_proc, timestep_limit=10 ** 9, exp_buffer_size=4 * TS, ts_per_iteration=TS,
                          ppo_epochs=2, ppo_batch_size=TS, ppo_minibatch_size=TS // 2, policy_layer_sizes=(64, 64), critic_layer_sizes=(64, 64),
                          checkpoints_save_folder=None, checkpoint_load_folder=None, save_every_ts=10 ** 12, log_to_wandb=False, random_seed=5,
                          standardize_obs=False, multi_discrete_bins=BINS)
    learner.agent.native_collect = native
    return learner


@pytest.mark.parametrize("native", [True, False], ids=["cpp_loop", "python_loop"])
def test_process_mode_learner_with_multidiscrete_action_masks_end_to_end(native):
    learner = make_learner(W.make_masked_nvec_env, 2, native)
    try:
        agent, pol = learner.agent, learner.ppo_learner.policy
        assert agent.masked and agent.n_actions == S and agent.mask_space_type == 1 and pol.splits == BINS
        flat0 = pol.arena.flat.detach().cpu().clone()
        rows = 0
        for it in range(2):
            exp, _, n_col, _ = agent.collect_timesteps(TS)
            assert len(exp) == 7 and (agent._native is not None) == native        # the loop the test asked for
            states, actions = np.asarray(exp[0]), np.asarray(exp[1])
            masks = agent.action_mask_rows
            assert masks is not None and masks.dtype == bool and masks.shape == (len(states), S) and len(states) >= TS
            assert actions.shape == (len(states), H)
            assert np.array_equal(masks, W.mask_of(states))
            assert W.head_valid_actions(masks, actions).all(), "an invalid action was collected"
            assert (np.asarray(exp[3]) < 500.0).all()                             # no step paid the out-of-range penalty
            with contextlib.redirect_stdout(io.StringIO()):
                learner.add_new_experience(exp)
                report = learner.ppo_learner.learn(learner.experience_buffer)
            rows += len(states)
            buf = learner.experience_buffer
            bm, bs, ba = buf.action_masks.cpu().numpy(), buf.states.cpu().numpy(), buf.actions.cpu().numpy()
            assert bm.shape == (rows, S) and ba.shape == (rows, H) and bs.shape[0] == rows
            assert np.array_equal(bm, W.mask_of(bs[:, :W.OBS_DIM]))               # the environment's mask function of the stored states
            assert W.head_valid_actions(bm, ba).all()
            assert all(np.isfinite(v) for v in report.values() if isinstance(v, float)), report
        assert not torch.equal(flat0, pol.arena.flat.detach().cpu())              # the parameters moved
        served = {k: g.calls for k, g in pol._graphs.items()}
        assert served and all(isinstance(k, tuple) and k[1] for k in served), served      # masked graphs only ...
        assert sum(served.values()) > 0 and all(g.masked for g in pol._graphs.values())   # ... and they served the small calls
    finally:
        learner.agent.cleanup()


def test_one_worker_cpp_loop_equals_python_loop_value_for_value():
    out = []
    for native in (False, True):
        learner = make_learner(W.make_masked_nvec_env, 1, native)
        try:
            torch.manual_seed(11)
            steps = []
            for k in (100, 37):
                exp, _, n_col, _ = learner.agent.collect_timesteps(k)
                steps.append((exp, n_col, np.array(learner.agent.action_mask_rows, copy=True)))
            assert (learner.agent._native is not None) == native
            out.append(steps)
        finally:
            learner.agent.cleanup()
    for (ea, na, ka), (eb, nb, kb) in zip(*out):
        assert na == nb
        for x, y, name in zip(ea, eb, ("states", "actions", "log_probs", "rewards", "next_states", "dones", "truncated")):
            assert np.asarray(x).shape == np.asarray(y).shape and np.array_equal(x, y), name
        assert ka.dtype == kb.dtype == bool and ka.shape == kb.shape == (len(ea[0]), S) and np.array_equal(ka, kb)
        assert np.array_equal(ka, W.mask_of(np.asarray(ea[0])))


@pytest.mark.parametrize("native", [True, False], ids=["cpp_loop", "python_loop"])
def test_an_empty_head_from_a_worker_raises_on_the_learner(native):
    learner = make_learner(W.make_empty_head_env, 1, native)
    try:
        with pytest.raises(ValueError, match=r"worker 0, agent 1, head 1 \(bins 2 \.\. 8\) has no valid bin"):
            learner.agent.collect_timesteps(TS)
        assert (learner.agent._native is not None) == native
        g = learner.ppo_learner.policy._graphs
        assert set(g) == {(16, True)} and g[(16, True)].calls == 3               # three steps were served, nothing for the bad one
    finally:
        learner.agent.cleanup()


def test_masks_with_one_entry_per_component_are_refused_when_the_learner_is_built():
    from rlgym_ppo_amd import Learner
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match=rf"\b{H} entries.*\b{S} logits"):
            Learner(W.make_narrow_mask_env, n_proc=1, min_inference_size=1, ts_per_iteration=TS, exp_buffer_size=4 * TS, ppo_batch_size=TS,
                    policy_layer_sizes=(64, 64), critic_layer_sizes=(64, 64), checkpoints_save_folder=None, checkpoint_load_folder=None,
                    log_to_wandb=False, random_seed=5, standardize_obs=False, multi_discrete_bins=BINS)
