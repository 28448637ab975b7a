"""Invalid-action masking end to end in process-mode collection: two worker processes whose 90-action environment has
action_masks(), the mask trailer on the wire, the C++ collection loop, the masked graph call of DiscreteFF.get_action, the masked
experience buffer and the masked update."""
import contextlib
import io
import warnings

import numpy as np
import pytest
import torch

import masked_wire_env

pytestmark = pytest.mark.gpu


def test_process_mode_learner_with_action_masks_end_to_end(capfd):
    from rlgym_ppo_amd import Learner
    ts, A, d = 256, 90, 31
    torch.manual_seed(3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with contextlib.redirect_stdout(io.StringIO()):
            learner = Learner(masked_wire_env.make_masked_env_90, n_proc=2, min_inference_size=2, timestep_limit=10 ** 9, exp_buffer_size=4 * ts,
                              ts_per_iteration=ts, ppo_epochs=2, ppo_batch_size=ts, ppo_minibatch_size=ts // 2, policy_layer_sizes=(64, 64),
                              critic_layer_sizes=(64, 64), checkpoints_save_folder=None, checkpoint_load_folder=None, save_every_ts=10 ** 12,
                              log_to_wandb=False, random_seed=5, standardize_obs=False)
        try:
            agent, pol = learner.agent, learner.ppo_learner.policy
            assert agent.masked and agent.n_actions == A
            flat0 = pol.arena.flat.detach().cpu().clone()
            rows = 0
            for it in range(2):
                exp, _, n_col, _ = agent.collect_timesteps(ts)
                assert len(exp) == 7 and agent._native is not None          # the C++ loop, not a fall-back to the Python one
                states, actions = np.asarray(exp[0]), np.asarray(exp[1]).reshape(-1).astype(np.int64)
                masks = agent.action_mask_rows
                assert masks is not None and masks.dtype == bool and masks.shape == (len(states), A) and len(states) >= ts
                assert np.array_equal(masks, masked_wire_env.mask_of(states, A))
                assert masks[np.arange(len(actions)), actions].all(), "an invalid action was collected"
                with contextlib.redirect_stdout(io.StringIO()):
                    learner.add_new_experience(exp)
                    report = learner.ppo_learner.learn(learner.experience_buffer)
                rows += len(states)
                buf = learner.experience_buffer
                bm, bs, ba = buf.action_masks.cpu().numpy(), buf.states.cpu().numpy(), buf.actions.cpu().numpy().reshape(-1).astype(np.int64)
                assert bm.shape == (rows, A) and bs.shape == (rows, d)
                assert np.array_equal(bm, masked_wire_env.mask_of(bs, A))   # the environment's mask function of the stored states
                assert bm[np.arange(rows), ba].all()
                assert all(np.isfinite(v) for v in report.values() if isinstance(v, float)), report
            assert not torch.equal(flat0, pol.arena.flat.detach().cpu())    # the parameters moved
            served = {k: g.calls for k, g in pol._graphs.items()}
            assert served and all(isinstance(k, tuple) and k[1] for k in served), served      # masked graphs only ...
            assert sum(served.values()) > 0 and all(g.masked for g in pol._graphs.values())   # ... and they served the small calls
        finally:
            learner.agent.cleanup()
    assert not any("UNMASKED" in str(w.message) for w in caught)
    assert "UNMASKED" not in capfd.readouterr().err
