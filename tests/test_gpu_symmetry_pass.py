"""The augmented pass: learn() with a symmetry set (a small buffer, one minibatch, tanh 64 x 2 networks: no hidden decision is discrete)
against the existing pass run by hip_pass.run_pass on host-built doubled arrays -- gradients and statistics bit-equal, the same kernels
see the same inputs -- and against ppo_yardstick.py's float64 restatement on the doubled batch under that file's own gate.  And a
Learner in vector mode with symmetry=..."""
import numpy as np
import pytest
import torch

import ppo_yardstick as Y
from hip_pass import L, run_pass   # noqa: F401 -- L is a fixture
from mirror_reference import mirror_actions, mirror_mask, mirror_rows, obs_symmetry
from rlgym_ppo_amd.ppo import ExperienceBuffer, LayerSizes, PPOLearner, Symmetry

pytestmark = pytest.mark.gpu
D, MB, BINS, CLIP, ENT, SEED = 20, 64, [3, 3, 2, 7, 7], 0.2, 0.005, 11
# head -> (policy_type == RLPPO_HEAD_*, act_space_size, action description)
CASES = {"discrete": (0, 33, np.arange(33)[::-1].copy()), "nvec": (1, BINS, ([0, 1, 2, 4, 3], [None, [2, 1, 0], None, None, None])),
         "diag": (3, 4, ([1, 0, 2, 3], [1, 1, -1, 1]))}


@pytest.mark.parametrize("head", list(CASES))
def test_augmented_pass_is_the_pass_on_doubled_arrays(L, head):
    code, space, desc = CASES[head]
    torch.manual_seed(3)
    sizes = LayerSizes((64, 64), "tanh")
    learner = PPOLearner(D, space, code, sizes, sizes, (0.1, 1.0), MB, 1, 3e-4, 3e-4, CLIP, ENT, MB, "cuda:0")
    kw = dict(pol_act="tanh", val_act="tanh")
    if head == "diag":
        learner.policy.fill_log_std(-0.3)
        kw["log_std"] = np.full(4, -0.3, np.float32)
    pol, val = ([(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in net.arena.linears] for net in (learner.policy, learner.value_net))
    rs = np.random.RandomState(5)
    obs = rs.randn(MB, D).astype(np.float32)
    bins, mask = (BINS if head == "nvec" else None), None
    if head == "discrete":   # masked; the stored action is valid
        acts = rs.randint(0, 33, MB).astype(np.float32)
        mask = rs.rand(MB, 33) < 0.7
        mask[np.arange(MB), acts.astype(int)] = True
    elif head == "nvec":
        acts = np.stack([rs.randint(0, b, MB) for b in BINS], 1).astype(np.float32)
    else:
        acts = rs.randn(MB, 4).astype(np.float32)
    adv, tgt = rs.randn(MB).astype(np.float32), rs.randn(MB).astype(np.float32)
    head_kw = lambda m: {} if head == "diag" else dict(bins=bins, mask=m)
    logp = Y.minibatch(torch.float64, head, pol, val, obs, acts, np.zeros(MB), adv, tgt, CLIP, ENT, 1.0, **kw, **head_kw(mask))["logp"]
    old = (logp + 0.05 * rs.randn(MB)).astype(np.float32)

    perm, sign = obs_symmetry(D)
    learner.set_symmetry(Symmetry(perm, sign, action=desc))
    buf, z, probes = ExperienceBuffer(MB, SEED, "cpu"), np.zeros(MB, np.float32), []
    buf.submit_experience(obs, acts, old, z, obs, z, z, tgt, adv, action_masks=mask)
    learner.grad_probe = lambda g: probes.append(g.detach().clone())
    report = learner.learn(buf)
    assert len(probes) == 1

    # the doubled batch, built on the host: the rows in the epoch's order, then their mirror images
    idx = np.random.RandomState(SEED).permutation(MB)
    twice = lambda x, m: np.concatenate([x[idx], m], 0)
    obs2, acts2 = twice(obs, mirror_rows(obs[idx], perm, sign, D)), twice(acts, mirror_actions(code, desc, acts[idx], bins))
    mask2 = None if mask is None else twice(mask, mirror_mask(code, desc, mask[idx], bins))
    old2, tgt2, adv2 = (twice(x, x[idx]) for x in (old, tgt, adv))
    r = run_pass(L, pol, val, obs2, acts2, old2, tgt2, adv2, np.arange(2 * MB), head=head, entry="ex", clip=CLIP, ent=ENT, mb_ratio=1.0, **kw, **head_kw(mask2))
    n_pol = learner.policy.arena.n_flat
    assert torch.equal(probes[0][:n_pol], r["gp"]) and torch.equal(probes[0][n_pol:], r["gv"]), "gradients differ from the pass on doubled arrays"
    for k, key in enumerate(("Policy Entropy", "Mean KL Divergence", "Value Function Loss", "SB3 Clip Fraction")):
        assert report[key] == r["stats"][k], (key, report[key], r["stats"][k])
    Y.gate(r, *(Y.minibatch(dt, head, pol, val, obs2, acts2, old2, adv2, tgt2, CLIP, ENT, 1.0, **kw, **head_kw(mask2)) for dt in (torch.float64, torch.float32)),
           f"symmetry pass, {head}")
    learner.set_symmetry(None)
    assert learner._sym is None and learner.symmetry is None


def test_learner_with_symmetry_in_vector_mode(L, tmp_path):
    """Two iterations with symmetry=callable: finite reports, one rlppo_mirror_batch per pass; without it the same passes and no such launch."""
    import rlgym_ppo_amd.learner as LM
    import synthetic_env
    calls, real, printer = [], L.rlppo_mirror_batch, LM.reporting.report_metrics

    def run(name, **kw):
        reports = []
        LM.reporting.report_metrics = lambda loggable_metrics, debug_metrics, wandb_run=None: reports.append(dict(loggable_metrics))
        learner = LM.Learner(synthetic_env.make_vector_env, vector_env=True, n_proc=1, timestep_limit=256, exp_buffer_size=128, ts_per_iteration=128,
                             ppo_epochs=1, ppo_batch_size=128, ppo_minibatch_size=64, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32),
                             checkpoints_save_folder=str(tmp_path / name), add_unix_timestamp=False, checkpoint_load_folder=None, save_every_ts=10 ** 12,
                             log_to_wandb=False, random_seed=5, min_inference_size=1, **kw)
        passes = L.rlppo_dbg_counter(2)
        try:
            learner._learn()
        finally:
            learner.agent.cleanup()
        return reports, L.rlppo_dbg_counter(2) - passes

    L.rlppo_mirror_batch = lambda *a: calls.append(a[1]._obj.mb) or real(*a)
    try:
        plain, n_plain = run("plain")
        assert calls == [] and len(plain) == 2
        sym, n_sym = run("sym", symmetry=lambda env: Symmetry(*obs_symmetry(env.obs_dim), action=np.arange(90)[::-1].copy()))
    finally:
        L.rlppo_mirror_batch, LM.reporting.report_metrics = real, printer
    assert n_sym == n_plain > 0 and calls == [128] * n_sym    # (two minibatches of 64 fused into one pass)
    assert len(sym) == 2 and all(np.isfinite(v) for v in sym[1].values()), sym
