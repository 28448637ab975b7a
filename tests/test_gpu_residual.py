"""Residual hidden layers (include/rlppo.h, "[res]"; csrc/residual.hip) on the GPU: the two row kernels alone, a whole minibatch pass
through PPOLearner with the rollout beside it, the one-hidden-layer identity, and a Learner.

Every comparison follows the rule of test_gpu_layer_norm.within: the truth is a torch restatement in float64 (for a pass: the learner's
own modules cast to double), the allowance 4 x the error of the same restatement in float32, with a floor of 4 ulp of the scale."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ppo_yardstick as A
from hip_pass import L, P, stream  # noqa: F401 -- L is the fixture
from test_gpu_layer_norm import ACTS, A_CODE, CLIP, ENT, GUARD, HEADS, OBS, ROWS, U32, within

pytestmark = pytest.mark.gpu
ACT_FN = {"relu": torch.relu, "tanh": torch.tanh, "elu": F.elu}
D_ACT = {"relu": lambda h: (h > 0).to(h.dtype), "tanh": lambda h: 1 - h * h, "elu": lambda h: torch.where(h > 0, torch.ones_like(h), h + 1)}


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("gnext", [False, True], ids=["top", "gnext"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("w", [1, 5, 128, 256, 300, 2048])
def test_row_kernels_against_float64(L, w, n, act, norm, gnext):
    pw = int(L.rlppo_padded_out(w))
    gen = torch.Generator().manual_seed(1000 * w + n)
    a, sp, p, gn = ACT_FN[act](torch.randn(n, w, generator=gen)), *(torch.randn(n, w, generator=gen) for _ in range(3))
    sp[0] = 1e3 + torch.randn(w, generator=gen)         # the stream's row of mean 1e3 and spread 1
    if n > 1:
        a[1], sp[1] = 0.25, 0.25                        # a constant row of the stream: var = 0, the epsilon alone

    def ref(dtype):   # the forward from its inputs; the backward from the SAVED stream, the float32 sum the kernel stored
        s = sp.to(dtype) + a.to(dtype)
        u = F.layer_norm(s, (w,), eps=1e-5) if norm else s
        saved = (sp + a).to(dtype).requires_grad_(True)
        g = torch.autograd.grad(F.layer_norm(saved, (w,), eps=1e-5), saved, p.to(dtype))[0] if norm else p.to(dtype)
        g = g + gn.to(dtype) if gnext else g
        return [s, g, g * D_ACT[act](a.to(dtype))] + ([u] if norm else [])

    def padded(x):   # [n + GUARD, pw]: NaN in the padded columns, 5 in the guard rows
        out = torch.full((n + GUARD, pw), float("nan"))
        out[:n, :w], out[n:] = x, 5.0
        return out.cuda()
    spd, ad, pd, gnd = (padded(x) for x in (sp, a, p, gn))

    def call(alias):
        nan = padded(sp * float("nan"))
        s, g, dz, u = spd.clone() if alias else nan.clone(), nan.clone(), pd.clone() if alias else nan.clone(), nan
        assert L.rlppo_row_res_fwd(stream(), P(s if alias else spd), pw, P(ad), pw, n, w, int(norm), P(s), pw, P(u) if norm else None, pw) == 0, L.rlppo_last_error()
        assert L.rlppo_row_res_bwd(stream(), P(ad), pw, P(s), pw, P(dz if alias else pd), pw, P(gnd) if gnext else None, pw, n, w, A_CODE[act], int(norm),
                                   P(g), pw, P(dz), pw) == 0, L.rlppo_last_error()
        return [t.cpu() for t in [s, g, dz] + ([u] if norm else [])]
    first, again, aliased = call(False), call(False), call(True)
    for name, got, b, c, r64, r32 in zip(("s", "g", "dz", "u"), first, again, aliased, ref(torch.float64), ref(torch.float32)):
        assert torch.equal(got, b), f"{name}: two runs differ"
        assert torch.equal(got, c), f"{name}: the aliased call (s == s_prev, dz == p) differs"
        assert (got[n:] == 5.0).all(), f"{name}: rows at and beyond n were touched"
        assert (got[:n, w:] == 0).all(), f"{name}: padded columns are not exact zeros"
        within(got[:n, :w], r64, r32, r64.abs().amax(1, keepdim=True), f"residual {name} w={w} n={n} {act} norm={norm} gnext={gnext}")


# ------------------------------------------------------------------------------------------------ 2. a whole pass, 3. the rollout
# ReLU: seeds for which no hidden pre-activation of the float64 run lies within 1e-4 of zero, found on the CPU for the discrete and the diag
# learner; the nvec head runs at the discrete head's seeds.  Every case asserts the property for the networks it built.
RELU_SEEDS = {('discrete', 'policy', True): 77, ('discrete', 'critic', True): 310, ('discrete', 'both', True): 249, ('diag', 'policy', True): 242,
              ('diag', 'critic', True): 30, ('diag', 'both', True): 95, ('discrete', 'policy', False): 332860, ('discrete', 'critic', False): 48028,
              ('discrete', 'both', False): 34192, ('diag', 'policy', False): 92984, ('diag', 'critic', False): 71860, ('diag', 'both', False): 17646}


def build(head, sizes_pol, sizes_val, seed):
    """A PPOLearner and 300 observations it acted on through the general path with noise of its own (the first 192, with made-up old
    log p, targets and advantages, are its experience).  The targets lie around 1, a unit off the fresh critic's outputs: the head's bias
    gradient, the mean residual, is then no cancelled sum, and the rule's floor -- ulps of the RESULT -- means what it says for it."""
    from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner
    torch.manual_seed(seed)
    ptype, space = HEADS[head]
    learner = PPOLearner(OBS, space, ptype, sizes_pol, sizes_val, (0.1, 1.0), ROWS, 1, 3e-4, 3e-4, CLIP, ENT, ROWS, "cuda:0")
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(300, OBS), -5, 5).astype(np.float32)
    learner.policy.act_graphs = False
    acts, logp = learner.policy.get_action(obs)
    exp = dict(obs=obs, acts=acts.float().reshape(300, -1).numpy(), logp=logp.numpy(), old=logp.numpy()[:ROWS] + 0.1 * rs.randn(ROWS).astype(np.float32),
               tgt=1 + rs.randn(ROWS).astype(np.float32), adv=rs.randn(ROWS).astype(np.float32))
    buf = ExperienceBuffer(ROWS, seed, "cpu")
    z = np.zeros(ROWS, np.float32)
    buf.submit_experience(obs[:ROWS], exp["acts"][:ROWS], exp["old"], z, obs[:ROWS], z, z, exp["tgt"], exp["adv"])
    return learner, exp, buf


def torch_pass(learner, head, exp, dtype):
    """The learner's own modules (deep copies on the CPU, cast to `dtype`, run by their own forward) -> (the gradients of one PPO
    minibatch over the first 192 rows in arena order, log p [300], the policy's outputs, the smallest |hidden pre-activation|, and the
    pass's statistics as learn() reports them, each with the scale of its allowance's floor: the value for entropy and value loss, 1 for
    the clip fraction, and for the KL term mean((r - 1) - log r) the largest |r - 1|, the size of the terms whose difference it is)."""
    cast = lambda m: copy.deepcopy(m).cpu().to(dtype)
    pol, val = cast(learner.policy.model), cast(learner.value_net.model)
    pol = pol[:-1] if head == "discrete" else pol   # (the discrete body ends in a Softmax: head_terms takes logits)
    ls = learner.policy.log_std.detach().cpu().to(dtype).requires_grad_(True) if head == "diag" else None
    t = {k: torch.as_tensor(v).to(dtype) for k, v in exp.items()}
    nearest = [float("inf")]
    for m in (pol, val):
        for lin in [x for x in m if isinstance(x, torch.nn.Linear)][:-1]:
            lin.register_forward_hook(lambda mod, i, o: nearest.__setitem__(0, min(nearest[0], float(o.detach()[:ROWS].abs().min()))))
    out = [pol(t["obs"]), val(t["obs"])]
    terms = lambda rows: A.head_terms(head, out[0][:rows], t["acts"][:rows], log_std=ls, bins=HEADS[head][1] if head == "nvec" else None)
    logp, entropy = terms(ROWS)
    ratio = torch.exp(logp - t["old"])
    (-torch.min(ratio * t["adv"], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * t["adv"]).mean() - entropy * ENT).backward(retain_graph=True)
    F.mse_loss(out[1][:ROWS].view(-1), t["tgt"]).backward()
    grads = [p.grad for p in pol.parameters()] + ([ls.grad] if ls is not None else []) + [p.grad for p in val.parameters()]
    with torch.no_grad():
        vloss, lr = F.mse_loss(out[1][:ROWS].view(-1), t["tgt"]), logp - t["old"]
        stats = {"Policy Entropy": (entropy.detach(), entropy.detach().abs()), "Value Function Loss": (vloss, vloss), "Mean KL Divergence": (((ratio - 1) - lr).mean(), (ratio - 1).abs().max()),
                 "SB3 Clip Fraction": (((ratio - 1).abs() > CLIP).to(dtype).mean(), 1.0)}
    return grads, terms(300)[0].detach(), out[0].detach(), nearest[0], stats


def hold_pass_and_rollout(head, act, which, norm, hidden, seed):
    from rlgym_ppo_amd.ppo import ExperienceBuffer, LayerSizes
    sizes = lambda on: LayerSizes(hidden, act, "layer" if norm else None, None, on)
    learner, exp, buf = build(head, sizes(which != "critic"), sizes(which != "policy"), seed)
    pol, label = learner.policy, f"{head} {act} {which} norm={norm} {hidden}"
    assert (pol.hidden_residual, learner.value_net.hidden_residual) == (which != "critic", which != "policy")
    g64, lp64, out64, nearest, st64 = torch_pass(learner, head, exp, torch.float64)
    g32, lp32, out32, _, st32 = torch_pass(learner, head, exp, torch.float32)
    assert act != "relu" or nearest > 1e-4, f"seed {seed}: a ReLU pre-activation of the float64 run lies {nearest:.1e} from zero"
    within(exp["logp"], lp64, lp32, lp64.abs().max(), f"rollout log p, general path, {label}")
    if head == "discrete":
        within(pol.get_output(exp["obs"]).cpu(), F.softmax(out64, -1), F.softmax(out32, -1), 1.0, f"rollout probabilities, {label}")
    noise = pol._draw_noise(8)
    a_eager, lp_eager = pol.get_action(exp["obs"][:8], noise=noise)
    pol.act_graphs = True
    a8, lp8 = pol.get_action(exp["obs"][:8], noise=noise)
    assert len(pol._graphs) == 1 and torch.equal(a8, a_eager) and torch.equal(lp8, lp_eager), "the graph-replayed call differs from the eager call"
    small = dict(exp, obs=np.tile(exp["obs"][:8], (38, 1))[:300], acts=np.tile(a8.float().reshape(8, -1).numpy(), (38, 1))[:300])
    within(lp8, torch_pass(learner, head, small, torch.float64)[1][:8], torch_pass(learner, head, small, torch.float32)[1][:8], lp64.abs().max(),
           f"rollout log p, graph replay, {label}")
    # the update's log p against the rollout's at unchanged weights: a pass whose old log p IS the rollout's, with both learning rates 0
    # (the weights stay what they are: the update magnitudes say so).  d = update - rollout log p of a row is at most 2a, a the allowance
    # both are held to; the KL term of a row is then at most d^2 / 2 (1 + d) + one rounding of exp(d) near 1 and one of the difference
    same = ExperienceBuffer(ROWS, seed, "cpu")
    z = np.zeros(ROWS, np.float32)
    same.submit_experience(exp["obs"][:ROWS], exp["acts"][:ROWS], exp["logp"][:ROWS], z, exp["obs"][:ROWS], z, z, exp["tgt"], exp["adv"])
    groups = learner.policy_optimizer.param_groups + learner.value_optimizer.param_groups
    rates = [g["lr"] for g in groups]
    for g in groups:
        g["lr"] = 0.0
    r0 = learner.learn(same)
    for g, lr in zip(groups, rates):
        g["lr"] = lr
    a2 = 2 * float(max(4 * (lp32 - lp64).abs().max(), 4 * U32 * lp64.abs().max()))
    print(f"[residual] update against rollout log p, {label}: KL {r0['Mean KL Divergence']:.2e}, bound {a2 * a2 + 2 * U32:.2e}")
    assert r0["Policy Update Magnitude"] == 0 and r0["Value Function Update Magnitude"] == 0 and r0["SB3 Clip Fraction"] == 0
    assert abs(r0["Mean KL Divergence"]) <= a2 * a2 + 2 * U32, (label, r0["Mean KL Divergence"])
    seen = []
    learner.grad_probe = lambda g: seen.append(g.detach().cpu().clone())
    report = learner.learn(buf)
    assert len(seen) == 1
    for name, (want, scale) in st64.items():
        within(report[name], want, st32[name][0], scale, f"{name} {label}")
    off = 0
    for i, (a, b) in enumerate(zip(g64, g32)):
        within(seen[0][off:off + a.numel()].view(a.shape), a, b, a.abs().max(), f"gradient {i} {label}")
        off += a.numel()
    assert off == seen[0].numel()


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("which", ["policy", "critic", "both"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("head", list(HEADS))
def test_pass_and_rollout_against_float64(L, head, act, which, norm):
    """13 -> 32 -> 32 -> 32 -> A with the skip stream in the policy, the critic or both: one learn() step on 192 rows (every parameter's
    gradient and the four statistics of its report), the log p and probabilities of the general rollout path at 300 observations and of
    the graph-replayed call at 8 (which equals the eager call bit for bit), and the update's log p against the rollout's through a pass
    at unchanged weights whose old log p is the rollout's."""
    seed = RELU_SEEDS[("diag" if head == "diag" else "discrete", which, norm)] if act == "relu" else 31
    hold_pass_and_rollout(head, act, which, norm, (32, 32, 32), seed)


def test_pass_at_width_300_two_hidden_layers(L):
    hold_pass_and_rollout("discrete", "tanh", "both", True, (300, 300), 31)   # the whole-wave kernels, a partial second chunk


# ------------------------------------------------------------------------------------------------ 4. one hidden layer: the flag changes nothing
@pytest.mark.parametrize("norm", [None, "layer"])
def test_one_hidden_layer_is_the_network_without_the_flag_bit_for_bit(L, norm):
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.ppo import LayerSizes
    runs = []
    for flag in (False, True):
        learner, exp, buf = build("discrete", *[LayerSizes((32,), "relu", norm, None, flag)] * 2, 7)
        assert learner.policy.hidden_residual == flag and bool(learner.policy.arena.hidden_act & N.ACT_RES) == flag
        seen = []
        learner.grad_probe = lambda g: seen.append(g.detach().cpu().clone())
        learner.learn(buf)
        runs.append((exp["logp"], exp["acts"], seen[0]))
    assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else torch.equal(a, b) for a, b in zip(*runs))
    dims, o = N.dims_array([107, 256, 256, 90]), N.ActOpts()
    assert L.rlppo_discrete_step_one_launch(dims, 3, 64, ctypes.byref(o)) == 1
    o.hidden_act = N.ACT_RES
    assert L.rlppo_discrete_step_one_launch(dims, 3, 64, ctypes.byref(o)) == 0


# ------------------------------------------------------------------------------------------------ 6. a Learner
def test_learner_two_iterations_and_a_checkpoint(L, tmp_path):
    import rlgym_ppo_amd.learner as LM
    import synthetic_env
    from rlgym_ppo_amd.ppo import LayerSizes, PPOLearner
    reports, printer = [], LM.reporting.report_metrics
    LM.reporting.report_metrics = lambda loggable_metrics, debug_metrics, wandb_run=None: reports.append(dict(loggable_metrics))
    learner = LM.Learner(synthetic_env.make_vector_env, vector_env=True, hidden_residual=True, hidden_layer_norm=True, n_proc=1, timestep_limit=256,
                         exp_buffer_size=128, ts_per_iteration=128, ppo_epochs=1, ppo_batch_size=128, policy_layer_sizes=(32, 32, 32),
                         critic_layer_sizes=(32, 32), checkpoints_save_folder=str(tmp_path / "c"), add_unix_timestamp=False, checkpoint_load_folder=None,
                         save_every_ts=10 ** 12, log_to_wandb=False, random_seed=5, min_inference_size=1)
    try:
        learner._learn()
    finally:
        LM.reporting.report_metrics = printer
        learner.agent.cleanup()
    assert len(reports) == 2 and all(np.isfinite(v) for v in reports[1].values()), reports
    assert learner.hidden_residuals == {"policy": True, "critic": True} and learner.hidden_norms == {"policy": "layer", "critic": "layer"}
    ppo = learner.ppo_learner
    ppo.save_to(str(tmp_path))
    torch.manual_seed(0)
    fresh = PPOLearner(107, 90, 0, LayerSizes((32, 32, 32), norm="layer", residual=True), LayerSizes((32, 32), norm="layer", residual=True), (0.1, 1.0), 128, 1,
                       3e-4, 3e-4, 0.2, 0.005, 128, "cuda:0")
    fresh.load_from(str(tmp_path))
    obs, noise = np.random.RandomState(1).randn(8, 107).astype(np.float32), ppo.policy._draw_noise(8)
    (a0, lp0), (a1, lp1) = ppo.policy.get_action(obs, noise=noise), fresh.policy.get_action(obs, noise=noise)
    assert torch.equal(a0, a1) and torch.equal(lp0, lp1)
