"""Hidden layer normalisation without learnable parameters (include/rlppo.h, "[norm]"; csrc/norm.hip) on the GPU: the two row
kernels alone, a whole minibatch pass through PPOLearner, and the rollout against the update path.

The tolerance rule of every comparison: the reference is the torch restatement in float64; the allowance is 4 x the largest error of
the SAME restatement run in float32 on the CPU against it (the factor covers a different but equally valid fp32 summation order),
with a floor of 4 ulp of the largest magnitude of the row (kernels) / of the tensor (gradients)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ppo_yardstick as A
from hip_pass import L, P, stream  # noqa: F401 -- L is the fixture

pytestmark = pytest.mark.gpu
ACTS = ("relu", "tanh", "elu")
U32 = float(np.finfo(np.float32).eps)
GUARD = 3   # rows behind row n that must stay as they were


def within(got, ref64, ref32, scale, label):
    """|got - ref64| <= max(4 max|ref32 - ref64|, 4 ulp x scale) elementwise; prints the achieved fraction of the allowance."""
    got, ref64, ref32 = (torch.as_tensor(x).double() for x in (got, ref64, ref32))
    allow = torch.maximum(4 * (ref32 - ref64).abs().max(), 4 * U32 * torch.as_tensor(scale).double()).expand_as(ref64)
    err = (got - ref64).abs()
    exact = err == 0
    frac = float((err[~exact] / allow[~exact]).max()) if (~exact).any() else 0.0
    print(f"[layer norm] {label}: {frac:.3f} of the allowance")
    assert torch.isfinite(got).all() and (exact | (err <= allow)).all(), (label, frac)


def restate(h, dy, w, act, dtype):
    """F.layer_norm of the activation output h [n, w] and, by autograd, its backward of dy times the activation's derivative from h."""
    h = h.to(dtype).requires_grad_(True)
    y = F.layer_norm(h, (w,), eps=1e-5)
    (dh,) = torch.autograd.grad(y, h, dy.to(dtype))
    hd = h.detach()
    d_act = {"relu": (hd > 0).to(dtype), "tanh": 1 - hd * hd, "elu": torch.where(hd > 0, torch.ones_like(hd), hd + 1)}[act]
    return y.detach(), dh * d_act


# ------------------------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("n", [1, 3, 65, 257])
@pytest.mark.parametrize("w", [1, 5, 16, 90, 256, 300, 1024])
def test_row_kernels_against_float64(L, w, n, act):
    pw = int(L.rlppo_padded_out(w))
    g = torch.Generator().manual_seed(1000 * w + n)
    h = {"relu": torch.relu, "tanh": torch.tanh, "elu": F.elu}[act](torch.randn(n, w, generator=g))
    h[0] = 1e3 + torch.randn(w, generator=g)            # mean 1e3, spread 1: a one-pass variance loses it
    if n > 1:
        h[1] = 0.5                                      # a constant row: var = 0, the epsilon alone
    dy = torch.randn(n, w, generator=g)
    (y64, dx64), (y32, dx32) = restate(h, dy, w, act, torch.float64), restate(h, dy, w, act, torch.float32)

    def padded(x, fill):   # [n + GUARD, pw]: NaN in the padded columns, `fill` in the guard rows
        out = torch.full((n + GUARD, pw), float("nan"))
        out[:n, :w], out[n:] = x, fill
        return out.cuda()
    hd, dyd = padded(h, 7.0), padded(dy, 7.0)
    run = {}
    for name in ("a", "b"):
        y = torch.full((n + GUARD, pw), float("nan"), device="cuda")
        dx = torch.full((n + GUARD, pw), float("nan"), device="cuda")
        y[n:], dx[n:] = 5.0, 5.0
        assert L.rlppo_row_norm_fwd(stream(), P(hd), pw, n, w, P(y), pw) == 0, L.rlppo_last_error()
        assert L.rlppo_row_norm_bwd(stream(), P(hd), pw, P(dyd), pw, n, w, A_CODE[act], P(dx), pw) == 0, L.rlppo_last_error()
        run[name] = (y.cpu(), dx.cpu())
    alias = dyd.clone()
    assert L.rlppo_row_norm_bwd(stream(), P(hd), pw, P(alias), pw, n, w, A_CODE[act], P(alias), pw) == 0, L.rlppo_last_error()
    y, dx = run["a"]
    assert torch.equal(y, run["b"][0]) and torch.equal(dx, run["b"][1]), "two runs differ"
    assert torch.equal(alias.cpu()[:n], dx[:n]) and (alias.cpu()[n:] == 7.0).all(), "dx == dy differs from the call that does not alias"
    assert (y[n:] == 5.0).all() and (dx[n:] == 5.0).all(), "rows at and beyond n were touched"
    assert (y[:n, w:] == 0).all() and (dx[:n, w:] == 0).all(), "padded columns are not exact zeros"
    within(y[:n, :w], y64, y32, y64.abs().amax(1, keepdim=True), f"fwd w={w} n={n}")
    within(dx[:n, :w], dx64, dx32, dx64.abs().amax(1, keepdim=True), f"bwd w={w} n={n} {act}")


A_CODE = {"relu": 0, "tanh": 1, "elu": 2}

# ------------------------------------------------------------------------------------------------ 2. a whole pass, 3. the rollout
OBS, ROWS, HIDDEN, CLIP, ENT = 13, 192, (32, 48), 0.2, 0.005
HEADS = {"discrete": (0, 6), "diag": (3, 3), "nvec": (1, [2, 4])}
# ReLU: seeds for which no hidden pre-activation of the float64 run lies within 1e-4 of zero (found on the CPU, asserted below)
RELU_SEEDS = {('discrete', 'policy'): 600, ('discrete', 'critic'): 153, ('discrete', 'both'): 44, ('diag', 'policy'): 409, ('diag', 'critic'): 1132,
              ('diag', 'both'): 45}


def build(head, act, which, seed):
    """A PPOLearner whose policy / critic / both are normalised, and 300 observations it acted on through the general path (the
    first 192 with made-up old log p, targets and advantages are its experience)."""
    from rlgym_ppo_amd.ppo import ExperienceBuffer, LayerSizes, PPOLearner
    torch.manual_seed(seed)
    sizes = lambda on: LayerSizes(HIDDEN, act, "layer" if on else None)
    ptype, space = HEADS[head]
    learner = PPOLearner(OBS, space, ptype, sizes(which != "critic"), sizes(which != "policy"), (0.1, 1.0), ROWS, 1, 3e-4, 3e-4, CLIP, ENT, ROWS, "cuda:0")
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(300, OBS), -5, 5).astype(np.float32)
    learner.policy.act_graphs = False
    acts, logp = learner.policy.get_action(obs)
    learner.policy.act_graphs = True
    exp = dict(obs=obs, acts=acts.float().reshape(300, -1).numpy(), logp=logp.numpy(), old=logp.numpy()[:ROWS] + 0.1 * rs.randn(ROWS).astype(np.float32),
               tgt=rs.randn(ROWS).astype(np.float32), adv=rs.randn(ROWS).astype(np.float32))
    buf = ExperienceBuffer(ROWS, seed, "cpu")
    z = np.zeros(ROWS, np.float32)
    buf.submit_experience(obs[:ROWS], exp["acts"][:ROWS], exp["old"], z, obs[:ROWS], z, z, exp["tgt"], exp["adv"])
    return learner, exp, buf


def torch_pass(learner, head, exp, dtype):
    """The learner's own torch modules (deep copies, on the CPU) in `dtype`: log p of every stored action, and one PPO minibatch over
    the first 192 rows -> (gradients per parameter in arena order, log p [300], the smallest |hidden pre-activation|)."""
    cast = lambda m: copy.deepcopy(m).cpu().to(dtype)
    pol, val = cast(learner.policy.model), cast(learner.value_net.model)
    pol = pol[:-1] if head == "discrete" else pol   # (the discrete body ends in a Softmax: head_terms takes logits)
    ls = learner.policy.log_std.detach().cpu().to(dtype).requires_grad_(True) if head == "diag" else None
    t = {k: torch.as_tensor(v).to(dtype) for k, v in exp.items()}
    nearest, out = float("inf"), []
    for m in (pol, val):
        x = t["obs"]
        for i, mod in enumerate(m):
            x = mod(x)
            if i % 2 == 0 and i < len(m) - 1:
                nearest = min(nearest, float(x.detach()[:ROWS].abs().min()))
        out.append(x)
    terms = lambda rows: A.head_terms(head, out[0][:rows], t["acts"][:rows], log_std=ls, bins=HEADS[head][1] if head == "nvec" else None)
    logp, entropy = terms(ROWS)
    ratio = torch.exp(logp - t["old"])
    (-torch.min(ratio * t["adv"], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * t["adv"]).mean() - entropy * ENT).backward(retain_graph=True)
    F.mse_loss(out[1][:ROWS].view(-1), t["tgt"]).backward()
    grads = [p.grad for p in pol.parameters()] + ([ls.grad] if ls is not None else []) + [p.grad for p in val.parameters()]
    return grads, terms(300)[0].detach(), nearest


@pytest.mark.parametrize("which", ["policy", "critic", "both"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("head", list(HEADS))
def test_pass_and_rollout_against_float64(L, head, act, which):
    """13 -> 32 -> 48 -> A, one learn() step on 192 rows whose batch gradient the learner's probe shows: every parameter tensor within
    the rule.  At unchanged weights get_action's log p -- the general path at 300 observations, the graph-replayed call at 8 -- is
    within the rule of the update path's log p of the same rows and actions."""
    seed = RELU_SEEDS[("diag" if head == "diag" else "discrete", which)] if act == "relu" else 31
    learner, exp, buf = build(head, act, which, seed)
    assert learner.policy.hidden_norm == (None if which == "critic" else "layer") and learner.value_net.hidden_norm == (None if which == "policy" else "layer")
    g64, lp64, nearest = torch_pass(learner, head, exp, torch.float64)
    g32, lp32, _ = torch_pass(learner, head, exp, torch.float32)
    assert act != "relu" or nearest > 1e-4, f"seed {seed}: a ReLU pre-activation of the float64 run lies {nearest:.1e} from zero"
    within(exp["logp"], lp64, lp32, lp64.abs().max(), f"rollout log p, general path, {head} {act} {which}")
    a8, lp8 = learner.policy.get_action(exp["obs"][:8])
    assert len(learner.policy._graphs) == 1
    small = dict(exp, obs=np.tile(exp["obs"][:8], (38, 1))[:300], acts=np.tile(a8.float().reshape(8, -1).numpy(), (38, 1))[:300])
    within(lp8, torch_pass(learner, head, small, torch.float64)[1][:8], torch_pass(learner, head, small, torch.float32)[1][:8], lp64.abs().max(),
           f"rollout log p, graph replay, {head} {act} {which}")
    seen = []
    learner.grad_probe = lambda g: seen.append(g.detach().cpu().clone())
    learner.learn(buf)
    assert len(seen) == 1
    off = 0
    for i, (a, b) in enumerate(zip(g64, g32)):
        got = seen[0][off:off + a.numel()].view(a.shape)
        off += a.numel()
        within(got, a, b, a.abs().max(), f"gradient {i} {head} {act} {which}")
    assert off == seen[0].numel()


def test_one_launch_answer_and_option_off_is_bit_identical(L):
    """rlppo_discrete_step_one_launch: 1 without the flag, 0 with it, on a shape the one-launch kernel covers; and a pass with the
    option off gives the gradients of the same call on an all-zero extension bit for bit."""
    from rlgym_ppo_amd import _native as N
    from hip_pass import run_pass
    from oracle import nets
    dims = N.dims_array([107, 256, 256, 90])
    o = N.ActOpts()
    assert L.rlppo_discrete_step_one_launch(dims, 3, 64, ctypes.byref(o)) == 1
    o.hidden_act = N.ACT_NORM
    assert L.rlppo_discrete_step_one_launch(dims, 3, 64, ctypes.byref(o)) == 0
    rs = np.random.RandomState(5)
    mk = lambda d: [(torch.as_tensor(rs.randn(o_, i_).astype(np.float32) / np.sqrt(i_)), torch.as_tensor(0.1 * rs.randn(o_).astype(np.float32)))
                    for i_, o_ in zip(d[:-1], d[1:])]
    pol, val = mk([OBS, 32, 48, 6]), mk([OBS, 32, 48, 1])
    obs = rs.randn(ROWS, OBS).astype(np.float32)
    args = (pol, val, obs, rs.randint(0, 6, ROWS).astype(np.float32), -1.8 + 0.1 * rs.randn(ROWS).astype(np.float32), rs.randn(ROWS).astype(np.float32),
            rs.randn(ROWS).astype(np.float32), np.arange(ROWS))
    plain, ex = (run_pass(L, *args, head="discrete", entry=e) for e in ("plain", "ex"))
    assert torch.equal(plain["gp"], ex["gp"]) and torch.equal(plain["gv"], ex["gv"]) and np.array_equal(plain["stats"], ex["stats"])
