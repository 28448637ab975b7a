"""The yardstick of the PPO update: one minibatch and a whole learn() of every policy head -- discrete (with an optional action
mask), multi-discrete for any nvec (with an optional mask), the reference's Gaussian, diagonal-Gaussian with a learnable log_std --
with the hidden activation ("relu", "tanh", "elu" with alpha = 1) and the critic's own observations as parameters, restated in torch
with autograd and run in float64 (the truth) and in float32 (what a correct float32 implementation is allowed to miss the truth by).

The tolerance rule of tests/fp64_gate.py: err(HIP, float64) <= max(1e-5, 1.5 x err(this file in float32, float64)), err = the
largest max|got - want| / max|want| over the tensors compared (gate).  Inputs are chosen by the callers (and asserted on the CPU,
from float64 alone: diag_gaussian_yardstick.assert_clear_of_clip_edges / assert_relu_clear) so that no ratio lies near a clip edge and
no ReLU pre-activation within its float32 rounding bound of 0.  With tanh / ELU no hidden decision is discrete: tanh is smooth, and
ELU with alpha = 1 has the derivative (h > 0 ? 1 : h + 1), CONTINUOUS at 0, so a pre-activation that float32 and float64 put on
different sides of 0 changes the gradient by O(|pre|), not by a whole term.

Where the inputs cannot be kept clear of ReLU decisions (the masked heads on 128-wide networks), masked_chain / masked_gate compare
under the decisions each implementation took (fp64_gate.hip_masks / cpu_masks / _check_flips), as tests/fp64_gate.py::gate does."""
import math

import numpy as np
import torch

import fp64_gate
from diag_gaussian_yardstick import logp_terms, row_entropy
from oracle import nets, ppo

ACT_FN = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}
FWD_RTOL, FWD_ATOL = 1e-5, 2e-6
STAT_NAMES = ("entropy", "kl", "value_loss", "clip_fraction", "policy_loss")   # RLPPO_STAT_* 0..4


def _t(x, dtype):
    return x.detach().to(dtype).clone() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype).clone()


def starts(bins):
    return [int(s) for s in np.cumsum((0,) + tuple(bins))[:-1]]


def mlp(params, x, act="relu", out_tanh=False, relu_masks=None):
    """relu_masks: the ReLU decisions of every hidden layer, imposed (pre * mask) instead of taken."""
    if nets._BF16_OPERANDS[0]:   # inside oracle.nets.bf16_operands(): the bf16 update precision's restatement (float32 runs only)
        assert act == "relu" and relu_masks is None
        return nets.mlp(params, x, "tanh" if out_tanh else None)
    h = x
    for i, (w, b) in enumerate(params):
        h = torch.nn.functional.linear(h, w, b)
        if i < len(params) - 1:
            h = ACT_FN[act](h) if relu_masks is None else h * torch.as_tensor(np.asarray(relu_masks[i]), dtype=h.dtype)
    return torch.tanh(h) if out_tanh else h


def forward64(params, obs, act, out_tanh=False):
    p64 = [(_t(w, torch.float64), _t(b, torch.float64)) for w, b in params]
    return mlp(p64, _t(obs, torch.float64), act, out_tanh).numpy()


def forward32(params, obs, act, out_tanh=False):
    p32 = [(_t(w, torch.float32), _t(b, torch.float32)) for w, b in params]
    return mlp(p32, _t(obs, torch.float32), act, out_tanh).numpy()


def assert_forward_close(got, want64, label=""):
    """A head's outputs: |dy| <= 1e-5 |y| + 2e-6 elementwise (the rule of fp64_gate.gauss_logp_check)."""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    d = np.abs(got - want64) - (FWD_RTOL * np.abs(want64) + FWD_ATOL)
    print(f"[act forward] {label}: max |dy| = {np.abs(got - want64).max():.2e}, worst margin {d.max():.2e}")
    assert d.max() <= 0, (label, float(d.max()))


def head_terms(head, z, acts, log_std=None, var=(0.1, 1.0), bins=None, mask=None):
    """(log p [n], entropy scalar) of stored actions under the head's distribution on the network output z (the Gaussian head's z
    is already tanh'ed).  mask (discrete: bool [n, A]; nvec: bool [n, sum(bins)]): invalid logits are -inf; the entropy runs over
    the valid actions.  nvec: a stored action its mask marks invalid contributes the literal value and no gradient through its own
    logit (its one-hot is dropped)."""
    n = z.shape[0]
    if head == "discrete":
        a = acts.long().view(-1, 1)
        if mask is None:
            p = torch.clamp(torch.softmax(z, -1), min=nets.PROB_MIN, max=1)
            lp = torch.log(p)
            return lp.gather(-1, a).view(-1), -(lp * p).sum(-1).mean()
        m = torch.as_tensor(np.asarray(mask, bool))
        p = torch.clamp(torch.softmax(z.masked_fill(~m, float("-inf")), -1), min=nets.PROB_MIN, max=1)
        lp = torch.log(p)
        return lp.gather(1, a).view(-1), -torch.where(m, lp * p, torch.zeros_like(p)).sum(-1).mean()
    if head == "gaussian":
        k = z.shape[1] // 2
        m, b = nets.var_map(*var)
        mean, std = z[:, :k], z[:, k:] * m + b
        return nets.gauss_logpdf(acts.view(n, k), mean, std).sum(1), (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)).mean()
    if head == "diag":
        return logp_terms(acts.view(n, -1), z, log_std).sum(-1), row_entropy(log_std)
    m = torch.ones(z.shape, dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask, bool))
    a = acts.long().view(n, len(bins))
    logp, entropy = 0.0, 0.0
    for h, (s, b) in enumerate(zip(starts(bins), bins)):
        zh, mh = z[:, s:s + b], m[:, s:s + b]
        lse = torch.logsumexp(zh.masked_fill(~mh, float("-inf")), -1, keepdim=True)
        ls = zh - lse                                                    # finite everywhere; only the valid entries are used
        p = torch.where(mh, torch.exp(ls), torch.zeros_like(ls))
        entropy = entropy - (p * torch.where(mh, ls, torch.zeros_like(ls))).sum(-1)
        ah = a[:, h:h + 1]
        za = zh.gather(1, ah)
        za = torch.where(mh.gather(1, ah), za, za.detach())
        logp = logp + (za - lse).view(-1)
    return logp, entropy.mean()


def minibatch(dtype, head, pol, val, obs, acts, old_logp, adv, targets, clip, ent_coef, mb_ratio, *, pol_act="relu", val_act="relu",
              cobs=None, log_std=None, adv_norm=None, value_clip=None, relu_masks=None, **head_kw):
    """One PPO minibatch through autograd in `dtype`: the project's surrogate / entropy / mb_ratio scaling and the value loss of
    oracle/ppo.py::minibatch_autograd.  cobs: the critic's own matrix [n, d_c] (default: obs); adv_norm: (mean, scale) of the batch or
    None; value_clip: c or None (Stable-Baselines3's clipped value prediction around v_old = target - A); relu_masks: (policy's,
    critic's) imposed ReLU decisions; head_kw: var / bins / mask of head_terms.  grad_log_std: empty unless the head is diag."""
    pol = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in pol]
    val = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in val]
    ls = _t(log_std, dtype).requires_grad_(True) if head == "diag" else None
    obs, acts, old, A0, tgt = (_t(x, dtype) for x in (obs, acts, old_logp, adv, targets))
    cobs = obs if cobs is None else _t(cobs, dtype)
    mp, mv = relu_masks if relu_masks is not None else (None, None)
    A = A0 if adv_norm is None else (A0 - adv_norm[0]) * adv_norm[1]
    v = mlp(val, cobs, val_act, relu_masks=mv).view_as(tgt)
    if value_clip is not None:
        v_old = tgt - A0
        v = v_old + torch.clamp(v - v_old, -value_clip, value_clip)
    logp, entropy = head_terms(head, mlp(pol, obs, pol_act, out_tanh=head == "gaussian", relu_masks=mp), acts, log_std=ls, **head_kw)
    ratio = torch.exp(logp - old)
    policy_loss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A).mean()
    value_loss = torch.nn.functional.mse_loss(v, tgt) * mb_ratio
    ((policy_loss - entropy * ent_coef) * mb_ratio).backward()
    value_loss.backward()
    with torch.no_grad():
        lr = logp - old
        kl = ((torch.exp(lr) - 1) - lr).mean().item()
        clip_fraction = (torch.abs(ratio - 1) > clip).to(dtype).mean().item()
    z = lambda p: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    return dict(logp=logp.detach().numpy(), ratio=ratio.detach().numpy(), entropy=float(entropy.detach()), kl=kl, clip_fraction=clip_fraction,
                policy_loss=policy_loss.item(), value_loss=(value_loss / mb_ratio).item(),
                grad_policy=[(z(w), z(b)) for w, b in pol], grad_log_std=z(ls) if ls is not None else np.zeros(0),
                grad_value=[(z(w), z(b)) for w, b in val])


def tensors(r):
    """Every gradient tensor of a result: policy layers, critic layers, log_std (diag)."""
    out = [t for wb in r["grad_policy"] for t in wb] + [t for wb in r["grad_value"] for t in wb]
    return out + ([r["grad_log_std"]] if len(r["grad_log_std"]) else [])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def err(got, want):
    return max(rel(g, w) for g, w in zip(got, want))


def gate(got, r64, r32, label, floor=1e-5, stats=True):
    """The tolerance rule on every gradient tensor and the five statistics of a HIP result `got` (hip_pass.run_pass's dict); prints
    both errors behind `label`.  The statistics are scalars that may be 0 (a clip fraction) or the small difference of large float32
    terms (the KL term (r - 1) - log r), so their error is taken relative to max(|want|, 1e-3) with 1e-7 absolute on top -- the
    allowance tests/fp64_gate.py::gate gives its statistics; this is an addition to the rule as written for tensors, not part of it."""
    e_hip, e_32 = err(tensors(got), tensors(r64)), err(tensors(r32), tensors(r64))
    print(f"{label}: err(HIP, fp64)={e_hip:.2e}  err(float32 yardstick, fp64)={e_32:.2e}")
    assert e_hip <= max(floor, 1.5 * e_32), (label, e_hip, e_32)
    if stats:
        for k, name in enumerate(STAT_NAMES):
            want, f32 = float(r64[name]), float(r32[name])
            d_hip, d_32 = abs(float(got["stats"][k]) - want), abs(f32 - want)
            scale = max(abs(want), 1e-3)
            print(f"    {name}: |HIP - fp64| = {d_hip:.2e}, |float32 yardstick - fp64| = {d_32:.2e} (value {want:.6g})")
            assert d_hip <= max(floor * scale + 1e-7, 1.5 * d_32), (label, name, float(got["stats"][k]), want, f32)
    return e_hip, e_32


# ------------------------------------------------------------------------------------------ a whole learn()
def learn(dtype, head, act, pol, val, buf, batch_size, mini_batch_size, n_epochs, clip, ent_coef, policy_lr, critic_lr, rng,
          log_std=None, max_grad_norm=0.5, weakest=None):
    """PPOLearner.learn in `dtype` with stock torch: per epoch one permutation (numpy legacy stream), batches of consecutive
    slices, the minibatch gradients summed, clip_grad_norm_ over the WHOLE policy (layers and log_std under one norm) and over the
    critic, torch.optim.Adam.  `act` is the hidden activation of both networks; the critic reads buf["critic_states"] when the buffer
    has them, else buf["states"].  -> (policy vector [layers | log_std], critic vector).  weakest (dict, float64 runs): per network the
    smallest |g_i| / max|g| every parameter has seen (oracle/ppo.py::learn64)."""
    pol = [(torch.nn.Parameter(_t(w, dtype)), torch.nn.Parameter(_t(b, dtype))) for w, b in pol]
    val = [(torch.nn.Parameter(_t(w, dtype)), torch.nn.Parameter(_t(b, dtype))) for w, b in val]
    ls = torch.nn.Parameter(_t(log_std, dtype)) if head == "diag" else None
    p_params = [p for wb in pol for p in wb] + ([ls] if ls is not None else [])
    v_params = [p for wb in val for p in wb]
    opt_p, opt_v = torch.optim.Adam(p_params, lr=policy_lr), torch.optim.Adam(v_params, lr=critic_lr)
    B = {k: _t(v, dtype) for k, v in buf.items()}
    cstates = B["critic_states"] if "critic_states" in B else B["states"]
    total = B["advantages"].shape[0]
    mb_ratio = mini_batch_size / batch_size
    for _ in range(n_epochs):
        idx = rng.permutation(total)
        start = 0
        while start + batch_size <= total:
            bi = idx[start:start + batch_size]
            start += batch_size
            opt_p.zero_grad()
            opt_v.zero_grad()
            for s in range(0, batch_size, mini_batch_size):
                mi = torch.as_tensor(bi[s:s + mini_batch_size])
                logp, entropy = head_terms(head, mlp(pol, B["states"][mi], act, out_tanh=head == "gaussian"), B["actions"][mi], log_std=ls)
                ratio = torch.exp(logp - B["log_probs"][mi])
                A = B["advantages"][mi]
                policy_loss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A).mean()
                ((policy_loss - entropy * ent_coef) * mb_ratio).backward()
                (torch.nn.functional.mse_loss(mlp(val, cstates[mi], act).view(-1), B["values"][mi]) * mb_ratio).backward()
            if weakest is not None:
                for key, params in (("pol", p_params), ("val", v_params)):
                    flat = np.abs(np.concatenate([p.grad.detach().numpy().ravel() for p in params]))
                    r = flat / max(flat.max(), 1e-300)
                    weakest[key] = r if key not in weakest else np.minimum(weakest[key], r)
            torch.nn.utils.clip_grad_norm_(v_params, max_grad_norm)
            torch.nn.utils.clip_grad_norm_(p_params, max_grad_norm)
            opt_v.step()
            opt_p.step()
    flat = lambda params: np.concatenate([p.detach().numpy().ravel() for p in params]).astype(np.float64)
    return flat(p_params), flat(v_params)


# ------------------------------------------------------------------------------ under imposed ReLU decisions: the masked heads
CLIP, ENT = 0.2, 0.005   # the masked tests' clip range and entropy coefficient


def masked_chain(head, pol, val, obs, acts, old, adv, tgt, mask, mb_ratio, dtype, mp=None, mv=None, bins=None):
    """The masked update (head "discrete" or "nvec", head_terms' mask semantics) in torch autograd, float64 under imposed ReLU
    decisions mp / mv or float32 (the CPU restatement, its own decisions).
    -> (grad_policy, grad_value, [entropy, kl, vloss, clipfrac, ploss], ratio)."""
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    Pp = [(T(w).requires_grad_(), T(b).requires_grad_()) for w, b in pol]
    Vp = [(T(w).requires_grad_(), T(b).requires_grad_()) for w, b in val]
    logp, entropy = head_terms(head, mlp(Pp, T(obs), relu_masks=mp), torch.as_tensor(np.asarray(acts)), bins=bins, mask=mask)
    lr = logp - T(old)
    ratio = torch.exp(lr)
    A = T(adv)
    ploss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * A).mean()
    vloss = ((mlp(Vp, T(obs), relu_masks=mv).view(-1) - T(tgt)) ** 2).mean()
    ((ploss - entropy * ENT) * mb_ratio).backward()
    (vloss * mb_ratio).backward()
    g = lambda ps: [(w.grad.detach().numpy().astype(np.float64), b.grad.detach().numpy().astype(np.float64)) for w, b in ps]
    stats = [float(x.detach()) for x in (entropy, ((ratio - 1) - lr).mean(), vloss, ((ratio - 1).abs() > CLIP).double().mean(), ploss)]
    return g(Pp), g(Vp), stats, ratio.detach().numpy().astype(np.float64)


def masked_gate(L, head, pol, val, pr, got, label, mb_ratio=1.0, bins=None):
    """err(HIP, fp64 under the HIP's ReLU decisions) <= max(1e-5, 1.5 x err(float32 torch restatement, fp64 under its own)), for the
    gradients and for the five statistics; both printed behind `label`.  pr: the rows of the pass (obs, acts, old, adv, tgt, mask);
    got = (grad_policy, grad_value, stats or None).  nvec: the caller has patched the oracle's bins
    (multidiscrete_nvec_yardstick.patch_oracle) -- the hidden layers know no mask: minibatch_analytic gives their float64
    pre-activations and rounding scales."""
    gp, gv, stats = got
    args = (pr["obs"], pr["acts"], pr["old"], pr["adv"], pr["tgt"], pr["mask"], mb_ratio)
    det = {}
    ppo.minibatch_analytic("multidiscrete" if head == "nvec" else head, pol, val, pr["obs"], pr["acts"], pr["old"], pr["adv"], pr["tgt"], CLIP,
                           ENT, mb_ratio, (0.1, 1.0), detail=det)
    cp, cv, cstats, _ = masked_chain(head, pol, val, *args, torch.float32, bins=bins)
    res = {}
    for who, g_p, g_v, st, mp, mv in (("hip", gp, gv, stats, fp64_gate.hip_masks(L, pol, pr["obs"]), fp64_gate.hip_masks(L, val, pr["obs"])),
                                      ("cpu", cp, cv, cstats, fp64_gate.cpu_masks(pol, pr["obs"]), fp64_gate.cpu_masks(val, pr["obs"]))):
        flips = fp64_gate._check_flips(pol, mp, det["pol"], who) + fp64_gate._check_flips(val, mv, det["val"], who)
        tp, tv, tstats, _ = masked_chain(head, pol, val, *args, torch.float64, mp, mv, bins=bins)
        e = fp64_gate.grads_err(list(g_p) + list(g_v), tp + tv)
        serr = None if st is None else [abs(float(st[k]) - tstats[k]) / max(abs(tstats[k]), 1e-12) for k in range(5)]
        res[who] = (e, serr, flips)
    more = f"  old log-probs redrawn {pr['redrawn']}, rows outside the clip interval {pr['outside']:.3f}" if "redrawn" in pr else ""
    print(f"{label}: err(HIP, fp64)={res['hip'][0]:.2e}  err(CPU fp32, fp64)={res['cpu'][0]:.2e}  ReLU flips HIP "
          f"{res['hip'][2]} / CPU {res['cpu'][2]}  stats (entropy, kl, vloss, clipfrac, ploss) HIP {res['hip'][1]} CPU {res['cpu'][1]}{more}")
    assert res["hip"][0] <= max(1e-5, 1.5 * res["cpu"][0]), (label, res["hip"][0], res["cpu"][0])
    if res["hip"][1] is not None:
        for k in range(5):
            assert res["hip"][1][k] <= max(1e-5, 1.5 * res["cpu"][1][k]), (label, "statistic", k, res["hip"][1][k], res["cpu"][1][k])
    return res
