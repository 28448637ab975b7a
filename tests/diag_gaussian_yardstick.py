"""The yardstick of the diagonal-Gaussian head with a learnable log_std (include/rlppo.h, "[diag]"): the head and the PPO minibatch
restated in torch with autograd, run in float64 (the truth) and in float32 (what a correct float32 implementation is allowed to
miss the truth by).  MLP with ReLU, Normal(mean, exp(log_std)), the project's surrogate / entropy / mb_ratio scaling and the value
loss of oracle/ppo.py::minibatch_autograd; entropy = sum over the action dimensions of Normal.entropy(), no division by k.

The tolerance rule of tests/fp64_gate.py: err(HIP, float64) <= max(1e-5, 1.5 x err(this file in float32, float64)), err = the
largest max|got - want| / max|want| over the tensors compared.  Inputs are chosen (and asserted here, on the CPU, from float64
alone) so that no ratio lies near a clip edge and no hidden pre-activation lies within its float32 rounding bound of 0: no discrete
decision is left for two float32 implementations to disagree on."""
import ctypes
import math

import numpy as np
import torch

from oracle import nets, ppo

U32 = 2.0 ** -24
ENT_C = 0.5 + 0.5 * math.log(2 * math.pi)   # 1.4189385332046727
HALF_LOG_2PI = math.log(math.sqrt(2 * math.pi))


def _t(x, dtype):
    return x.detach().to(dtype).clone() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype).clone()


def mlp(params, x):
    if nets._BF16_OPERANDS[0]:   # inside oracle.nets.bf16_operands(): the bf16 update precision's restatement (float32 runs only)
        return nets.mlp(params, x)
    h = x
    for i, (w, b) in enumerate(params):
        h = torch.nn.functional.linear(h, w, b)
        if i < len(params) - 1:
            h = torch.relu(h)
    return h


def logp_terms(acts, mean, log_std):
    """Normal.log_prob's three terms in its order, closed form."""
    var = torch.exp(log_std) ** 2
    return -((acts - mean) ** 2) / (2 * var) - log_std - HALF_LOG_2PI


def row_entropy(log_std):
    return (ENT_C + log_std).sum()


def check_closed_form(mean, log_std, acts):
    """float64: the closed forms above equal torch.distributions.Normal's to 1e-12."""
    mean, log_std, acts = _t(mean, torch.float64), _t(log_std, torch.float64), _t(acts, torch.float64)
    dist = torch.distributions.Normal(mean, torch.exp(log_std).expand_as(mean))
    e_lp = (logp_terms(acts, mean, log_std) - dist.log_prob(acts)).abs().max().item()
    e_ent = (row_entropy(log_std) - dist.entropy().sum(-1)).abs().max().item()
    assert e_lp <= 1e-12 and e_ent <= 1e-12, (e_lp, e_ent)
    return e_lp, e_ent


def sample64(pol, log_std, obs, eps):
    """float64: (mean, actions = mean + exp(log_std) eps, log p of those actions)."""
    p64 = [(_t(w, torch.float64), _t(b, torch.float64)) for w, b in pol]
    mean = mlp(p64, _t(obs, torch.float64))
    ls = _t(log_std, torch.float64)
    act = mean + torch.exp(ls) * _t(eps, torch.float64)
    return mean.numpy(), act.numpy(), logp_terms(act, mean, ls).sum(-1).numpy()


def adv_stats(adv):
    """(mean, 1 / (std + 1e-8)) of a batch's advantages, unbiased std: rlppo_adv_stats."""
    a = np.asarray(adv, np.float64)
    return float(a.mean()), float(1.0 / (a.std(ddof=1) + 1e-8))


def minibatch(dtype, pol, log_std, val, obs, acts, old_logp, adv, targets, clip, ent_coef, mb_ratio, adv_norm=None, value_clip=None):
    """One PPO minibatch through autograd in `dtype`.  adv_norm: (mean, scale) of the batch or None; value_clip: c or None
    (Stable-Baselines3's clipped value prediction around v_old = target - A)."""
    pol = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in pol]
    val = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in val]
    ls = _t(log_std, dtype).requires_grad_(True)
    obs, acts, old, A0, tgt = (_t(x, dtype) for x in (obs, acts, old_logp, adv, targets))
    acts = acts.view(obs.shape[0], -1)
    A = A0 if adv_norm is None else (A0 - adv_norm[0]) * adv_norm[1]
    v = mlp(val, obs).view_as(tgt)
    if value_clip is not None:
        v_old = tgt - A0
        v = v_old + torch.clamp(v - v_old, -value_clip, value_clip)
    logp = logp_terms(acts, mlp(pol, obs), ls).sum(-1)
    entropy = row_entropy(ls)   # the same for every row: its mean over the rows is itself
    ratio = torch.exp(logp - old)
    clipped = torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    policy_loss = -torch.min(ratio * A, clipped * A).mean()
    value_loss = torch.nn.functional.mse_loss(v, tgt) * mb_ratio
    ((policy_loss - entropy * ent_coef) * mb_ratio).backward()
    value_loss.backward()
    with torch.no_grad():
        lr = logp - old
        kl = ((torch.exp(lr) - 1) - lr).mean().item()
        clip_fraction = (torch.abs(ratio - 1) > clip).to(dtype).mean().item()
    z = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)
    return dict(logp=logp.detach().numpy(), ratio=ratio.detach().numpy(), entropy=entropy.item(), kl=kl, clip_fraction=clip_fraction,
                policy_loss=policy_loss.item(), value_loss=(value_loss / mb_ratio).item(),
                grad_policy=[(z(w).numpy(), z(b).numpy()) for w, b in pol], grad_log_std=z(ls).numpy(),
                grad_value=[(z(w).numpy(), z(b).numpy()) for w, b in val])


STAT_NAMES = ("entropy", "kl", "value_loss", "clip_fraction", "policy_loss")   # RLPPO_STAT_* 0..4


def tensors(r):
    """Every gradient tensor of a result: policy layers, log_std, critic layers."""
    return [t for wb in r["grad_policy"] for t in wb] + [r["grad_log_std"]] + [t for wb in r["grad_value"] for t in wb]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def err(got, want):
    return max(rel(g, w) for g, w in zip(got, want))


def assert_clear_of_clip_edges(ratio, clip, margin=1e-4):
    """No ratio of the float64 run within `margin` of a clip edge (float32 carries ~1e-6 of rounding in a ratio), and rows on both
    sides of both edges."""
    r = np.asarray(ratio, np.float64)
    d = np.minimum(np.abs(r - (1.0 - clip)), np.abs(r - (1.0 + clip)))
    assert d.min() > margin, ("a ratio sits near a clip edge: regenerate the seed", float(d.min()))


def assert_relu_clear(params, obs, who=""):
    """No hidden pre-activation of the float64 forward within its float32 rounding bound of 0 (the bound of tests/fp64_gate.py,
    with its factor 2 of slack): B_l = (K_l + 2) u (sum_k |h_k w_jk| + |b_j|) + |W_l| B_(l-1).  A seed that trips it is replaced."""
    p64 = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in params]
    det = {}
    ppo._fwd64(p64, np.asarray(obs, np.float64), detail=det)
    prev = None
    for l, (pre, scale) in enumerate(zip(det.get("pre", []), det.get("scale", []))):
        w = np.abs(p64[l][0])
        bound = (w.shape[1] + 2) * U32 * scale
        if prev is not None:
            bound = bound + prev @ w.T
        prev = bound
        worst = float((np.abs(pre) / bound).min())
        assert worst > 2.0, (who, "a hidden pre-activation sits within float32 rounding of 0: regenerate the seed", l, worst)


def gate(got_tensors, got_stats, r64, r32, label, floor=1e-5):
    """The tolerance rule on every gradient tensor and the five statistics; prints both errors.  The statistics are scalars that may
    be 0 (a clip fraction) or the small difference of large float32 terms (the KL term (r - 1) - log r), so their error is taken
    relative to max(|want|, 1e-3) with 1e-7 absolute on top -- the allowance tests/fp64_gate.py::gate gives its statistics; this is
    an addition to the rule as written for tensors, not part of it."""
    e_hip, e_32 = err(got_tensors, tensors(r64)), err(tensors(r32), tensors(r64))
    print(f"[diag fp64 gate] {label}: err(HIP, fp64)={e_hip:.2e}  err(float32 yardstick, fp64)={e_32:.2e}")
    assert e_hip <= max(floor, 1.5 * e_32), (label, e_hip, e_32)
    if got_stats is not None:
        for k, name in enumerate(STAT_NAMES):
            want, f32 = float(r64[name]), float(r32[name])
            d_hip, d_32 = abs(float(got_stats[k]) - want), abs(f32 - want)
            scale = max(abs(want), 1e-3)
            print(f"    {name}: |HIP - fp64| = {d_hip:.2e}, |float32 yardstick - fp64| = {d_32:.2e} (value {want:.6g})")
            assert d_hip <= max(floor * scale + 1e-7, 1.5 * d_32), (label, name, float(got_stats[k]), want, f32)
    return e_hip, e_32


# ------------------------------------------------------------------------------------------ a whole learn()
def learn(dtype, pol, log_std, val, buf, batch_size, mini_batch_size, n_epochs, clip, ent_coef, policy_lr, critic_lr, rng,
          max_grad_norm=0.5, weakest=None):
    """PPOLearner.learn in `dtype` with stock torch: per epoch one permutation (numpy legacy stream), batches of consecutive
    slices, the minibatch gradients summed, clip_grad_norm_ over the WHOLE policy (layers and log_std under one norm) and over the
    critic, torch.optim.Adam.  Returns (policy vector [layers | log_std], critic vector).  weakest (dict, float64 runs): per
    network the smallest |g_i| / max|g| every parameter has seen (oracle/ppo.py::learn64)."""
    pol = [(torch.nn.Parameter(_t(w, dtype)), torch.nn.Parameter(_t(b, dtype))) for w, b in pol]
    val = [(torch.nn.Parameter(_t(w, dtype)), torch.nn.Parameter(_t(b, dtype))) for w, b in val]
    ls = torch.nn.Parameter(_t(log_std, dtype))
    p_params = [p for wb in pol for p in wb] + [ls]
    v_params = [p for wb in val for p in wb]
    opt_p, opt_v = torch.optim.Adam(p_params, lr=policy_lr), torch.optim.Adam(v_params, lr=critic_lr)
    B = {k: _t(v, dtype) for k, v in buf.items()}
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
                obs, acts = B["states"][mi], B["actions"][mi].view(len(mi), -1)
                logp = logp_terms(acts, mlp(pol, obs), ls).sum(-1)
                ratio = torch.exp(logp - B["log_probs"][mi])
                A = B["advantages"][mi]
                policy_loss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A).mean()
                ((policy_loss - row_entropy(ls) * ent_coef) * mb_ratio).backward()
                (torch.nn.functional.mse_loss(mlp(val, obs).view(-1), B["values"][mi]) * mb_ratio).backward()
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


# ------------------------------------------------------------------------------------------ the HIP side
def run_minibatch_diag(L, pol, log_std, val, obs_all, acts_all, old_all, tgt_all, adv_all, idx, clip, ent, mb_ratio, ring=None,
                       precision="fp32", adv_norm=None, value_clip=0.0, kl_slots=False, stop=None, grads=None, scratch_pad=64, n_rows=None):
    """One pass of rlppo_ppo_minibatch_diag.  The gradient arena of the policy is [layers | log_std] (the tail behind the layers), as
    NetArena lays it out.  grads = (gp, gv): accumulate into these arenas instead of fresh zeroed ones.  The scratch is prefilled
    with NaN bit patterns (the pass must need no zeroing) and carries `scratch_pad` canary bytes behind it.  n_rows = 0: the
    buffer's row count is withheld (rlppo_minibatch_args.n_rows == 0: the rows are gathered into the workspace first).
    -> dict(gp=flat policy arena, gv, stats, grad_policy, grad_log_std, grad_value, kl=slots or None)."""
    from oracle import nets
    from rlgym_ppo_amd import _native as N
    from test_gpu_kernels import Net, check, dev, stream
    if ring is not None:
        rot = lambda x: np.roll(np.asarray(x), ring, axis=0)
        obs_all, acts_all, old_all, tgt_all, adv_all = (rot(x) for x in (obs_all, acts_all, old_all, tgt_all, adv_all))
    P_, V_ = Net(L, pol), Net(L, val)
    k = P_.dims[-1]
    states = P_.pad(obs_all)
    acts = dev(np.asarray(acts_all, np.float32).reshape(len(obs_all), -1))
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim = N.HEAD_DIAG_GAUSSIAN, P_.nl, V_.nl, acts.shape[1]
    a.pol_dims = ctypes.cast(P_.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(V_.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.precision = {"fp32": N.PRECISION_FP32, "bf16": N.PRECISION_BF16, "x3": N.PRECISION_X3}[precision]
    n_net = P_.flat.numel()
    gp, gv = grads if grads is not None else (torch.zeros(n_net + k, device="cuda"), torch.zeros_like(V_.flat))
    lsd = dev(log_std)
    old, tgt, adv = dev(old_all), dev(tgt_all), dev(adv_all)
    idxd = dev(idx, torch.int64)
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    mb = len(idx)
    ws_bytes = int(L.rlppo_minibatch_workspace_bytes_for(P_.dims_c, P_.nl, V_.dims_c, V_.nl, mb, a.precision))
    ws = torch.full(((ws_bytes + 3) // 4,), -1, dtype=torch.int32, device="cuda")   # 0xFFFFFFFF: a NaN in every float
    a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = P_.packed.data_ptr(), V_.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
    keep = []
    if precision == "bf16":
        for net, names in ((P_, ("pol_packed_r", "pol_wb16")), (V_, ("val_packed_r", "val_wb16"))):
            pr = torch.zeros_like(net.packed)
            wb = torch.zeros(int(L.rlppo_wb16_elems(net.dims_c, net.nl)), dtype=torch.bfloat16, device="cuda")
            check(L, L.rlppo_net_pack_bf16(stream(), net.dims_c, net.nl, ctypes.c_void_p(net.flat.data_ptr()), ctypes.c_void_p(pr.data_ptr()),
                                           ctypes.c_void_p(wb.data_ptr())))
            setattr(a, names[0], pr.data_ptr())
            setattr(a, names[1], wb.data_ptr())
            keep += [pr, wb]
    if precision == "x3":
        for net, name in ((P_, "pol_wb16"), (V_, "val_wb16")):
            pl = torch.zeros(max(int(L.rlppo_x3_elems(net.dims_c, net.nl)), 8), dtype=torch.bfloat16, device="cuda")
            check(L, L.rlppo_net_pack_x3(stream(), net.dims_c, net.nl, ctypes.c_void_p(net.packed.data_ptr()), ctypes.c_void_p(pl.data_ptr())))
            setattr(a, name, pl.data_ptr())
            keep.append(pl)
    a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], states.shape[0] if n_rows is None else n_rows, acts.data_ptr()
    a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idxd.data_ptr(), mb
    if ring is not None:
        a.ring_base, a.ring_cap = ring, len(obs_all)
    a.clip_range, a.ent_coef, a.mb_ratio = clip, ent, mb_ratio
    a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
    if adv_norm is not None:
        an = dev(np.asarray(adv_norm, np.float32))
        a.adv_norm = an.data_ptr()
    a.value_clip = float(value_clip)
    slots = None
    if kl_slots:
        slots = torch.full((int(L.rlppo_kl_slots_doubles(mb)),), float("nan"), dtype=torch.float64, device="cuda")
        a.kl_slots = slots.data_ptr()
    if stop is not None:
        sw = torch.full((1,), int(stop), dtype=torch.int32, device="cuda")
        a.stop_word = sw.data_ptr()
    sb = int(L.rlppo_diag_scratch_bytes(mb, k))
    assert sb == ((mb + 255) // 256) * k * 8   # one row of k doubles per workgroup of 256 rows
    scratch = torch.full((sb + scratch_pad,), 0xFF, dtype=torch.uint8, device="cuda")
    check(L, L.rlppo_ppo_minibatch_diag(stream(), ctypes.byref(a), ctypes.c_void_p(lsd.data_ptr()), ctypes.c_void_p(gp.data_ptr() + 4 * n_net),
                                        ctypes.c_void_p(scratch.data_ptr()), sb))
    torch.cuda.synchronize()
    assert (scratch[sb:] == 0xFF).all(), "the pass wrote behind its scratch region"
    gpc, gvc = gp.cpu(), gv.cpu()
    return dict(gp=gp, gv=gv, stats=stats.cpu().numpy(), grad_policy=[(w.numpy(), b.numpy()) for w, b in nets.unflatten(gpc[:n_net], pol)],
                grad_log_std=gpc[n_net:].numpy(), grad_value=[(w.numpy(), b.numpy()) for w, b in nets.unflatten(gvc, val)],
                kl=None if slots is None else slots.cpu().numpy())
