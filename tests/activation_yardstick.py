"""The yardstick of the hidden-activation choice (Learner(hidden_activation=...), ppo.LayerSizes; include/rlppo.h, "[act]"): an MLP
whose hidden activation is a parameter ("relu", "tanh", "elu" with alpha = 1) and the PPO minibatch of the four heads -- discrete,
multi-discrete for any nvec with an optional mask, the reference's Gaussian, diagonal-Gaussian -- restated in torch with autograd,
run in float64 (the truth) and in float32 (what a correct float32 implementation is allowed to miss the truth by).

The tolerance rule is the project's (tests/fp64_gate.py, tests/diag_gaussian_yardstick.py): err(HIP, float64) <= max(1e-5, 1.5 x
err(this file in float32, float64)), err = the largest max|got - want| / max|want| over the tensors compared; the five report
statistics as diag_gaussian_yardstick.gate treats them.  Forward outputs: |dy| <= 1e-5 |y| + 2e-6 elementwise (the rule of
fp64_gate.gauss_logp_check for a head's outputs).  Inputs are asserted clear of the clip edges from float64 alone
(assert_clear_of_clip_edges).

With tanh / ELU no hidden decision is discrete: tanh is smooth, and ELU with alpha = 1 has the derivative (h > 0 ? 1 : h + 1), which
is CONTINUOUS at 0 (both sides give 1), so a pre-activation that float32 and float64 put on different sides of 0 changes the
gradient by O(|pre|), not by a whole term -- no counterpart of diag_gaussian_yardstick.assert_relu_clear is needed, and none is
applied."""
import ctypes
import math

import numpy as np
import torch

import diag_gaussian_yardstick as DY
from diag_gaussian_yardstick import STAT_NAMES, assert_clear_of_clip_edges, err, rel  # noqa: F401
from oracle import nets

ACT_CODE = {"relu": 0, "tanh": 1, "elu": 2}
ACT_FN = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}
HEAD_CODE = {"discrete": 0, "nvec": 1, "gaussian": 2, "diag": 3}
FWD_RTOL, FWD_ATOL = 1e-5, 2e-6


def _t(x, dtype):
    return x.detach().to(dtype).clone() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype).clone()


def mlp(params, x, act, out_tanh=False):
    h = x
    for i, (w, b) in enumerate(params):
        h = torch.nn.functional.linear(h, w, b)
        if i < len(params) - 1:
            h = ACT_FN[act](h)
    return torch.tanh(h) if out_tanh else h


def forward64(params, obs, act, out_tanh=False):
    p64 = [(_t(w, torch.float64), _t(b, torch.float64)) for w, b in params]
    return mlp(p64, _t(obs, torch.float64), act, out_tanh).numpy()


def forward32(params, obs, act, out_tanh=False):
    p32 = [(_t(w, torch.float32), _t(b, torch.float32)) for w, b in params]
    return mlp(p32, _t(obs, torch.float32), act, out_tanh).numpy()


def assert_forward_close(got, want64, label=""):
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    d = np.abs(got - want64) - (FWD_RTOL * np.abs(want64) + FWD_ATOL)
    print(f"[act forward] {label}: max |dy| = {np.abs(got - want64).max():.2e}, worst margin {d.max():.2e}")
    assert d.max() <= 0, (label, float(d.max()))


def starts(bins):
    return [int(s) for s in np.cumsum((0,) + tuple(bins))[:-1]]


def head_terms(head, z, acts, dtype, log_std=None, var=(0.1, 1.0), bins=None, mask=None):
    """(log p [n], entropy scalar) of stored actions under the head's distribution on the network output z (the Gaussian head's z
    is already tanh'ed).  The formulas are those of oracle/nets.py, diag_gaussian_yardstick.py and masked_multidiscrete_yardstick.py."""
    n = z.shape[0]
    if head == "discrete":
        p = torch.clamp(torch.softmax(z, -1), min=nets.PROB_MIN, max=1)
        lp = torch.log(p)
        return lp.gather(-1, acts.long().view(-1, 1)).view(-1), -(lp * p).sum(-1).mean()
    if head == "gaussian":
        k = z.shape[1] // 2
        m, b = nets.var_map(*var)
        mean, std = z[:, :k], z[:, k:] * m + b
        return nets.gauss_logpdf(acts.view(n, k), mean, std).sum(1), (0.5 + 0.5 * math.log(2 * math.pi) + torch.log(std)).mean()
    if head == "diag":
        return DY.logp_terms(acts.view(n, -1), z, log_std).sum(-1), DY.row_entropy(log_std)
    m = torch.ones(z.shape, dtype=torch.bool) if mask is None else torch.as_tensor(np.asarray(mask, bool))
    a = acts.long().view(n, len(bins))
    logp, entropy = 0.0, 0.0
    for h, (s, b) in enumerate(zip(starts(bins), bins)):
        zh, mh = z[:, s:s + b], m[:, s:s + b]
        lse = torch.logsumexp(zh.masked_fill(~mh, float("-inf")), -1, keepdim=True)
        ls = zh - lse
        p = torch.where(mh, torch.exp(ls), torch.zeros_like(ls))
        entropy = entropy - (p * torch.where(mh, ls, torch.zeros_like(ls))).sum(-1)
        logp = logp + (zh.gather(1, a[:, h:h + 1]) - lse).view(-1)
    return logp, entropy.mean()


def minibatch(dtype, head, pol_act, val_act, pol, val, obs, acts, old_logp, adv, targets, clip, ent_coef, mb_ratio, log_std=None, **hk):
    """One PPO minibatch through autograd in `dtype` -> the dict of diag_gaussian_yardstick.minibatch (grad_log_std: empty unless diag)."""
    pol = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in pol]
    val = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in val]
    ls = _t(log_std, dtype).requires_grad_(True) if head == "diag" else None
    obs, acts, old, A, tgt = (_t(x, dtype) for x in (obs, acts, old_logp, adv, targets))
    v = mlp(val, obs, val_act).view_as(tgt)
    logp, entropy = head_terms(head, mlp(pol, obs, pol_act, out_tanh=head == "gaussian"), acts, dtype, log_std=ls, **hk)
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
    out = [t for wb in r["grad_policy"] for t in wb] + [t for wb in r["grad_value"] for t in wb]
    return out + ([r["grad_log_std"]] if len(r["grad_log_std"]) else [])


def gate(got, r64, r32, label, floor=1e-5, stats=True):
    """diag_gaussian_yardstick.gate's rule on every gradient tensor and the five statistics of a HIP result `got`; prints both errors."""
    e_hip, e_32 = err(tensors(got), tensors(r64)), err(tensors(r32), tensors(r64))
    print(f"[act fp64 gate] {label}: err(HIP, fp64)={e_hip:.2e}  err(float32 yardstick, fp64)={e_32:.2e}")
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
    """PPOLearner.learn in `dtype` with stock torch (diag_gaussian_yardstick.learn with the head and the activation as parameters;
    `act` is the hidden activation of both networks).  -> (policy vector [layers | log_std], critic vector); weakest as there."""
    pol = [(torch.nn.Parameter(_t(w, dtype)), torch.nn.Parameter(_t(b, dtype))) for w, b in pol]
    val = [(torch.nn.Parameter(_t(w, dtype)), torch.nn.Parameter(_t(b, dtype))) for w, b in val]
    ls = torch.nn.Parameter(_t(log_std, dtype)) if head == "diag" else None
    p_params = [p for wb in pol for p in wb] + ([ls] if ls is not None else [])
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
                obs = B["states"][mi]
                logp, entropy = head_terms(head, mlp(pol, obs, act, out_tanh=head == "gaussian"), B["actions"][mi], dtype, log_std=ls)
                ratio = torch.exp(logp - B["log_probs"][mi])
                A = B["advantages"][mi]
                policy_loss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A).mean()
                ((policy_loss - entropy * ent_coef) * mb_ratio).backward()
                (torch.nn.functional.mse_loss(mlp(val, obs, act).view(-1), B["values"][mi]) * mb_ratio).backward()
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
def run_pass(L, head, pol_act, val_act, pol, val, obs_all, acts_all, old_all, tgt_all, adv_all, idx, clip, ent, mb_ratio, log_std=None,
             var=(0.1, 1.0), bins=None, mask=None, ring=None, n_rows=None, grads=None, entry="ex", precision="fp32"):
    """One pass through rlppo_ppo_minibatch_ex (entry = "ex": the extension carries the activations and the head's extras;
    "ex_zero": an all-zero extension; "ex_null": a NULL one; "plain": rlppo_ppo_minibatch).  The workspace is prefilled with NaN bit
    patterns.  mask: bool [rows, sum(bins)].  -> dict(gp, gv, stats, grad_policy, grad_log_std, grad_value, rc, msg)."""
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.util import action_mask as AM
    from test_gpu_kernels import Net, dev, stream
    if ring is not None:
        rot = lambda x: None if x is None else np.roll(np.asarray(x), ring, axis=0)
        obs_all, acts_all, old_all, tgt_all, adv_all, mask = (rot(x) for x in (obs_all, acts_all, old_all, tgt_all, adv_all, mask))
    P_, V_ = Net(L, pol), Net(L, val)
    k = P_.dims[-1] if head == "diag" else 0
    states = P_.pad(obs_all)
    acts = dev(np.asarray(acts_all, np.float32).reshape(len(obs_all), -1))
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim = HEAD_CODE[head], P_.nl, V_.nl, acts.shape[1]
    a.pol_dims = ctypes.cast(P_.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(V_.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.precision = {"fp32": N.PRECISION_FP32, "bf16": N.PRECISION_BF16, "x3": N.PRECISION_X3}[precision]
    n_net = P_.flat.numel()
    gp, gv = grads if grads is not None else (torch.zeros(n_net + k, device="cuda"), torch.zeros_like(V_.flat))
    old, tgt, adv = dev(old_all), dev(tgt_all), dev(adv_all)
    idxd = dev(idx, torch.int64)
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    mb = len(idx)
    ws_bytes = int(L.rlppo_minibatch_workspace_bytes_for(P_.dims_c, P_.nl, V_.dims_c, V_.nl, mb, a.precision))
    ws = torch.full(((ws_bytes + 3) // 4,), -1, dtype=torch.int32, device="cuda")   # 0xFFFFFFFF: a NaN in every float
    a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = P_.packed.data_ptr(), V_.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
    a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], states.shape[0] if n_rows is None else n_rows, acts.data_ptr()
    a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idxd.data_ptr(), mb
    if ring is not None:
        a.ring_base, a.ring_cap = ring, len(obs_all)
    a.clip_range, a.ent_coef, a.mb_ratio = clip, ent, mb_ratio
    a.var_m, a.var_b = nets.var_map(*var)
    a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
    keep = []
    if mask is not None:
        words = AM.pack(torch.as_tensor(np.asarray(mask, bool)), sum(bins), "cuda")
        a.action_mask, a.mask_words = words.data_ptr(), words.shape[1]
        keep.append(words)
    ext = N.MinibatchExt()
    if entry == "ex":
        ext.pol_hidden_act, ext.val_hidden_act = ACT_CODE[pol_act], ACT_CODE[val_act]
        if head == "nvec":
            nvec = N.dims_array(bins)
            ext.md_nvec, ext.md_heads = ctypes.cast(nvec, ctypes.POINTER(ctypes.c_int32)), len(bins)
            keep.append(nvec)
        if head == "diag":
            lsd = dev(log_std)
            sb = int(L.rlppo_diag_scratch_bytes(mb, k))
            scratch = torch.full((sb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
            ext.log_std, ext.log_std_grad, ext.scratch, ext.scratch_bytes = lsd.data_ptr(), gp.data_ptr() + 4 * n_net, scratch.data_ptr(), sb
            keep += [lsd, scratch]
    if entry == "plain":
        rc = L.rlppo_ppo_minibatch(stream(), ctypes.byref(a))
    else:
        rc = L.rlppo_ppo_minibatch_ex(stream(), ctypes.byref(a), None if entry == "ex_null" else ctypes.byref(ext))
    msg = L.rlppo_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    if entry == "ex" and head == "diag" and rc == 0:
        assert (keep[-1][sb:] == 0xFF).all(), "the pass wrote behind its scratch region"
    gpc, gvc = gp.cpu(), gv.cpu()
    return dict(gp=gp, gv=gv, stats=stats.cpu().numpy(), rc=rc, msg=msg,
                grad_policy=[(w.numpy(), b.numpy()) for w, b in nets.unflatten(gpc[:n_net], pol)], grad_log_std=gpc[n_net:].numpy(),
                grad_value=[(w.numpy(), b.numpy()) for w, b in nets.unflatten(gvc, val)])
