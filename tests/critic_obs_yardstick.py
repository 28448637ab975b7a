"""The yardstick of the asymmetric actor-critic (include/rlppo.h, "[critic rows]"; PPOLearner(obs_space_size=ObsSizes(d, d_c)),
ExperienceBuffer.critic_states, Learner(critic_observations=True)): the PPO minibatch and a whole learn() of
tests/activation_yardstick.py with ONE change -- the critic reads a matrix of its own (`cobs`, [n, d_c]) where the policy reads `obs` --
restated in torch with autograd, in float64 (the truth) and float32 (what a correct float32 implementation may miss the truth by), and
the HIP side of one pass through rlppo_ppo_minibatch_critic.

The tolerance rule is the project's (activation_yardstick.gate): err(HIP, float64) <= max(1e-5, 1.5 x err(float32 yardstick, float64))."""
import ctypes

import numpy as np
import torch

import activation_yardstick as A
from activation_yardstick import ACT_CODE, HEAD_CODE, _t, gate, head_terms, mlp, tensors  # noqa: F401
from oracle import nets

COUNTER = 15   # rlppo_dbg_counter: passes with separate critic rows


def minibatch(dtype, head, pol_act, val_act, pol, val, obs, cobs, acts, old_logp, adv, targets, clip, ent_coef, mb_ratio, log_std=None, **hk):
    """activation_yardstick.minibatch with the critic on `cobs`: the two losses share nothing but the rows' order."""
    pol = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in pol]
    val = [(_t(w, dtype).requires_grad_(True), _t(b, dtype).requires_grad_(True)) for w, b in val]
    ls = _t(log_std, dtype).requires_grad_(True) if head == "diag" else None
    obs, cobs, acts, old, adv_, tgt = (_t(x, dtype) for x in (obs, cobs, acts, old_logp, adv, targets))
    v = mlp(val, cobs, val_act).view_as(tgt)
    logp, entropy = head_terms(head, mlp(pol, obs, pol_act, out_tanh=head == "gaussian"), acts, dtype, log_std=ls, **hk)
    ratio = torch.exp(logp - old)
    policy_loss = -torch.min(ratio * adv_, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv_).mean()
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


def learn(dtype, head, act, pol, val, buf, batch_size, mini_batch_size, n_epochs, clip, ent_coef, policy_lr, critic_lr, rng, log_std=None,
          max_grad_norm=0.5, weakest=None):
    """activation_yardstick.learn with the critic on buf["critic_states"]."""
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
                logp, entropy = head_terms(head, mlp(pol, B["states"][mi], act, out_tanh=head == "gaussian"), B["actions"][mi], dtype, log_std=ls)
                ratio = torch.exp(logp - B["log_probs"][mi])
                adv = B["advantages"][mi]
                policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv).mean()
                ((policy_loss - entropy * ent_coef) * mb_ratio).backward()
                (torch.nn.functional.mse_loss(mlp(val, B["critic_states"][mi], act).view(-1), B["values"][mi]) * mb_ratio).backward()
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


def pad_rows(x, ld):
    """[n, d] -> device rows [n, ld], zero-padded (ld a multiple of 4, >= the padded width of d)."""
    x = np.asarray(x, np.float32)
    out = torch.zeros((x.shape[0], ld), dtype=torch.float32)
    out[:, :x.shape[1]] = torch.as_tensor(x)
    return out.cuda()


def run_pass(L, head, pol_act, val_act, pol, val, obs_all, acts_all, old_all, tgt_all, adv_all, idx, clip, ent, mb_ratio, cobs_all=None, critic_ld=None,
             log_std=None, var=(0.1, 1.0), bins=None, mask=None, ring=None, n_rows=None, grads=None, precision="fp32", entry="critic",
             ws_fn=None, states_ld=None):
    """One pass.  entry = "critic": rlppo_ppo_minibatch_critic with the critic's matrix `cobs_all` at leading dimension critic_ld
    (default: its padded width); "critic_null": the same entry point with critic == NULL; "critic_null_states": with a struct whose
    `states` is NULL; "ex": rlppo_ppo_minibatch_ex (cobs_all unused: one matrix for both).  ws_fn: the workspace size function
    (default: the entry point's own).  The workspace is prefilled with NaN bit patterns and has a guard band behind it that must
    come back untouched.  -> dict(gp, gv, stats, grad_policy, grad_log_std, grad_value, rc, msg)."""
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.util import action_mask as AM
    from test_gpu_kernels import Net, dev, stream
    if ring is not None:
        rot = lambda x: None if x is None else np.roll(np.asarray(x), ring, axis=0)
        obs_all, cobs_all, acts_all, old_all, tgt_all, adv_all, mask = (rot(x) for x in (obs_all, cobs_all, acts_all, old_all, tgt_all, adv_all, mask))
    P_, V_ = Net(L, pol), Net(L, val)
    k = P_.dims[-1] if head == "diag" else 0
    states = pad_rows(obs_all, states_ld or P_.ld_in)
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
    with_rows = entry == "critic"
    if ws_fn is None:
        ws_fn = L.rlppo_minibatch_workspace_bytes_critic if with_rows else L.rlppo_minibatch_workspace_bytes_for
    ws_bytes = int(ws_fn(P_.dims_c, P_.nl, V_.dims_c, V_.nl, mb, a.precision))
    guard = 1024
    ws = torch.full(((ws_bytes + 3) // 4 + guard,), -1, dtype=torch.int32, device="cuda")   # 0xFFFFFFFF: a NaN in every float
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
        width = sum(bins) if bins is not None else P_.dims[-1]
        words = AM.pack(torch.as_tensor(np.asarray(mask, bool)), width, "cuda")
        a.action_mask, a.mask_words = words.data_ptr(), words.shape[1]
        keep.append(words)
    x3 = precision == "x3"
    if x3:   # the split-bf16 planes of both networks
        for net, field in ((P_, "pol_wb16"), (V_, "val_wb16")):
            planes = torch.zeros(max(8, int(L.rlppo_x3_elems(net.dims_c, net.nl))), dtype=torch.int16, device="cuda")
            assert L.rlppo_net_pack_x3(stream(), net.dims_c, net.nl, ctypes.c_void_p(net.packed.data_ptr()), ctypes.c_void_p(planes.data_ptr())) == 0
            setattr(a, field, planes.data_ptr())
            keep.append(planes)
    ext = N.MinibatchExt()
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
    cr = N.CriticRows()
    if with_rows:
        cstates = pad_rows(cobs_all, critic_ld or V_.ld_in)
        cr.states, cr.ld_states = cstates.data_ptr(), cstates.shape[1]
        keep.append(cstates)
    if entry == "ex":
        rc = L.rlppo_ppo_minibatch_ex(stream(), ctypes.byref(a), ctypes.byref(ext))
    else:
        rc = L.rlppo_ppo_minibatch_critic(stream(), ctypes.byref(a), ctypes.byref(ext), None if entry == "critic_null" else ctypes.byref(cr))
    msg = L.rlppo_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    assert (ws[(ws_bytes + 3) // 4:] == -1).all(), "the pass wrote behind its workspace"
    gpc, gvc = gp.cpu(), gv.cpu()
    return dict(gp=gp, gv=gv, stats=stats.cpu().numpy(), rc=rc, msg=msg,
                grad_policy=[(w.numpy(), b.numpy()) for w, b in nets.unflatten(gpc[:n_net], pol)], grad_log_std=gpc[n_net:].numpy(),
                grad_value=[(w.numpy(), b.numpy()) for w, b in nets.unflatten(gvc, val)])
