"""The device side of the GPU tests, once: the library handle, the small pointer helpers, a network's device images (Net) and ONE
runner of a PPO minibatch pass through every exported form of it (run_pass).  A helper module: it holds no test."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nets

ACT_CODE = {"relu": 0, "tanh": 1, "elu": 2}
HEAD_CODE = {"discrete": 0, "nvec": 1, "multidiscrete": 1, "gaussian": 2, "diag": 3}   # RLPPO_HEAD_*
GUARD_WORDS = 1024     # int32 words behind the workspace of every pass
SCRATCH_CANARY = 64    # bytes behind the diag head's scratch region


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from rlgym_ppo_amd import _native as N
    return N.lib()


def dev(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x)).to("cuda", dtype=dtype).contiguous()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def relerr(a, b):
    a = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a, np.float64)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def check(L, rc):
    assert rc == 0, L.rlppo_last_error()


def pad_rows(x, ld):
    """[n, d] -> device rows [n, ld], zero-padded (ld a multiple of 4, >= the padded width of d)."""
    x = np.asarray(x, np.float32)
    out = torch.zeros((x.shape[0], ld), dtype=torch.float32)
    out[:, :x.shape[1]] = torch.as_tensor(x)
    return out.cuda()


class Net:
    def __init__(self, L, params):
        from rlgym_ppo_amd import _native as N
        self.L = L
        self.params = params
        self.dims = [params[0][0].shape[1]] + [w.shape[0] for w, _ in params]
        self.nl = len(params)
        self.dims_c = N.dims_array(self.dims)
        self.flat = dev(nets.flatten(params))
        self.packed = torch.zeros(int(L.rlppo_packed_floats(self.dims_c, self.nl)), device="cuda")
        check(L, L.rlppo_net_pack(stream(), self.dims_c, self.nl, P(self.flat), P(self.packed)))
        self.ld_in = int(L.rlppo_padded_width(self.dims[0]))
        self.ld_out = int(L.rlppo_padded_out(self.dims[-1]))

    def pad(self, obs, f64=False):
        src = dev(obs, torch.float64 if f64 else torch.float32)
        n, d = src.shape
        out = torch.full((n, self.ld_in), float("nan"), device="cuda")
        check(self.L, self.L.rlppo_pad_rows(stream(), P(src), int(f64), n, d, d, P(out), self.ld_in, 0, 0.0, 1.0))
        return out

    def ws(self, n):
        return torch.empty(int(self.L.rlppo_forward_workspace_bytes(self.dims_c, self.nl, n)), dtype=torch.uint8, device="cuda")


def _images(L, a, P_, V_, mode):
    """The weight images of update precision `mode` ("bf16": rounded packed image + bf16 blocks; "x3": the split-bf16 planes)."""
    keep = []
    for net, who in ((P_, "pol"), (V_, "val")):
        if mode == "bf16":
            pr = torch.zeros_like(net.packed)
            wb = torch.zeros(int(L.rlppo_wb16_elems(net.dims_c, net.nl)), dtype=torch.bfloat16, device="cuda")
            check(L, L.rlppo_net_pack_bf16(stream(), net.dims_c, net.nl, P(net.flat), P(pr), P(wb)))
            setattr(a, who + "_packed_r", pr.data_ptr())
            keep.append(pr)
        else:
            wb = torch.zeros(max(int(L.rlppo_x3_elems(net.dims_c, net.nl)), 8), dtype=torch.bfloat16, device="cuda")
            check(L, L.rlppo_net_pack_x3(stream(), net.dims_c, net.nl, P(net.packed), P(wb)))
        setattr(a, who + "_wb16", wb.data_ptr())
        keep.append(wb)
    return keep


def run_pass(L, pol, val, obs_all, acts_all, old_all, tgt_all, adv_all, idx, *, head, entry="plain", clip=0.2, ent=0.005, mb_ratio=1.0,
             pol_act="relu", val_act="relu", bins=None, general=True, log_std=None, var=(0.1, 1.0), mask=None, mask_heads=False,
             cobs=None, critic_ld=None, states_ld=None, precision=None, process_precision=None, ring=None, n_rows=None, grads=None,
             adv_norm=None, value_clip=0.0, kl_slots=False, stop=None, scale=None, ws_fn=None, join=False, dz=False, raise_rc=True):
    """One PPO minibatch pass over rows `idx` of a buffer (obs_all [N, d], acts_all, old_all, tgt_all, adv_all).

    entry: "plain" rlppo_ppo_minibatch | "nvec" rlppo_ppo_minibatch_nvec with `bins` (general=False: NULL nvec, the fixed kernel) |
      "diag" rlppo_ppo_minibatch_diag | "ex" rlppo_ppo_minibatch_ex with the extension filled in ("ex_zero": all-zero, "ex_null": NULL) |
      "critic" rlppo_ppo_minibatch_critic with the critic's matrix `cobs` at leading dimension critic_ld (cobs None: critic == NULL;
      "critic_null": NULL whatever cobs; "critic_null_states": a struct whose `states` is NULL) | "vnorm" rlppo_ppo_minibatch_vnorm
      with the four floats `scale` (None: vnorm == NULL).
    head: "discrete" | "nvec" / "multidiscrete" | "gaussian" | "diag" (log_std given; the policy's gradient arena is [layers | log_std]).
    precision: None (RLPPO_PRECISION_DEFAULT, the workspace sized by rlppo_minibatch_workspace_bytes) or "fp32" / "bf16" / "x3" of
      THIS call; process_precision "bf16" / "x3": the process default is set around the call (rlppo_set_update_precision) and restored.
    mask: bool [N, n_actions], host array or device tensor (mask_heads: with AM.pack's per-head check); ring = base: the buffer is
      handed over as a ring of capacity N, stored rotated so that logical row i lives at physical row (i + base) % N, idx stays logical; n_rows = 0: the buffer's row
      count is withheld; states_ld: the leading dimension of the policy's rows (default: the padded width, through rlppo_pad_rows);
      grads = (gp, gv): accumulate into these arenas; adv_norm: (mean, scale); kl_slots: armed, NaN-filled; stop: a stop word of that
      value; ws_fn: the workspace size function; join: rlppo_ppo_join afterwards; dz: return the policy's output buffer [mb][padded
      outputs] after the pass (the loss kernel's in-place gradient); raise_rc=False: a non-zero return code comes back as rc / msg.

    Every call: the workspace is prefilled with 0xFFFFFFFF words (a NaN in every float: the pass must need no zeroing) and has a guard
    band of other words behind it that must come back untouched; the diag head's scratch is prefilled 0xFF with canary bytes behind it.
    -> dict(gp, gv: the device arenas; stats; grad_policy, grad_log_std, grad_value: numpy; rc, msg, kl: slots or None, dz, ws,
    layers: (policy, critic) per-layer torch gradients on the host)."""
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.util import action_mask as AM
    if ring is not None:
        rot = lambda x: None if x is None else torch.roll(x, ring, 0) if isinstance(x, torch.Tensor) else np.roll(np.asarray(x), ring, axis=0)
        obs_all, cobs, acts_all, old_all, tgt_all, adv_all, mask = (rot(x) for x in (obs_all, cobs, acts_all, old_all, tgt_all, adv_all, mask))
    P_, V_ = Net(L, pol), Net(L, val)
    k = P_.dims[-1] if head == "diag" else 0
    states = P_.pad(obs_all) if states_ld is None else pad_rows(obs_all, states_ld)
    acts = dev(np.asarray(acts_all, np.float32).reshape(len(obs_all), -1))
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim = HEAD_CODE[head], P_.nl, V_.nl, acts.shape[1]
    a.pol_dims = ctypes.cast(P_.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(V_.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.precision = {None: N.PRECISION_DEFAULT, "fp32": N.PRECISION_FP32, "bf16": N.PRECISION_BF16, "x3": N.PRECISION_X3}[precision]
    n_net = P_.flat.numel()
    gp, gv = grads if grads is not None else (torch.zeros(n_net + k, device="cuda"), torch.zeros_like(V_.flat))
    old, tgt, adv = dev(old_all), dev(tgt_all), dev(adv_all)
    idxd = dev(idx, torch.int64)
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    mb = len(idx)
    a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = P_.packed.data_ptr(), V_.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
    a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], states.shape[0] if n_rows is None else n_rows, acts.data_ptr()
    a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idxd.data_ptr(), mb
    if ring is not None:
        a.ring_base, a.ring_cap = ring, len(obs_all)
    a.clip_range, a.ent_coef, a.mb_ratio, a.value_clip = clip, ent, mb_ratio, float(value_clip)
    a.var_m, a.var_b = nets.var_map(*var)
    keep = []
    if mask is not None:
        m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask, bool))
        words = AM.pack(m, sum(bins) if bins is not None else P_.dims[-1], "cuda", heads=bins if mask_heads else None)
        a.action_mask, a.mask_words = words.data_ptr(), words.shape[1]
        keep.append(words)
    if adv_norm is not None:
        keep.append(dev(np.asarray(adv_norm, np.float32)))
        a.adv_norm = keep[-1].data_ptr()
    slots = None
    if kl_slots:
        slots = torch.full((int(L.rlppo_kl_slots_doubles(mb)),), float("nan"), dtype=torch.float64, device="cuda")
        a.kl_slots = slots.data_ptr()
    if stop is not None:
        keep.append(torch.full((1,), int(stop), dtype=torch.int32, device="cuda"))
        a.stop_word = keep[-1].data_ptr()
    nvec = N.dims_array(bins) if bins is not None and general else None
    lsd = scratch = None
    if head == "diag":
        lsd = dev(log_std)
        sb = int(L.rlppo_diag_scratch_bytes(mb, k))
        assert sb == ((mb + 255) // 256) * k * 8   # one row of k doubles per workgroup of 256 rows
        scratch = torch.full((sb + SCRATCH_CANARY,), 0xFF, dtype=torch.uint8, device="cuda")
        scratch[sb:] = canary = (torch.arange(SCRATCH_CANARY, device="cuda") * 37 % 251).to(torch.uint8)
    ext = N.MinibatchExt()
    if entry not in ("ex_zero", "ex_null"):
        ext.pol_hidden_act, ext.val_hidden_act = ACT_CODE[pol_act], ACT_CODE[val_act]
        if head == "nvec":
            ext.md_nvec, ext.md_heads = ctypes.cast(nvec, ctypes.POINTER(ctypes.c_int32)), len(bins)
        if head == "diag":
            ext.log_std, ext.log_std_grad, ext.scratch, ext.scratch_bytes = lsd.data_ptr(), gp.data_ptr() + 4 * n_net, scratch.data_ptr(), sb
    with_rows = cobs is not None and entry in ("critic", "vnorm")
    cr = N.CriticRows()
    if with_rows:
        keep.append(pad_rows(cobs, critic_ld or V_.ld_in))
        cr.states, cr.ld_states = keep[-1].data_ptr(), keep[-1].shape[1]
    crp = ctypes.byref(cr) if with_rows or entry == "critic_null_states" else None
    vn = N.ValueNormArg()
    if scale is not None:
        keep.append(dev(scale))
        vn.scale = keep[-1].data_ptr()
    restore = process_precision is not None
    if restore:
        check(L, L.rlppo_set_update_precision({"bf16": 1, "x3": 2}[process_precision]))
    try:
        if (process_precision or precision) in ("bf16", "x3"):
            keep += _images(L, a, P_, V_, process_precision or precision)
        if ws_fn is not None or precision is not None or with_rows:
            ws_fn = ws_fn or (L.rlppo_minibatch_workspace_bytes_critic if with_rows else L.rlppo_minibatch_workspace_bytes_for)
            ws_bytes = int(ws_fn(P_.dims_c, P_.nl, V_.dims_c, V_.nl, mb, a.precision))
        else:
            ws_bytes = int(L.rlppo_minibatch_workspace_bytes(P_.dims_c, P_.nl, V_.dims_c, V_.nl, mb))
        ws_words = (ws_bytes + 3) // 4
        ws = torch.full((ws_words + GUARD_WORDS,), -1, dtype=torch.int32, device="cuda")   # 0xFFFFFFFF: a NaN in every float
        ws[ws_words:] = guard = torch.arange(GUARD_WORDS, dtype=torch.int32, device="cuda") * 40503 + 0x1234567   # (not the prefill's words)
        a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
        if entry == "plain":
            rc = L.rlppo_ppo_minibatch(stream(), ctypes.byref(a))
        elif entry == "nvec":
            rc = L.rlppo_ppo_minibatch_nvec(stream(), ctypes.byref(a), nvec, len(bins))
        elif entry == "diag":
            rc = L.rlppo_ppo_minibatch_diag(stream(), ctypes.byref(a), P(lsd), ctypes.c_void_p(gp.data_ptr() + 4 * n_net), P(scratch), sb)
        elif entry in ("ex", "ex_zero", "ex_null"):
            rc = L.rlppo_ppo_minibatch_ex(stream(), ctypes.byref(a), None if entry == "ex_null" else ctypes.byref(ext))
        elif entry in ("critic", "critic_null", "critic_null_states"):
            rc = L.rlppo_ppo_minibatch_critic(stream(), ctypes.byref(a), ctypes.byref(ext), crp)
        else:
            assert entry == "vnorm", entry
            rc = L.rlppo_ppo_minibatch_vnorm(stream(), ctypes.byref(a), ctypes.byref(ext), crp, None if scale is None else ctypes.byref(vn))
        msg = L.rlppo_last_error().decode() if rc else ""
        if raise_rc:
            assert rc == 0, msg
        if join:
            check(L, L.rlppo_ppo_join(stream()))
        torch.cuda.synchronize()
    finally:
        if restore:
            check(L, L.rlppo_set_update_precision(0))
    assert torch.equal(ws[ws_words:], guard), "the pass wrote behind its workspace"
    if scratch is not None:
        assert torch.equal(scratch[sb:], canary), "the pass wrote behind its scratch region"
    out_buf = None
    if dz:
        before = sum(int(L.rlppo_padded_out(d)) for d in P_.dims[1:-1])   # the hidden layers' outputs lie in front of the head's
        out_buf = ws.view(torch.float32)[mb * before: mb * (before + P_.ld_out)].view(mb, P_.ld_out).cpu().numpy()
    gpc, gvc = gp.cpu(), gv.cpu()
    layers = nets.unflatten(gpc[:n_net], pol), nets.unflatten(gvc, val)   # per layer (dW, db), torch on the host
    return dict(gp=gp, gv=gv, stats=stats.cpu().numpy(), rc=rc, msg=msg, kl=None if slots is None else slots.cpu().numpy(), dz=out_buf, ws=ws,
                layers=layers, grad_policy=[(w.numpy(), b.numpy()) for w, b in layers[0]], grad_log_std=gpc[n_net:].numpy(),
                grad_value=[(w.numpy(), b.numpy()) for w, b in layers[1]])


def triple(r):
    """(grad_policy, grad_value, stats) of a run_pass result, the gradients as torch tensors per layer (without a diag head's log_std
    tail): what tests/fp64_gate.py::gate and ppo_yardstick.masked_gate take; with dz behind them where the pass was asked for it."""
    out = (*r["layers"], r["stats"])
    return out if r["dz"] is None else out + (r["dz"],)


def run_minibatch(L, head, pol, val, obs_all, acts_all, old_all, tgt_all, adv_all, idx, clip, ent, mb_ratio, var=(0.1, 1.0),
                  precision="fp32", ring=None):
    """rlppo_ppo_minibatch in the process's update precision (bf16 / x3: set around the call) -> (grad_policy, grad_value, stats)."""
    r = run_pass(L, pol, val, obs_all, acts_all, old_all, tgt_all, adv_all, idx, head=head, clip=clip, ent=ent, mb_ratio=mb_ratio, var=var,
                 process_precision=None if precision == "fp32" else precision, ring=ring)
    return triple(r)
