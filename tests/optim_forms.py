"""The case matrix of the parameter-side kernels (csrc/pack.hip, rows.hip, optim.hip, stats.hip), through the C ABI alone: for every
entry point the smallest shapes at which a shared step (the workgroup sum, the ticketed pair sum, the Adam element, the KL gate's one
kernel, the per-row scalar gather, the pad-rows dispatch) can go wrong.  A case is a name and a function that runs its launches on
the library `_native` has loaded and returns its output buffers; `digest` is one sha256 over all of them.

tools/optim_equivalence.py runs the matrix on two libraries and compares; tests/test_gpu_optim_forms.py runs it on this tree and
compares with tests/golden/optim_forms_sha256.json, recorded from the library of the commit before the split of optim.hip.

THREE_OPERATION cases: the pair form without a sync block adds its workgroups' sums with an atomic; with one workgroup per network
the sum has one addend and the form is bit-reproducible, which is the only size at which it is digested."""
import ctypes
import hashlib

import numpy as np
import torch

from hip_pass import P, check, dev, run_pass, stream

NETS = {"a": [5, 7, 3], "b": [5, 4, 1], "big": [300, 700, 3]}   # 66, 29 and 212,803 parameters (> 128 x 1536: the stride loop runs)
HYPER = ((0.5, 3e-4, 0.9, 0.999, 1e-8), (1e-3, 1e-3, 0.8, 0.99, 1e-8))   # (max_norm, lr, beta1, beta2, eps) of network a / b


def _bytes(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        return x.view(torch.uint8).numpy().tobytes()
    return np.ascontiguousarray(x).tobytes()


def digest(outputs):
    """{name: tensor / array} -> sha256 over the names and the bytes, in name order."""
    h = hashlib.sha256()
    for name in sorted(outputs):
        h.update(name.encode() + b"\0" + _bytes(outputs[name]) + b"\1")
    return h.hexdigest()


def _N():
    from rlgym_ppo_amd import _native as N
    return N


def _nan(n, dtype=torch.float32):
    return torch.full((int(n),), float("nan"), dtype=dtype, device="cuda")


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pack.hip
def pack(L, dims, bf16):
    N = _N()
    dc, nl = N.dims_array(dims), len(dims) - 1
    flat = dev((np.random.RandomState(len(dims)).randn(int(L.rlppo_flat_floats(dc, nl))) * 0.1).astype(np.float32))
    packed = _nan(L.rlppo_packed_floats(dc, nl))
    if not bf16:
        check(L, L.rlppo_net_pack(stream(), dc, nl, P(flat), P(packed)))
        _sync()
        return dict(packed=packed)
    wb = torch.full((int(L.rlppo_wb16_elems(dc, nl)),), -1, dtype=torch.int16, device="cuda")
    check(L, L.rlppo_net_pack_bf16(stream(), dc, nl, P(flat), P(packed), P(wb)))
    _sync()
    return dict(packed_r=packed, wb16=wb)


# ------------------------------------------------------------------------------------------------ rows.hip
def pad(L, f64, form):
    """n = 3, d = 5 into rows of 8: form "copy" / "scalar" (rlppo_pad_rows, standardise off / on) / "feature" (per-feature)."""
    rs = np.random.RandomState(3)
    obs = (rs.randn(3, 5) * 4 + 1).astype(np.float32)
    obs[1, 2], obs[2, 4] = 40.0, -40.0   # both clamps
    src = dev(obs, torch.float64 if f64 else torch.float32)
    out = _nan(3 * 8)
    if form == "feature":
        mean, std = dev(rs.randn(5).astype(np.float32)), dev((rs.rand(5) * 3 + 0.1).astype(np.float32))
        check(L, L.rlppo_pad_rows_per_feature(stream(), P(src), int(f64), 3, 5, 5, P(out), 8, P(mean), P(std)))
    else:
        check(L, L.rlppo_pad_rows(stream(), P(src), int(f64), 3, 5, 5, P(out), 8, int(form == "scalar"), 0.73, 2.9))
    _sync()
    return dict(rows=out)


def _gather_src(rs, rows, ld):
    return dev(rs.randn(rows, ld).astype(np.float32))


def gather_rows(L):
    rs = np.random.RandomState(4)
    src, idx, dst = _gather_src(rs, 9, 12), dev([7, 0, 8, 3, 3], torch.int64), _nan(5 * 8)
    check(L, L.rlppo_gather_rows(stream(), P(src), 12, P(idx), P(dst), 8, 5))
    _sync()
    return dict(dst=dst)


def gather_rows2(L, ring, meta):
    N = _N()
    rs = np.random.RandomState(5)
    k = 2
    keep = [_gather_src(rs, 9, 12), _gather_src(rs, 9, 4), dev(rs.randn(9, k).astype(np.float32))] + [dev(rs.randn(9).astype(np.float32)) for _ in range(3)]
    idx = dev([7, 0, 8, 3, 3], torch.int64)
    out = dict(p=_nan(5 * 8), c=_nan(5 * 4), act=_nan(5 * k), old=_nan(5), adv=_nan(5), tgt=_nan(5), zero=_nan(5))
    g = N.Gather2Args()
    g.src, g.ld_src, g.dst, g.width = keep[0].data_ptr(), 12, out["p"].data_ptr(), 8
    g.critic_src, g.critic_ld_src, g.critic_dst, g.critic_width = keep[1].data_ptr(), 4, out["c"].data_ptr(), 4
    g.idx, g.n = idx.data_ptr(), 5
    if ring:
        g.ring_base, g.ring_cap = 4, 9
    if meta:
        g.actions, g.old_logp, g.advantages, g.targets, g.act_dim = keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), k
        g.g_act, g.g_old, g.g_adv, g.g_tgt, g.zero_n = (out[x].data_ptr() for x in ("act", "old", "adv", "tgt", "zero"))
    check(L, L.rlppo_gather_rows2(stream(), ctypes.byref(g)))
    _sync()
    return out


def pass_gather(L, form):
    """One rlppo_ppo_minibatch over 64 of 100 rows: the per-row scalars ride in the pass's gather launch ("rows": gather_rows_kernel;
    "ring": the same through a ring; "critic": gather_rows2_kernel; "table": gather_meta_kernel, with the first layers fetching their
    rows through its row table where their shapes allow it -- the counter of such passes is part of the output)."""
    from oracle import nets
    torch.manual_seed(9)
    rs = np.random.RandomState(9)
    d, hid, k = (107, (256, 256), 90) if form == "table" else (20, (32,), 7)
    pol, val = nets.init_mlp(d, hid, k), nets.init_mlp(12 if form == "critic" else d, hid, 1)
    obs, cobs = rs.randn(100, d).astype(np.float32), rs.randn(100, 12).astype(np.float32)
    acts, old = rs.randint(0, k, 100).astype(np.float32), (-1.5 + 0.3 * rs.randn(100)).astype(np.float32)
    adv, tgt = rs.randn(100).astype(np.float32), rs.randn(100).astype(np.float32)
    idx = rs.permutation(100)[:64]
    extra = {}
    if form == "table":
        check(L, L.rlppo_dbg_set(26, 2))
        before = L.rlppo_dbg_counter(4)
    try:
        r = run_pass(L, pol, val, obs, acts, old, tgt, adv, idx, head="discrete", ring=37 if form == "ring" else None,
                     **(dict(entry="critic", cobs=cobs) if form == "critic" else {}))
    finally:
        if form == "table":
            check(L, L.rlppo_dbg_set(26, 1))
            extra["row_table_passes"] = np.int64(L.rlppo_dbg_counter(4) - before)
    return dict(gp=r["gp"], gv=r["gv"], stats=r["stats"], **extra)


def welford(L, n, d, f64):
    rs = np.random.RandomState(n + d)
    ld = (d + 3) // 4 * 4
    dt, tt = (np.float64, torch.float64) if f64 else (np.float32, torch.float32)
    mean, m2 = dev(rs.randn(d).astype(dt), tt), dev((rs.rand(d) * 30).astype(dt), tt)
    x = dev((rs.randn(n, ld) * 2 + 0.5).astype(np.float32))
    check(L, L.rlppo_welford_increment(stream(), P(x), ld, n, d, P(mean), P(m2), 37, int(f64)))
    _sync()
    return dict(mean=mean, m2=m2)


def welford_merge(L, d, f64):
    rs = np.random.RandomState(d)
    dt, tt = (np.float64, torch.float64) if f64 else (np.float32, torch.float32)
    mean, m2 = dev(rs.randn(d).astype(dt), tt), dev((rs.rand(d) * 30).astype(dt), tt)
    om, om2 = dev(rs.randn(d).astype(np.float32)), dev((rs.rand(d) * 20).astype(np.float32))
    check(L, L.rlppo_welford_merge(stream(), d, P(mean), P(m2), 37, P(om), P(om2), 21, int(f64)))
    _sync()
    return dict(mean=mean, m2=m2)


# ------------------------------------------------------------------------------------------------ optim.hip
def clip_adam(L, n):
    rs = np.random.RandomState(n)
    p, m, v = dev((rs.randn(n) * 0.2).astype(np.float32)), dev((rs.randn(n) * 1e-2).astype(np.float32)), dev((rs.rand(n) * 1e-4).astype(np.float32))
    gn = _nan(1, torch.float64)
    out = {}
    for step, scale in ((3, 1.0), (4, 1e-3)):   # clipped, then not
        g = dev((rs.randn(n) * scale).astype(np.float32))
        check(L, L.rlppo_clip_adam(stream(), P(p), P(g), P(m), P(v), n, 0.5, 3e-4, 0.9, 0.999, 1e-8, step, P(gn)))
        _sync()
        out.update({f"{x}{step}": t.clone() for x, t in (("p", p), ("g", g), ("m", m), ("v", v), ("gn", gn))})
    return out


class _Net:
    def __init__(self, L, dims, tail, seed):
        N = _N()
        self.dc, self.nl, self.rs = N.dims_array(dims), len(dims) - 1, np.random.RandomState(seed)
        self.n = int(L.rlppo_flat_floats(self.dc, self.nl)) + tail
        self.p = dev((self.rs.randn(self.n) * 0.1).astype(np.float32))
        self.m, self.v, self.g = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.packed = _nan(L.rlppo_packed_floats(self.dc, self.nl))
        check(L, L.rlppo_net_pack(stream(), self.dc, self.nl, P(self.p), P(self.packed)))
        self.gn = _nan(1, torch.float64)
        self.skip = torch.zeros(1, dtype=torch.int32, device="cuda")

    def desc(self, hyper, step, lr):
        d = _N().OptNet()
        d.dims, d.n_layers = ctypes.cast(self.dc, ctypes.POINTER(ctypes.c_int32)), self.nl
        d.params, d.grads, d.exp_avg, d.exp_avg_sq = self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr()
        d.packed, d.gnorm2, d.skip_word = self.packed.data_ptr(), self.gn.data_ptr(), self.skip.data_ptr()
        d.max_norm, _, d.beta1, d.beta2, d.eps = hyper
        d.lr, d.step = lr, step
        return d


def pair(L, nets, entry, one_launch, tails=(0, 0), skip=None):
    """Two optimiser steps (a clipped and an unclipped gradient) of a pair of networks through `entry` ("pack2" / "tail" / "lr": the
    rates in device memory, the descriptors carrying a rate nobody may use); skip: the network whose skip word is set."""
    N = _N()
    net = [_Net(L, NETS[name], tail, 11 + k) for k, (name, tail) in enumerate(zip(nets, tails))]
    sync = torch.zeros(N.OPT_SYNC_BYTES // 4, dtype=torch.int32, device="cuda") if one_launch else None   # zeroed ONCE
    rates = torch.tensor([HYPER[0][1], HYPER[1][1]], dtype=torch.float64, device="cuda")
    if skip is not None:
        net[skip].skip.fill_(7)
    out = {}
    for step, scale in ((1, 1.0), (2, 1e-4)):
        for x in net:
            x.g.copy_(dev((x.rs.randn(x.n) * scale).astype(np.float32)))
        a, b = (x.desc(h, step, 123.0 if entry == "lr" else h[1]) for x, h in zip(net, HYPER))
        if entry == "pack2":
            rc = L.rlppo_clip_adam_pack2(stream(), ctypes.byref(a), ctypes.byref(b), P(sync))
        elif entry == "tail":
            rc = L.rlppo_clip_adam_pack2_tail(stream(), ctypes.byref(a), ctypes.byref(b), P(sync), tails[0], tails[1])
        else:
            rc = L.rlppo_clip_adam_pack2_lr(stream(), ctypes.byref(a), ctypes.byref(b), P(sync), tails[0], tails[1],
                                            ctypes.c_void_p(rates.data_ptr()), ctypes.c_void_p(rates.data_ptr() + 8))
        check(L, rc)
        _sync()
        for k, x in enumerate(net):
            out.update({f"{name}{k}_{step}": t.clone() for name, t in (("p", x.p), ("g", x.g), ("m", x.m), ("v", x.v), ("packed", x.packed))})
            if skip != k:   # (a skipped network's norm is not formed)
                out[f"gn{k}_{step}"] = x.gn.clone()
    if one_launch:
        out["sync_header"] = sync[:4].clone()   # arrival counter, generation, give-ups, the sequence number that counted one
        assert sync[0].item() == 0 and sync[1].item() == 2 and sync[2].item() == 0
    out["rates"] = rates
    return out


PAIR_FORMS = [("pack2", (0, 0), None), ("tail", (3, 3), None), ("tail", (3, 0), 0), ("tail", (0, 3), 1), ("lr", (3, 0), None), ("lr", (0, 0), 1)]


# ------------------------------------------------------------------------------------------------ stats.hip
def adv_stats(L, n, kind):
    N = _N()
    rs = np.random.RandomState(n)
    rows = n + 11
    adv = np.full(rows, 0.37, np.float32) if kind == "constant" else (rs.randn(rows) * 2 + 0.5).astype(np.float32)
    idx = rs.randint(0, rows, n)
    ws = torch.zeros(N.ADV_STATS_WS_BYTES // 4, dtype=torch.int32, device="cuda")
    out = _nan(2)
    d_idx, d_adv = dev(idx, torch.int64), dev(adv)
    base, cap = (5, rows) if kind == "ring" else (0, 0)
    check(L, L.rlppo_adv_stats(stream(), P(d_idx), n, P(d_adv), base, cap, P(out), P(ws)))
    _sync()
    return dict(out=out, ws=ws)


def value_norm(L, sizes, nan_at=None):
    """Consecutive updates of one state with batches of `sizes`; nan_at: the batch that holds a NaN."""
    N = _N()
    rs = np.random.RandomState(sum(sizes))
    state, scale = torch.zeros(4, dtype=torch.float64, device="cuda"), dev([0.0, 1.0, 1.0, 0.0])
    ws = torch.zeros(N.VALUE_NORM_WS_BYTES, dtype=torch.uint8, device="cuda")
    out = {}
    for i, n in enumerate(sizes):
        x = (rs.randn(n) * 3 + 1.5 * i).astype(np.float32)
        if nan_at == i:
            x[n // 2] = np.nan
        xd = dev(x)
        check(L, L.rlppo_value_norm_update(stream(), P(xd), n, P(state), P(scale), P(ws)))
        _sync()
        out.update({f"state{i}": state.clone(), f"scale{i}": scale.clone(), f"ws{i}": ws.clone()})
    return out


KL_STRIDE = 320   # doubles per pass region >= 2 + 257


def _kl_image(counts):
    rs = np.random.RandomState(40 + sum(counts))
    img, kl = np.full(len(counts) * KL_STRIDE, np.nan), 0.0
    for p, c in enumerate(counts):
        slots = 10.0 ** rs.uniform(-8.0, -2.0, c)
        ratio = float(np.float32(1.0 / (2.0 + 1.7 * p)))
        img[p * KL_STRIDE:p * KL_STRIDE + 2 + c] = np.concatenate([[float(c), ratio], slots])
        kl += ratio * float(np.sum(slots))
    return img, kl   # (kl: the host's left-to-right sum, close to the device's KL_b: it only places the thresholds)


def kl_gate(L, counts, lr_entry):
    """Every branch of the gate on one slot image: phases 0 / 1 / 2, KL_b just below and just above the threshold, a stop word that is
    already set; with the rate rule (lr_entry) every branch of it including both clamps, and the call without stop and host words."""
    N = _N()
    img, kl = _kl_image(counts)
    slots = dev(img, torch.float64)
    out = {}
    below, above = kl * (1 - 2.0 ** -30), kl * (1 + 2.0 ** -30)

    def run(tag, phase, threshold, stop=0, desired=None, bounds=(1e-5, 1e-2), exchange=None, bare=False):
        rates = torch.tensor([3e-4, 1e-3, 7e-3], dtype=torch.float64, device="cuda")
        klo = torch.tensor([-7.0], dtype=torch.float64, device="cuda")
        ex = _nan(2) if exchange is None else dev(exchange)
        stopw = torch.tensor([stop], dtype=torch.int32, device="cuda")
        host = torch.full((2,), -1, dtype=torch.int32).pin_memory()
        g, a = N.KlGateArgs(), N.LrAdaptArgs()
        g.kl_slots, g.slot_stride, g.n_passes, g.phase, g.threshold = slots.data_ptr(), KL_STRIDE, len(counts), phase, threshold
        g.exchange, g.batch, g.done_value = ex.data_ptr(), 4, 77
        if not bare:
            g.stop_word, g.host_words = stopw.data_ptr(), host.data_ptr()
        a.lr, a.n_lr, a.desired_kl, a.factor, (a.lr_min, a.lr_max) = rates.data_ptr(), 3, desired or kl, 1.5, bounds
        a.kl_out = klo.data_ptr()
        if lr_entry:
            check(L, L.rlppo_kl_gate_lr(stream(), ctypes.byref(g), ctypes.byref(a)))
        else:
            check(L, L.rlppo_kl_gate(stream(), ctypes.byref(g)))
        _sync()
        out.update({f"{tag}_{k}": t.clone() for k, t in (("rates", rates), ("kl", klo), ("exchange", ex), ("stop", stopw), ("host", host))})
        return ex

    run("p0_no_stop", 0, above)
    run("p0_stop", 0, below)
    run("p0_stop_was_set", 0, below, stop=3)
    ex = run("p1", 1, below)
    words = ex.cpu().numpy()
    total = 2.0 * (float(words[0]) + float(words[1]))
    run("p2_no_stop", 2, total * (1 + 2.0 ** -30), exchange=2 * words)   # (two ranks with the same share)
    run("p2_stop", 2, total * (1 - 2.0 ** -30), exchange=2 * words)
    if lr_entry:
        run("down", 0, 1e30, desired=kl / 4)                              # KL_b > 2 desired: every rate / 1.5
        run("down_clamped", 0, 1e30, desired=kl / 4, bounds=(5e-4, 1e-2))   # ... the first one stops at lr_min
        run("up", 0, 1e30, desired=kl * 4)                                # KL_b < desired / 2: every rate x 1.5
        run("up_clamped", 0, 1e30, desired=kl * 4, bounds=(1e-5, 8e-3))   # ... the last one stops at lr_max
        run("stay", 0, 1e30, desired=kl)
        run("stop_moves_no_rate", 0, below, desired=kl / 4)
        run("bare", 0, below, desired=kl / 4, bare=True)                  # no stop word, no host words: device memory only
    return out


def learn_report(L, n_pol, n_val):
    N = _N()
    g = torch.Generator(device="cuda").manual_seed(n_pol)
    pb, pn = torch.randn(n_pol, device="cuda", generator=g), torch.randn(n_pol, device="cuda", generator=g)
    vb, vn = torch.randn(n_val, device="cuda", generator=g), torch.randn(n_val, device="cuda", generator=g)
    ws = torch.zeros(N.REPORT_WS_BYTES, dtype=torch.uint8, device="cuda")
    out = torch.zeros(N.REPORT_OUT_DOUBLES, dtype=torch.float64).pin_memory()
    done = torch.zeros(1, dtype=torch.int32).pin_memory()
    word, extra = torch.tensor([3], dtype=torch.int32, device="cuda"), torch.tensor([11.0], dtype=torch.float64, device="cuda")
    stats = torch.arange(1, N.N_STATS + 1, dtype=torch.float64, device="cuda") * 0.5
    a = N.ReportArgs()
    a.pol_before, a.pol_now, a.n_pol, a.val_before, a.val_now, a.n_val = pb.data_ptr(), pn.data_ptr(), n_pol, vb.data_ptr(), vn.data_ptr(), n_val
    a.stats, a.add_passes, a.timeout_word, a.extra = stats.data_ptr(), 4.0, word.data_ptr(), extra.data_ptr()
    a.out, a.done_word, a.done_value, a.ws = out.data_ptr(), done.data_ptr(), 1001, ws.data_ptr()
    check(L, L.rlppo_learn_report(stream(), ctypes.byref(a)))
    _sync()
    return dict(inputs=torch.cat([pb[:64], vn[-64:]]), out=out.clone(), done=done.clone(), stats=stats, ws=ws)


# ------------------------------------------------------------------------------------------------ the matrix
def _matrix():
    m = {}
    for name, dims in (("5_7_3", [5, 7, 3]), ("107_64_64_90", [107, 64, 64, 90])):
        m[f"pack-{name}"] = lambda L, d=dims: pack(L, d, False)
        m[f"pack_bf16-{name}"] = lambda L, d=dims: pack(L, d, True)
    for f64 in (False, True):
        for form in ("copy", "scalar", "feature"):
            m[f"pad_rows-{form}-{'f64' if f64 else 'f32'}"] = lambda L, f=f64, s=form: pad(L, f, s)
    m["gather_rows"] = gather_rows
    for ring in (False, True):
        for meta in (False, True):
            m[f"gather_rows2-{'ring' if ring else 'plain'}-{'meta' if meta else 'rows'}"] = lambda L, r=ring, w=meta: gather_rows2(L, r, w)
    for form in ("rows", "ring", "critic", "table"):
        m[f"pass_gather-{form}"] = lambda L, f=form: pass_gather(L, f)
    for f64 in (False, True):
        for d in (5, 130):
            for n in (1, 17):
                m[f"welford-n{n}-d{d}-{'f64' if f64 else 'f32'}"] = lambda L, n=n, d=d, f=f64: welford(L, n, d, f)
            m[f"welford_merge-d{d}-{'f64' if f64 else 'f32'}"] = lambda L, d=d, f=f64: welford_merge(L, d, f)
    for n in (1, 255):
        m[f"clip_adam-n{n}"] = lambda L, n=n: clip_adam(L, n)
    for one in (False, True):
        form = "one_launch" if one else "three_operations"
        for entry, tails, skip in PAIR_FORMS:
            m[f"pair-{form}-{entry}-tails{tails[0]}_{tails[1]}-skip_{'none' if skip is None else 'ab'[skip]}"] = \
                lambda L, o=one, e=entry, t=tails, s=skip: pair(L, ("a", "b"), e, o, t, s)
    for entry, tails in (("pack2", (0, 0)), ("lr", (3, 0))):
        m[f"pair-one_launch-{entry}-tails{tails[0]}_{tails[1]}-big"] = lambda L, e=entry, t=tails: pair(L, ("big", "b"), e, True, t)
    for n in (1, 2, 513, 70001):
        m[f"adv_stats-n{n}"] = lambda L, n=n: adv_stats(L, n, "random")
    for kind in ("constant", "ring"):
        m[f"adv_stats-n513-{kind}"] = lambda L, k=kind: adv_stats(L, 513, k)
    for n in (1, 513, 70001):
        m[f"value_norm-n{n}"] = lambda L, n=n: value_norm(L, (n,))
    m["value_norm-three_updates"] = lambda L: value_norm(L, (513, 2, 700))
    m["value_norm-nan_batch"] = lambda L: value_norm(L, (513, 513, 64), nan_at=1)
    for counts in ((1,), (257,), (1, 1, 1), (257, 1, 257)):
        for lr_entry in (False, True):
            m[f"{'kl_gate_lr' if lr_entry else 'kl_gate'}-slots_{'_'.join(map(str, counts))}"] = lambda L, c=counts, e=lr_entry: kl_gate(L, c, e)
    for n_pol, n_val in ((1, 16385), (200003, 70001)):
        m[f"learn_report-{n_pol}_{n_val}"] = lambda L, a=n_pol, b=n_val: learn_report(L, a, b)
    return m


MATRIX = _matrix()
THREE_OPERATION = sorted(k for k in MATRIX if k.startswith("pair-three_operations"))


def case_ids():
    return sorted(MATRIX)


def run_case(L, case):
    return digest(MATRIX[case](L))
