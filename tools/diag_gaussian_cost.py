"""What the diagonal-Gaussian head (RLPPO_HEAD_DIAG_GAUSSIAN, learnable log_std) costs beside the reference's Gaussian head
(RLPPO_HEAD_GAUSSIAN), on the SAME build, alternating, at the BASELINE configs[4] shape (obs 231, 512 x 4, k = 8):
  * one 65,536-row and one 524,288-row pass of the update (rlppo_ppo_minibatch against rlppo_ppo_minibatch_diag, fp32, device events);
  * the 4096-row rollout call on padded device rows (rlppo_gaussian_act against rlppo_diag_gaussian_act);
  * the graph-replayed small call of the policy classes at 8 and 80 host observations (host clock around get_action);
  * the fused optimiser step of both networks without a parameter tail (rlppo_clip_adam_pack2) and with log_std's tail of 8
    (rlppo_clip_adam_pack2_tail), one launch with the grid barrier and three operations;
  * the log_std reduction by itself at 524,288 and 65,536 rows (rlppo_dbg_diag_loss): the loss launch alone (which forms the
    per-workgroup partial sums), the fixed-order finish alone, both -- beside the spread of the 524,288-row pass.
No target is fixed in advance: medians and spread ((max - min) / median) over the rounds are recorded, stamped with rlppo_build_id().
usage: python tools/diag_gaussian_cost.py [--rounds R] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402

OBS, HIDDEN, K = 231, (512, 512, 512, 512), 8
P = lambda t: ctypes.c_void_p(t.data_ptr())


def summary(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3),
            "spread": round(float((max(v) - min(v)) / np.median(v)), 4), "rounds": [round(float(x), 3) for x in v]}


def alternate(legs, rounds, reps):
    """legs: name -> fn().  Every round times every leg (device events, `reps` calls), in turn; round 0 warms up."""
    for fn in legs.values():
        fn()
    bench.time_region(next(iter(legs.values())), 3, warm_s=0.3)   # clock ramp
    res = {k: [] for k in legs}
    for r in range(rounds + 1):
        for k, fn in legs.items():
            ms = bench.time_region(fn, reps, warm=1)
            if r:
                res[k].append(ms * 1e3)
    return {k: summary(v) for k, v in res.items()}


def compare(out, a, b):
    diff = out[a]["median"] / out[b]["median"] - 1.0
    out[f"{a}_vs_{b}"] = round(diff, 4)
    out[f"{a}_vs_{b}_within_spread"] = bool(abs(diff) <= max(out[a]["spread"], out[b]["spread"]))


class Net:
    def __init__(self, dims):
        L = N.lib()
        self.dims, self.nl, self.dims_c = dims, len(dims) - 1, N.dims_array(dims)
        self.n = int(L.rlppo_flat_floats(self.dims_c, self.nl))
        self.flat = torch.randn(self.n, device="cuda") * 0.05
        self.packed = torch.zeros(int(L.rlppo_packed_floats(self.dims_c, self.nl)), device="cuda")
        N.check(L.rlppo_net_pack(bench_stream(), self.dims_c, self.nl, P(self.flat), P(self.packed)))
        self.ld_in = int(L.rlppo_padded_width(dims[0]))


def bench_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def pass_legs(mb, n_buf):
    """One fp32 pass of mb rows out of an n_buf-row buffer for both heads -> {name: fn}."""
    L = N.lib()
    rs = np.random.RandomState(0)
    val = Net([OBS, *HIDDEN, 1])
    states = torch.zeros(n_buf, val.ld_in, device="cuda")
    states[:, :OBS] = torch.randn(n_buf, OBS, device="cuda").clamp_(-5, 5)
    acts = (torch.randn(n_buf, K, device="cuda") * 0.5).contiguous()
    old = torch.randn(n_buf, device="cuda") * 0.3 - 6.0
    tgt, adv = torch.randn(n_buf, device="cuda"), torch.randn(n_buf, device="cuda")
    idx = torch.as_tensor(rs.permutation(n_buf)[:mb]).cuda()
    stats = torch.zeros(N.N_STATS, dtype=torch.float64, device="cuda")
    legs, keep = {}, [val, states, acts, old, tgt, adv, idx, stats]
    for name, head, n_out in (("gaussian", N.HEAD_GAUSSIAN, 2 * K), ("diag", N.HEAD_DIAG_GAUSSIAN, K)):
        pol = Net([OBS, *HIDDEN, n_out])
        a = N.MinibatchArgs()
        a.head, a.pol_layers, a.val_layers, a.act_dim, a.precision = head, pol.nl, val.nl, K, N.PRECISION_FP32
        a.pol_dims = ctypes.cast(pol.dims_c, ctypes.POINTER(ctypes.c_int32))
        a.val_dims = ctypes.cast(val.dims_c, ctypes.POINTER(ctypes.c_int32))
        gp, gv = torch.zeros(pol.n + K, device="cuda"), torch.zeros(val.n, device="cuda")
        ws_bytes = int(L.rlppo_minibatch_workspace_bytes_for(pol.dims_c, pol.nl, val.dims_c, val.nl, mb, a.precision))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = pol.packed.data_ptr(), val.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
        a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], n_buf, acts.data_ptr()
        a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idx.data_ptr(), mb
        a.clip_range, a.ent_coef, a.mb_ratio, a.var_m, a.var_b = 0.2, 0.005, 1.0, 0.45, 0.55
        a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
        keep += [pol, gp, gv, ws, a]
        st = bench_stream()
        if head == N.HEAD_GAUSSIAN:
            legs[name] = lambda a=a, st=st: N.check(L.rlppo_ppo_minibatch(st, ctypes.byref(a)))
        else:
            ls = torch.zeros(K, device="cuda")
            sb = int(L.rlppo_diag_scratch_bytes(mb, K))
            scratch = torch.empty(sb, dtype=torch.uint8, device="cuda")
            keep += [ls, scratch]
            legs[name] = lambda a=a, st=st, ls=ls, gp=gp, pol=pol, scratch=scratch, sb=sb: N.check(
                L.rlppo_ppo_minibatch_diag(st, ctypes.byref(a), P(ls), ctypes.c_void_p(gp.data_ptr() + 4 * pol.n), P(scratch), sb))
    return legs, keep


def rollout_legs(n):
    L = N.lib()
    legs, keep = {}, []
    eps = torch.randn(n, K, device="cuda")
    st = bench_stream()
    for name, n_out in (("gaussian", 2 * K), ("diag", K)):
        pol = Net([OBS, *HIDDEN, n_out])
        rows = torch.zeros(n, pol.ld_in, device="cuda")
        rows[:, :OBS] = torch.randn(n, OBS, device="cuda").clamp_(-5, 5)
        act, logp = torch.empty(n, K, device="cuda"), torch.empty(n, device="cuda")
        ws = torch.empty(int(L.rlppo_forward_workspace_bytes(pol.dims_c, pol.nl, n)), dtype=torch.uint8, device="cuda")
        ls = torch.zeros(K, device="cuda")
        keep += [pol, rows, act, logp, ws, ls]
        if name == "gaussian":
            legs[name] = lambda pol=pol, rows=rows, act=act, logp=logp, ws=ws: N.check(L.rlppo_gaussian_act(
                st, pol.dims_c, pol.nl, P(pol.packed), P(rows), pol.ld_in, n, P(eps), 0.45, 0.55, P(act), P(logp), P(ws), ws.numel(), None))
        else:
            legs[name] = lambda pol=pol, rows=rows, act=act, logp=logp, ws=ws, ls=ls: N.check(L.rlppo_diag_gaussian_act(
                st, pol.dims_c, pol.nl, P(pol.packed), P(rows), pol.ld_in, n, P(eps), P(ls), P(act), P(logp), P(ws), ws.numel(), None))
    return legs, keep + [eps]


def small_call(rounds, calls=300):
    """us per get_action on 8 / 80 host observations (host clock; the call ends when the results are on the host)."""
    from rlgym_ppo_amd.ppo import ContinuousPolicy, DiagGaussianPolicy
    torch.manual_seed(0)
    pols = {"gaussian": ContinuousPolicy(OBS, 2 * K, HIDDEN, "cuda:0"), "diag": DiagGaussianPolicy(OBS, K, HIDDEN, "cuda:0")}
    out = {"unit": "us per get_action call (host clock, %d calls per measurement, one graph replay per call)" % calls}
    for n in (8, 80):
        obs = np.clip(np.random.RandomState(n).randn(n, OBS), -5, 5).astype(np.float32)
        res = {k: [] for k in pols}
        for r in range(rounds + 1):
            for k, pol in pols.items():
                for _ in range(20):
                    pol.get_action(obs)
                t0 = time.perf_counter()
                for _ in range(calls):
                    pol.get_action(obs)
                if r:
                    res[k].append((time.perf_counter() - t0) / calls * 1e6)
        o = {k: summary(v) for k, v in res.items()}
        compare(o, "diag", "gaussian")
        o["graph_replays"] = {k: int(sum(g.calls for g in pol._graphs.values())) for k, pol in pols.items()}
        out[f"{n}_observations"] = o
    return out


def optimiser_legs(one_launch):
    L = N.lib()
    st = bench_stream()
    legs, keep = {}, []
    for name, tail in (("no_tail", 0), ("tail_8", K)):
        descs = []
        for dims, t in (([OBS, *HIDDEN, 1], 0), ([OBS, *HIDDEN, K], tail)):
            net = Net(dims)
            n = net.n + t
            p, g, m, v = (torch.randn(n, device="cuda") * 0.01 for _ in range(4))
            v.abs_()
            gn = torch.zeros(1, dtype=torch.float64, device="cuda")
            d = N.OptNet()
            d.dims, d.n_layers = ctypes.cast(net.dims_c, ctypes.POINTER(ctypes.c_int32)), net.nl
            d.params, d.grads, d.exp_avg, d.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            d.packed, d.gnorm2 = net.packed.data_ptr(), gn.data_ptr()
            d.max_norm, d.lr, d.beta1, d.beta2, d.eps, d.step = 0.5, 3e-4, 0.9, 0.999, 1e-8, 7
            descs.append(d)
            keep += [net, p, g, m, v, gn]
        sync = torch.zeros(N.OPT_SYNC_BYTES // 4, dtype=torch.int32, device="cuda") if one_launch else None
        keep += [descs, sync]
        sp = None if sync is None else P(sync)
        if tail:
            legs[name] = lambda d=descs, sp=sp: N.check(L.rlppo_clip_adam_pack2_tail(st, ctypes.byref(d[0]), ctypes.byref(d[1]), sp, 0, K))
        else:
            legs[name] = lambda d=descs, sp=sp: N.check(L.rlppo_clip_adam_pack2(st, ctypes.byref(d[0]), ctypes.byref(d[1]), sp))
    return legs, keep


def reduction_legs(mb):
    """The head's loss step alone on [mb][32] head outputs: loss launch, finish, both."""
    L = N.lib()
    st = bench_stream()
    y0 = torch.randn(mb, 32, device="cuda")
    y = y0.clone()
    acts, old, adv = torch.randn(mb, K, device="cuda"), torch.randn(mb, device="cuda") - 8.0, torch.randn(mb, device="cuda")
    ls, grad = torch.zeros(K, device="cuda"), torch.zeros(K, device="cuda")
    stats = torch.zeros(N.N_STATS, dtype=torch.float64, device="cuda")
    sb = int(L.rlppo_diag_scratch_bytes(mb, K))
    scratch = torch.zeros(sb, dtype=torch.uint8, device="cuda")
    call = lambda part: (lambda: N.check(L.rlppo_dbg_diag_loss(st, P(y), 32, K, P(acts), P(old), P(adv), mb, 0.2, 0.005, 1.0, P(ls), P(grad), P(scratch),
                                                               sb, P(stats), part)))
    return {"loss_launch": call(1), "finish": call(2), "loss_and_finish": call(0)}, [y0, y, acts, old, adv, ls, grad, stats, scratch]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_gaussian_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/diag_gaussian_cost.py measures on the GPU: no HIP device visible")
    L = N.lib()
    out = {"build_id": L.rlppo_build_id().decode(), "device": torch.cuda.get_device_name(0), "shape": {"obs": OBS, "hidden": HIDDEN, "k": K},
           "rounds": args.rounds}
    legs, keep = pass_legs(65536, 131072)
    o = alternate(legs, args.rounds, 10)
    compare(o, "diag", "gaussian")
    o["unit"] = "us per 65,536-row fp32 pass (device events, 10 passes per measurement)"
    out["pass_65536"] = o
    del legs, keep
    legs, keep = pass_legs(524288, 524288)
    o = alternate(legs, args.rounds, 3)
    compare(o, "diag", "gaussian")
    o["unit"] = "us per 524,288-row fp32 pass (device events, 3 passes per measurement)"
    out["pass_524288"] = o
    del legs, keep
    torch.cuda.empty_cache()
    legs, keep = rollout_legs(4096)
    o = alternate(legs, args.rounds, 50)
    compare(o, "diag", "gaussian")
    o["unit"] = "us per 4096-row rollout call on padded device rows (device events, 50 calls per measurement)"
    out["rollout_4096"] = o
    del legs, keep
    out["small_call"] = small_call(args.rounds)
    for one_launch in (True, False):
        legs, keep = optimiser_legs(one_launch)
        o = alternate(legs, args.rounds, 50)
        compare(o, "tail_8", "no_tail")
        o["unit"] = "us per optimiser step of both cfg5 networks (device events, 50 steps per measurement)"
        out["optimiser_" + ("one_launch" if one_launch else "three_operations")] = o
        del legs, keep
    for mb in (524288, 65536):
        legs, keep = reduction_legs(mb)
        o = alternate(legs, args.rounds, 50)
        o["unit"] = "us per call on %d rows, k = 8 (device events, 50 calls per measurement)" % mb
        o["partial_sum_rows"] = (mb + 255) // 256
        out[f"log_std_reduction_{mb}"] = o
        del legs, keep
    p = out["pass_524288"]["diag"]
    out["finish_524288_vs_pass_524288_spread"] = {
        "finish_us": out["log_std_reduction_524288"]["finish"]["median"], "pass_spread_us": round(p["spread"] * p["median"], 3),
        "within": bool(out["log_std_reduction_524288"]["finish"]["median"] <= p["spread"] * p["median"])}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "small_call"}, indent=1)[:6000])
    print("small_call:", json.dumps(out["small_call"])[:1500])


if __name__ == "__main__":
    main()
