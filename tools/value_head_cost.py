"""What the categorical critic (Learner(ppo_value_head=...), include/rlppo.h "[vbins]") costs, on ONE build, alternating:
  * its two row kernels alone at 65,536 x {51, 101, 255} bins (rlppo_dbg_value_bins_loss, both kinds; rlppo_value_bins_readout) beside
    a device copy of the same padded matrix (the loss reads and writes it once: one copy of it; the readout only reads it);
  * one 65,536-row fp32 pass of the update at the flagship shape (obs 107, 256 x 3, 90 discrete actions): one-output critic by default,
    one-output critic through the plain form, critic with 101 HL-Gauss bins.
No target is fixed in advance: medians and spread ((max - min) / median) over the rounds are recorded, stamped with rlppo_build_id().
--bench NAME=FILE ... : `bench.py --gpus 1 --steps 20 --warmup 5` result lines (this commit, its parent) to record beside them.
usage: python tools/value_head_cost.py [--rounds R] [--out FILE.json] [--bench NAME=FILE ...]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rlgym_ppo_amd import _native as N  # noqa: E402
from tools import activation_cost as AC  # noqa: E402
from tools.diag_gaussian_cost import Net, P, alternate, bench_stream  # noqa: E402

BINS = lambda n, kind=1: N.ValueBinsArg(kind, n, -10.0, 10.0, 0.75)


def kernel_legs(rows, n):
    L = N.lib()
    ld = int(L.rlppo_padded_out(n))
    z0, z = 4 * torch.randn(rows, ld, device="cuda"), torch.empty(rows, ld, device="cuda")
    tgt, values, stats = 8 * torch.randn(rows, device="cuda"), torch.empty(rows, device="cuda"), torch.zeros(N.N_STATS, dtype=torch.float64, device="cuda")
    hl, th, st = BINS(n, 1), BINS(n, 2), bench_stream()
    # (the loss overwrites its logits with gradients of magnitude 1 / rows: still finite logits for the next repetition)
    z.copy_(z0)
    loss = lambda b: lambda: N.check(L.rlppo_dbg_value_bins_loss(st, P(z), ld, ctypes.byref(b), P(tgt), rows, 1.0, None, P(stats)))
    legs = {"loss_hl_gauss": loss(hl), "loss_two_hot": loss(th),
            "readout": lambda: N.check(L.rlppo_value_bins_readout(st, P(z0), ld, ctypes.byref(hl), P(values), rows)),
            "copy_of_the_matrix": lambda: z.copy_(z0)}
    return legs, [z0, z, tgt, values, stats, hl, th]


def pass_legs(mb, n_buf, n_bins):
    """One pass per leg on one buffer: critic [.., 1] by default and forced plain (activation_cost's switches), critic [.., n_bins] with bins."""
    L = N.lib()
    rs = np.random.RandomState(0)
    pol, nets = Net([AC.OBS, *AC.HIDDEN, AC.A]), {1: Net([AC.OBS, *AC.HIDDEN, 1]), n_bins: Net([AC.OBS, *AC.HIDDEN, n_bins])}
    states = torch.zeros(n_buf, pol.ld_in, device="cuda")
    states[:, :AC.OBS] = torch.randn(n_buf, AC.OBS, device="cuda").clamp_(-5, 5)
    acts, old = torch.randint(0, AC.A, (n_buf,), device="cuda").float(), torch.randn(n_buf, device="cuda") * 0.3 - 4.5
    tgt, adv = torch.randn(n_buf, device="cuda"), torch.randn(n_buf, device="cuda")
    idx = torch.as_tensor(rs.permutation(n_buf)[:mb]).cuda()
    stats, gp, st = torch.zeros(N.N_STATS, dtype=torch.float64, device="cuda"), torch.zeros(pol.n, device="cuda"), bench_stream()
    legs, keep, bins = {}, [pol, nets, states, acts, old, tgt, adv, idx, stats, gp], BINS(n_bins)
    for name, out, plain in (("scalar", 1, False), ("scalar_plain", 1, True), (f"bins_{n_bins}", n_bins, False)):
        val = nets[out]
        a, gv = N.MinibatchArgs(), torch.zeros(val.n, device="cuda")
        a.head, a.pol_layers, a.val_layers, a.act_dim, a.precision = N.HEAD_DISCRETE, pol.nl, val.nl, 1, N.PRECISION_FP32
        a.pol_dims, a.val_dims = (ctypes.cast(d, ctypes.POINTER(ctypes.c_int32)) for d in (pol.dims_c, val.dims_c))
        ws = torch.empty(int(L.rlppo_minibatch_workspace_bytes_for(pol.dims_c, pol.nl, val.dims_c, val.nl, mb, a.precision)), dtype=torch.uint8, device="cuda")
        a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = pol.packed.data_ptr(), val.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
        a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], n_buf, acts.data_ptr()
        a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idx.data_ptr(), mb
        a.clip_range, a.ent_coef, a.mb_ratio = 0.2, 0.005, 1.0
        a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws.numel()
        call = lambda a=a, b=bins if out > 1 else None: N.check(L.rlppo_ppo_minibatch_vbins(st, ctypes.byref(a), None, None, None, None if b is None else ctypes.byref(b)))
        legs[name] = AC.switched(call, AC.PLAIN_PASS) if plain else call
        keep += [a, gv, ws]
    return legs, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "value_head_cost.json"))
    ap.add_argument("--bench", action="append", default=[], help="NAME=FILE: the last line of FILE is a bench.py JSON result line")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/value_head_cost.py measures on the GPU: no HIP device visible")
    L = N.lib()
    out = {"build_id": L.rlppo_build_id().decode(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "shape": {"obs": AC.OBS, "hidden": AC.HIDDEN, "actions": AC.A, "value_range": [-10.0, 10.0], "sigma_ratio": 0.75}}
    builds = [(f"row_kernels_65536x{n}", lambda n=n: kernel_legs(65536, n), 50, "us per launch / copy") for n in (51, 101, 255)]
    builds.append(("pass_65536", lambda: pass_legs(65536, 131072, 101), 10, "us per 65,536-row fp32 pass"))
    for key, build, reps, unit in builds:
        legs, keep = build()
        o = alternate(legs, args.rounds, reps)
        o["unit"] = unit + f" (device events, {reps} per measurement)"
        if "scalar" in o:
            o["ratios"] = {"bins_over_scalar": round(o["bins_101"]["median"] / o["scalar"]["median"], 4),
                           "bins_over_scalar_plain": round(o["bins_101"]["median"] / o["scalar_plain"]["median"], 4)}
        else:
            o["ratios"] = {k + "_over_copy": round(o[k]["median"] / o["copy_of_the_matrix"]["median"], 4) for k in ("loss_hl_gauss", "loss_two_hot", "readout")}
        out[key] = o
        del legs, keep
        torch.cuda.empty_cache()
    for item in args.bench:
        name, path = item.split("=", 1)
        lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
        out.setdefault("bench", {})[name] = json.loads(lines[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "bench"}, indent=1)[:5000])


if __name__ == "__main__":
    main()
