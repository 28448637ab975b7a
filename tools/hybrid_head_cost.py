"""What the hybrid head's kernels cost (csrc/hybrid.hip: one 16-lane group per row, the row split by head, tiles staged through LDS):
  * the 65,536-row loss launch (+ the finish of its log_std reduction) at k = 5, nvec = [2, 2, 2] and at k = 3, nvec = [64] * 8, beside
    the two thread-per-row launches it replaces ON THE SAME COLUMNS of the same matrix -- the diag loss on columns [0, k), the [nvec]
    loss on columns [k, k + S) -- and beside a device copy of the logits matrix (the HBM floor: one read and one write of it);
  * the 4,096-row act call (layer chain 107 -> 256 -> 256 -> outputs + sampling kernel): rlppo_hybrid_act beside
    rlppo_diag_gaussian_act + rlppo_multidiscrete_act_nvec, each with its own chain;
  * (--parent DIR: a built checkout of the parent commit) the bench.py headline of this tree against the parent's.
Legs alternate in one process, rotating over SETS buffer sets; medians and spread over the rounds (tools/gae_bootstrap_cost.py's
harness); the record is stamped with rlppo_build_id().  What is measured is recorded; no ratio is promised.
usage: python tools/hybrid_head_cost.py [--rounds R] [--parent DIR] [--bench-rounds R] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gae_bootstrap_cost import alternate, bench_leg  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402

CONFIGS = {"k5_nvec_2x3": (5, [2, 2, 2]), "k3_nvec_64x8": (3, [64] * 8)}
SETS, MB, ACT_ROWS, OBS, HID = 3, 65536, 4096, 107, (256, 256)
P = lambda t: ctypes.c_void_p(t.data_ptr())
stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def loss_legs(L, k, nvec, rounds):
    H, S = len(nvec), sum(nvec)
    ld = int(L.rlppo_padded_out(k + S))
    nv = N.dims_array(nvec)
    rs = np.random.RandomState(0)
    log_std = torch.as_tensor(rs.uniform(-0.5, 0.2, k).astype(np.float32)).cuda()
    acts = torch.as_tensor(np.concatenate([rs.randn(MB, k), (rs.rand(MB, H) * np.asarray(nvec)).astype(np.int64)], 1).astype(np.float32)).cuda()
    a_d, a_n = acts[:, :k].contiguous(), acts[:, k:].contiguous()
    old, adv = torch.as_tensor((-3.0 + 0.3 * rs.randn(MB)).astype(np.float32)).cuda(), torch.as_tensor(rs.randn(MB).astype(np.float32)).cuda()
    sb = int(L.rlppo_diag_scratch_bytes(MB, k))
    scratch, gls, stats = torch.empty(sb, dtype=torch.uint8, device="cuda"), torch.zeros(k, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
    legs = {"hybrid": [], "diag_plus_nvec": [], "copy": []}
    for _ in range(SETS):
        # (one spare row: the [nvec] launch on columns [k, ..) zeroes ld - S columns from ITS column 0, k of them in the next row)
        y, y2 = torch.randn(MB + 1, ld, device="cuda"), torch.empty(MB + 1, ld, device="cuda")
        legs["hybrid"].append(lambda y=y: N.check(L.rlppo_dbg_hybrid_loss(stream(), P(y), ld, k, nv, H, P(acts), P(old), P(adv), MB, 0.2, 0.005, 1.0,
                                                                          P(log_std), P(gls), P(scratch), sb, P(stats), 0)))

        def both(y=y):
            N.check(L.rlppo_dbg_diag_loss(stream(), P(y), ld, k, P(a_d), P(old), P(adv), MB, 0.2, 0.005, 1.0, P(log_std), P(gls), P(scratch), sb, P(stats), 0))
            N.check(L.rlppo_dbg_nvec_loss(stream(), ctypes.c_void_p(y.data_ptr() + 4 * k), ld, nv, H, P(a_n), P(old), P(adv), MB, 0.2, 0.005, 1.0, P(stats)))
        legs["diag_plus_nvec"].append(both)
        legs["copy"].append(lambda y=y, y2=y2: y2[:MB].copy_(y[:MB]))
    out = alternate(legs, rounds)
    out["hybrid_vs_thread_per_row"] = round(out["hybrid"]["median"] / out["diag_plus_nvec"]["median"], 4)
    out["hybrid_vs_copy"] = round(out["hybrid"]["median"] / out["copy"]["median"], 4)
    out["unit"] = f"us per launch group, {MB} rows of ld {ld} floats ({k} + {S} columns in use), rotation over {SETS} matrices, HIP events"
    return out


def act_legs(L, k, nvec, rounds):
    H, S, B = len(nvec), sum(nvec), max(nvec)
    nv = N.dims_array(nvec)
    n = ACT_ROWS
    nets = {}
    for name, out in (("hybrid", k + S), ("diag", k), ("nvec", S)):
        dims = [OBS, *HID, out]
        dims_c = N.dims_array(dims)
        flat = 0.05 * torch.randn(int(L.rlppo_flat_floats(dims_c, 3)), device="cuda")
        packed = torch.zeros(int(L.rlppo_packed_floats(dims_c, 3)), device="cuda")
        N.check(L.rlppo_net_pack(stream(), dims_c, 3, P(flat), P(packed)))
        ws = torch.empty(int(L.rlppo_forward_workspace_bytes(dims_c, 3, n)), dtype=torch.uint8, device="cuda")
        nets[name] = (dims_c, packed, ws)
    ld_in = int(L.rlppo_padded_width(OBS))
    log_std = torch.zeros(k, device="cuda")
    legs = {"hybrid": [], "diag_plus_nvec": []}
    for _ in range(SETS):
        obs = torch.zeros(n, ld_in, device="cuda")
        obs[:, :OBS].normal_()
        eps, q = torch.randn(n, k, device="cuda"), torch.empty(n * H, B, device="cuda").exponential_(1)
        act, a_d, a_n = torch.empty(n, k + H, device="cuda"), torch.empty(n, k, device="cuda"), torch.empty(n, H, dtype=torch.int64, device="cuda")
        logp = torch.empty(n, device="cuda")
        keep = (obs, eps, q, act, a_d, a_n, logp)

        def hybrid(t=keep):
            d, pk, ws = nets["hybrid"]
            N.check(L.rlppo_hybrid_act(stream(), d, 3, P(pk), P(t[0]), ld_in, n, k, nv, H, P(t[1]), P(t[2]), P(log_std), P(t[3]), P(t[6]), P(ws),
                                       ws.numel(), None))

        def both(t=keep):
            d, pk, ws = nets["diag"]
            N.check(L.rlppo_diag_gaussian_act(stream(), d, 3, P(pk), P(t[0]), ld_in, n, P(t[1]), P(log_std), P(t[4]), P(t[6]), P(ws), ws.numel(), None))
            d, pk, ws = nets["nvec"]
            N.check(L.rlppo_multidiscrete_act_nvec(stream(), d, 3, P(pk), P(t[0]), ld_in, n, P(t[2]), P(t[5]), P(t[6]), P(ws), ws.numel(), None, nv, H))
        legs["hybrid"].append(hybrid)
        legs["diag_plus_nvec"].append(both)
    out = alternate(legs, rounds)
    out["hybrid_vs_two_calls"] = round(out["hybrid"]["median"] / out["diag_plus_nvec"]["median"], 4)
    out["unit"] = f"us per act call of {n} rows, {OBS} -> 256 -> 256 -> outputs; the two-call leg runs two layer chains"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = N.lib()
    record = {"device": torch.cuda.get_device_name(0), "build_id": L.rlppo_build_id().decode(), "rounds": a.rounds}
    for name, (k, nvec) in CONFIGS.items():
        record[name] = {"k": k, "nvec": nvec, "loss_us": loss_legs(L, k, nvec, a.rounds)}
        torch.cuda.empty_cache()
        record[name]["act_us"] = act_legs(L, k, nvec, a.rounds)
        print(name, json.dumps(record[name]), flush=True)
    if a.parent:
        record["bench_headline"] = bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
