"""What residual hidden layers (Learner(hidden_residual=...), include/rlppo.h "[res]") cost, on ONE build, alternating, at the flagship
shape (obs 107, 256 x 3, 90 discrete actions):
  * one 65,536-row fp32 pass of the update: default ReLU, ReLU through the plain form, normalised, normalised + residual, and the
    residual alone;
  * the two row kernels alone at 65,536 x 256 (rlppo_row_res_fwd / _bwd, with the norm) against a device copy of the matrices each
    moves (the forward reads two and writes two: a copy of two matrices; the backward reads four and writes two: a copy of three);
  * the 4096-row rlppo_discrete_act call as the layer chain: ReLU, normalised, normalised + residual, the residual alone.
No target is fixed in advance: medians and spread ((max - min) / median) over the rounds are recorded, stamped with rlppo_build_id().
--bench NAME=FILE ... : `bench.py --gpus 1 --steps 20 --warmup 5` result lines (this commit, its parent) to record beside them.
usage: python tools/residual_cost.py [--rounds R] [--out FILE.json] [--bench NAME=FILE ...]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rlgym_ppo_amd import _native as N  # noqa: E402
from tools import activation_cost as AC  # noqa: E402
from tools.diag_gaussian_cost import P, alternate, bench_stream  # noqa: E402

BOTH = N.ACT_NORM | N.ACT_RES
PASS_CONFIGS = (("relu", 0, False), ("relu_plain", 0, True), ("relu_norm", N.ACT_NORM, False), ("relu_norm_res", BOTH, False), ("relu_res", N.ACT_RES, False))
CHAIN_CONFIGS = (("relu_plain", 0, True),) + PASS_CONFIGS[2:]


def pass_legs(mb, n_buf):
    """activation_cost's pass legs for PASS_CONFIGS on one workspace sized for the normalised residual networks (it serves every leg)."""
    L = N.lib()
    return AC.pass_legs(mb, n_buf, PASS_CONFIGS, lambda *a: L.rlppo_minibatch_workspace_bytes_res(*a, 0, BOTH, BOTH))


def rollout_legs(n):
    L = N.lib()
    return AC.rollout_legs(n, CHAIN_CONFIGS, lambda *a: L.rlppo_forward_workspace_bytes_act(*a, BOTH))


def kernel_legs(n, w):
    L = N.lib()
    a, s, p, gn = (torch.relu(torch.randn(n, w, device="cuda")) for _ in range(4))
    so, u, g, dz = (torch.empty_like(a) for _ in range(4))
    src, dst = torch.empty(3 * n * w, device="cuda"), torch.empty(3 * n * w, device="cuda")
    st = bench_stream()
    copy = lambda k: lambda: dst[:k].copy_(src[:k])   # (a device-to-device copy on the same stream)
    legs = {"fwd": lambda: N.check(L.rlppo_row_res_fwd(st, P(s), w, P(a), w, n, w, 1, P(so), w, P(u), w)),
            "copy_2_matrices": copy(2 * n * w),
            "bwd": lambda: N.check(L.rlppo_row_res_bwd(st, P(a), w, P(s), w, P(p), w, P(gn), w, n, w, 0, 1, P(g), w, P(dz), w)),
            "copy_3_matrices": copy(3 * n * w)}
    return legs, [a, s, p, gn, so, u, g, dz, src, dst]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_cost.json"))
    ap.add_argument("--bench", action="append", default=[], help="NAME=FILE: the last line of FILE is a bench.py JSON result line")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/residual_cost.py measures on the GPU: no HIP device visible")
    L = N.lib()
    out = {"build_id": L.rlppo_build_id().decode(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "shape": {"obs": AC.OBS, "hidden": AC.HIDDEN, "actions": AC.A},
           "configurations": {"relu": "default", "relu_plain": "rlppo_dbg_set 26=0 29=0 32=0 19=0 (pass), 27=0 (rollout)",
                              "relu_norm": "hidden_act RLPPO_ACT_NORM, both networks", "relu_norm_res": "RLPPO_ACT_NORM | RLPPO_ACT_RES, both networks",
                              "relu_res": "RLPPO_ACT_RES, both networks"}}
    for key, build, reps, unit in (("pass_65536", lambda: pass_legs(65536, 131072), 10, "us per 65,536-row fp32 pass"),
                                   ("row_kernels_65536x256", lambda: kernel_legs(65536, 256), 50, "us per launch / copy"),
                                   ("rollout_4096", lambda: rollout_legs(4096), 50,
                                    "us per 4096-row rlppo_discrete_act call on padded device rows, layer chain")):
        legs, keep = build()
        o = alternate(legs, args.rounds, reps)
        o["unit"] = unit + f" (device events, {reps} per measurement)"
        if "relu_norm_res" in o:
            o["ratios"] = {"norm_res_over_norm": round(o["relu_norm_res"]["median"] / o["relu_norm"]["median"], 4),
                           "res_over_relu_plain": round(o["relu_res"]["median"] / o["relu_plain"]["median"], 4)}
        else:
            o["ratios"] = {"fwd_over_copy": round(o["fwd"]["median"] / o["copy_2_matrices"]["median"], 4),
                           "bwd_over_copy": round(o["bwd"]["median"] / o["copy_3_matrices"]["median"], 4)}
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
    print(json.dumps({k: v for k, v in out.items() if k != "bench"}, indent=1)[:6000])


if __name__ == "__main__":
    main()
