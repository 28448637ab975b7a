"""What hidden layer normalisation (Learner(hidden_layer_norm=...), include/rlppo.h "[norm]") costs, on ONE build, alternating, at the
flagship shape (obs 107, 256 x 3, 90 discrete actions):
  * one 65,536-row fp32 pass of the update: default ReLU, ReLU through the plain form, ReLU + normalisation of both networks;
  * the two row kernels alone at 65,536 x 256 (rlppo_row_norm_fwd / _bwd) against a device copy of the bytes each moves (the
    forward reads and writes the matrix once: one copy of it; the backward reads two and writes one: a copy of 1.5 matrices);
  * the 4096-row rlppo_discrete_act call: one launch (default), the ReLU layer chain, the chain with normalisation.
No target is fixed in advance: medians and spread ((max - min) / median) over the rounds are recorded, stamped with rlppo_build_id().
--bench NAME=FILE ... : `bench.py --gpus 1 --steps 20 --warmup 5` result lines (this commit, its parent) to record beside them.
usage: python tools/layer_norm_cost.py [--rounds R] [--out FILE.json] [--bench NAME=FILE ...]"""
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

AC.CONFIGS = (("relu", 0, False), ("relu_plain", 0, True), ("relu_norm", N.ACT_NORM, False))   # the legs its pass / rollout builders make


def pass_legs(mb, n_buf):
    """activation_cost's pass legs on a workspace sized for the normalised pass (it serves the other two as well)."""
    L = N.lib()
    sized = L.rlppo_minibatch_workspace_bytes_for
    norm_sized = lambda *a: L.rlppo_minibatch_workspace_bytes_norm(*a, 0, N.ACT_NORM, N.ACT_NORM)
    L.rlppo_minibatch_workspace_bytes_for = norm_sized
    try:
        return AC.pass_legs(mb, n_buf)
    finally:
        L.rlppo_minibatch_workspace_bytes_for = sized


def kernel_legs(n, w):
    L = N.lib()
    h, dy = torch.relu(torch.randn(n, w, device="cuda")), torch.randn(n, w, device="cuda")
    y, dx = torch.empty_like(h), torch.empty_like(h)
    src, dst = torch.empty(3 * n * w // 2, device="cuda"), torch.empty(3 * n * w // 2, device="cuda")
    st = bench_stream()
    copy = lambda k: lambda: dst[:k].copy_(src[:k])   # (a device-to-device copy on the same stream)
    legs = {"fwd": lambda: N.check(L.rlppo_row_norm_fwd(st, P(h), w, n, w, P(y), w)),
            "copy_1_matrix": copy(n * w),
            "bwd": lambda: N.check(L.rlppo_row_norm_bwd(st, P(h), w, P(dy), w, n, w, 0, P(dx), w)),
            "copy_1.5_matrices": copy(3 * n * w // 2)}
    return legs, [h, dy, y, dx, src, dst]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layer_norm_cost.json"))
    ap.add_argument("--bench", action="append", default=[], help="NAME=FILE: the last line of FILE is a bench.py JSON result line")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/layer_norm_cost.py measures on the GPU: no HIP device visible")
    L = N.lib()
    out = {"build_id": L.rlppo_build_id().decode(), "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "shape": {"obs": AC.OBS, "hidden": AC.HIDDEN, "actions": AC.A},
           "configurations": {"relu": "default", "relu_plain": "rlppo_dbg_set 26=0 29=0 32=0 19=0 (pass), 27=0 (rollout)",
                              "relu_norm": "hidden_act RLPPO_ACT_NORM, both networks"}}
    for key, build, reps, unit in (("pass_65536", lambda: pass_legs(65536, 131072), 10, "us per 65,536-row fp32 pass"),
                                   ("row_kernels_65536x256", lambda: kernel_legs(65536, 256), 50, "us per launch / copy"),
                                   ("rollout_4096", lambda: AC.rollout_legs(4096), 50, "us per 4096-row rlppo_discrete_act call on padded device rows")):
        legs, keep = build()
        o = alternate(legs, args.rounds, reps)
        o["unit"] = unit + f" (device events, {reps} per measurement)"
        if "relu_norm" in o:
            o["ratios"] = {"norm_over_relu": round(o["relu_norm"]["median"] / o["relu"]["median"], 4),
                           "norm_over_relu_plain": round(o["relu_norm"]["median"] / o["relu_plain"]["median"], 4)}
        else:
            o["ratios"] = {"fwd_over_copy": round(o["fwd"]["median"] / o["copy_1_matrix"]["median"], 4),
                           "bwd_over_copy": round(o["bwd"]["median"] / o["copy_1.5_matrices"]["median"], 4)}
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
