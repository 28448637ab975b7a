"""What mirror-symmetry augmentation costs, on one build in one session, legs alternating:
  * rlppo_mirror_batch at 65,536 rows x 128 floats (discrete head, 90 actions, a shuffled minibatch of a ring), COLD (rotating over
    buffer sets), beside a device-to-device copy that moves the same bytes: the kernel reads the rows once and writes them twice, the
    copy reads and writes one and a half times the matrix;
  * one PPOLearner.learn of a 65,536-row buffer in one pass (256 x 3 networks), with the symmetry set and without;
  * (--parent DIR: a built checkout of the parent commit) the bench.py headline of this tree against the parent's, alternating: the
    headline sets no symmetry and runs none of the new code.
Medians and spread over the rounds; the record is stamped with rlppo_build_id().  What is measured is recorded; no ratio is promised.
usage: python tools/symmetry_cost.py [--rounds R] [--parent DIR] [--bench-rounds R] [--out FILE.json]"""
import argparse
import contextlib
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from gae_bootstrap_cost import alternate, bench_leg, compare, summary  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402
from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner, Symmetry  # noqa: E402
from rlgym_ppo_amd.ppo.symmetry import BoundSymmetry  # noqa: E402

ROWS, D, LD, A, SETS = 65536, 120, 128, 90, 6


def field_symmetry(d, n_actions):
    """A left-right mirror as a typical table: the two halves of the observation swapped, every fifth column's sign flipped."""
    h = d // 2
    perm = np.concatenate([np.arange(h, 2 * h), np.arange(h), np.arange(2 * h, d)])
    sign = np.where(np.arange(d) % 5 == 2, -1.0, 1.0)
    sign[:h] = sign[h:2 * h]
    return Symmetry(perm, sign, action=np.arange(n_actions)[::-1].copy())


def kernel_leg(rounds):
    L = N.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sym = field_symmetry(D, A)
    bound = BoundSymmetry(sym, sym.host_tables(N.HEAD_DISCRETE, D, LD, n_actions=A), N.HEAD_DISCRETE, "cuda")
    nbytes = int(L.rlppo_mirror_staging_bytes(ROWS, LD, 0, 1, 0, None))
    rs = np.random.RandomState(0)
    legs, keep = {"mirror": [], "copy": []}, []
    for _ in range(SETS):
        states = torch.zeros(ROWS, LD, device="cuda")
        states[:, :D] = torch.randn(ROWS, D, device="cuda")
        acts = torch.randint(0, A, (ROWS,), device="cuda").float()
        old, tgt, adv = (torch.randn(ROWS, device="cuda") for _ in range(3))
        idx = torch.as_tensor(rs.permutation(ROWS)).cuda()
        staging = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        a = N.MinibatchArgs()
        a.head, a.act_dim, a.mb, a.ld_states, a.ring_base, a.ring_cap = N.HEAD_DISCRETE, 1, ROWS, LD, ROWS // 3, ROWS
        a.states, a.actions, a.old_logp, a.targets, a.advantages, a.idx = (t.data_ptr() for t in (states, acts, old, tgt, adv, idx))
        src, dst = torch.empty(3 * ROWS * LD // 2, device="cuda"), torch.empty(3 * ROWS * LD // 2, device="cuda")
        keep.append((states, acts, old, tgt, adv, idx, staging, a, src, dst))
        legs["mirror"].append(lambda a=a, s=staging: N.check(L.rlppo_mirror_batch(st, ctypes.byref(a), None, ctypes.byref(bound.desc), s.data_ptr(), nbytes)))
        legs["copy"].append(lambda s=src, d=dst: d.copy_(s))
    out = alternate(legs, rounds)
    compare(out, "mirror", "copy")
    moved = 3 * ROWS * LD * 4
    out["unit"] = "us per cold launch (rotation over %d buffer sets, HIP events); %d rows x %d floats through a shuffled index and a ring" % (SETS, ROWS, LD)
    out["row_bytes_moved"] = moved
    out["GBps"] = {k: round(moved / (out[k]["median"] * 1e-6) / 1e9, 1) for k in ("mirror", "copy")}
    return out


def pass_leg(rounds):
    with contextlib.redirect_stdout(sys.stderr):
        learner = PPOLearner(107, A, 0, bench.HID, bench.HID, (0.1, 1.0), ROWS, 1, 3e-4, 3e-4, 0.2, 0.005, ROWS, "cuda:0")
    sym = field_symmetry(107, A)
    rs = np.random.RandomState(1)
    obs = rs.randn(ROWS, 107).astype(np.float32)
    acts = rs.randint(0, A, ROWS).astype(np.float32)
    z = np.zeros(ROWS, np.float32)
    buf = ExperienceBuffer(ROWS, 0, "cpu")
    buf.submit_experience(obs, acts, (-4.5 + 0.05 * rs.randn(ROWS)).astype(np.float32), z, obs, z, z, rs.randn(ROWS).astype(np.float32),
                          rs.randn(ROWS).astype(np.float32))
    res = {"augmented": [], "plain": []}
    for r in range(rounds + 1):   # (round 0 warms up)
        for name in res:
            learner.set_symmetry(sym if name == "augmented" else None)
            torch.cuda.synchronize()
            t = time.perf_counter()
            learner.learn(buf)
            torch.cuda.synchronize()
            if r:
                res[name].append((time.perf_counter() - t) * 1e3)
    out = {k: summary(v) for k, v in res.items()}
    compare(out, "augmented", "plain")
    out["unit"] = "ms per learn() of one %d-row pass + optimiser step + report (256 x 3 networks), host clock around a device synchronise" % ROWS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}
    record["kernel_us"] = kernel_leg(a.rounds)
    print("kernel:", json.dumps(record["kernel_us"]), flush=True)
    torch.cuda.empty_cache()
    record["pass_ms"] = pass_leg(a.rounds)
    print("pass:", json.dumps(record["pass_ms"]), flush=True)
    torch.cuda.empty_cache()
    if a.parent:
        record["bench_headline"] = bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
