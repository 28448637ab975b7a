"""What invalid-action masking costs, and that the unmasked paths cost what they did:
  * PPOLearner.learn() at the headline shape (bench.py: 524,288-row buffer, B = 524,288, MB = 65,536, 256x3 nets, 90 actions, 10 epochs)
    on an unmasked buffer and on one with a random ~2/3-valid mask per row, alternating;
  * the 4096-observation rollout step (DiscreteFF.step, noise resident on the device), unmasked and masked, alternating;
  * (--parent DIR: a built checkout of the parent commit) the unmasked bench.py headline of this tree against the parent's,
    alternating, each in a fresh process.
Medians and spread (min .. max) over the rounds; the record is stamped with rlppo_build_id().
usage: python tools/action_mask_cost.py [--rounds R] [--parent DIR] [--bench-rounds R] [--out FILE.json]"""
import argparse
import contextlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402
from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner  # noqa: E402
from rlgym_ppo_amd.util import action_mask as AM  # noqa: E402


def summary(ms):
    return {"median": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4),
            "spread": round(float((max(ms) - min(ms)) / np.median(ms)), 4), "rounds": [round(float(x), 4) for x in ms]}


def learn_leg(rounds):
    n, B, MB, A = bench.N_SAMPLES, bench.BATCH, bench.MINIBATCH, bench.ACT
    rs = np.random.RandomState(1)
    obs = np.clip(rs.randn(n, bench.OBS), -5, 5).astype(np.float32)
    z = np.zeros(n, np.float32)
    torch.manual_seed(1)
    with contextlib.redirect_stdout(sys.stderr):
        learner = PPOLearner(bench.OBS, A, 0, bench.HID, bench.HID, (0.1, 1.0), B, 10, 3e-4, 3e-4, 0.2, 0.005, MB, "cuda:0")
    mask = rs.rand(n, A) < 2.0 / 3.0
    acts = rs.randint(0, A, n)
    mask[np.arange(n), acts] = True   # the stored action is valid under its own mask
    old = (-np.log(A) + 0.1 * rs.randn(n)).astype(np.float32)
    tgt, adv = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    bufs = {}
    for name in ("unmasked", "masked"):
        buf = ExperienceBuffer(n, 1, "cpu")
        kw = dict(action_masks=mask) if name == "masked" else {}
        buf.submit_experience(obs, acts.astype(np.float32), old, z, obs[:1].repeat(n, 0), z, z, tgt, adv, **kw)
        bufs[name] = buf
    res = {k: [] for k in bufs}
    for r in range(rounds + 1):  # (round 0 warms up)
        for name, buf in bufs.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            learner.learn(buf)
            torch.cuda.synchronize()
            if r:
                res[name].append((time.perf_counter() - t) * 1e3)
    out = {k: summary(v) for k, v in res.items()}
    out["masked_vs_unmasked"] = round(out["masked"]["median"] / out["unmasked"]["median"] - 1.0, 4)
    out["valid_fraction"] = round(float(mask.mean()), 4)
    return out


def rollout_leg(rounds, n=4096, calls=200):
    from rlgym_ppo_amd.ppo.discrete_policy import DiscreteFF
    torch.manual_seed(2)
    A = bench.ACT
    pol = DiscreteFF(bench.OBS, A, bench.HID, "cuda:0")
    rs = np.random.RandomState(2)
    obs = torch.from_numpy(np.clip(rs.randn(n, bench.OBS), -5, 5).astype(np.float32)).cuda()
    q = torch.empty(n, A, device="cuda").exponential_(1)
    m = rs.rand(n, A) < 2.0 / 3.0
    m[np.arange(n), rs.randint(0, A, n)] = True
    packed = AM.Packed(AM.pack(m, A, "cuda"), A)
    c0 = int(N.lib().rlppo_dbg_counter(0))
    res = {"unmasked": [], "masked": []}
    for r in range(rounds + 1):
        for name in res:
            kw = dict(action_mask=packed) if name == "masked" else {}
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(calls):
                pol.step(obs, noise=q, to_host=False, **kw)
            torch.cuda.synchronize()
            if r:
                res[name].append((time.perf_counter() - t) / calls * 1e6)
    out = {k: summary(v) for k, v in res.items()}
    out["unit"] = "us per step of %d observations (device-resident observations, noise and mask; %d calls back to back)" % (n, calls)
    out["one_launch_calls"] = int(N.lib().rlppo_dbg_counter(0)) - c0
    out["masked_vs_unmasked"] = round(out["masked"]["median"] / out["unmasked"]["median"] - 1.0, 4)
    return out


def bench_leg(rounds, parent):
    trees = {"branch": ROOT, "parent": os.path.abspath(parent)}
    res = {k: [] for k in trees}
    for r in range(rounds):
        for name, d in trees.items():
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=d, capture_output=True,
                               text=True, timeout=600)
            line = [x for x in p.stdout.splitlines() if x.startswith("{") and '"metric"' in x][-1]
            res[name].append(float(json.loads(line)["value"]))
    out = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": round((max(v) - min(v)) / float(np.median(v)), 4),
               "rounds": v} for k, v in res.items()}
    out["unit"] = "samples/s, bench.py --gpus 1 --steps 20 --warmup 5, a fresh process per run, alternating"
    out["branch_vs_parent"] = round(out["branch"]["median"] / out["parent"]["median"] - 1.0, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}
    record["rollout_step"] = rollout_leg(a.rounds)
    print("rollout step:", json.dumps(record["rollout_step"]), flush=True)
    record["learn_ms"] = learn_leg(a.rounds)
    print("learn():", json.dumps(record["learn_ms"]), flush=True)
    torch.cuda.empty_cache()
    if a.parent:
        record["bench_headline"] = bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
