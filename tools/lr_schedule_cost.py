"""What the KL-adaptive learning-rate schedule costs: ms per PPOLearner.learn() with lr_schedule "constant", with target_kl armed
where it never triggers (1e9: the KL slots, the per-step gate and the host's look-behind on it, the rate still in the descriptor) and
with lr_schedule "adaptive" (the slots, the gate with the rate rule, the optimiser step reading its rate from device memory; no host
wait).  One build, one process, one learner per workload; the configurations alternate inside every round (the layout of
tools/ppo_options_cost.py), the median over the rounds and their spread are reported, at
  * the headline workload (bench.py: 524,288-row buffer, B = 524,288, MB = 65,536, 256x3 nets, 90 actions, 10 epochs) and
  * a rank's share of it in an 8-rank job (65,536 rows, one 65,536-row pass per optimiser step, 10 epochs).
The adaptive runs pin lr_min = lr_max = the initial rate, so that every round measures the same update -- the launches are the same
whichever branch the rule takes.
usage: python tools/lr_schedule_cost.py [--rounds R] [--out FILE.json]"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner  # noqa: E402

OFF = dict(lr_schedule="constant", target_kl=None)
SETS = [("constant", {}), ("target_kl", dict(target_kl=1e9)), ("adaptive", dict(lr_schedule="adaptive"))]


def workload(n, B, MB, epochs):
    rs = np.random.RandomState(1)
    obs = np.clip(rs.randn(n, bench.OBS), -5, 5).astype(np.float32)
    z = np.zeros(n, np.float32)
    torch.manual_seed(1)
    with contextlib.redirect_stdout(sys.stderr):
        learner = PPOLearner(bench.OBS, bench.ACT, 0, bench.HID, bench.HID, (0.1, 1.0), B, epochs, 3e-4, 3e-4, 0.2, 0.005, MB, "cuda:0")
    learner.desired_kl, learner.lr_bounds = 0.01, (3e-4, 3e-4)   # (pinned: every round measures the same update)
    buf = ExperienceBuffer(n, 1, "cpu")
    buf.submit_experience(obs, rs.randint(0, bench.ACT, n).astype(np.float32), (-np.log(bench.ACT) + 0.1 * rs.randn(n)).astype(np.float32),
                          z, obs[:1].repeat(n, 0), z, z, rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32))
    return learner, buf


def measure(learner, buf, rounds, reps):
    res = {name: [] for name, _ in SETS}
    for _ in range(rounds):
        for name, opts in SETS:
            for k, v in dict(OFF, **opts).items():
                setattr(learner, k, v)
            learner.learn(buf)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                learner.learn(buf)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t) / reps * 1e3)
    base = float(np.median(res["constant"]))
    return {name: {"ms": round(float(np.median(v)), 4), "vs_constant": round(float(np.median(v)) / base - 1.0, 4),
                   "spread": round((max(v) - min(v)) / float(np.median(v)), 4), "rounds_ms": [round(x, 3) for x in v]}
            for name, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = [("headline: buffer 524,288, B 524,288, MB 65,536, 10 epochs", (bench.N_SAMPLES, bench.BATCH, bench.MINIBATCH, 10), 3),
            ("rank share: buffer 65,536, B = MB = 65,536, 10 epochs", (bench.MINIBATCH, bench.MINIBATCH, bench.MINIBATCH, 10), 10)]
    record = {"device": torch.cuda.get_device_name(0), "unit": "ms per learn(), median over rounds; spread = (max - min) / median",
              "legs": {}}
    for label, shape, reps in legs:
        learner, buf = workload(*shape)
        out = measure(learner, buf, a.rounds, reps)
        record["legs"][label] = out
        print(label)
        for name, r in out.items():
            print("  %-10s %9.3f ms  %+6.2f %%  (spread %.2f %%)" % (name, r["ms"], 100 * r["vs_constant"], 100 * r["spread"]))
        del learner, buf
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
