"""What the options beyond the reference cost: ms per PPOLearner.learn() with every option off, each option alone and all of them
together, interleaved in one process (each configuration measured in every round, the median over the rounds), at
  * the headline workload (bench.py: 524,288-row buffer, B = 524,288, MB = 65,536, 256x3 nets, 10 epochs) and
  * the reference's defaults (buffer 150,000, B = MB = 50,000, 1 and 10 epochs).
target_kl is priced where it never triggers (1e9): every step runs, plus the per-step gate and the host's look-behind on it.
usage: python tools/ppo_options_cost.py [--rounds R] [--out FILE.json]"""
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

OFF = dict(normalize_advantages=False, value_clip_range=None, target_kl=None, max_grad_norm=0.5)
SETS = [("off", {}), ("normalize_advantages", dict(normalize_advantages=True)), ("value_clip_range", dict(value_clip_range=0.2)),
        ("target_kl", dict(target_kl=1e9)), ("max_grad_norm", dict(max_grad_norm=1.0)),
        ("all", dict(normalize_advantages=True, value_clip_range=0.2, target_kl=1e9, max_grad_norm=1.0))]


def workload(n, B, MB, epochs):
    rs = np.random.RandomState(1)
    obs = np.clip(rs.randn(n, bench.OBS), -5, 5).astype(np.float32)
    z = np.zeros(n, np.float32)
    torch.manual_seed(1)
    with contextlib.redirect_stdout(sys.stderr):
        learner = PPOLearner(bench.OBS, bench.ACT, 0, bench.HID, bench.HID, (0.1, 1.0), B, epochs, 3e-4, 3e-4, 0.2, 0.005, MB, "cuda:0")
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
    off = float(np.median(res["off"]))
    return {name: {"ms": round(float(np.median(v)), 4), "vs_off": round(float(np.median(v)) / off - 1.0, 4),
                   "rounds_ms": [round(x, 3) for x in v]} for name, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = [("headline: buffer 524,288, B 524,288, MB 65,536, 10 epochs", (bench.N_SAMPLES, bench.BATCH, bench.MINIBATCH, 10), 3),
            ("reference defaults: buffer 150,000, B = MB = 50,000, 1 epoch", (bench.REF_BUFFER, bench.REF_BATCH, bench.REF_BATCH, 1), 10),
            ("reference defaults: buffer 150,000, B = MB = 50,000, 10 epochs", (bench.REF_BUFFER, bench.REF_BATCH, bench.REF_BATCH, 10), 3)]
    record = {"device": torch.cuda.get_device_name(0), "unit": "ms per learn(), median over rounds", "legs": {}}
    for label, shape, reps in legs:
        learner, buf = workload(*shape)
        out = measure(learner, buf, a.rounds, reps)
        record["legs"][label] = out
        print(label)
        for name, r in out.items():
            print("  %-22s %9.3f ms  %+6.2f %%" % (name, r["ms"], 100 * r["vs_off"]))
        del learner, buf
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
