"""What the V-trace recompute costs:
  * the 8192 x 256 scan, COLD (rotating over bench.GAE_SETS buffer sets: every scan streams from HBM), rlppo_gae_vtrace beside
    rlppo_gae_boot on the same flags, alternating in one process (the V-trace scan reads two more streams and writes one fewer:
    36 algorithmic bytes per step against 32);
  * Learner(gae_vtrace=True) at the reference's own configuration -- a 150,000-row buffer, 50,000 steps per iteration, 10 epochs of
    50,000-row batches, 256x3 networks: the whole recompute (value pass over the buffer, log-probabilities, scan, write-back) against
    one PPOLearner.learn of that buffer, alternating, host clock around a device synchronise;
  * (--parent DIR: a built checkout of the parent commit) the bench.py headline of this tree against the parent's, alternating.
Medians and spread over the rounds; the record is stamped with rlppo_build_id().  What is measured is recorded; no ratio is promised.
usage: python tools/gae_vtrace_cost.py [--rounds R] [--parent DIR] [--bench-rounds R] [--out FILE.json]"""
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


def scan_leg(rounds):
    L = N.lib()
    rews, dones, trunc, values = bench.gae_inputs()
    n = rews.shape[0]
    rs = np.random.RandomState(1)
    boot = np.where((trunc != 0) & (dones == 0), rs.randn(n), np.nan).astype(np.float32)
    lpo = (-1.5 + 0.5 * rs.randn(n)).astype(np.float32)
    lpn = (lpo + rs.uniform(np.log(0.5), np.log(2.0), size=n)).astype(np.float32)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    legs = {"boot": [], "vtrace": []}
    for _ in range(bench.GAE_SETS):
        r, d, t, v, b, ln, lo = (torch.as_tensor(x).cuda() for x in (rews, dones, trunc, values, boot, lpn, lpo))
        vt, adv, ret = (torch.empty(n, device="cuda") for _ in range(3))
        keep = (r, d, t, v, b, ln, lo, vt, adv, ret)
        legs["boot"].append(lambda k=keep: N.check(L.rlppo_gae_boot(st, P(k[0]), P(k[1]), P(k[2]), P(k[3]), P(k[4]), n, 0.99, 0.95, 1.7,
                                                                    P(k[7]), P(k[8]), P(k[9]), P(ws), ws.numel())))
        legs["vtrace"].append(lambda k=keep: N.check(L.rlppo_gae_vtrace(st, P(k[0]), P(k[1]), P(k[2]), P(k[3]), P(k[4]), None, P(k[5]), P(k[6]), n,
                                                                        0.99, 0.95, 1.0, 1.0, 1.7, P(k[7]), P(k[8]), P(ws), ws.numel())))
    out = alternate(legs, rounds)
    assert bool(torch.isfinite(keep[8]).all()) and int(ws[4:8].view(torch.int32).item()) == 0
    compare(out, "vtrace", "boot")
    out["unit"] = "us per cold scan of %d steps (rotation over %d buffer sets, HIP events)" % (n, bench.GAE_SETS)
    out["algorithmic_bytes"] = {"boot": 32 * n, "vtrace": 36 * n}
    return out


def recompute_leg(rounds):
    from rlgym_ppo_amd import Learner
    with contextlib.redirect_stdout(sys.stderr):
        learner = Learner(bench.BenchVectorEnv, vector_env=True, n_proc=1, timestep_limit=10**9, exp_buffer_size=150_000, ts_per_iteration=50_000,
                          ppo_epochs=10, ppo_batch_size=50_000, ppo_minibatch_size=50_000, policy_layer_sizes=bench.HID,
                          critic_layer_sizes=bench.HID, checkpoints_save_folder=None, checkpoint_load_folder=None, save_every_ts=10**12,
                          log_to_wandb=False, random_seed=123, gae_vtrace=True)
    res = {"recompute": [], "learn": []}
    try:
        learner.ppo_learner.policy.noise_mode = "device"
        with contextlib.redirect_stdout(sys.stderr):
            for _ in range(4):   # fill the ring and wrap it
                exp, _, n, _ = learner.agent.collect_timesteps(50_000)
                learner.add_new_experience(exp)
        last = learner.ppo_learner.value_net.forward_padded(learner.agent.value_input_rows)[n:]
        for r in range(rounds + 1):
            for name in res:
                torch.cuda.synchronize()
                t = time.perf_counter()
                if name == "recompute":
                    learner._recompute_buffer_targets(last, None, None)
                else:
                    with contextlib.redirect_stdout(sys.stderr):
                        learner.ppo_learner.learn(learner.experience_buffer)
                torch.cuda.synchronize()
                if r:
                    res[name].append((time.perf_counter() - t) * 1e3)
    finally:
        learner.agent.cleanup()
    out = {k: summary(v) for k, v in res.items()}
    out["recompute_share_of_learn"] = round(out["recompute"]["median"] / out["learn"]["median"], 4)
    out["unit"] = "ms, host clock around a device synchronise; buffer of %d rows, learn = 10 epochs x 3 batches of 50,000" % len(learner.experience_buffer)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}
    record["scan_us"] = scan_leg(a.rounds)
    print("scan:", json.dumps(record["scan_us"]), flush=True)
    torch.cuda.empty_cache()
    record["recompute_ms"] = recompute_leg(a.rounds)
    print("recompute:", json.dumps(record["recompute_ms"]), flush=True)
    torch.cuda.empty_cache()
    if a.parent:
        record["bench_headline"] = bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
