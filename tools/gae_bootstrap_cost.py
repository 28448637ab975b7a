"""What bootstrapping truncated trajectories from V(next state) costs, and that the plain paths cost what they did:
  * the 8192 x 256 GAE scan, COLD (rotating over bench.GAE_SETS buffer sets: every scan streams from HBM), alternating in ONE process:
      - rlppo_gae of this tree and (--parent DIR) rlppo_gae of the parent's library, both loaded side by side;
      - rlppo_gae_boot with one truncated step per 256-step trajectory, and with one per 16 steps, each beside rlppo_gae on the same
        flags (boot_values are NaN wherever they are not to be used);
  * Learner.add_new_experience at the headline shape (4096 agents x 128 steps, bench.BenchVectorEnv) with gae_bootstrap_truncated
    off and on, alternating on one collect (the environment never truncates: the m = 4096 flush steps bootstrap from the rows the
    agents act on next);
  * (--parent DIR: a built checkout of the parent commit) the bench.py headline of this tree against the parent's, alternating, each
    in a fresh process, and a byte comparison of what `bench.py --dump-outputs` writes in the two trees.
Medians and spread ((max - min) / median) over the rounds; the record is stamped with rlppo_build_id().
  * (--sparse-lib FILE) beside the two bootstrap scans, the same scans by a build that reads boot_values sparsely, behind the flags.
usage: python tools/gae_bootstrap_cost.py [--rounds R] [--parent DIR] [--sparse-lib FILE] [--bench-rounds R] [--out FILE.json]"""
import argparse
import contextlib
import ctypes
import filecmp
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402

CYCLES = 30   # times through the buffer sets per measurement: 300 scans


def summary(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4),
            "spread": round(float((max(v) - min(v)) / np.median(v)), 4), "rounds": [round(float(x), 4) for x in v]}


def compare(out, a, b):
    """a against b: the relative difference of the medians and whether it lies within the larger of the two measured spreads."""
    diff = out[a]["median"] / out[b]["median"] - 1.0
    out[f"{a}_vs_{b}"] = round(diff, 4)
    out[f"{a}_vs_{b}_within_spread"] = bool(abs(diff) <= max(out[a]["spread"], out[b]["spread"]))


def load_beside(path, names=("rlppo_gae", "rlppo_gae_workspace_bytes", "rlppo_build_id", "rlppo_last_error")):
    """Another build of the library in this process, next to the one the package has loaded."""
    L = ctypes.CDLL(os.path.abspath(path))
    for name in names:
        getattr(L, name).restype, getattr(L, name).argtypes = N.SIGNATURES[name]
    return L


def load_parent(parent):
    return load_beside(os.path.join(parent, "rlgym_ppo_amd", "librlppo.so"))


def scan_sets(host, boot=None):
    """bench.GAE_SETS independent input + output sets in HBM -> {entry: launch closures}, outputs of set 0."""
    L = N.lib()
    rews, dones, trunc, values = host
    n = rews.shape[0]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    sets = []
    for _ in range(bench.GAE_SETS):
        ins = [torch.as_tensor(x).cuda() for x in (rews, dones, trunc, values)]
        outs = [torch.empty(n, device="cuda") for _ in range(3)]
        b = None if boot is None else torch.as_tensor(boot).cuda()
        sets.append((ins, outs, b))
    # (argument lists are built once: a launch closure does nothing but the call)
    args = [([P(t) for t in i], [n, 0.99, 0.95, float(np.float32(1.7))] + [P(t) for t in o + [ws]] + [ws.numel()], None if b is None else P(b))
            for i, o, b in sets]

    def plain(lib):
        return [lambda h=h, t=t: N.check(lib.rlppo_gae(st, *h, *t)) for h, t, _ in args]

    def booted(lib=L):
        return [lambda h=h, t=t, b=b: N.check(lib.rlppo_gae_boot(st, *h, b, *t)) for h, t, b in args]
    return plain, booted, sets, n


def alternate(legs, rounds):
    for fns in legs.values():
        for fn in fns:
            fn()
    bench.time_region(next(iter(legs.values()))[0], 1, warm_s=0.3)   # clock ramp
    res = {k: [] for k in legs}
    for r in range(rounds + 1):  # (round 0 warms up)
        for k, fns in legs.items():
            ms = bench.time_rotating(fns, CYCLES)
            if r:
                res[k].append(ms * 1e3)
    return {k: summary(v) for k, v in res.items()}


def scan_leg(rounds, parent, sparse_lib=None):
    out = {"unit": "us per cold scan of 8192 x 256 steps (rotation over %d buffer sets, %d scans per measurement, HIP events)"
                   % (bench.GAE_SETS, CYCLES * bench.GAE_SETS)}
    host = bench.gae_inputs()
    n = host[0].shape[0]
    # 1. the plain scan, this tree against the parent's library
    plain, _, sets, _ = scan_sets(host)
    legs = {"branch": plain(N.lib())}
    if parent:
        PL = load_parent(parent)
        out["parent_build_id"] = PL.rlppo_build_id().decode()
        legs["parent"] = plain(PL)
    ref = None
    for k, fns in legs.items():   # the two libraries compute the same bits
        fns[0]()
        got = [t.clone() for t in sets[0][1]]
        assert ref is None or all(torch.equal(a, b) for a, b in zip(got, ref)), k
        ref = got
    out["no_bootstrap"] = alternate(legs, rounds)
    if parent:
        compare(out["no_bootstrap"], "branch", "parent")
    del plain, legs, sets
    torch.cuda.empty_cache()
    # 2. the bootstrap form beside the plain scan on the same flags
    for name, every in (("one_truncated_per_256", 256), ("one_truncated_per_16", 16)):
        rews, _, _, values = host
        dones, trunc = np.zeros(n, np.float32), np.zeros(n, np.float32)
        trunc[every - 1::every] = 1.0
        boot = np.full(n, np.nan, np.float32)
        boot[every - 1::every] = np.random.RandomState(every).randn(n // every).astype(np.float32)
        plain, booted, sets, _ = scan_sets((rews, dones, trunc, values), boot)
        legs = {"plain": plain(N.lib()), "boot": booted()}
        if sparse_lib:   # the A/B build that reads boot_values behind the flags, at the truncated steps only (csrc/gae.hip: GAE_BOOT_DENSE_V)
            DL = load_beside(sparse_lib, ("rlppo_gae_boot", "rlppo_last_error"))
            booted()[0]()
            want = [t.clone() for t in sets[0][1]]
            legs["boot_sparse"] = booted(DL)
            legs["boot_sparse"][0]()
            assert all(torch.equal(a, b) for a, b in zip(sets[0][1], want)), "the sparse build computes other bits"
        res = alternate(legs, rounds)
        assert all(bool(torch.isfinite(t).all()) for t in sets[0][1])
        compare(res, "boot", "plain")
        if sparse_lib:
            compare(res, "boot_sparse", "plain")
            res["algorithmic_bytes_sparse"] = 28 * n + 32 * (n // every)   # one 32-byte sector per truncated step
        res["truncated_steps"] = n // every
        res["algorithmic_bytes"] = {"plain": 28 * n, "boot": 32 * n}
        out[name] = res
        del plain, booted, sets, legs
        torch.cuda.empty_cache()
    return out


def experience_leg(rounds):
    from rlgym_ppo_amd import Learner
    with contextlib.redirect_stdout(sys.stderr):
        learner = Learner(bench.BenchVectorEnv, vector_env=True, n_proc=1, timestep_limit=10**9, exp_buffer_size=bench.N_SAMPLES,
                          ts_per_iteration=bench.N_SAMPLES, ppo_epochs=1, ppo_batch_size=bench.BATCH, ppo_minibatch_size=bench.MINIBATCH,
                          policy_layer_sizes=bench.HID, critic_layer_sizes=bench.HID, checkpoints_save_folder=None,
                          checkpoint_load_folder=None, save_every_ts=10**12, log_to_wandb=False, random_seed=123,
                          gae_bootstrap_truncated=True)
    res = {"off": [], "on": []}
    try:
        learner.ppo_learner.policy.noise_mode = "device"
        exp, _, n, _ = learner.agent.collect_timesteps(bench.N_SAMPLES)
        m = int(learner.agent.bootstrap_steps.size)
        for r in range(rounds + 1):
            for name in res:
                learner.gae_bootstrap_truncated = name == "on"   # (off: the manager's bootstrap rows are simply not looked at)
                torch.cuda.synchronize()
                t = time.perf_counter()
                learner.add_new_experience(exp)
                torch.cuda.synchronize()
                if r:
                    res[name].append((time.perf_counter() - t) * 1e3)
    finally:
        learner.agent.cleanup()
    out = {k: summary(v) for k, v in res.items()}
    compare(out, "on", "off")
    out["unit"] = "ms per add_new_experience of %d steps (value pass + GAE + buffer submit, host clock around a device synchronise)" % n
    out["bootstrapped_steps"] = m
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
    compare(out, "branch", "parent")
    # what the last timed step computed, byte for byte
    with tempfile.TemporaryDirectory() as tmp:
        names = {}
        for name, d in trees.items():
            dump = os.path.join(tmp, name)
            subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", dump], cwd=d,
                           capture_output=True, text=True, timeout=600, check=True)
            names[name] = sorted(os.listdir(dump))
        same = names["branch"] == names["parent"] and len(names["branch"]) > 0 and all(
            filecmp.cmp(os.path.join(tmp, "branch", f), os.path.join(tmp, "parent", f), shallow=False) for f in names["branch"])
    out["dump_outputs"] = {"files": names["branch"], "byte_identical": bool(same)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--sparse-lib", default=None, help="a variant build with -DGAE_BOOT_DENSE_V=0 (make -C rlgym_ppo_amd/csrc variant "
                                                      "NAME=gae_boot_sparse SRC=gae DEFS=-DGAE_BOOT_DENSE_V=0 -> build/variants/)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}
    record["scan_us"] = scan_leg(a.rounds, a.parent, a.sparse_lib)
    print("scan:", json.dumps(record["scan_us"]), flush=True)
    record["add_new_experience_ms"] = experience_leg(a.rounds)
    print("add_new_experience:", json.dumps(record["add_new_experience_ms"]), flush=True)
    torch.cuda.empty_cache()
    if a.parent:
        record["bench_headline"] = bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
