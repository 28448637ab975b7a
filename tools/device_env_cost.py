"""What the device interface of VectorAgentManager costs and saves, on ONE build, alternating rounds:
  * a collect of tests/device_vector_env.py::IntegerEnv at 4096 agents x 128 steps (256 x 3 networks, 90 actions, device-drawn
    noise) through the device interface (torch backend: the _DeviceEnv side of VectorAgentManager's collect loop) and through the host
    interface (numpy backend: the _HostEnv side), both with the one-launch DiscreteFF.step: collect time, steps/s, and the host time per step (device interface: the host's enqueue time before its one
    read, over the steps; host interface: the collect time over the steps -- its host waits for every step);
  * rlppo_rollout_record alone at 4096 agents, nobody ending and everybody ending (HIP events);
  * the end-of-collect transposition: rlppo_rollout_to_trajectory_major against the torch copies the host side made before it;
  * the extra dense value pass of gae_bootstrap_truncated (all N next-state rows) against the 4096 rows of the flush;
  * (--parent DIR: a built checkout of the parent commit) the bench.py headline of this tree against the parent's and a byte
    comparison of `bench.py --dump-outputs` (tools/gae_bootstrap_cost.py::bench_leg).
Medians and spread ((max - min) / median) over the rounds; the record is stamped with rlppo_build_id().
usage: python tools/device_env_cost.py [--rounds R] [--parent DIR] [--bench-rounds R] [--out profiles/device_env_cost.json]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
import device_vector_env as E  # noqa: E402
from gae_bootstrap_cost import bench_leg, compare, summary  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402

NA, T, D, A, HID = 4096, 128, 107, 90, (256, 256, 256)
DEV = "cuda:0"
P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
ST = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def collect_leg(rounds):
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    from rlgym_ppo_amd.ppo import DiscreteFF
    mgrs = {}
    for side in ("device", "host"):
        torch.manual_seed(1)
        pol = DiscreteFF(D, A, HID, DEV)
        pol.noise_mode = "device"
        mgr = VectorAgentManager(pol, seed=5, standardize_obs=True)
        mgr.init_processes(0, lambda: E.IntegerEnv(n_agents=NA, obs_dim=D, n_actions=A, device=torch.device(DEV) if side == "device" else None))
        mgrs[side] = mgr
    res = {k: [] for k in mgrs}
    enq = []
    for r in range(rounds + 1):   # (round 0 warms up)
        for side, mgr in mgrs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mgr.collect_timesteps(NA * T)
            torch.cuda.synchronize()
            if r:
                res[side].append((time.perf_counter() - t0) * 1e3)
                if side == "device":
                    enq.append(mgr.last_enqueue_seconds * 1e6 / T)
    out = {k: summary(v) for k, v in res.items()}
    compare(out, "device", "host")
    for k in res:
        out[k]["steps_per_second"] = round(NA * T / (out[k]["median"] * 1e-3))
    out["host_us_per_step"] = {"device_interface_enqueue": summary(enq), "host_interface": round(out["host"]["median"] * 1e3 / T, 1)}
    out["unit"] = "ms per collect of %d agents x %d steps (host clock around a device synchronise), device-drawn noise" % (NA, T)
    for mgr in mgrs.values():
        mgr.cleanup()
    return out


def record_leg(rounds):
    L = N.lib()
    rs = np.random.RandomState(0)
    r = torch.from_numpy(rs.randn(NA).astype(np.float32)).to(DEV)
    zeros, ones = torch.zeros(NA, device=DEV), torch.ones(NA, device=DEV)
    rdt = torch.empty((3, T, NA), device=DEV)
    ep, state = torch.zeros(NA, dtype=torch.float64, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    legs = {"nobody_ends": lambda: N.check(L.rlppo_rollout_record(ST(), P(r), 0, P(zeros), 0, P(zeros), 0, NA, 5, T, P(rdt), P(ep), P(state), P(None))),
            "everybody_ends": lambda: N.check(L.rlppo_rollout_record(ST(), P(r), 0, P(ones), 0, P(zeros), 0, NA, 5, T, P(rdt), P(ep), P(state), P(None)))}
    res = {k: [] for k in legs}
    bench.time_region(legs["nobody_ends"], 50, warm_s=0.3)
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(bench.time_region(fn, 200) * 1e3)
    out = {k: summary(v) for k, v in res.items()}
    out["unit"] = "us per rlppo_rollout_record launch at %d agents, back to back (HIP events over 200 launches)" % NA
    return out


def transpose_leg(rounds):
    L = N.lib()
    ld = int(L.rlppo_padded_width(D))
    N_ = NA * T
    S = torch.randn((T + 1, NA, ld), device=DEV)
    acts, logp, rdt = torch.randn((T, NA, 1), device=DEV), torch.randn((T, NA), device=DEV), torch.randn((3, T, NA), device=DEV)
    flat, nxt = torch.empty((N_ + 1, ld), device=DEV), torch.empty((N_, ld), device=DEV)
    a_o, small = torch.empty((N_, 1), device=DEV), torch.empty((4, N_), device=DEV)

    def fused():
        N.check(L.rlppo_rollout_to_trajectory_major(ST(), P(S), P(acts), P(logp), P(rdt), NA, T, ld, 1, P(None), P(None), P(flat), P(nxt), P(a_o),
                                                    P(small[0]), P(small[1]), P(small[2]), P(small[3])))

    def copies():   # the host side's former end of a collect, with the flags already on the device
        flat[:N_].view(NA, T, ld).copy_(S[:T].transpose(0, 1))
        nxt.view(NA, T, ld).copy_(S[1:].transpose(0, 1))
        flat[N_].copy_(S[T][NA - 1])
        return acts.view(T, NA).t().reshape(N_, 1), logp.t().reshape(N_), rdt.transpose(1, 2).contiguous()
    fused()
    want = (flat.clone(), nxt.clone())
    flat.zero_(), nxt.zero_()
    copies()
    assert torch.equal(flat, want[0]) and torch.equal(nxt, want[1])
    legs = {"fused_launch": fused, "torch_copies": copies}
    res = {k: [] for k in legs}
    bench.time_region(fused, 5, warm_s=0.3)
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(bench.time_region(fn, 10) * 1e3)
    out = {k: summary(v) for k, v in res.items()}
    compare(out, "fused_launch", "torch_copies")
    moved = (2 * (T + 1) * NA * ld + 2 * N_ * ld) * 4
    out["unit"] = "us per end-of-collect transposition, %d agents x %d steps x %d floats (HIP events over 10)" % (NA, T, ld)
    out["bytes_fused"] = ((T + 1) * NA * ld + (2 * N_ + 1) * ld) * 4
    out["bytes_copies"] = moved
    return out


def dense_value_leg(rounds):
    from rlgym_ppo_amd.ppo import ValueEstimator
    torch.manual_seed(2)
    vn = ValueEstimator(D, HID, DEV)
    ld = vn.arena.ld_in
    rows = torch.randn((NA * T, ld), device=DEV)
    rows[:, D:] = 0
    legs = {"dense_all_rows": lambda: vn.forward_padded(rows), "flush_rows_only": lambda: vn.forward_padded(rows[:NA])}
    res = {k: [] for k in legs}
    bench.time_region(legs["dense_all_rows"], 3, warm_s=0.3)
    for _ in range(rounds):
        for k, fn in legs.items():
            res[k].append(bench.time_region(fn, 10) * 1e3)
    out = {k: summary(v) for k, v in res.items()}
    out["unit"] = "us per value pass (256 x 3 critic): all %d next-state rows against the %d rows of the flush" % (NA * T, NA)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}
    for name, leg in (("collect_ms", collect_leg), ("record_kernel_us", record_leg), ("transposition_us", transpose_leg),
                      ("bootstrap_value_pass_us", dense_value_leg)):
        record[name] = leg(a.rounds)
        print(name + ":", json.dumps(record[name]), flush=True)
        torch.cuda.empty_cache()
    if a.parent:
        record["bench_headline"] = bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
