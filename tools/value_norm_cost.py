"""What value normalisation (Learner(ppo_normalize_value=True), include/rlppo.h "[vnorm]") costs, on ONE build in one session,
alternating:
  * the 8192 x 256 GAE scan, COLD (rotating over bench.GAE_SETS buffer sets: every scan streams from HBM): rlppo_gae beside
    rlppo_gae_norm with a value_scale, and rlppo_gae_boot (one truncated step per 256) beside rlppo_gae_norm with boot values and a
    value_scale -- next to the bootstrap form's recorded cost (profiles/gae_bootstrap_cost.json), the yardstick for concern;
  * rlppo_value_norm_update at 524,288 targets, cold (one target array per buffer set);
  * one 65,536-row fp32 pass of the update at the flagship shape (obs 107, 256 x 3, 90 discrete actions) through
    rlppo_ppo_minibatch_vnorm with and without a scale (without: rlppo_ppo_minibatch_critic's path);
  * (--parent DIR: a built checkout of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5` of this tree against the
    parent's, alternating, each in a fresh process; both result lines of the last round are recorded.
Medians and spread ((max - min) / median) over the rounds; the record is stamped with rlppo_build_id().  No target is fixed in advance.
usage: python tools/value_norm_cost.py [--rounds R] [--parent DIR] [--bench-rounds R] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402
from tools import diag_gaussian_cost as DC  # noqa: E402
from tools import gae_bootstrap_cost as GC  # noqa: E402

P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
OBS, HIDDEN, A = 107, (256, 256, 256), 90
SCALE = [-212.7, 1.0 / 37.3, 37.3, 0.0]


def scan_leg(rounds):
    L = N.lib()
    out = {"unit": "us per cold scan of 8192 x 256 steps (rotation over %d buffer sets, %d scans per measurement, HIP events)"
                   % (bench.GAE_SETS, GC.CYCLES * bench.GAE_SETS)}
    rews, _, _, values = bench.gae_inputs()
    n = rews.shape[0]
    dones, trunc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    trunc[255::256] = 1.0
    boot = np.full(n, np.nan, np.float32)
    boot[255::256] = np.random.RandomState(256).randn(n // 256).astype(np.float32)
    plain, booted, sets, _ = GC.scan_sets((rews, dones, trunc, values), boot)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    scale = torch.tensor(SCALE, dtype=torch.float32, device="cuda")

    def normed(with_boot):
        fns = []
        for ins, outs, b in sets:
            head = [P(t) for t in ins] + [P(b) if with_boot else None, P(scale)]
            tail = [n, 0.99, 0.95, float(np.float32(1.7))] + [P(t) for t in outs + [ws]] + [ws.numel()]
            fns.append(lambda head=head, tail=tail: N.check(L.rlppo_gae_norm(st, *head, *tail)))
        return fns
    legs = {"plain": plain(L), "norm": normed(False), "boot": booted(), "boot_norm": normed(True)}
    res = GC.alternate(legs, rounds)
    assert all(bool(torch.isfinite(t).all()) for t in sets[0][1])
    GC.compare(res, "norm", "plain")
    GC.compare(res, "boot", "plain")
    GC.compare(res, "boot_norm", "boot")
    GC.compare(res, "boot_norm", "plain")
    out.update(res)
    out["truncated_steps"] = n // 256
    recorded = os.path.join(ROOT, "profiles", "gae_bootstrap_cost.json")
    if os.path.exists(recorded):
        with open(recorded) as f:
            out["bootstrap_form_recorded_boot_vs_plain"] = json.load(f)["scan_us"]["one_truncated_per_256"]["boot_vs_plain"]
    del legs, sets
    torch.cuda.empty_cache()
    return out


def update_leg(rounds, n=524288):
    L = N.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    scale = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device="cuda")
    ws = torch.zeros(N.VALUE_NORM_WS_BYTES, dtype=torch.uint8, device="cuda")
    # (cold: a set of inputs as large as the scan's between two uses of one target array)
    sets = [(40.0 + 25.0 * torch.randn(n, device="cuda"), torch.empty(14 * n, device="cuda")) for _ in range(bench.GAE_SETS)]

    def one(x, filler):
        filler.zero_()   # evicts the targets from the caches; timed apart below and subtracted
        N.check(L.rlppo_value_norm_update(st, P(x), n, P(state), P(scale), P(ws)))
    legs = {"evict_and_update": [lambda x=x, f=f: one(x, f) for x, f in sets], "evict_only": [lambda f=f: f.zero_() for _, f in sets],
            "update_warm": [lambda x=sets[0][0]: N.check(L.rlppo_value_norm_update(st, P(x), n, P(state), P(scale), P(ws)))] * bench.GAE_SETS}
    res = GC.alternate(legs, rounds)
    res["update_cold_median"] = round(res["evict_and_update"]["median"] - res["evict_only"]["median"], 4)
    res["unit"] = "us per call at %d targets (HIP events; cold = behind a %d MB fill that evicts them, the fill's own time subtracted)" % (n, 14 * n * 4 // 10 ** 6)
    assert float(state[0].item()) > 0 and float(state[3].item()) == 0.0
    del legs, sets
    torch.cuda.empty_cache()
    return res


def pass_leg(rounds, mb=65536, reps=20):
    L = N.lib()
    n_buf = 2 * mb
    rs = np.random.RandomState(0)
    pol, val = DC.Net([OBS, *HIDDEN, A]), DC.Net([OBS, *HIDDEN, 1])
    states = torch.zeros(n_buf, pol.ld_in, device="cuda")
    states[:, :OBS] = torch.randn(n_buf, OBS, device="cuda").clamp_(-5, 5)
    acts = torch.randint(0, A, (n_buf,), device="cuda").float()
    old = torch.randn(n_buf, device="cuda") * 0.3 - 4.5
    tgt, adv = 40.0 + 25.0 * torch.randn(n_buf, device="cuda"), torch.randn(n_buf, device="cuda")
    idx = torch.as_tensor(rs.permutation(n_buf)[:mb]).cuda()
    stats = torch.zeros(N.N_STATS, dtype=torch.float64, device="cuda")
    gp, gv = torch.zeros(pol.n, device="cuda"), torch.zeros(val.n, device="cuda")
    ws_bytes = int(L.rlppo_minibatch_workspace_bytes_for(pol.dims_c, pol.nl, val.dims_c, val.nl, mb, N.PRECISION_FP32))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    scale = torch.tensor([38.7, 1.0 / 24.3, 24.3, 0.0], dtype=torch.float32, device="cuda")
    st = DC.bench_stream()
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.precision = N.HEAD_DISCRETE, pol.nl, val.nl, 1, N.PRECISION_FP32
    a.pol_dims = ctypes.cast(pol.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(val.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = pol.packed.data_ptr(), val.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
    a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], n_buf, acts.data_ptr()
    a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idx.data_ptr(), mb
    a.clip_range, a.ent_coef, a.mb_ratio = 0.2, 0.005, 1.0
    a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
    vn = N.ValueNormArg()
    vn.scale = scale.data_ptr()
    legs = {"without": lambda: N.check(L.rlppo_ppo_minibatch_vnorm(st, ctypes.byref(a), None, None, None)),
            "with": lambda: N.check(L.rlppo_ppo_minibatch_vnorm(st, ctypes.byref(a), None, None, ctypes.byref(vn)))}
    o = DC.alternate(legs, rounds, reps)
    o["unit"] = "us per %d-row fp32 pass (device events, %d passes per measurement)" % (mb, reps)
    DC.compare(o, "with", "without")
    return o


def bench_leg(rounds, parent):
    trees = {"branch": ROOT, "parent": os.path.abspath(parent)}
    res, lines = {k: [] for k in trees}, {}
    for r in range(rounds):
        for name, d in trees.items():
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=d, capture_output=True,
                               text=True, timeout=600)
            line = [x for x in p.stdout.splitlines() if x.startswith("{") and '"metric"' in x][-1]
            lines[name] = json.loads(line)
            res[name].append(float(lines[name]["value"]))
    out = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v), "spread": round((max(v) - min(v)) / float(np.median(v)), 4),
               "rounds": v} for k, v in res.items()}
    out["unit"] = "samples/s, bench.py --gpus 1 --steps 20 --warmup 5, a fresh process per run, alternating"
    GC.compare(out, "branch", "parent")
    out["branch_vs_parent_within_2_percent"] = bool(abs(out["branch_vs_parent"]) <= 0.02)
    out["result_lines_last_round"] = lines
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(record, f, indent=1)
    for key, fn in (("scan_us", lambda: scan_leg(a.rounds)), ("value_norm_update_us", lambda: update_leg(a.rounds)),
                    ("pass_us", lambda: pass_leg(a.rounds))):
        record[key] = fn()
        print(key + ":", json.dumps(record[key]), flush=True)
        save()
    torch.cuda.empty_cache()
    if a.parent:
        record["bench_headline"] = bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
        save()


if __name__ == "__main__":
    main()
