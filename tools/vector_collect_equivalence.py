"""Shows that VectorAgentManager's ONE collect loop (collect_timesteps with its environment's and head's sides) computes, byte for
byte, what the three hand-copied step loops it replaced computed, and that no form of it got slower.

    python tools/vector_collect_equivalence.py --parent DIR [--rounds 5] [--no-bench] [--out profiles/vector_collect_refactor.json]

DIR is a built `git worktree` of the parent commit.  The tool reaches the manager through its public surface only
(tests/vector_collect_forms.py), so this one file drives both trees, each in fresh child processes under `timeout`; every exit status
is checked and the first failure ends the run.
  * digest leg: the matrix of tests/test_gpu_vector_collect_forms.py (with the fused-step flip) on the parent and on this tree, one
    sha256 per case over every output of every form; exits non-zero unless every digest is identical;
  * time leg: a collect of tests/device_vector_env.py::IntegerEnv at 4096 agents x 128 steps, obs 107, 256 x 3 networks, 90 actions,
    device-drawn noise (the workload of tools/device_env_cost.py) through four forms -- host step (DiscreteFF.step), host chain (the
    diagonal-Gaussian head, 6 actions), device step, device chain (DiscreteFF without fused_step) -- parent and this tree alternating,
    a fresh process per round: one warm-up collect, then the timed ones; for the device forms `last_enqueue_seconds` as well; and the
    number of host waits torch's sync debug mode counts in one collect.  Verdict per form: this tree's median is no more than the
    parent's median plus the parent's own round-to-round spread (max - min);
  * bench leg: one alternating pair of `bench.py --gpus 1 --steps 20 --warmup 5 --full` lines (headline and the iteration's collect)."""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA, T, D, A, HID = 4096, 128, 107, 90, (256, 256, 256)
DEV = "cuda:0"
TIME_FORMS = ("host_step", "host_chain", "device_step", "device_chain")
BENCH_BOX = 0.02   # the box-to-box spread of the headline that README.md records


# ------------------------------------------------------------------------------------------------ children (one tree each)
def _enter(tree):
    sys.path.insert(0, os.path.join(ROOT, "tests"))   # the environments and the matrix: this tree's, for both
    sys.path.insert(0, os.path.abspath(tree))         # the package under test


def child_digest(tree):
    _enter(tree)
    import vector_collect_forms as F
    out = {}
    for case in F.cases():
        out[F.case_id(case)] = F.digest({F.form_name(s, f): F.run_form(case, s, f) for s, f in F.forms(case["head"])})
    for side in ("host", "device"):
        out[f"flip-{side}-" + F.case_id(F.FLIP_CASE)] = F.digest({"flipped": F.run_form(F.FLIP_CASE, side, True, flip=True)})
    return out


def child_time(tree, collects):
    _enter(tree)
    import torch
    import device_vector_env as E
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    from rlgym_ppo_amd.ppo import DiagGaussianPolicy, DiscreteFF
    out = {}
    for form in TIME_FORMS:
        side, head = form.split("_")
        torch.manual_seed(1)
        if form == "host_chain":
            pol = DiagGaussianPolicy(D, 6, HID, DEV)
        else:
            pol = DiscreteFF(D, A, HID, DEV)
            pol.noise_mode, pol.fused_step = "device", head == "step"
        mgr = VectorAgentManager(pol, seed=5, standardize_obs=True)
        mgr.init_processes(0, lambda: E.IntegerEnv(n_agents=NA, obs_dim=D, n_actions=A, device=torch.device(DEV) if side == "device" else None))
        ms, enq = [], []
        for i in range(collects + 1):   # (collect 0 warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mgr.collect_timesteps(NA * T)
            torch.cuda.synchronize()
            if i:
                ms.append((time.perf_counter() - t0) * 1e3)
                if side == "device":
                    enq.append(mgr.last_enqueue_seconds * 1e3)
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                mgr.collect_timesteps(NA * T)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        out[form] = dict(ms=ms, enqueue_ms=enq, waits=sum("synchroniz" in str(w.message).lower() for w in rec))
        mgr.cleanup()
        del mgr, pol
        torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------ the parent process
def run_child(tree, mode, limit, *extra):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--tree", tree, *extra]
    p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"{mode} child on {tree} ended with status {p.returncode}: stopping")
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])


def run_bench(tree, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"],
                       cwd=tree, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(f"bench.py on {tree} ended with status {p.returncode}: stopping")
    line = json.loads([x for x in p.stdout.splitlines() if x.startswith("{") and '"metric"' in x][-1])
    return dict(value=line["value"], unit=line["unit"], iteration=line.get("iteration"))


def stats(v):
    v = sorted(v)
    mid = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return dict(median=round(mid, 3), min=round(v[0], 3), max=round(v[-1], 3), spread=round(v[-1] - v[0], 3), samples=[round(x, 3) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--collects", type=int, default=2, help="timed collects per form and round")
    ap.add_argument("--no-digest", action="store_true")
    ap.add_argument("--no-time", action="store_true")
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vector_collect_refactor.json"))
    ap.add_argument("--child", choices=("digest", "time"))
    ap.add_argument("--tree")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_digest(a.tree) if a.child == "digest" else child_time(a.tree, a.collects)), flush=True)
        return 0
    if not a.parent:
        ap.error("--parent DIR is required")
    trees = {"parent": os.path.abspath(a.parent), "branch": ROOT}
    record = json.load(open(a.out)) if os.path.exists(a.out) else {}   # (the legs may be run one at a time)
    verdict = record.setdefault("verdict", {})

    def save():
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    if not a.no_digest:
        got = {name: run_child(tree, "digest", 900) for name, tree in trees.items()}
        differing = sorted(k for k in set(got["parent"]) | set(got["branch"]) if got["parent"].get(k) != got["branch"].get(k))
        record["digests"] = dict(cases=len(got["branch"]), sha256=got["branch"], differing={k: [got["parent"].get(k), got["branch"].get(k)] for k in differing})
        verdict["digests_identical"] = not differing and len(got["branch"]) > 0
        print(f"digest leg: {len(got['branch'])} cases, differing: {differing}", flush=True)
        save()
    if not a.no_time:
        raw = {name: {f: dict(ms=[], enqueue_ms=[], waits=[]) for f in TIME_FORMS} for name in trees}
        for r in range(a.rounds):
            for name in (("parent", "branch"), ("branch", "parent"))[r % 2]:   # (who goes first alternates too)
                tree = trees[name]
                one = run_child(tree, "time", 600, "--collects", str(a.collects))
                for f in TIME_FORMS:
                    raw[name][f]["ms"] += one[f]["ms"]
                    raw[name][f]["enqueue_ms"] += one[f]["enqueue_ms"]
                    raw[name][f]["waits"].append(one[f]["waits"])
                print(f"time leg: round {r} {name}: " + ", ".join(f"{f} {min(one[f]['ms']):.1f} ms" for f in TIME_FORMS), flush=True)
        times = {"unit": f"ms per collect of {NA} agents x {T} steps (host clock around a device synchronise); {a.rounds} rounds of {a.collects} "
                         "collects per tree, alternating, a fresh process per round; waits = host synchronisations torch counts in one collect"}
        not_slower, waits_ok = {}, {}
        for f in TIME_FORMS:
            times[f] = {name: dict(collect_ms=stats(raw[name][f]["ms"]), waits_per_collect=max(raw[name][f]["waits"]),
                                   **({"enqueue_ms": stats(raw[name][f]["enqueue_ms"])} if raw[name][f]["enqueue_ms"] else {})) for name in trees}
            p, b = times[f]["parent"], times[f]["branch"]
            not_slower[f] = b["collect_ms"]["median"] <= p["collect_ms"]["median"] + p["collect_ms"]["spread"]
            waits_ok[f] = b["waits_per_collect"] <= (1 if f.startswith("device") else p["waits_per_collect"])
        record["collect_times"] = times
        verdict["not_slower"], verdict["waits_not_more"] = not_slower, waits_ok
        save()
    if not a.no_bench:
        lines = {name: run_bench(tree, 1100) for name, tree in trees.items()}
        record["bench_full"] = lines
        verdict["bench_headline_within_box_spread"] = abs(lines["branch"]["value"] / lines["parent"]["value"] - 1.0) <= BENCH_BOX
        save()
    record["verdict"]["all"] = verdict["all"] = all(v for k, x in verdict.items() if k != "all" for v in (x.values() if isinstance(x, dict) else [x]))
    save()
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["all"] and verdict.get("digests_identical", True) else 1


if __name__ == "__main__":
    sys.exit(main())
