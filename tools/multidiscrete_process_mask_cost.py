"""What invalid-action masking of the multi-discrete head costs in the small get_action call and in process-mode collection, and that
the unmasked paths cost what they did (the multi-discrete counterpart of tools/process_mask_cost.py):
  (a) MultiDiscreteFF.get_action on 8 and 80 host observations (256x3 policy, bins NVEC of tools/bench_process_multidiscrete_mask_env.py):
      the masked graph call (a random mask, two-thirds valid, every head with a valid bin), the masked eager call
      (policy.act_graphs = False) and the unmasked graph call, alternating round by round;
  (b) process-mode collection, 8 worker processes x 2 agents, on the same synthetic MultiDiscrete environment with and without
      action_masks(), alternating, each in a fresh process;
  (c) (--parent DIR: a built checkout of the parent commit) the unmasked multi-discrete small call and the bench.py headline of this
      tree against the parent's, alternating, each in a fresh process, and bench.py --dump-outputs of the two compared byte for byte.
Medians and spread (min .. max) over the rounds; the record is stamped with rlppo_build_id().
usage: python tools/multidiscrete_process_mask_cost.py [--rounds R] [--collect-rounds R] [--parent DIR] [--bench-rounds R] [--out FILE.json]"""
import argparse
import contextlib
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_process_multidiscrete_mask_env as E  # noqa: E402

OBS, HID = 107, (256, 256, 256)
NVEC, S = list(E.NVEC), E.S
FORMS = ("masked_graph", "masked_eager", "unmasked_graph")


def summary(v):
    med = float(np.median(v))
    return {"median": round(med, 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3),
            "spread": round(float((max(v) - min(v)) / med), 4), "rounds": [round(float(x), 3) for x in v]}


def random_mask(rs, n):
    m = rs.rand(n, S) < 2.0 / 3.0
    s = 0
    for b in NVEC:
        m[np.arange(n), s + rs.randint(0, b, n)] = True
        s += b
    return m


def small_call_leg(rounds, calls=300, forms=FORMS):
    """us per get_action call (median of `calls` calls per round and form, the forms alternating round by round)."""
    from rlgym_ppo_amd.ppo import MultiDiscreteFF
    out = {}
    for n in (8, 80):
        torch.manual_seed(2)
        pol = MultiDiscreteFF(OBS, HID, "cuda:0", bins=NVEC)
        rs = np.random.RandomState(n)
        obs = np.clip(rs.randn(n, OBS), -5, 5).astype(np.float32)
        m = random_mask(rs, n)
        res = {k: [] for k in forms}
        for r in range(rounds + 1):  # (round 0 warms up: graph capture, noise pipeline)
            for name in forms:
                pol.act_graphs = name != "masked_eager"
                kw = {} if name == "unmasked_graph" else dict(action_mask=m)
                ts = []
                for _ in range(calls):
                    t = time.perf_counter()
                    pol.get_action(obs, **kw)
                    ts.append(time.perf_counter() - t)
                if r:
                    res[name].append(1e6 * float(np.median(ts)))
        pol.act_graphs = True
        leg = {k: summary(v) for k, v in res.items()}
        leg["graphs"] = {str(k): dict(calls=g.calls, masked=bool(g.masked), push=bool(g.push), poll_timeouts=g.poll_timeouts)
                         for k, g in pol._graphs.items()}
        if "masked_graph" in leg:
            leg["masked_graph_vs_masked_eager"] = round(leg["masked_graph"]["median"] / leg["masked_eager"]["median"] - 1.0, 4)
            leg["masked_graph_vs_unmasked_graph"] = round(leg["masked_graph"]["median"] / leg["unmasked_graph"]["median"] - 1.0, 4)
        out["n%d" % n] = leg
    out["unit"] = "us per get_action call, host observations, 256x3 policy, bins %s; median of %d calls per round" % (NVEC, calls)
    return out


def collect_once(masked, n_proc=8, timesteps=50_000):
    """One warm and one timed collection in THIS process -> a dict (run in a child: --collect-child)."""
    from rlgym_ppo_amd import Learner
    with contextlib.redirect_stdout(sys.stderr):
        learner = Learner(E.make_masked_env if masked else E.make_env, n_proc=n_proc, min_inference_size=80, timestep_limit=10**9,
                          exp_buffer_size=150_000, ts_per_iteration=timesteps, ppo_epochs=1, ppo_batch_size=50_000, ppo_minibatch_size=50_000,
                          policy_layer_sizes=HID, critic_layer_sizes=HID, checkpoints_save_folder=None, checkpoint_load_folder=None,
                          save_every_ts=10**12, log_to_wandb=False, random_seed=123, multi_discrete_bins=NVEC)
    try:
        pol, agent = learner.ppo_learner.policy, learner.agent
        agent.collect_timesteps(4_000)
        calls = []
        inner = pol.get_action

        def counted(obs, *a, **k):
            t = time.perf_counter()
            out = inner(obs, *a, **k)
            calls.append((len(obs), time.perf_counter() - t))
            return out
        pol.get_action = counted
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exp, _, n, _ = agent.collect_timesteps(timesteps)
        dt = time.perf_counter() - t0
        secs = np.array([c[1] for c in calls])
        masks = agent.action_mask_rows
        if masked:   # every component of every collected action is valid under the mask it was sampled under
            a = np.asarray(exp[1]).reshape(-1, len(NVEC)).astype(np.int64)
            assert masks is not None and masks.shape == (len(a), S)
            s = 0
            for h, b in enumerate(NVEC):
                assert masks[np.arange(len(a)), s + a[:, h]].all(), h
                s += b
        else:
            assert masks is None
        return dict(steps_per_s=round(n / dt), seconds=round(dt, 3), timesteps=int(n), get_action_calls=len(calls),
                    us_per_get_action_median=round(1e6 * float(np.median(secs)), 1), frac_of_wall_in_get_action=round(float(secs.sum() / dt), 3),
                    collector="C++" if agent._native is not None else "Python",
                    graphs={str(k): g.calls for k, g in pol._graphs.items()})
    finally:
        learner.agent.cleanup()


def child(args, cwd=ROOT, timeout=300):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError("child %s failed (%d): %s" % (args, p.returncode, p.stderr[-2000:]))
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])


def collect_leg(rounds):
    res = {"unmasked": [], "masked": []}
    for _ in range(rounds):
        for name in res:
            res[name].append(child(["--collect-child", name]))
    out = {k: dict(steps_per_s=summary([r["steps_per_s"] for r in v]), us_per_get_action=summary([r["us_per_get_action_median"] for r in v]),
                   last=v[-1]) for k, v in res.items()}
    out["masked_vs_unmasked_steps_per_s"] = round(out["masked"]["steps_per_s"]["median"] / out["unmasked"]["steps_per_s"]["median"] - 1.0, 4)
    out["unit"] = "process-mode collection, 8 worker processes x 2 agents, MultiDiscrete%s, 50,000 timesteps, a fresh process per run, alternating" % (tuple(NVEC),)
    return out


def parent_leg(rounds, bench_rounds, parent):
    """The unmasked multi-discrete small call and the headline of this tree against a built checkout of the parent commit."""
    parent = os.path.abspath(parent)
    trees = {"branch": ROOT, "parent": parent}
    small = {k: [] for k in trees}
    for _ in range(rounds):
        for name, d in trees.items():   # (this file run against the other tree's package: --tree)
            small[name].append(child(["--small-child", "--tree", d]))
    out = {"small_call_unmasked_us": {"n%d" % n: {k: summary([r["n%d" % n] for r in v]) for k, v in small.items()} for n in (8, 80)}}
    res = {k: [] for k in trees}
    dumps = {k: tempfile.mkdtemp(prefix="dump_" + k) for k in trees}
    for r in range(bench_rounds):
        for name, d in trees.items():
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", dumps[name]], cwd=d,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise RuntimeError("bench.py in %s failed (%d): %s" % (d, p.returncode, p.stderr[-2000:]))
            line = [x for x in p.stdout.splitlines() if x.startswith("{") and '"metric"' in x][-1]
            res[name].append(float(json.loads(line)["value"]))
    head = {k: summary(v) for k, v in res.items()}
    head["unit"] = "samples/s, bench.py --gpus 1 --steps 20 --warmup 5, a fresh process per run, alternating"
    head["branch_vs_parent"] = round(head["branch"]["median"] / head["parent"]["median"] - 1.0, 4)
    names = sorted(os.listdir(dumps["branch"]))
    same = names == sorted(os.listdir(dumps["parent"])) and all(
        filecmp.cmp(os.path.join(dumps["branch"], f), os.path.join(dumps["parent"], f), shallow=False) for f in names)
    head["dump_outputs"] = {"files": len(names), "byte_identical": bool(same)}
    out["bench_headline"] = head
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--collect-rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--collect-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--small-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.tree:   # the package of another checkout
        sys.path.insert(0, os.path.abspath(a.tree))
    if a.collect_child:
        print(json.dumps(collect_once(a.collect_child == "masked")))
        return
    if a.small_child:
        leg = small_call_leg(3, forms=("unmasked_graph",))
        print(json.dumps({k: v["unmasked_graph"]["median"] for k, v in leg.items() if k != "unit"}))
        return
    from rlgym_ppo_amd import _native as N
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(record, f, indent=1)
    record["get_action_us"] = small_call_leg(a.rounds)
    print("get_action:", json.dumps(record["get_action_us"]), flush=True)
    save()
    torch.cuda.empty_cache()
    record["process_collect"] = collect_leg(a.collect_rounds)
    print("process_collect:", json.dumps(record["process_collect"]), flush=True)
    save()
    if a.parent:
        record["against_parent"] = parent_leg(a.rounds, a.bench_rounds, a.parent)
        print("against the parent:", json.dumps(record["against_parent"]), flush=True)
        save()


if __name__ == "__main__":
    main()
