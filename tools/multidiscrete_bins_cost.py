"""What the general multi-discrete kernels (any nvec) cost against the fixed ones on the bins both can run, the reference's
[3, 3, 3, 3, 3, 2, 2, 2]: a policy with `_force_general` set takes the general kernels there (rlppo_multidiscrete_act_nvec,
rlppo_ppo_minibatch_nvec).  Fixed and general alternate inside every round of one process; medians over the rounds with their spread.
  * pass:    one rlppo_ppo_minibatch pass of 65,536 rows (256x3 nets) -- the two forms differ in the loss launch alone, so the
             difference of the two pass times is the difference of the two loss launches;
  * act:     the 4096-row rollout call (forward chain + sampling launch; the difference is the sampling launch's);
  * learn:   PPOLearner.learn() of policy_type 1, buffer 131,072, B = 131,072, MB = 65,536, 2 epochs.
usage: python tools/multidiscrete_bins_cost.py [--rounds R] [--out FILE.json]"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlgym_ppo_amd import _native as N  # noqa: E402
from rlgym_ppo_amd.engine import stream_ptr  # noqa: E402
from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner  # noqa: E402

OBS, HID, MB = 107, (256, 256, 256), 65536
FORMS = (("fixed", False), ("general", True))


def workload(n, B, epochs):
    rs = np.random.RandomState(1)
    obs = np.clip(rs.randn(n, OBS), -5, 5).astype(np.float32)
    z = np.zeros(n, np.float32)
    torch.manual_seed(1)
    with contextlib.redirect_stdout(sys.stderr):
        learner = PPOLearner(OBS, 8, 1, HID, HID, (0.1, 1.0), B, epochs, 3e-4, 3e-4, 0.2, 0.005, MB, "cuda:0")
    act = np.stack([rs.randint(0, b, n) for b in learner.policy.splits], 1).astype(np.float32)
    buf = ExperienceBuffer(n, 1, "cpu")
    buf.submit_experience(obs, act, (-7.5 + 0.1 * rs.randn(n)).astype(np.float32), z, obs[:1].repeat(n, 0), z, z, rs.randn(n).astype(np.float32),
                          rs.randn(n).astype(np.float32))
    return learner, buf


def events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def pass_fn(learner, buf):
    args = learner._minibatch_args(buf)
    idx = torch.randperm(len(buf), device="cuda")[:MB].contiguous()
    args.idx, args.mb, args.mb_ratio = idx.data_ptr(), MB, 1.0
    keep = (args, idx)
    return lambda: N.check(learner._pass(stream_ptr(), keep[0]))


def act_fn(pol, n=4096):
    a = pol.arena
    rows = a.stage_obs(np.clip(np.random.RandomState(2).randn(n, OBS), -5, 5).astype(np.float32))
    q = torch.empty(pol._noise_shape(n), device="cuda").exponential_(1)
    actions, logp, ws = torch.empty((n, pol.n_heads), dtype=torch.int64, device="cuda"), torch.empty(n, device="cuda"), a.forward_ws(n)
    a.ensure_packed()
    return lambda: pol._act_launch(rows, n, q, actions, logp, ws)


def learn_ms(learner, buf, reps):
    learner.learn(buf)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        learner.learn(buf)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def summary(res):
    out = {}
    for name, v in res.items():
        out[name] = {"median": round(float(np.median(v)), 5), "min": round(float(min(v)), 5), "max": round(float(max(v)), 5),
                     "rounds": [round(x, 5) for x in v]}
    out["general_minus_fixed"] = round(out["general"]["median"] - out["fixed"]["median"], 5)
    out["general_vs_fixed"] = round(out["general"]["median"] / out["fixed"]["median"] - 1.0, 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    learner, buf = workload(2 * MB, 2 * MB, 2)
    pol = learner.policy
    legs = {"pass_65536_rows_ms": {k: [] for k, _ in FORMS}, "act_4096_rows_ms": {k: [] for k, _ in FORMS},
            "learn_131072_rows_2_epochs_ms": {k: [] for k, _ in FORMS}}
    c6 = N.lib().rlppo_dbg_counter(6)
    for _ in range(a.rounds):
        for name, general in FORMS:
            pol._force_general = general
            legs["pass_65536_rows_ms"][name].append(events_ms(pass_fn(learner, buf), 20))
            learner._grad_all.zero_()
            learner._stats.zero_()
            legs["act_4096_rows_ms"][name].append(events_ms(act_fn(pol), 50))
            legs["learn_131072_rows_2_epochs_ms"][name].append(learn_ms(learner, buf, 3))
    pol._force_general = False
    assert N.lib().rlppo_dbg_counter(6) > c6   # the general kernels really ran
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "bins": list(pol.splits),
              "unit": "ms; fixed and general alternate in every round of one process, median / min / max over the rounds",
              "rounds": a.rounds, "legs": {k: summary(v) for k, v in legs.items()}}
    for k, v in record["legs"].items():
        print("%-32s fixed %9.4f  general %9.4f  (%+.4f ms, %+.2f %%)  spread fixed %.4f..%.4f general %.4f..%.4f" % (
            k, v["fixed"]["median"], v["general"]["median"], v["general_minus_fixed"], 100 * v["general_vs_fixed"], v["fixed"]["min"],
            v["fixed"]["max"], v["general"]["min"], v["general"]["max"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
