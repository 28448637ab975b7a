"""What invalid-action masking costs on the multi-discrete head's general kernels, on one build: no mask, an all-valid mask and a
60 %-valid mask (every bin valid with probability 0.6, one bin forced valid per head) alternate inside every round of one process;
medians over the rounds with their spread.
  * act:   the 4096-row rollout call (forward chain + sampling launch; the forms differ in the sampling launch alone);
  * pass:  one rlppo_ppo_minibatch_nvec pass of 65,536 rows (256x3 nets; the forms differ in the loss launch alone),
on bins (2, 7, 3, 11, 2) and on the reference's bins [3, 3, 3, 3, 3, 2, 2, 2] (there `no mask` is the general kernels too:
`_force_general`, as tools/multidiscrete_bins_cost.py runs them).
usage: python tools/multidiscrete_mask_cost.py [--rounds R] [--out FILE.json]"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlgym_ppo_amd import _native as N  # noqa: E402
from rlgym_ppo_amd.engine import stream_ptr  # noqa: E402
from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner  # noqa: E402
from rlgym_ppo_amd.util import action_mask as AM  # noqa: E402

OBS, HID, MB, ACT_ROWS = 107, (256, 256, 256), 65536, 4096
FORMS = ("no_mask", "all_valid", "valid_60")
BINS = ((2, 7, 3, 11, 2), (3, 3, 3, 3, 3, 2, 2, 2))


def masks(rs, n, bins):
    """The three forms' masks [n, S] (None: no mask)."""
    S = sum(bins)
    m = rs.rand(n, S) < 0.6
    s = 0
    for b in bins:
        m[np.arange(n), s + rs.randint(0, b, n)] = True
        s += b
    return {"no_mask": None, "all_valid": np.ones((n, S), bool), "valid_60": m}


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


def workload(bins):
    """-> (learner, {form: pass closure}, {form: act closure}, valid fraction of the 60 % masks)."""
    rs = np.random.RandomState(1)
    n = MB
    obs = np.clip(rs.randn(n, OBS), -5, 5).astype(np.float32)
    z = np.zeros(n, np.float32)
    torch.manual_seed(1)
    with contextlib.redirect_stdout(sys.stderr):
        learner = PPOLearner(OBS, list(bins), 1, HID, HID, (0.1, 1.0), n, 1, 3e-4, 3e-4, 0.2, 0.005, MB, "cuda:0")
    pol = learner.policy
    pol._force_general = True   # the reference's bins: the general kernels without a mask too
    mk = masks(rs, n, bins)
    # stored actions valid under the 60 % mask (and so under the others)
    act = np.zeros((n, len(bins)), np.float32)
    s = 0
    for h, b in enumerate(bins):
        sub = mk["valid_60"][:, s:s + b]
        act[:, h] = (sub * rs.rand(n, b)).argmax(1)
        s += b
    old = (-float(np.log(np.asarray(bins, np.float64)).sum()) + 0.1 * rs.randn(n)).astype(np.float32)
    tgt, adv = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    idx = torch.randperm(n, device="cuda").contiguous()
    passes, keep = {}, []
    for form in FORMS:
        buf = ExperienceBuffer(n, 1, "cpu")
        kw = {} if mk[form] is None else dict(action_masks=mk[form])
        buf.submit_experience(obs, act, old, z, obs[:1].repeat(n, 0), z, z, tgt, adv, **kw)
        args = learner._minibatch_args(buf)
        args.idx, args.mb, args.mb_ratio = idx.data_ptr(), MB, 1.0
        keep.append((buf, args))
        passes[form] = (lambda a: lambda: N.check(learner._pass(stream_ptr(), a)))(args)
    a = pol.arena
    rows = a.stage_obs(obs[:ACT_ROWS])
    q = torch.empty(pol._noise_shape(ACT_ROWS), device="cuda").exponential_(1)
    actions = torch.empty((ACT_ROWS, pol.n_heads), dtype=torch.int64, device="cuda")
    logp, ws = torch.empty(ACT_ROWS, device="cuda"), a.forward_ws(ACT_ROWS)
    a.ensure_packed()
    acts = {}
    for form in FORMS:
        words = None if mk[form] is None else AM.pack(mk[form][:ACT_ROWS], sum(bins), "cuda")
        keep.append(words)
        acts[form] = (lambda w: lambda: pol._act_launch(rows, ACT_ROWS, q, actions, logp, ws, mask_words=w))(words)
    return learner, passes, acts, keep, float(mk["valid_60"].mean())


def summary(res):
    out = {}
    for name, v in res.items():
        out[name] = {"median": round(float(np.median(v)), 5), "min": round(float(min(v)), 5), "max": round(float(max(v)), 5),
                     "rounds": [round(x, 5) for x in v]}
    for name in FORMS[1:]:
        out[name + "_vs_no_mask"] = round(out[name]["median"] / out["no_mask"]["median"] - 1.0, 5)
        out[name + "_minus_no_mask_ms"] = round(out[name]["median"] - out["no_mask"]["median"], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds,
              "unit": "ms; the three forms alternate in every round of one process, median / min / max over the rounds", "bins": {}}
    for bins in BINS:
        learner, passes, acts, keep, frac = workload(bins)
        legs = {"act_4096_rows_ms": {k: [] for k in FORMS}, "pass_65536_rows_ms": {k: [] for k in FORMS}}
        c6 = N.lib().rlppo_dbg_counter(6)
        for _ in range(a.rounds):
            for form in FORMS:
                legs["act_4096_rows_ms"][form].append(events_ms(acts[form], 50))
                legs["pass_65536_rows_ms"][form].append(events_ms(passes[form], 20))
                learner._grad_all.zero_()
                learner._stats.zero_()
        assert N.lib().rlppo_dbg_counter(6) > c6   # the general kernels really ran
        rec = {"valid_fraction_of_valid_60": round(frac, 4), "legs": {k: summary(v) for k, v in legs.items()}}
        record["bins"][str(list(bins))] = rec
        for k, v in rec["legs"].items():
            print("%-26s %-20s no mask %9.4f  all-valid %9.4f (%+.2f %%)  60 %%-valid %9.4f (%+.2f %%)  spread no mask %.4f..%.4f" % (
                str(list(bins)), k, v["no_mask"]["median"], v["all_valid"]["median"], 100 * v["all_valid_vs_no_mask"],
                v["valid_60"]["median"], 100 * v["valid_60_vs_no_mask"], v["no_mask"]["min"], v["no_mask"]["max"]), flush=True)
        del learner, passes, acts, keep
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
