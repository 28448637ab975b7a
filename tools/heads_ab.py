"""A/B of the policy-head kernels (csrc/heads.hip) of this tree's library against another build of it -- the parent commit's, built
from a scratch checkout (`git worktree add ../parent HEAD~1 && make -C ../parent/rlgym_ppo_amd/csrc`) and copied to build/variants/.
RLPPO_LIB selects the library; every GPU step is a fresh process under its own time limit, the two libraries alternate, and the first
non-zero exit status ends the run.
  * dump:  a fixed, seeded call of every head entry point (rlppo_discrete_act with and without a mask, rlppo_discrete_probs with and
           without, rlppo_categorical_select, each at 90 / 300 / 1500 actions = 2 / 8 / 32 elements per lane; rlppo_gaussian_act at
           k = 8 and 40; rlppo_multidiscrete_act and _act_nvec) and one rlppo_ppo_minibatch / _nvec pass per head and discrete width
           class, masked and unmasked, plain and with normalised advantages + value clipping + armed KL slots -- every output as .npy
           (actions, log-probabilities, probabilities, the gradient arena, the statistics, the KL slots), compared byte for byte;
  * legs:  ms per 65,536-row pass (256x3 nets: discrete 90 actions unmasked / masked, gaussian, multi-discrete fixed / general) and
           per 4096-row act call of each head (the discrete one as the layer chain: its one-launch form is csrc/fused_act.hip);
  * bench: `bench.py --gpus 1 --steps 20 --warmup 5` per library (bench.py and the Python package are the same in both trees): the
           headline, and the first round's --dump-outputs compared byte for byte.
A leg passes if its min .. max range overlaps the parent's, or its median is within the parent's own spread of the parent's median.
usage: python tools/heads_ab.py --parent-lib build/variants/librlppo_parent.so [--parts dump,legs,bench] [--rounds 7] [--out FILE.json]
       (an existing FILE.json is updated part by part, so the parts may run in separate sessions)"""
import argparse
import contextlib
import ctypes
import filecmp
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OBS, HID, MB = 107, (256, 256, 256), 65536
WIDTHS = (90, 300, 1500)
CLIP, ENT = 0.2, 0.005


# ------------------------------------------------------------------------------------------------ the child: one library, one process
def observations(n, seed):
    return np.clip(np.random.RandomState(seed).randn(n, OBS), -5, 5).astype(np.float32)


def masks(n, A, seed):
    """~2/3 valid, every row at least one valid action except row 5 (no valid action: all-valid), on the device (no host check)."""
    import torch
    rs = np.random.RandomState(seed)
    m = rs.rand(n, A) < 0.66
    m[np.arange(n), rs.randint(0, A, n)] = True
    m[5] = False
    return m, torch.from_numpy(m).cuda()


def learner_and_buffer(policy_type, act_space, n, seed, masked=False, hidden=HID):
    """A PPOLearner whose one minibatch is the whole n-row buffer; actions and old log-probabilities are the policy's own draws (+ 0.1 N(0, 1))."""
    import torch
    from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(sys.stderr):
        learner = PPOLearner(OBS, act_space, policy_type, hidden, hidden, (0.1, 1.0), n, 1, 3e-4, 3e-4, CLIP, ENT, n, "cuda:0")
    rs = np.random.RandomState(seed)
    obs = observations(n, seed)
    m = masks(n, act_space, seed)[1] if masked else None
    act, logp = learner.policy.get_action(obs, action_mask=m) if masked else learner.policy.get_action(obs)
    act = np.asarray(torch.as_tensor(act).cpu(), np.float32).reshape(n, -1)
    old = (np.asarray(torch.as_tensor(logp).cpu(), np.float32).reshape(n) + 0.1 * rs.randn(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    buf = ExperienceBuffer(n, seed, "cpu")
    more = dict(action_masks=m) if masked else {}
    buf.submit_experience(obs, act[:, 0] if policy_type == 0 else act, old, z, obs[:1].repeat(n, 0), z, z, rs.randn(n).astype(np.float32),
                          rs.randn(n).astype(np.float32), **more)
    return learner, buf


def pass_fn(learner, buf, mb, options=None):
    """-> (fn running one pass of mb rows and joining its streams, the option state to keep alive)."""
    import torch
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.engine import stream_ptr
    args = learner._minibatch_args(buf)
    idx = torch.from_numpy(np.random.RandomState(3).permutation(len(buf))[:mb]).cuda().contiguous()
    args.idx, args.mb, args.mb_ratio = idx.data_ptr(), mb, 1.0
    keep = [args, idx]
    if options:  # normalised advantages, value clipping, armed KL slots (never stopping)
        adv = torch.tensor([0.05, 0.9], device="cuda")
        kl = torch.zeros(int(N.lib().rlppo_kl_slots_doubles(mb)), dtype=torch.float64, device="cuda")
        stop = torch.zeros(4, dtype=torch.int32, device="cuda")
        args.adv_norm, args.value_clip, args.kl_slots, args.stop_word = adv.data_ptr(), 0.2, kl.data_ptr(), stop.data_ptr()
        keep += [adv, kl, stop]

    def fn():
        N.check(learner._pass(stream_ptr(), args))
        N.check(N.lib().rlppo_ppo_join(stream_ptr()))
    return fn, keep


def act_fn(pol, n, seed, words=None, probs=None):
    """-> (fn running the policy's rollout call on n staged rows with fixed noise, (actions, log-probabilities[, probabilities]))."""
    import torch
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.engine import ptr, stream_ptr
    a = pol.arena
    rows = a.stage_obs(observations(n, seed))
    shape = pol._noise_shape(n)
    g = torch.Generator().manual_seed(seed)
    noise = (torch.empty(shape).normal_(0, 1, generator=g) if hasattr(pol, "affine_map") else torch.empty(shape).exponential_(1, generator=g)).cuda()
    actions, logp, ws = pol._action_buffer(n).cuda(), torch.empty(n, device="cuda"), a.forward_ws(n)
    a.ensure_packed()
    if words is None and probs is None:
        return (lambda: pol._act_launch(rows, n, noise, actions, logp, ws)), (actions, logp)
    opts = None
    if words is not None:
        opts = N.ActOpts()
        opts.action_mask, opts.mask_words = words.data_ptr(), words.shape[1]
    fn = lambda: N.check(N.lib().rlppo_discrete_act(stream_ptr(), a.dims_c, a.n_layers, ptr(a.packed), ptr(rows), rows.shape[1], n, ptr(noise),
                                                    ptr(actions), ptr(logp), ptr(probs), ptr(ws), ws.numel(),
                                                    ctypes.byref(opts) if opts is not None else None))
    return fn, (actions, logp, probs, noise, rows, opts, words)


def child_dump(out_dir):
    import torch
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.engine import ptr, stream_ptr
    from rlgym_ppo_amd.ppo.continuous_policy import ContinuousPolicy
    from rlgym_ppo_amd.ppo.discrete_policy import DiscreteFF
    from rlgym_ppo_amd.ppo.multi_discrete_policy import MultiDiscreteFF
    from rlgym_ppo_amd.util import action_mask as AM
    os.makedirs(out_dir, exist_ok=True)

    def save(name, *tensors):
        torch.cuda.synchronize()
        for i, t in enumerate(tensors):
            np.save(os.path.join(out_dir, f"{name}.{i}.npy"), t.detach().cpu().numpy())

    n = 777
    for A in WIDTHS:
        torch.manual_seed(A)
        pol = DiscreteFF(OBS, A, (128, 96), "cuda:0")  # (128, 96): the layer chain + the sampling kernel of heads.hip, not the one-launch kernel
        m_dev = masks(n, A, A)[1]
        for tag, m in (("plain", None), ("masked", m_dev)):
            words = None if m is None else AM.pack(m, A, "cuda")
            fn, out = act_fn(pol, n, A, words=words, probs=torch.full((n, A), float("nan"), device="cuda"))
            fn()
            save(f"discrete_act_{A}_{tag}", *out[:3])
            rows = out[4]
            soft = pol._probs(rows, clamp=False, action_mask=m)[0]
            clamped, best = pol._probs(rows, clamp=True, want_argmax=True, action_mask=m)
            save(f"discrete_probs_{A}_{tag}", soft, clamped, best)
            if m is None:
                act, lp = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, device="cuda")
                N.check(N.lib().rlppo_categorical_select(stream_ptr(), ptr(clamped), A, n, A, ptr(out[3]), ptr(act), ptr(lp)))
                save(f"categorical_select_{A}", act, lp)
    for k in (8, 40):
        torch.manual_seed(k)
        fn, out = act_fn(ContinuousPolicy(OBS, 2 * k, HID, "cuda:0"), n, k)
        fn()
        save(f"gaussian_act_{k}", *out)
    for tag, bins, general in (("fixed", None, False), ("general", None, True), ("nvec", [5, 3, 64, 2, 7, 1, 33], False)):
        torch.manual_seed(7)
        pol = MultiDiscreteFF(OBS, HID, "cuda:0", bins=bins)
        pol._force_general = general
        fn, out = act_fn(pol, n, 7)
        fn()
        save(f"multidiscrete_act_{tag}", *out)
    # one pass per head and discrete width class; 4099 rows: a last partial block in every loss grid (16, 4 and 256 rows per block)
    n = 4099
    cases = [(f"discrete_{A}_{tag}", 0, A, masked) for A in WIDTHS for tag, masked in (("plain", False), ("masked", True))]
    cases += [("gaussian_8", 2, 8, False), ("gaussian_40", 2, 40, False), ("multidiscrete_fixed", 1, 8, False),
              ("multidiscrete_general", 1, 8, False), ("multidiscrete_nvec", 1, [5, 3, 64, 2, 7, 1, 33], False)]
    c6 = N.lib().rlppo_dbg_counter(6)
    for name, ptype, space, masked in cases:
        learner, buf = learner_and_buffer(ptype, space, n, 11, masked, hidden=(128, 128))
        if name == "multidiscrete_general":
            learner.policy._force_general = True
        for tag, options in (("plain", False), ("options", True)):
            fn, keep = pass_fn(learner, buf, n, options)
            learner._grad_all.zero_()
            learner._stats.zero_()
            fn()
            save(f"pass_{name}_{tag}", learner._grad_all, learner._stats, *(keep[3:4] if options else ()))
    assert N.lib().rlppo_dbg_counter(6) > c6   # the general multi-discrete kernels really ran
    print(json.dumps({"build_id": N.lib().rlppo_build_id().decode(), "files": len(os.listdir(out_dir))}))


def events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def child_legs():
    import torch
    from rlgym_ppo_amd import _native as N
    res = {}
    N.check(N.lib().rlppo_dbg_set(27, 0))  # the discrete act call as the layer chain (heads.hip's sampling kernel)
    for name, ptype, space, masked, general in (("discrete", 0, 90, False, False), ("discrete_masked", 0, 90, True, False), ("gaussian", 2, 8, False, False),
                                                ("multidiscrete_fixed", 1, 8, False, False), ("multidiscrete_general", 1, 8, False, True)):
        learner, buf = learner_and_buffer(ptype, space, 2 * MB, 1, masked)
        if general:
            learner.policy._force_general = True
        fn, keep = pass_fn(learner, buf, MB)
        res[f"pass_65536_rows_{name}_ms"] = events_ms(fn, 20)
        if not masked:
            fn, keep = act_fn(learner.policy, 4096, 2)
            res[f"act_4096_rows_{name}_ms"] = events_ms(fn, 50)
        del learner, buf, fn, keep
        torch.cuda.empty_cache()
    print(json.dumps({"build_id": N.lib().rlppo_build_id().decode(), "legs": res}))


# ------------------------------------------------------------------------------------------------------------------- the parent
def run(cmd, lib, limit):
    """One GPU step in a fresh process under its own time limit; a non-zero exit status ends the whole run.  -> its last JSON line."""
    env = dict(os.environ)
    env.pop("RLPPO_LIB", None)
    if lib:
        env["RLPPO_LIB"] = lib
    print("+", os.path.basename(lib) if lib else "tree", " ".join(cmd[1:]), flush=True)
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=limit, cwd=ROOT)
    if out.returncode != 0:
        print(out.stdout[-2000:])
        sys.exit(f"heads_ab: exit status {out.returncode}, stopping")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def same_files(a, b):
    """Byte comparison of two dump directories -> (files, the names that differ or are missing on one side)."""
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = [f for f in names if not (os.path.exists(os.path.join(a, f)) and os.path.exists(os.path.join(b, f))
                                    and filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False))]
    return len(names), bad


def verdict(tree, parent):
    """One timing leg (lower is better unless the caller flipped the sign): ranges overlap, or the median within the parent's spread."""
    t, p = np.asarray(tree), np.asarray(parent)
    overlap = t.min() <= p.max() and p.min() <= t.max()
    near = abs(np.median(t) - np.median(p)) <= p.max() - p.min()
    s = lambda v: dict(median=round(float(np.median(v)), 5), min=round(float(v.min()), 5), max=round(float(v.max()), 5), rounds=[round(float(x), 5) for x in v])
    return dict(tree=s(t), parent=s(p), tree_vs_parent=round(float(np.median(t) / np.median(p) - 1.0), 5), ranges_overlap=bool(overlap),
                median_within_parent_spread=bool(near), passes=bool(overlap or near))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parts", default="dump,legs,bench")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "heads_ab"), help="where the dumps go (about 150 MB)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="+", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_dump(a.child[1]) if a.child[0] == "dump" else child_legs()
    parent_lib = os.path.abspath(a.parent_lib)
    libs = (("parent", parent_lib), ("tree", None))
    me = [sys.executable, os.path.abspath(__file__)]
    record = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
    record["unit"] = "ms; a fresh process per library and round, the libraries alternating; median / min / max over the rounds"
    ok = True
    for part in a.parts.split(","):
        if part == "dump":
            ids = {name: run(me + ["--child", "dump", os.path.join(a.work, "dump_" + name)], lib, 600)["build_id"] for name, lib in libs}
            n, bad = same_files(os.path.join(a.work, "dump_tree"), os.path.join(a.work, "dump_parent"))
            record["build_ids"], record["dump"] = ids, dict(files=n, differing=bad, identical=not bad)
            ok &= not bad
        elif part == "legs":
            legs = {}
            for _ in range(a.rounds):
                for name, lib in libs:
                    for k, v in run(me + ["--child", "legs"], lib, 600)["legs"].items():
                        legs.setdefault(k, {}).setdefault(name, []).append(v)
            record["legs"] = {k: verdict(v["tree"], v["parent"]) for k, v in legs.items()}
            record["legs_rounds"] = a.rounds
        elif part == "bench":
            ms = {"parent": [], "tree": []}
            for r in range(a.rounds):
                for name, lib in libs:
                    dump = ["--dump-outputs", os.path.join(a.work, "bench_" + name)] if r == 0 else []
                    ms[name].append(run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"] + dump, lib, 900)["ms_per_step"])
            n, bad = same_files(os.path.join(a.work, "bench_tree"), os.path.join(a.work, "bench_parent"))
            record["bench_ms_per_step"], record["bench_rounds"] = verdict(ms["tree"], ms["parent"]), a.rounds
            record["bench_dump"] = dict(files=n, differing=bad, identical=not bad)
            ok &= not bad
    for k, v in list(record.get("legs", {}).items()) + ([("bench_ms_per_step", record["bench_ms_per_step"])] if "bench_ms_per_step" in record else []):
        print("%-44s tree %9.4f (%.4f .. %.4f)  parent %9.4f (%.4f .. %.4f)  %+.2f %%  %s" % (
            k, v["tree"]["median"], v["tree"]["min"], v["tree"]["max"], v["parent"]["median"], v["parent"]["min"], v["parent"]["max"],
            100 * v["tree_vs_parent"], "passes" if v["passes"] else "FAILS"))
        ok &= v["passes"]
    for k in ("dump", "bench_dump"):
        if k in record:
            print(k, record[k])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
