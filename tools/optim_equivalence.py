"""Shows that the parameter-side kernels after the split of csrc/optim.hip (pack.hip, rows.hip, optim.hip, stats.hip over reduce.hpp)
compute, bit for bit, what the one file computed, and that nothing got slower.

    python tools/optim_equivalence.py --parent-lib build/parent/rlgym_ppo_amd/librlppo.so [--legs digest,ab,share8,costs] [--rounds 5]
                                      [--out profiles/optim_refactor.json] [--golden tests/golden/optim_forms_sha256.json]

Only the library changed, so this tree's Python drives both: every run is a fresh child process under `timeout`, with RLPPO_LIB set
to the parent's library (built from a `git worktree` of the parent commit) or unset for this tree's.  Every exit status is checked and
the first failure ends the run.
  * digest leg: the matrix of tests/optim_forms.py, one sha256 per case over every output buffer -- on the parent TWICE (a case on
    which it does not agree with itself is reported by name and dropped; only the three-operation pair form may be), then on this
    tree.  Exits non-zero unless every remaining digest is identical.  --golden writes the parent's digests where
    tests/test_gpu_optim_forms.py reads them.
  * ab / share8 legs: tools/ab_lib.py against the parent's library, the headline / the 8-rank share, alternating processes.
  * costs leg: tools/ppo_options_cost.py, tools/value_norm_cost.py and tools/lr_schedule_cost.py, alternating processes in the same
    way (a round = one process per library, its figures = that process's medians).
Verdict per timed figure: this tree's median is no more than the parent's median plus the parent's own round-to-round spread
(max - min)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COST_TOOLS = ("ppo_options_cost", "value_norm_cost", "lr_schedule_cost")


def child_digest():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import optim_forms as F
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    return {"lib": N.LIB_PATH, "build_id": L.rlppo_build_id().decode(), "sha256": {c: F.run_case(L, c) for c in F.case_ids()}}


def run(cmd, limit, parent_lib=None, echo=False):
    """One child under its own time limit -> its stdout (echo: passed on line by line as it comes); any non-zero status ends the
    whole run."""
    env = {k: v for k, v in os.environ.items() if k != "RLPPO_LIB"}
    if parent_lib:
        env["RLPPO_LIB"] = parent_lib
    p = subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, *cmd], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE if not echo else None, text=True)
    if echo:
        lines = []
        for line in p.stdout:
            lines.append(line)
            print("  | " + line, end="", flush=True)
        p.wait()
        p = subprocess.CompletedProcess(p.args, p.returncode, "".join(lines), "")
    else:
        out, err = p.communicate()
        p = subprocess.CompletedProcess(p.args, p.returncode, out, err)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit(f"{' '.join(cmd)} ({'parent' if parent_lib else 'branch'}) ended with status {p.returncode}: stopping")
    return p.stdout


def stats(v):
    s = sorted(v)
    mid = s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])
    return dict(median=round(mid, 4), spread=round(s[-1] - s[0], 4), samples=[round(x, 4) for x in v])


def figures(node, path=""):
    """The timed figures of a cost tool's record: every dict that carries its rounds, or a median with its min and max."""
    if isinstance(node, dict):
        rounds = next((node[k] for k in ("rounds_ms", "rounds_us", "rounds") if isinstance(node.get(k), list) and node[k]), None)
        if rounds is not None and all(isinstance(x, (int, float)) for x in rounds):
            yield path, stats(rounds)
        elif all(isinstance(node.get(k), (int, float)) for k in ("median", "min", "max")):
            yield path, dict(median=node["median"], spread=round(node["max"] - node["min"], 4))
        else:
            for k, v in node.items():
                yield from figures(v, f"{path}/{k}" if path else k)


def not_slower(parent, branch):
    return branch["median"] <= parent["median"] + parent["spread"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="librlppo.so of a built worktree of the parent commit")
    ap.add_argument("--legs", default="digest,ab,share8,costs")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of fresh processes per library")
    ap.add_argument("--inner-rounds", type=int, default=3, help="--rounds of a cost tool inside one process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_refactor.json"))
    ap.add_argument("--golden", default=None, help="write the parent's digests to this file")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child_digest()), flush=True)
        return 0
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        ap.error("--parent-lib: the parent's librlppo.so is required")
    parent = os.path.abspath(a.parent_lib)
    legs = a.legs.split(",")
    record = json.load(open(a.out)) if os.path.exists(a.out) else {}   # (the legs may be run one at a time)
    verdict = record.setdefault("verdict", {})
    me = os.path.abspath(__file__)

    def save():
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")

    if "digest" in legs:
        last = lambda out: json.loads([x for x in out.splitlines() if x.startswith("{")][-1])
        p1, p2, br = last(run([me, "--child"], 300, parent)), last(run([me, "--child"], 300, parent)), last(run([me, "--child"], 300))
        assert p1["lib"] == parent and br["lib"] != parent, (p1["lib"], br["lib"])
        dropped = sorted(c for c in p1["sha256"] if p1["sha256"][c] != p2["sha256"][c])
        kept = [c for c in sorted(p1["sha256"]) if c not in dropped]
        differing = {c: [p1["sha256"][c], br["sha256"].get(c)] for c in kept if p1["sha256"][c] != br["sha256"].get(c)}
        bad_drop = [c for c in dropped if not c.startswith("pair-three_operations")]
        record["digests"] = dict(parent_build_id=p1["build_id"], branch_build_id=br["build_id"], cases=len(kept), sha256=br["sha256"],
                                 dropped_parent_disagrees_with_itself=dropped, differing=differing)
        verdict["digests_identical"] = not differing and not bad_drop and len(kept) > 0 and set(br["sha256"]) == set(p1["sha256"])
        print(f"digest leg: {len(kept)} cases compared, dropped {dropped}, differing {sorted(differing)}", flush=True)
        if a.golden:
            with open(a.golden, "w") as f:
                json.dump({"recorded_from_build_id": p1["build_id"], "sha256": {c: p1["sha256"][c] for c in kept}}, f, indent=1)
                f.write("\n")
        save()
        if not verdict["digests_identical"]:
            print(json.dumps(verdict), flush=True)
            return 1
    if "ab" in legs or "share8" in legs:
        ab = record.setdefault("ab_lib", {})
        for leg, name, extra in (("ab", "headline_ms_per_step", []), ("share8", "share8_ms_per_learn", ["share8"])):
            if leg not in legs:
                continue
            out = run([os.path.join(ROOT, "tools", "ab_lib.py"), parent, str(a.rounds), *extra], 1100, echo=True)
            got = {k: [float(x) for x in re.findall(rf"^{k} ([0-9.]+)$", out, re.M)] for k in ("default", "variant")}
            assert len(got["default"]) == len(got["variant"]) == a.rounds, out
            ab[name] = dict(parent=stats(got["variant"]), branch=stats(got["default"]))
            ab[name]["not_slower"] = not_slower(ab[name]["parent"], ab[name]["branch"])
            print(f"ab leg: {name}: parent {ab[name]['parent']['median']} (spread {ab[name]['parent']['spread']}), branch {ab[name]['branch']['median']}", flush=True)
            save()
        verdict["ab_not_slower"] = {k: v["not_slower"] for k, v in ab.items()}
    if "costs" in legs:
        # a round is one fresh process per library (who goes first alternates), a figure of the round that process's own median
        costs = record.setdefault("costs", {})
        for tool in COST_TOOLS:
            per = {"parent": {}, "branch": {}}
            for r in range(a.rounds):
                for name in (("parent", "branch"), ("branch", "parent"))[r % 2]:
                    with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                        run([os.path.join(ROOT, "tools", tool + ".py"), "--rounds", str(a.inner_rounds), "--out", tmp.name], 600,
                            parent if name == "parent" else None)
                        for k, fig in figures(json.load(open(tmp.name))):
                            per[name].setdefault(k, []).append(fig["median"])
                print(f"costs leg: {tool}: round {r} done", flush=True)
            costs[tool] = {k: dict(parent=stats(per["parent"][k]), branch=stats(per["branch"][k])) for k in per["parent"]}
            for v in costs[tool].values():
                v["not_slower"] = not_slower(v["parent"], v["branch"])
            print(f"costs leg: {tool}: " + ", ".join(f"{k} {v['parent']['median']} -> {v['branch']['median']}" for k, v in costs[tool].items()), flush=True)
            save()
        verdict["costs_not_slower"] = {t: all(v["not_slower"] for v in costs[t].values()) for t in COST_TOOLS}
    verdict["all"] = all(v for k, x in verdict.items() if k != "all" for v in (x.values() if isinstance(x, dict) else [x]))
    save()
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["all"] else 1


if __name__ == "__main__":
    sys.exit(main())
