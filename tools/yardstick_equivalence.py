"""Shows that tests/ppo_yardstick.py computes, bit for bit, what the per-feature yardsticks it replaced computed.

    python tools/yardstick_equivalence.py --parent-tests DIR [--record]

DIR is the tests/ directory of the commit before the fold (for example a `git worktree` of it).  In one process the old modules
(diag_gaussian_yardstick, activation_yardstick, critic_obs_yardstick, masked_multidiscrete_yardstick, test_gpu_action_mask) and
the new one are imported under different names and run on the same inputs, in float64 and in float32 (the float32 run sets the
tolerance of every gate, so it must not move either); every returned array and scalar is compared with tobytes() equality.  Tiny
shapes, where indexing goes wrong: obs 13, hidden (16, 16), 40 rows, mb_ratio 0.25 and 1.0, bins (2, 7, 3).  The rows with an invalid
stored action are kept inside the clip range, where the rule about them decides a gradient (check_invalid_rows asserts it);
minibatch under such a mask is held to masked_chain's policy gradient, the rule's predecessor.

Writes profiles/yardstick_equivalence.json and exits non-zero unless every case is identical.  One entry per run: identical
true/false, the number of outputs and ONE sha256 over the outputs' own sha256 ("name:digest" lines in name order); an output that
differs is listed by name with both digests.  --per-output lists every output's sha256 (about 100 KB, not meant to be committed).
--record: also writes tests/golden/ppo_yardstick_answers.npz -- the inputs and the float64 answers
of the OLD functions on a dozen of the cases, which tests/test_ppo_yardstick_host.py holds the new module to."""
import argparse
import contextlib
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLD_MODULES = ("fp64_gate", "diag_gaussian_yardstick", "activation_yardstick", "critic_obs_yardstick", "multidiscrete_nvec_yardstick",
               "masked_multidiscrete_yardstick", "synthetic_env", "test_gpu_action_mask")
NEW_MODULES = ("fp64_gate", "diag_gaussian_yardstick", "ppo_yardstick")
D, CD, HID, N, BINS, K = 13, 9, (16, 16), 40, (2, 7, 3), 3
CLIP, ENT = 0.2, 0.005
INVALID_ROWS = (5, 11, 17, 23, 29)   # rows whose stored action the *_invalid masks mark invalid
DTYPES = {"float64": torch.float64, "float32": torch.float32}


def load(directory, names, prefix):
    """Imports `names` from `directory` and files them in sys.modules under prefix + name, so both generations can coexist."""
    sys.path.insert(0, directory)
    try:
        mods = {n: importlib.import_module(n) for n in names}
    finally:
        sys.path.remove(directory)
    for n in list(sys.modules):
        f = getattr(sys.modules[n], "__file__", None) or ""
        if os.path.dirname(os.path.abspath(f)) == os.path.abspath(directory):
            sys.modules[prefix + n] = sys.modules.pop(n)
    return mods


def make_inputs(nets, head_terms64):
    """One problem per head on shared observations; old log-probabilities = the float64 log p + N(0, 0.2^2)."""
    torch.manual_seed(7)
    rs = np.random.RandomState(7)
    S = sum(BINS)
    x = dict(obs=rs.randn(N, D).astype(np.float32), cobs=rs.randn(N, CD).astype(np.float32), adv=rs.randn(N).astype(np.float32),
             tgt=rs.randn(N).astype(np.float32), log_std=rs.uniform(-1.0, 0.5, K).astype(np.float32))
    for who, net in (("val", nets.init_mlp(D, HID, 1)), ("cval", nets.init_mlp(CD, HID, 1)), ("pol_discrete", nets.init_mlp(D, HID, S)),
                     ("pol_nvec", nets.init_mlp(D, HID, S)), ("pol_gaussian", nets.init_mlp(D, HID, 2 * K)), ("pol_diag", nets.init_mlp(D, HID, K))):
        for l, (w, b) in enumerate(net):
            x[f"{who}.{l}.w"], x[f"{who}.{l}.b"] = w.numpy(), b.numpy()
    x["acts_discrete"] = rs.randint(0, S, N).astype(np.float32)
    x["acts_nvec"] = np.stack([rs.randint(0, b, N) for b in BINS], 1).astype(np.float32)
    x["acts_gaussian"] = rs.uniform(-0.9, 0.9, (N, K)).astype(np.float32)
    x["acts_diag"] = rs.randn(N, K).astype(np.float32)
    m = rs.rand(N, S) < 0.6
    m[np.arange(N), x["acts_discrete"].astype(int)] = True
    x["mask_discrete"] = m
    m, s = rs.rand(N, S) < 0.6, 0
    for h, b in enumerate(BINS):
        m[np.arange(N), s + x["acts_nvec"][:, h].astype(int)] = True
        s += b
    x["mask_nvec"] = m
    bad = m.copy()                         # INVALID_ROWS: the stored action of head 1 is invalid, its neighbour valid
    for r in INVALID_ROWS:
        a = int(x["acts_nvec"][r, 1])
        bad[r, BINS[0] + a], bad[r, BINS[0] + (a + 1) % BINS[1]] = False, True
    x["mask_nvec_invalid"] = bad
    bad = x["mask_discrete"].copy()
    for r in INVALID_ROWS:
        a = int(x["acts_discrete"][r])
        bad[r, a], bad[r, (a + 1) % S] = False, True
    x["mask_discrete_invalid"] = bad
    for head in ("discrete", "nvec", "gaussian", "diag"):
        x["old_" + head] = (head_terms64(head, params(x, "pol_" + head), x) + 0.2 * rs.randn(N)).astype(np.float32)
    # under an invalid-action mask the old log-probabilities come from the MASKED log p (the literal value on the invalid rows), with
    # small noise on those rows: they stay on the unclipped branch of the surrogate, where the row's gradient is not zero
    noise = 0.2 * rs.randn(N)
    noise[list(INVALID_ROWS)] = 0.03 * rs.randn(len(INVALID_ROWS))
    for head in ("discrete", "nvec"):
        key = f"mask_{head}_invalid"
        x[f"old_{head}_invalid"] = (head_terms64(head, params(x, "pol_" + head), x, x[key]) + noise).astype(np.float32)
    return x


def params(x, who):
    return [(torch.as_tensor(x[f"{who}.{l}.w"]), torch.as_tensor(x[f"{who}.{l}.b"])) for l in range(len(HID) + 1)]


def case_list():
    cases = []
    for i, head in enumerate(("discrete", "nvec", "gaussian", "diag")):
        for j, act in enumerate(("relu", "tanh", "elu")):
            cases.append(dict(kind="minibatch", via="activation", head=head, pol_act=act, val_act=("relu", "tanh", "elu")[(i + j) % 3],
                              mb_ratio=(0.25, 1.0)[(i + j) % 2]))
    cases.append(dict(kind="minibatch", via="activation", head="nvec", pol_act="tanh", val_act="relu", mb_ratio=0.25, mask="mask_nvec"))
    cases.append(dict(kind="minibatch", via="masked_rule", head="nvec", pol_act="relu", val_act="relu", mb_ratio=1.0, mask="mask_nvec_invalid",
                      old="old_nvec_invalid"))
    for adv_norm, value_clip in ((False, None), (True, None), (False, 0.3), (True, 0.3)):
        cases.append(dict(kind="minibatch", via="diag", head="diag", pol_act="relu", val_act="relu", mb_ratio=0.25, adv_norm=adv_norm,
                          value_clip=value_clip))
    cases.append(dict(kind="minibatch", via="critic", head="discrete", pol_act="tanh", val_act="tanh", mb_ratio=0.25, cobs=True))
    cases.append(dict(kind="minibatch", via="critic", head="diag", pol_act="elu", val_act="elu", mb_ratio=1.0, cobs=True))
    cases.append(dict(kind="minibatch", via="critic", head="nvec", pol_act="relu", val_act="relu", mb_ratio=1.0, cobs=True, mask="mask_nvec"))
    cases.append(dict(kind="minibatch", via="diag", head="diag", pol_act="relu", val_act="relu", mb_ratio=1.0, adv_norm=False, value_clip=None,
                      bf16="operands", dtypes=["float32"]))
    cases.append(dict(kind="minibatch", via="diag", head="diag", pol_act="relu", val_act="relu", mb_ratio=1.0, adv_norm=True, value_clip=0.3,
                      bf16="operands+sum64", dtypes=["float32"]))
    cases.append(dict(kind="learn", via="activation", head="discrete", act="tanh"))
    cases.append(dict(kind="learn", via="diag", head="diag", act="relu"))
    cases.append(dict(kind="learn", via="critic", head="discrete", act="tanh", cobs=True))
    cases.append(dict(kind="learn", via="critic", head="diag", act="relu", cobs=True))
    for head in ("discrete", "nvec"):
        for mask in ("mask_" + head, f"mask_{head}_invalid"):
            extra = dict(old=f"old_{head}_invalid") if mask.endswith("_invalid") else {}
            cases.append(dict(kind="masked_chain", head=head, mask=mask, mb_ratio=0.25, imposed=True, dtypes=["float64"], **extra))
            cases.append(dict(kind="masked_chain", head=head, mask=mask, mb_ratio=1.0, imposed=False, dtypes=["float32"], **extra))
    for c in cases:
        c.setdefault("dtypes", ["float64", "float32"])
        c["name"] = " ".join(f"{k}={v}" for k, v in c.items() if k not in ("dtypes", "name"))
    return cases


def pinned(case):
    """The dozen-odd float64 cases whose answers the host test keeps: every head, every activation, every option once."""
    if "float64" not in case["dtypes"]:
        return False
    if case["kind"] == "minibatch" and case["via"] == "activation" and not case.get("mask"):
        return (case["head"], case["pol_act"]) in (("discrete", "relu"), ("nvec", "tanh"), ("gaussian", "elu"), ("diag", "tanh"))
    if case["kind"] == "minibatch" and case["via"] == "diag":
        return bool(case["adv_norm"]) and case["value_clip"] is not None
    if case["kind"] == "learn":
        return (case["via"], case["head"]) in (("activation", "discrete"), ("diag", "diag"), ("critic", "discrete"))
    if case["kind"] == "masked_chain":
        return case["mask"] in ("mask_discrete", "mask_nvec_invalid")
    return case["via"] == "masked_rule" or case["head"] != "nvec" or case["via"] != "critic"


def precision_context(nets, case):
    if case.get("bf16") == "operands":
        return nets.bf16_operands()
    if case.get("bf16") == "operands+sum64":
        stack = contextlib.ExitStack()
        stack.enter_context(nets.bf16_operands())
        stack.enter_context(nets.sum64())
        return stack
    return contextlib.nullcontext()


def learn_buffer(x, case):
    buf = dict(states=x["obs"], actions=x["acts_" + case["head"]], log_probs=x["old_" + case["head"]], values=x["tgt"], advantages=x["adv"])
    if case.get("cobs"):
        buf["critic_states"] = x["cobs"]
    return buf


LEARN = dict(batch_size=20, mini_batch_size=10, n_epochs=2, clip=CLIP, ent_coef=ENT, policy_lr=3e-4, critic_lr=1e-3)


def head_kw(x, case):
    kw = {}
    if case["head"] == "nvec":
        kw["bins"] = BINS
    if case.get("mask"):
        kw["mask"] = x[case["mask"]]
    return kw


def relu_masks(gate_mod, x, case):
    pol, val = params(x, "pol_" + case["head"]), params(x, "val")
    return (gate_mod.cpu_masks(pol, x["obs"]), gate_mod.cpu_masks(val, x["obs"])) if case["imposed"] else (None, None)


def policy_grads64(grad_policy):
    return dict(grad_policy=[(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in grad_policy])


def run_old(old, x, case, dtype):
    head = case["head"]
    pol, val = params(x, "pol_" + head), params(x, "cval" if case.get("cobs") else "val")
    rows = (x["obs"], x["acts_" + head], x[case.get("old", "old_" + head)], x["adv"], x["tgt"])
    DY, A, CY = old["diag_gaussian_yardstick"], old["activation_yardstick"], old["critic_obs_yardstick"]
    if case["kind"] == "minibatch":
        tail = (CLIP, ENT, case["mb_ratio"])
        with precision_context(DY.nets, case):
            if case["via"] == "diag":
                return DY.minibatch(dtype, pol, x["log_std"], val, *rows, *tail, adv_norm=DY.adv_stats(x["adv"]) if case["adv_norm"] else None,
                                    value_clip=case["value_clip"])
            if case["via"] == "masked_rule":   # the predecessor of minibatch's invalid-action rule is masked_chain's (its policy side)
                return policy_grads64(old["masked_multidiscrete_yardstick"].masked_chain(pol, val, *rows, x[case["mask"]], BINS, case["mb_ratio"],
                                                                                         dtype)[0])
            if case["via"] == "activation":
                return A.minibatch(dtype, head, case["pol_act"], case["val_act"], pol, val, *rows, *tail, log_std=x["log_std"], **head_kw(x, case))
            return CY.minibatch(dtype, head, case["pol_act"], case["val_act"], pol, val, x["obs"], x["cobs"], *rows[1:], *tail, log_std=x["log_std"],
                                **head_kw(x, case))
    if case["kind"] == "learn":
        weakest = {}
        args = (learn_buffer(x, case), *LEARN.values(), np.random.RandomState(3))
        if case["via"] == "diag":
            out = DY.learn(dtype, pol, x["log_std"], val, *args, weakest=weakest)
        else:
            out = (A if case["via"] == "activation" else CY).learn(dtype, head, case["act"], pol, val, *args, log_std=x["log_std"], weakest=weakest)
        return dict(policy=out[0], critic=out[1], weakest_pol=weakest["pol"], weakest_val=weakest["val"])
    mp, mv = relu_masks(old["fp64_gate"], x, case)
    args = (pol, val, *rows, x[case["mask"]])
    if head == "discrete":
        out = old["test_gpu_action_mask"].masked_chain(*args, case["mb_ratio"], dtype, mp, mv)
    else:
        out = old["masked_multidiscrete_yardstick"].masked_chain(*args, BINS, case["mb_ratio"], dtype, mp, mv)
    return dict(grad_policy=out[0], grad_value=out[1], stats=np.asarray(out[2]), ratio=out[3])


def run_new(new, x, case, dtype):
    PY = new["ppo_yardstick"]
    head = case["head"]
    pol, val = params(x, "pol_" + head), params(x, "cval" if case.get("cobs") else "val")
    rows = (x["obs"], x["acts_" + head], x[case.get("old", "old_" + head)], x["adv"], x["tgt"])
    if case["kind"] == "minibatch":
        with precision_context(PY.nets, case):
            r = PY.minibatch(dtype, head, pol, val, *rows, CLIP, ENT, case["mb_ratio"], pol_act=case["pol_act"], val_act=case["val_act"],
                             cobs=x["cobs"] if case.get("cobs") else None, log_std=x["log_std"],
                             adv_norm=new["diag_gaussian_yardstick"].adv_stats(x["adv"]) if case.get("adv_norm") else None,
                             value_clip=case.get("value_clip"), **head_kw(x, case))
        return policy_grads64(r["grad_policy"]) if case["via"] == "masked_rule" else r
    if case["kind"] == "learn":
        weakest = {}
        out = PY.learn(dtype, head, case["act"], pol, val, learn_buffer(x, case), *LEARN.values(), np.random.RandomState(3), log_std=x["log_std"],
                       weakest=weakest)
        return dict(policy=out[0], critic=out[1], weakest_pol=weakest["pol"], weakest_val=weakest["val"])
    mp, mv = relu_masks(new["fp64_gate"], x, case)
    out = PY.masked_chain(head, pol, val, *rows, x[case["mask"]], case["mb_ratio"], dtype, mp, mv, bins=BINS if head == "nvec" else None)
    return dict(grad_policy=out[0], grad_value=out[1], stats=np.asarray(out[2]), ratio=out[3])


def check_invalid_rows(old, new, x):
    """The invalid stored actions are where the rule 'the literal value and no gradient through its own logit' decides something:
    (1) every such row lies strictly inside the clip range with a non-zero advantage, so its surrogate gradient is alive;
    (2) d(sum log p)/dz at the row's own logit is exactly 0 under ppo_yardstick.head_terms and exactly 1 under the parent's
        activation_yardstick.head_terms, which has no such rule (the no-detach form);
    (3) hence ppo_yardstick.minibatch and the parent's activation_yardstick.minibatch DIFFER in the policy gradient on this mask,
        as they must (the issue moves masked_chain's rule into head_terms), and agree to the bit on the mask without invalid actions
        (a run of the case list)."""
    A, PY = old["activation_yardstick"], new["ppo_yardstick"]
    pol, val, rows = params(x, "pol_nvec"), params(x, "val"), list(INVALID_ROWS)
    for head in ("nvec", "discrete"):
        r = run_new(new, x, dict(kind="masked_chain", head=head, mask=f"mask_{head}_invalid", old=f"old_{head}_invalid", mb_ratio=1.0, imposed=False),
                    torch.float64)
        assert (np.abs(r["ratio"][rows] - 1.0) < CLIP - 1e-3).all() and (np.abs(x["adv"][rows]) > 0.05).all(), (head, r["ratio"][rows], x["adv"][rows])
    own = BINS[0] + x["acts_nvec"][rows, 1].astype(int)
    acts = torch.as_tensor(x["acts_nvec"], dtype=torch.float64)
    grads = []
    for terms in (lambda z: PY.head_terms("nvec", z, acts, bins=BINS, mask=x["mask_nvec_invalid"]),
                  lambda z: A.head_terms("nvec", z, acts, torch.float64, bins=BINS, mask=x["mask_nvec_invalid"])):
        z = torch.as_tensor(A.forward64(pol, x["obs"], "relu")).requires_grad_(True)
        terms(z)[0].sum().backward()
        grads.append(z.grad.numpy()[rows, own])
    assert (grads[0] == 0.0).all() and (grads[1] == 1.0).all(), grads
    args = (pol, val, x["obs"], x["acts_nvec"], x["old_nvec_invalid"], x["adv"], x["tgt"], CLIP, ENT, 1.0)
    with_rule = PY.minibatch(torch.float64, "nvec", *args, bins=BINS, mask=x["mask_nvec_invalid"])
    without = A.minibatch(torch.float64, "nvec", "relu", "relu", *args, bins=BINS, mask=x["mask_nvec_invalid"])
    gap = PY.err([t for wb in with_rule["grad_policy"] for t in wb], [t for wb in without["grad_policy"] for t in wb])
    assert gap > 1e-3 and np.array_equal(with_rule["ratio"], without["ratio"]), gap
    print(f"invalid stored actions, rows {rows}: inside the clip range; own-logit gradient 0 with the rule, 1 without; the policy gradient "
          f"without the rule is {gap:.2e} away")


def flatten(result):
    """{name: ndarray} of every array and scalar of a result, layer lists expanded."""
    out = {}
    for k, v in result.items():
        if isinstance(v, list):
            for l, (w, b) in enumerate(v):
                out[f"{k}.{l}.w"], out[f"{k}.{l}.b"] = np.asarray(w), np.asarray(b)
        else:
            out[k] = np.asarray(v)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tests", required=True)
    ap.add_argument("--tests", default=os.path.join(ROOT, "tests"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yardstick_equivalence.json"))
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--per-output", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    old = load(os.path.abspath(a.parent_tests), OLD_MODULES, "parent_tests.")
    new = load(os.path.abspath(a.tests), NEW_MODULES, "branch_tests.")
    A = old["activation_yardstick"]

    def logp64(head, pol, x, mask=None):
        z = torch.as_tensor(A.forward64(pol, x["obs"], "relu", out_tanh=head == "gaussian"))
        acts = torch.as_tensor(x["acts_" + head], dtype=torch.float64)
        if head == "discrete" and mask is not None:   # (the parent's head_terms has no masked discrete form: test_gpu_action_mask's)
            p = torch.clamp(torch.softmax(z.masked_fill(~torch.as_tensor(mask), float("-inf")), -1), min=1e-11, max=1)
            return torch.log(p).gather(1, acts.long().view(-1, 1)).view(-1).numpy()
        return A.head_terms(head, z, acts, torch.float64, log_std=torch.as_tensor(x["log_std"], dtype=torch.float64), bins=BINS,
                            mask=mask)[0].numpy()

    x = make_inputs(A.nets, logp64)
    check_invalid_rows(old, new, x)
    report, answers, all_same = [], {}, True
    for case in case_list():
        for dname in case["dtypes"]:
            o, n = flatten(run_old(old, x, case, DTYPES[dname])), flatten(run_new(new, x, case, DTYPES[dname]))
            same = o.keys() == n.keys() and all(o[k].dtype == n[k].dtype and o[k].shape == n[k].shape and o[k].tobytes() == n[k].tobytes()
                                                for k in o)
            all_same &= same
            sha = lambda r: {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in sorted(r.items())}
            so, sn = sha(o), sha(n)
            entry = dict(case=case["name"], dtype=dname, identical=bool(same), outputs=len(so),
                         sha256=hashlib.sha256("\n".join(f"{k}:{d}" for k, d in so.items()).encode()).hexdigest())
            if not same:
                entry["differing"] = {k: [so.get(k), sn.get(k)] for k in sorted(set(so) | set(sn)) if so.get(k) != sn.get(k)}
            if a.per_output:
                entry["per_output"] = so
            report.append(entry)
            print(("identical  " if same else "DIFFERENT  ") + dname + "  " + case["name"])
            if dname == "float64":
                answers[case["name"]] = o
    with open(a.out, "w") as f:
        head = dict(shapes=dict(obs=D, critic_obs=CD, hidden=HID, rows=N, bins=BINS), runs=len(report), all_identical=bool(all_same))
        f.write(json.dumps(head)[:-1] + ', "results": [\n' + ",\n".join(" " + json.dumps(r) for r in report) + "\n]}\n")
    if a.record:
        keep = [c for c in case_list() if pinned(c)]
        store = {"in." + k: v for k, v in x.items()}
        store["meta"] = np.asarray(json.dumps(dict(bins=BINS, clip=CLIP, ent=ENT, layers=len(HID) + 1, learn=LEARN, cases=keep)))
        for i, c in enumerate(keep):
            for k, v in answers[c["name"]].items():
                if not k.startswith("weakest"):   # (a diagnostic of learn(), as large as the parameters: compared above, not kept)
                    store[f"out.{i}.{k}"] = np.asarray(v, np.float64)
        np.savez_compressed(os.path.join(a.tests, "golden", "ppo_yardstick_answers.npz"), **store)
        print(f"recorded {len(keep)} float64 cases from the parent's functions")
    print(f"{len(report)} runs, all identical: {all_same}")
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
