"""The pin of the single truth: tests/ppo_yardstick.py in float64 against the answers of the per-feature yardsticks it replaced
(tests/golden/ppo_yardstick_answers.npz: recorded from those functions, before they were folded, by tools/yardstick_equivalence.py
--record, with the inputs beside them).  Tiny cases -- obs 13, hidden (16, 16), 40 rows, bins (2, 7, 3) -- of every head, every hidden
activation, the masks (a row with an invalid stored action included), adv_norm + value_clip, the critic's own observations, a whole
learn() and masked_chain under imposed ReLU decisions.  Every statistic and every gradient tensor to 1e-12 of its largest magnitude,
the project's float64 threshold (diag_gaussian_yardstick.check_closed_form): several hundred times the float64 rounding of these
16-term contractions, so another CPU's BLAS stays inside it."""
import json

import numpy as np
import torch

import fp64_gate
import ppo_yardstick as PY
from diag_gaussian_yardstick import adv_stats


def flatten(result):
    out = {}
    for k, v in result.items():
        if isinstance(v, list):
            for l, (w, b) in enumerate(v):
                out[f"{k}.{l}.w"], out[f"{k}.{l}.b"] = np.asarray(w), np.asarray(b)
        else:
            out[k] = np.asarray(v)
    return out


def recompute(g, meta, case):
    x = lambda k: g["in." + k]
    net = lambda who: [(torch.as_tensor(x(f"{who}.{l}.w")), torch.as_tensor(x(f"{who}.{l}.b"))) for l in range(meta["layers"])]
    head = case["head"]
    pol, val = net("pol_" + head), net("cval" if case.get("cobs") else "val")
    rows = (x("obs"), x("acts_" + head), x(case.get("old", "old_" + head)), x("adv"), x("tgt"))
    bins = tuple(meta["bins"]) if head == "nvec" else None
    if case["kind"] == "minibatch":
        kw = dict(bins=bins) if bins else {}
        if case.get("mask"):
            kw["mask"] = x(case["mask"])
        r = PY.minibatch(torch.float64, head, pol, val, *rows, meta["clip"], meta["ent"], case["mb_ratio"], pol_act=case["pol_act"],
                         val_act=case["val_act"], cobs=x("cobs") if case.get("cobs") else None, log_std=x("log_std"),
                         adv_norm=adv_stats(x("adv")) if case.get("adv_norm") else None, value_clip=case.get("value_clip"), **kw)
        # ("masked_rule": recorded from masked_chain, the predecessor of the invalid-stored-action rule -- its policy gradient)
        return dict(grad_policy=r["grad_policy"]) if case["via"] == "masked_rule" else r
    if case["kind"] == "learn":
        buf = dict(states=x("obs"), actions=rows[1], log_probs=rows[2], values=x("tgt"), advantages=x("adv"))
        if case.get("cobs"):
            buf["critic_states"] = x("cobs")
        weakest = {}
        out = PY.learn(torch.float64, head, case["act"], pol, val, buf, *meta["learn"].values(), np.random.RandomState(3), log_std=x("log_std"),
                       weakest=weakest)
        assert set(weakest) == {"pol", "val"}
        return dict(policy=out[0], critic=out[1])
    masks = (fp64_gate.cpu_masks(pol, x("obs")), fp64_gate.cpu_masks(val, x("obs"))) if case["imposed"] else (None, None)
    out = PY.masked_chain(head, pol, val, *rows, x(case["mask"]), case["mb_ratio"], torch.float64, *masks, bins=bins)
    return dict(grad_policy=out[0], grad_value=out[1], stats=np.asarray(out[2]), ratio=out[3])


def test_ppo_yardstick_reproduces_the_answers_of_the_yardsticks_it_replaced(golden):
    z = golden("ppo_yardstick_answers")
    g = {k: z[k] for k in z.files}
    meta = json.loads(str(g["meta"]))
    assert len(meta["cases"]) >= 12
    worst = 0.0
    for i, case in enumerate(meta["cases"]):
        got = flatten(recompute(g, meta, case))
        want = {k[len(f"out.{i}."):]: g[k] for k in g if k.startswith(f"out.{i}.")}
        assert got.keys() == want.keys(), case["name"]
        for k, w in want.items():
            assert got[k].shape == w.shape, (case["name"], k)
            if w.size:
                e = float(np.abs(got[k] - w).max() / max(np.abs(w).max(), 1e-300))
                worst = max(worst, e)
                assert e <= 1e-12, (case["name"], k, e)
    print(f"[ppo yardstick pin] {len(meta['cases'])} cases, worst |got - recorded| / max|recorded| = {worst:.1e}")
