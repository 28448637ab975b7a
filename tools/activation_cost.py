"""What the hidden-activation choice (Learner(hidden_activation=...), include/rlppo.h "[act]") costs, on ONE build, alternating, at the
flagship shape (obs 107, 256 x 3, 90 discrete actions):
  * one 65,536-row fp32 pass of the update (rlppo_ppo_minibatch_ex, device events);
  * the 4096-row rollout call on padded device rows (rlppo_discrete_act);
for four configurations:
  relu        the default: ReLU bitmasks, folded value head, (from 262,144 rows) paired launches; the one-launch rollout kernel
  relu_plain  ReLU forced through the form a tanh / ELU network takes -- rlppo_dbg_set 26 = 0, 29 = 0, 32 = 0, 19 = 0 for the pass
              (gather pass, two chains, no folded head, dX by the saved activation), 27 = 0 for the rollout call (the layer chain):
              what the FORM costs, apart from the epilogue
  tanh, elu   the two new activations: what the EPILOGUE costs on top of the form
No target is fixed in advance: medians and spread ((max - min) / median) over the rounds are recorded, stamped with rlppo_build_id().
--bench FILE.json ... : `bench.py --gpus 1 --steps 20 --warmup 5` result lines (this commit, its parent) to record beside them.
usage: python tools/activation_cost.py [--rounds R] [--out FILE.json] [--bench NAME=FILE ...]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rlgym_ppo_amd import _native as N  # noqa: E402
from tools.diag_gaussian_cost import Net, P, alternate, bench_stream  # noqa: E402

OBS, HIDDEN, A = 107, (256, 256, 256), 90
PLAIN_PASS, PLAIN_ROLLOUT = ((26, 0), (29, 0), (32, 0), (19, 0)), ((27, 0),)
DEFAULTS = {26: 1, 29: 1, 32: 1, 19: 1, 27: 1}
CONFIGS = (("relu", 0, False), ("relu_plain", 0, True), ("tanh", 1, False), ("elu", 2, False))


def switched(fn, switches):
    """fn() with the given rlppo_dbg_set switches, restored afterwards (the switches are read when a call is made)."""
    L = N.lib()

    def run():
        for k, v in switches:
            N.check(L.rlppo_dbg_set(k, v))
        try:
            fn()
        finally:
            for k, _ in switches:
                N.check(L.rlppo_dbg_set(k, DEFAULTS[k]))
    return run


def pass_legs(mb, n_buf):
    L = N.lib()
    rs = np.random.RandomState(0)
    pol, val = Net([OBS, *HIDDEN, A]), Net([OBS, *HIDDEN, 1])
    states = torch.zeros(n_buf, val.ld_in, device="cuda")
    states[:, :OBS] = torch.randn(n_buf, OBS, device="cuda").clamp_(-5, 5)
    acts = torch.randint(0, A, (n_buf,), device="cuda").float()
    old = torch.randn(n_buf, device="cuda") * 0.3 - 4.5
    tgt, adv = torch.randn(n_buf, device="cuda"), torch.randn(n_buf, device="cuda")
    idx = torch.as_tensor(rs.permutation(n_buf)[:mb]).cuda()
    stats = torch.zeros(N.N_STATS, dtype=torch.float64, device="cuda")
    gp, gv = torch.zeros(pol.n, device="cuda"), torch.zeros(val.n, device="cuda")
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.precision = N.HEAD_DISCRETE, pol.nl, val.nl, 1, N.PRECISION_FP32
    a.pol_dims = ctypes.cast(pol.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(val.dims_c, ctypes.POINTER(ctypes.c_int32))
    ws_bytes = int(L.rlppo_minibatch_workspace_bytes_for(pol.dims_c, pol.nl, val.dims_c, val.nl, mb, a.precision))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = pol.packed.data_ptr(), val.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
    a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], n_buf, acts.data_ptr()
    a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idx.data_ptr(), mb
    a.clip_range, a.ent_coef, a.mb_ratio = 0.2, 0.005, 1.0
    a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
    st = bench_stream()
    legs, keep = {}, [pol, val, states, acts, old, tgt, adv, idx, stats, gp, gv, ws, a]
    for name, code, plain in CONFIGS:
        ext = N.MinibatchExt()
        ext.pol_hidden_act = ext.val_hidden_act = code
        keep.append(ext)
        call = lambda ext=ext: N.check(L.rlppo_ppo_minibatch_ex(st, ctypes.byref(a), ctypes.byref(ext)))
        legs[name] = switched(call, PLAIN_PASS) if plain else call
    return legs, keep


def rollout_legs(n):
    L = N.lib()
    pol = Net([OBS, *HIDDEN, A])
    rows = torch.zeros(n, pol.ld_in, device="cuda")
    rows[:, :OBS] = torch.randn(n, OBS, device="cuda").clamp_(-5, 5)
    q = torch.empty(n, A, device="cuda").exponential_(1)
    act, logp = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, device="cuda")
    ws = torch.empty(int(L.rlppo_forward_workspace_bytes(pol.dims_c, pol.nl, n)), dtype=torch.uint8, device="cuda")
    st = bench_stream()
    legs, keep = {}, [pol, rows, q, act, logp, ws]
    for name, code, plain in CONFIGS:
        o = N.ActOpts()
        o.hidden_act = code
        keep.append(o)
        call = lambda o=o: N.check(L.rlppo_discrete_act(st, pol.dims_c, pol.nl, P(pol.packed), P(rows), pol.ld_in, n, P(q), P(act), P(logp), None, P(ws),
                                                        ws.numel(), ctypes.byref(o)))
        legs[name] = switched(call, PLAIN_ROLLOUT) if plain else call
    return legs, keep


def ratios(o):
    base, plain = o["relu"]["median"], o["relu_plain"]["median"]
    o["ratios"] = {"relu_plain_over_relu": round(plain / base, 4), "tanh_over_relu": round(o["tanh"]["median"] / base, 4),
                   "elu_over_relu": round(o["elu"]["median"] / base, 4), "tanh_over_relu_plain": round(o["tanh"]["median"] / plain, 4),
                   "elu_over_relu_plain": round(o["elu"]["median"] / plain, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "activation_cost.json"))
    ap.add_argument("--bench", action="append", default=[], help="NAME=FILE: the last line of FILE is a bench.py JSON result line")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/activation_cost.py measures on the GPU: no HIP device visible")
    L = N.lib()
    out = {"build_id": L.rlppo_build_id().decode(), "device": torch.cuda.get_device_name(0), "shape": {"obs": OBS, "hidden": HIDDEN, "actions": A},
           "rounds": args.rounds, "configurations": {"relu": "default", "relu_plain": "rlppo_dbg_set 26=0 29=0 32=0 19=0 (pass), 27=0 (rollout)",
                                                     "tanh": "hidden_act 1", "elu": "hidden_act 2"}}
    legs, keep = pass_legs(65536, 131072)
    c0 = [int(L.rlppo_dbg_counter(k)) for k in (2, 3, 4)]
    o = alternate(legs, args.rounds, 10)
    o["unit"] = "us per 65,536-row fp32 pass (device events, 10 passes per measurement)"
    o["pass_form_counters_moved"] = dict(zip(("passes", "paired", "gather_fused"), [int(L.rlppo_dbg_counter(k)) - c for k, c in zip((2, 3, 4), c0)]))
    ratios(o)
    out["pass_65536"] = o
    del legs, keep
    torch.cuda.empty_cache()
    legs, keep = rollout_legs(4096)
    o = alternate(legs, args.rounds, 50)
    o["unit"] = "us per 4096-row rlppo_discrete_act call on padded device rows (device events, 50 calls per measurement)"
    ratios(o)
    out["rollout_4096"] = o
    for item in args.bench:
        name, path = item.split("=", 1)
        lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
        out.setdefault("bench", {})[name] = json.loads(lines[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "bench"}, indent=1)[:5000])


if __name__ == "__main__":
    main()
