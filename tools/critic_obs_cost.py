"""What a critic with observations of its own (Learner(critic_observations=True), include/rlppo.h "[critic rows]") costs, on ONE build,
alternating, at the flagship shape (obs 107, 256 x 3, 90 discrete actions):
  * one 65,536-row and one 524,288-row fp32 pass of the update (device events), in the variants
      symmetric            rlppo_ppo_minibatch_ex on one matrix: the default (from 262,144 rows: paired launches, gather-fused first layers)
      symmetric_unpaired   the same with rlppo_dbg_set(29, 0): what the pairing alone is worth at that size (the 524,288-row pass only)
      critic_same_width    rlppo_ppo_minibatch_critic, the critic's matrix a second copy of the rows (width 107): never paired
      critic_214           rlppo_ppo_minibatch_critic, a critic of input width 214 on its own matrix
    with the pass-form counters (passes / paired / gather-fused / separate critic rows) each variant moved;
  * one 4096-agent x 128-step collect of tests/device_vector_env.py::IntegerEnv with and without critic_observations() of width 214,
    through the host interface and the device interface (the _HostEnv / _DeviceEnv sides of VectorAgentManager's collect loop).
No target is fixed in advance: medians and spread ((max - min) / median) over the rounds are recorded, stamped with rlppo_build_id().
--bench NAME=FILE ... : `bench.py --gpus 1 --steps 20 --warmup 5` result lines (this commit, its parent) to record beside them.
usage: python tools/critic_obs_cost.py [--rounds R] [--out FILE.json] [--bench NAME=FILE ...]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from rlgym_ppo_amd import _native as N  # noqa: E402
from tools.diag_gaussian_cost import Net, alternate, bench_stream, compare, summary  # noqa: E402

OBS, COBS, HIDDEN, A = 107, 214, (256, 256, 256), 90
NA, T = 4096, 128
COUNTERS = (("passes", 2), ("paired", 3), ("gather_fused", 4), ("separate_critic_rows", N.COUNTER_CRITIC_ROWS_PASS))


def pass_legs(mb, n_buf, unpaired):
    L = N.lib()
    rs = np.random.RandomState(0)
    pol, val, wide = Net([OBS, *HIDDEN, A]), Net([OBS, *HIDDEN, 1]), Net([COBS, *HIDDEN, 1])

    def rows(width, ld):
        x = torch.zeros(n_buf, ld, device="cuda")
        x[:, :width] = torch.randn(n_buf, width, device="cuda").clamp_(-5, 5)
        return x
    states, wide_rows = rows(OBS, pol.ld_in), rows(COBS, wide.ld_in)
    copy = states.clone()
    acts = torch.randint(0, A, (n_buf,), device="cuda").float()
    old = torch.randn(n_buf, device="cuda") * 0.3 - 4.5
    tgt, adv = torch.randn(n_buf, device="cuda"), torch.randn(n_buf, device="cuda")
    idx = torch.as_tensor(rs.permutation(n_buf)[:mb]).cuda()
    stats = torch.zeros(N.N_STATS, dtype=torch.float64, device="cuda")
    gp, gv, gw = torch.zeros(pol.n, device="cuda"), torch.zeros(val.n, device="cuda"), torch.zeros(wide.n, device="cuda")
    size = lambda fn, v: int(fn(pol.dims_c, pol.nl, v.dims_c, v.nl, mb, N.PRECISION_FP32))
    ws_bytes = max(size(L.rlppo_minibatch_workspace_bytes_for, val), size(L.rlppo_minibatch_workspace_bytes_critic, val),
                   size(L.rlppo_minibatch_workspace_bytes_critic, wide))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    st = bench_stream()
    keep = [pol, val, wide, states, wide_rows, copy, acts, old, tgt, adv, idx, stats, gp, gv, gw, ws]

    def args(v, grad):
        a = N.MinibatchArgs()
        a.head, a.pol_layers, a.val_layers, a.act_dim, a.precision = N.HEAD_DISCRETE, pol.nl, v.nl, 1, N.PRECISION_FP32
        a.pol_dims = ctypes.cast(pol.dims_c, ctypes.POINTER(ctypes.c_int32))
        a.val_dims = ctypes.cast(v.dims_c, ctypes.POINTER(ctypes.c_int32))
        a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = pol.packed.data_ptr(), v.packed.data_ptr(), gp.data_ptr(), grad.data_ptr()
        a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], n_buf, acts.data_ptr()
        a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idx.data_ptr(), mb
        a.clip_range, a.ent_coef, a.mb_ratio = 0.2, 0.005, 1.0
        a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
        keep.append(a)
        return a

    def critic(x):
        cr = N.CriticRows()
        cr.states, cr.ld_states = x.data_ptr(), x.shape[1]
        keep.append(cr)
        return cr
    a_sym, a_wide, cr_same, cr_wide = args(val, gv), args(wide, gw), critic(copy), critic(wide_rows)
    symmetric = lambda: N.check(L.rlppo_ppo_minibatch_ex(st, ctypes.byref(a_sym), None))

    def symmetric_unpaired():
        N.check(L.rlppo_dbg_set(29, 0))
        try:
            symmetric()
        finally:
            N.check(L.rlppo_dbg_set(29, 1))
    legs = {"symmetric": symmetric}
    if unpaired:
        legs["symmetric_unpaired"] = symmetric_unpaired
    legs["critic_same_width"] = lambda: N.check(L.rlppo_ppo_minibatch_critic(st, ctypes.byref(a_sym), None, ctypes.byref(cr_same)))
    legs["critic_214"] = lambda: N.check(L.rlppo_ppo_minibatch_critic(st, ctypes.byref(a_wide), None, ctypes.byref(cr_wide)))
    return legs, keep


def pass_record(mb, n_buf, rounds, reps, unpaired):
    L = N.lib()
    legs, keep = pass_legs(mb, n_buf, unpaired)
    forms = {}
    for name, fn in legs.items():   # which form each variant takes: one call each, by the counters
        c0 = [int(L.rlppo_dbg_counter(k)) for _, k in COUNTERS]
        fn()
        forms[name] = {label: int(L.rlppo_dbg_counter(k)) - c for (label, k), c in zip(COUNTERS, c0)}
    o = alternate(legs, rounds, reps)
    o["unit"] = "us per %d-row fp32 pass (device events, %d passes per measurement)" % (mb, reps)
    o["form_counters_moved_by_one_call"] = forms
    for name in legs:
        if name != "symmetric":
            compare(o, name, "symmetric")
    if unpaired:
        compare(o, "critic_same_width", "symmetric_unpaired")
    del legs, keep
    torch.cuda.empty_cache()
    return o


def collect_record(rounds):
    import device_vector_env as E
    from rlgym_ppo_amd.batched_agents import VectorAgentManager
    from rlgym_ppo_amd.ppo import DiscreteFF, ValueEstimator

    class CriticIntegerEnv(E.IntegerEnv):
        """IntegerEnv with critic_observations() of width 214, written over the same backend (integers, one exact division)."""

        def __init__(self, **kw):
            super().__init__(**kw)
            self.jc = self._arange(COBS)

        def critic_observations(self):
            k = (self.a[:, None] * 29 + self.jc[None, :] * 13 + self.t[:, None] * 5 + self.g * 7) % 19 - 9
            return self._f32(k) / 4.0
    mgrs = {}
    for side in ("device", "host"):
        for critic in (False, True):
            torch.manual_seed(1)
            pol = DiscreteFF(OBS, A, HIDDEN, "cuda:0")
            pol.noise_mode = "device"
            mgr = VectorAgentManager(pol, seed=5, standardize_obs=True)
            mgr.critic_observations = critic
            cls = CriticIntegerEnv if critic else E.IntegerEnv
            mgr.init_processes(0, lambda: cls(n_agents=NA, obs_dim=OBS, n_actions=A, device=torch.device("cuda:0") if side == "device" else None))
            if critic:
                mgr.value_net = ValueEstimator(COBS, HIDDEN, "cuda:0")
            mgrs[side + ("_critic_214" if critic else "")] = mgr
    res = {k: [] for k in mgrs}
    for r in range(rounds + 1):   # (round 0 warms up)
        for name, mgr in mgrs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mgr.collect_timesteps(NA * T)
            torch.cuda.synchronize()
            if r:
                res[name].append((time.perf_counter() - t0) * 1e3)
    out = {k: summary(v) for k, v in res.items()}
    compare(out, "device_critic_214", "device")
    compare(out, "host_critic_214", "host")
    rows = mgrs["device_critic_214"].critic_value_input_rows
    out["critic_rows_shape"] = list(rows.shape)
    out["unit"] = "ms per collect of %d agents x %d steps (host clock around a device synchronise), device-drawn noise" % (NA, T)
    for mgr in mgrs.values():
        mgr.cleanup()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "critic_obs_cost.json"))
    ap.add_argument("--bench", action="append", default=[], help="NAME=FILE: the last line of FILE is a bench.py JSON result line")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/critic_obs_cost.py measures on the GPU: no HIP device visible")
    L = N.lib()
    out = {"build_id": L.rlppo_build_id().decode(), "device": torch.cuda.get_device_name(0),
           "shape": {"obs": OBS, "critic_obs": COBS, "hidden": HIDDEN, "actions": A}, "rounds": args.rounds}
    out["pass_65536"] = pass_record(65536, 131072, args.rounds, 10, False)
    print("pass_65536:", json.dumps(out["pass_65536"]), flush=True)
    out["pass_524288"] = pass_record(524288, 524288, args.rounds, 3, True)
    print("pass_524288:", json.dumps(out["pass_524288"]), flush=True)
    out["collect_ms"] = collect_record(args.rounds)
    print("collect_ms:", json.dumps(out["collect_ms"]), flush=True)
    for item in args.bench:
        name, path = item.split("=", 1)
        lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
        out.setdefault("bench", {})[name] = json.loads(lines[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
