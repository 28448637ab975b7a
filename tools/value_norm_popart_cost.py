"""What PopArt's weight-preserving step (Learner(ppo_value_norm_popart=True), include/rlppo.h "[vnorm]") costs, on ONE build in one
session, alternating:
  * the statistic's launch at 524,288 targets with the rescale (rlppo_value_norm_update_popart, n_w = 256 and 512 last-layer weights
    at an odd float offset, as in an arena) beside the launch without it (rlppo_value_norm_update, the yardstick: the existing entry
    point on the same build) -- WARM, and COLD behind a fill that evicts targets and weights, the fill's own time subtracted;
  * the extra rlppo_net_pack of the critic (obs 107, hidden 256 x 3 and 512 x 3, one output) that the bumped native_epoch causes
    once per iteration, before the first launch that reads the packed image;
  * (--parent DIR: a built checkout of the parent commit) `bench.py --gpus 1 --steps 20 --warmup 5` of this tree against the
    parent's, alternating, each in a fresh process; both result lines of the last round are recorded (the headline runs none of the
    new code: tools/value_norm_cost.py's leg).
Medians and spread ((max - min) / median) over the rounds; the record is stamped with rlppo_build_id().  No target is fixed in advance.
usage: python tools/value_norm_popart_cost.py [--rounds R] [--parent DIR] [--bench-rounds R] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from rlgym_ppo_amd import _native as N  # noqa: E402
from tools import diag_gaussian_cost as DC  # noqa: E402
from tools import gae_bootstrap_cost as GC  # noqa: E402
from tools import value_norm_cost as VC  # noqa: E402

P = VC.P
OBS = 107


def update_leg(rounds, n_w, n=524288):
    L = N.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    scale = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float32, device="cuda")
    ws = torch.zeros(N.VALUE_NORM_WS_BYTES, dtype=torch.uint8, device="cuda")
    arena = torch.randn(7 + n_w + 1, device="cuda") / n_w ** 0.5
    w, b = arena[7:7 + n_w], arena[7 + n_w:]
    # (cold: a set of inputs as large as the scan's between two uses of one target array -- tools/value_norm_cost.py)
    sets = [(40.0 + 25.0 * torch.randn(n, device="cuda"), torch.empty(14 * n, device="cuda")) for _ in range(bench.GAE_SETS)]
    plain = lambda x: N.check(L.rlppo_value_norm_update(st, P(x), n, P(state), P(scale), P(ws)))
    popart = lambda x: N.check(L.rlppo_value_norm_update_popart(st, P(x), n, P(state), P(scale), P(ws), P(w), n_w, P(b)))

    def behind_a_fill(fn, x, filler):
        filler.zero_()   # evicts the targets and the weights from the caches; timed apart and subtracted
        fn(x)
    legs = {"plain_warm": [lambda x=sets[0][0]: plain(x)] * bench.GAE_SETS, "popart_warm": [lambda x=sets[0][0]: popart(x)] * bench.GAE_SETS,
            "evict_and_plain": [lambda x=x, f=f: behind_a_fill(plain, x, f) for x, f in sets],
            "evict_and_popart": [lambda x=x, f=f: behind_a_fill(popart, x, f) for x, f in sets],
            "evict_only": [lambda f=f: f.zero_() for _, f in sets]}
    res = GC.alternate(legs, rounds)
    GC.compare(res, "popart_warm", "plain_warm")
    GC.compare(res, "evict_and_popart", "evict_and_plain")
    res["plain_cold_median"] = round(res["evict_and_plain"]["median"] - res["evict_only"]["median"], 4)
    res["popart_cold_median"] = round(res["evict_and_popart"]["median"] - res["evict_only"]["median"], 4)
    res["rescale_warm_us"] = round(res["popart_warm"]["median"] - res["plain_warm"]["median"], 4)
    res["rescale_cold_us"] = round(res["evict_and_popart"]["median"] - res["evict_and_plain"]["median"], 4)
    res["unit"] = ("us per call at %d targets, n_w = %d (HIP events; cold = behind a %d MB fill that evicts targets and weights, the fill's own "
                   "time subtracted)" % (n, n_w, 14 * n * 4 // 10 ** 6))
    assert float(state[0].item()) > 0 and float(state[3].item()) == 0.0 and bool(torch.isfinite(arena).all())
    del legs, sets
    torch.cuda.empty_cache()
    return res


def repack_leg(rounds, reps=50):
    L = N.lib()
    st = DC.bench_stream()
    nets = {h: DC.Net([OBS, h, h, h, 1]) for h in (256, 512)}
    legs = {f"net_pack_{h}x3": (lambda v=v: N.check(L.rlppo_net_pack(st, v.dims_c, v.nl, P(v.flat), P(v.packed)))) for h, v in nets.items()}
    o = DC.alternate(legs, rounds, reps)
    o["unit"] = "us per rlppo_net_pack of the critic (obs %d, one output; device events, %d calls per measurement): once per iteration" % (OBS, reps)
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its own librlppo.so)")
    ap.add_argument("--bench-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    record = {"device": torch.cuda.get_device_name(0), "build_id": N.lib().rlppo_build_id().decode(), "rounds": a.rounds}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(record, f, indent=1)
    for key, fn in (("update_us_n_w_256", lambda: update_leg(a.rounds, 256)), ("update_us_n_w_512", lambda: update_leg(a.rounds, 512)),
                    ("critic_repack_us", lambda: repack_leg(a.rounds))):
        record[key] = fn()
        print(key + ":", json.dumps(record[key]), flush=True)
        save()
    torch.cuda.empty_cache()
    if a.parent:
        record["bench_headline"] = VC.bench_leg(a.bench_rounds, a.parent)
        print("bench.py headline:", json.dumps(record["bench_headline"]), flush=True)
        save()


if __name__ == "__main__":
    main()
