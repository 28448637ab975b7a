"""The entry layer's answers, table-wise, on the CPU: what every exported form of the PPO pass, the GAE scan, the fused optimiser
step, the KL gate and the workspace sizes returns -- (return value, rlppo_last_error() text) -- for each optional part absent,
present or malformed.  No call can reach a launch: every pass carries a slot beyond RLPPO_MAX_SLOTS (the last argument check, as in
tests/test_multidiscrete_nvec_host.py) and every other call fails a check or has nothing to do.

The expected answers (tests/golden/entry_layer_answers.json) were recorded once, with `answers()` below, from the library of commit
35f7616 -- the last one whose exported forms were a fall-through ladder -- and are compared exactly: the entry layer may be
rearranged, its answers may not move."""
import ctypes
import itertools
import json
import os

from rlgym_ppo_amd import _native as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entry_layer_answers.json")
SLOT_BEYOND = 99
I32P = ctypes.POINTER(ctypes.c_int32)
# head -> (policy outputs, act_dim)
HEADS = {N.HEAD_DISCRETE: (90, 1), N.HEAD_MULTIDISCRETE: (21, 8), N.HEAD_GAUSSIAN: (16, 8), N.HEAD_DIAG_GAUSSIAN: (6, 6)}
REFERENCE_BINS, OTHER_BINS = (3, 3, 3, 3, 3, 2, 2, 2), (2, 7, 3, 11, 2)
FAKE = 0x100000   # placeholder addresses: 16-byte aligned, distinct, never dereferenced
CRITIC_WIDTH, CRITIC_LD = 29, 32


def _answer(L, rc):
    return [int(rc), L.rlppo_last_error().decode() if rc else ""]


def _args(L, head, critic_width=None, precision=N.PRECISION_FP32, keep=None):
    n_out, act_dim = HEADS[head]
    pol, val = N.dims_array([107, 128, 128, n_out]), N.dims_array([critic_width or 107, 128, 128, 1])
    keep.extend((pol, val))
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.slot, a.precision = head, 3, 3, act_dim, SLOT_BEYOND, precision
    a.pol_dims, a.val_dims = ctypes.cast(pol, I32P), ctypes.cast(val, I32P)
    for k, f in enumerate(("pol_packed", "val_packed", "pol_grad", "val_grad", "states", "actions", "old_logp", "targets", "advantages",
                           "idx", "stats", "workspace", "pol_wb16", "val_wb16")):
        setattr(a, f, FAKE + 0x1000 * k)
    a.ld_states, a.n_rows, a.mb = 112, 2048, 300
    a.clip_range, a.ent_coef, a.mb_ratio, a.var_m, a.var_b = 0.2, 0.005, 1.0, 1.0, 0.0
    a.ws_bytes = L.rlppo_minibatch_workspace_bytes_critic(pol, 3, val, 3, a.mb, precision)   # (the larger plan: enough for every form)
    return a


def _ext(kind, keep):
    """The rlppo_minibatch_ext of a case; None = a NULL pointer."""
    if kind == "null":
        return None
    e = N.MinibatchExt()
    if kind == "bytes_only":
        e.scratch_bytes = 64
    elif kind in ("diag", "scratch_misaligned"):
        e.log_std, e.log_std_grad, e.scratch_bytes = FAKE + 0x20000, FAKE + 0x21000, 1 << 20
        e.scratch = FAKE + 0x22000 + (4 if kind == "scratch_misaligned" else 0)
    elif kind == "nvec":
        nv = N.dims_array(REFERENCE_BINS)
        keep.append(nv)
        e.md_nvec, e.md_heads = ctypes.cast(nv, I32P), len(REFERENCE_BINS)
    elif kind == "tanh":
        e.pol_hidden_act = N.ACT_TANH
    elif kind == "bad_act":
        e.val_hidden_act = 7
    else:
        assert kind == "zeroed"
    return e


def _critic(kind):
    if kind == "null":
        return None
    c = N.CriticRows()
    c.ld_states = CRITIC_LD
    if kind != "no_states":
        c.states = FAKE + 0x30000 + (4 if kind == "misaligned" else 0)
    if kind == "bad_ld":
        c.ld_states = 30
    return c


def _vnorm(kind):
    if kind == "null":
        return None
    v = N.ValueNormArg()
    if kind != "no_scale":
        v.scale = FAKE + 0x40000 + (4 if kind == "misaligned" else 0)
    return v


EXT_KINDS = ("null", "zeroed", "bytes_only", "diag", "scratch_misaligned", "nvec", "tanh", "bad_act")
CRITIC_KINDS = ("null", "no_states", "states", "misaligned", "bad_ld")
VNORM_KINDS = ("null", "no_scale", "scale", "misaligned")


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _pass_answers(L, out):
    keep = []
    for head in HEADS:
        a = _args(L, head, keep=keep)
        out[f"plain/head{head}"] = _answer(L, L.rlppo_ppo_minibatch(None, ctypes.byref(a)))
        for name, bins in (("null", None), ("reference", REFERENCE_BINS), ("other", OTHER_BINS), ("no_heads", ())):
            nv = None if bins is None else N.dims_array(bins or REFERENCE_BINS)
            out[f"nvec/head{head}/{name}"] = _answer(L, L.rlppo_ppo_minibatch_nvec(None, ctypes.byref(a), nv, len(bins or ())))
        ok = dict(log_std=FAKE + 0x20000, log_std_grad=FAKE + 0x21000, scratch=FAKE + 0x22000, scratch_bytes=1 << 20)
        for name, change in (("ok", {}), ("no_log_std", dict(log_std=None)), ("no_grad", dict(log_std_grad=None)), ("no_scratch", dict(scratch=None)),
                             ("scratch_misaligned", dict(scratch=FAKE + 0x22004)), ("scratch_small", dict(scratch_bytes=8)),
                             ("bytes_only", dict(log_std=None, log_std_grad=None, scratch=None, scratch_bytes=64))):
            d = dict(ok, **change)
            out[f"diag/head{head}/{name}"] = _answer(L, L.rlppo_ppo_minibatch_diag(None, ctypes.byref(a), d["log_std"], d["log_std_grad"],
                                                                                  d["scratch"], d["scratch_bytes"]))
        for ek, ck, vk in itertools.product(EXT_KINDS, CRITIC_KINDS, VNORM_KINDS):
            e, c, v = _ext(ek, keep), _critic(ck), _vnorm(vk)
            # the critic observes its own width wherever its rows are given
            a = _args(L, head, critic_width=CRITIC_WIDTH if ck not in ("null", "no_states") else None, keep=keep)
            if ck == "null" and vk == "null":
                out[f"ex/head{head}/{ek}"] = _answer(L, L.rlppo_ppo_minibatch_ex(None, ctypes.byref(a), _ref(e)))
            if vk == "null":
                out[f"critic/head{head}/{ek}/{ck}"] = _answer(L, L.rlppo_ppo_minibatch_critic(None, ctypes.byref(a), _ref(e), _ref(c)))
            out[f"vnorm/head{head}/{ek}/{ck}/{vk}"] = _answer(L, L.rlppo_ppo_minibatch_vnorm(None, ctypes.byref(a), _ref(e), _ref(c), _ref(v)))
    # the other update precisions where an optional part refuses them (bf16 with critic rows, tanh outside fp32) or needs their images
    for prec, ek, ck in itertools.product((N.PRECISION_DEFAULT, N.PRECISION_BF16, N.PRECISION_X3, 4), ("zeroed", "tanh"), ("null", "states")):
        a = _args(L, N.HEAD_DISCRETE, critic_width=CRITIC_WIDTH if ck == "states" else None, precision=prec, keep=keep)
        e, c, v = _ext(ek, keep), _critic(ck), _vnorm("scale")
        out[f"precision{prec}/ex/{ek}"] = _answer(L, L.rlppo_ppo_minibatch_ex(None, ctypes.byref(a), _ref(e)))
        out[f"precision{prec}/critic/{ek}/{ck}"] = _answer(L, L.rlppo_ppo_minibatch_critic(None, ctypes.byref(a), _ref(e), _ref(c)))
        out[f"precision{prec}/vnorm/{ek}/{ck}"] = _answer(L, L.rlppo_ppo_minibatch_vnorm(None, ctypes.byref(a), _ref(e), _ref(c), _ref(v)))
    # NULL args through every form; mb == 0 (nothing to do) behind a misaligned scratch
    e, c, v = _ext("diag", keep), _critic("states"), _vnorm("scale")
    out["null_args/plain"] = _answer(L, L.rlppo_ppo_minibatch(None, None))
    out["null_args/nvec"] = _answer(L, L.rlppo_ppo_minibatch_nvec(None, None, None, 0))
    out["null_args/diag"] = _answer(L, L.rlppo_ppo_minibatch_diag(None, None, None, None, None, 0))
    out["null_args/diag_misaligned"] = _answer(L, L.rlppo_ppo_minibatch_diag(None, None, None, None, 4, 0))
    out["null_args/ex"] = _answer(L, L.rlppo_ppo_minibatch_ex(None, None, _ref(e)))
    out["null_args/critic"] = _answer(L, L.rlppo_ppo_minibatch_critic(None, None, _ref(e), _ref(c)))
    out["null_args/vnorm"] = _answer(L, L.rlppo_ppo_minibatch_vnorm(None, None, _ref(e), _ref(c), _ref(v)))
    a = _args(L, N.HEAD_DISCRETE, keep=keep)
    a.mb = 0
    for ek in ("null", "scratch_misaligned"):
        e = _ext(ek, keep)
        out[f"no_rows/ex/{ek}"] = _answer(L, L.rlppo_ppo_minibatch_ex(None, ctypes.byref(a), _ref(e)))
        out[f"no_rows/vnorm/{ek}"] = _answer(L, L.rlppo_ppo_minibatch_vnorm(None, ctypes.byref(a), _ref(e), None, _ref(v)))


def _gae_answers(L, out):
    p = [FAKE + 0x1000 * k for k in range(10)]   # rews, dones, truncated, values, boot, scale, targets, advantages, returns, workspace
    for name, n, drop in (("no_rows", 0, ()), ("negative_rows", -1, ()), ("no_rews", 1000, (0,)), ("no_values", 1000, (3,)), ("no_targets", 1000, (6,)),
                          ("no_advantages", 1000, (7,)), ("no_returns", 1000, (8,)), ("no_workspace", 1000, (9,)), ("no_outputs", 1000, (6, 7, 8))):
        q = [None if k in drop else x for k, x in enumerate(p)]
        out[f"gae/{name}"] = _answer(L, L.rlppo_gae(None, q[0], q[1], q[2], q[3], n, 0.99, 0.95, 1.0, q[6], q[7], q[8], q[9], 1 << 20))
        for boot in (None, q[4]):
            tag = f"{name}/boot{int(boot is not None)}"
            out[f"gae_boot/{tag}"] = _answer(L, L.rlppo_gae_boot(None, q[0], q[1], q[2], q[3], boot, n, 0.99, 0.95, 1.0, q[6], q[7], q[8], q[9], 1 << 20))
            for scale in (None, q[5]):
                out[f"gae_norm/{tag}/scale{int(scale is not None)}"] = _answer(
                    L, L.rlppo_gae_norm(None, q[0], q[1], q[2], q[3], boot, scale, n, 0.99, 0.95, 1.0, q[6], q[7], q[8], q[9], 1 << 20))


def _opt_net(keep, **change):
    dims = N.dims_array([107, 128, 128, 90])
    keep.append(dims)
    d = N.OptNet()
    d.dims, d.n_layers = ctypes.cast(dims, I32P), 3
    for k, f in enumerate(("params", "grads", "exp_avg", "exp_avg_sq", "packed", "gnorm2")):
        setattr(d, f, FAKE + 0x1000 * k)
    d.max_norm, d.lr, d.beta1, d.beta2, d.eps, d.step = 0.5, 3e-4, 0.9, 0.999, 1e-8, 1
    for f, v in change.items():
        setattr(d, f, v)
    return d


def _optimizer_answers(L, out):
    keep = []
    good, rate = _opt_net(keep), FAKE + 0x50000
    nets = {"no_a": (None, good), "no_b": (good, None), "no_params": (_opt_net(keep, params=None), good), "step0": (good, _opt_net(keep, step=0)),
            "no_layers": (_opt_net(keep, n_layers=0), good)}
    for name, (a, b) in nets.items():
        out[f"pack2/{name}"] = _answer(L, L.rlppo_clip_adam_pack2(None, _ref(a), _ref(b), None))
        for tails in ((0, 0), (6, 0), (-1, 0), (0, -2)):
            out[f"pack2_tail/{name}/{tails}"] = _answer(L, L.rlppo_clip_adam_pack2_tail(None, _ref(a), _ref(b), None, *tails))
            for rname, rates in (("null", (None, None)), ("aligned", (rate, rate + 8)), ("a_misaligned", (rate + 4, rate + 8)), ("b_misaligned", (rate, rate + 12))):
                out[f"pack2_lr/{name}/{tails}/{rname}"] = _answer(L, L.rlppo_clip_adam_pack2_lr(None, _ref(a), _ref(b), None, *tails, *rates))
    # sound descriptors: only what fails a later check may be called
    for tails in ((-1, 0), (0, -2)):
        out[f"pack2_tail/good/{tails}"] = _answer(L, L.rlppo_clip_adam_pack2_tail(None, _ref(good), _ref(good), None, *tails))
        out[f"pack2_lr/good/{tails}"] = _answer(L, L.rlppo_clip_adam_pack2_lr(None, _ref(good), _ref(good), None, *tails, rate, rate + 8))
    out["pack2_lr/good/misaligned"] = _answer(L, L.rlppo_clip_adam_pack2_lr(None, _ref(good), _ref(good), None, 0, 0, rate, rate + 4))


def _gate(**change):
    g = N.KlGateArgs()
    g.kl_slots, g.slot_stride, g.n_passes, g.phase, g.threshold = FAKE, 8, 2, 0, 0.03
    g.exchange, g.stop_word, g.host_words, g.batch, g.done_value = FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, 1, 1
    for f, v in change.items():
        setattr(g, f, v)
    return g


def _adapt(**change):
    l = N.LrAdaptArgs()
    l.lr, l.n_lr, l.desired_kl, l.factor, l.lr_min, l.lr_max = FAKE + 0x4000, 2, 0.01, 1.5, 1e-5, 1e-2
    for f, v in change.items():
        setattr(l, f, v)
    return l


def _gate_answers(L, out):
    gates = {"no_slots": dict(kl_slots=None), "negative_passes": dict(n_passes=-1), "stride2": dict(slot_stride=2), "phase3": dict(phase=3),
             "phase_negative": dict(phase=-1), "no_stop_word": dict(stop_word=None), "phase1_no_exchange": dict(phase=1, exchange=None),
             "phase2_no_exchange": dict(phase=2, exchange=None), "no_host_words": dict(host_words=None),
             "phase2_no_host_words": dict(phase=2, host_words=None), "no_stop_no_host": dict(stop_word=None, host_words=None)}
    out["kl_gate/null"] = _answer(L, L.rlppo_kl_gate(None, None))
    for name, change in gates.items():
        g = _gate(**change)
        out[f"kl_gate/{name}"] = _answer(L, L.rlppo_kl_gate(None, ctypes.byref(g)))
    # the _lr form: every gate case before a NULL and a sound adapt struct would launch once accepted, so the sound gate cases that
    # rlppo_kl_gate_lr accepts (no stop word, no host words) meet a malformed adapt struct: its text shows they got that far
    out["kl_gate_lr/null/null"] = _answer(L, L.rlppo_kl_gate_lr(None, None, None))
    for name, change in dict(gates, sound={}).items():
        g = _gate(**change)
        out[f"kl_gate_lr/{name}/null"] = _answer(L, L.rlppo_kl_gate_lr(None, ctypes.byref(g), None))
        l = _adapt(n_lr=0)
        out[f"kl_gate_lr/{name}/no_rates"] = _answer(L, L.rlppo_kl_gate_lr(None, ctypes.byref(g), ctypes.byref(l)))
    adapts = {"no_lr": dict(lr=None), "lr_misaligned": dict(lr=FAKE + 0x4004), "too_many": dict(n_lr=99), "kl_zero": dict(desired_kl=0.0),
              "kl_nan": dict(desired_kl=float("nan")), "factor_one": dict(factor=1.0), "min_zero": dict(lr_min=0.0), "bounds_reversed": dict(lr_min=1e-2, lr_max=1e-5),
              "max_inf": dict(lr_max=float("inf"))}
    g = _gate(stop_word=None, host_words=None)
    for name, change in adapts.items():
        l = _adapt(**change)
        out[f"kl_gate_lr/sound/{name}"] = _answer(L, L.rlppo_kl_gate_lr(None, ctypes.byref(g), ctypes.byref(l)))


def _workspace_answers(L, out):
    shapes = {"small": ([107, 128, 128, 90], [29, 128, 128, 1], 300), "large": ([231, 256, 256, 256, 21], [40, 512, 1], 65536),
              "no_rows": ([107, 128, 128, 90], [107, 128, 128, 1], -5), "bad_dims": ([107, 0, 90], [107, 128, 1], 300)}
    for name, (pol, val, mb) in shapes.items():
        p, v = N.dims_array(pol), N.dims_array(val)
        out[f"workspace/{name}"] = [int(L.rlppo_minibatch_workspace_bytes(p, len(pol) - 1, v, len(val) - 1, mb)), ""]
        for prec in (0, 1, 2, 3, 4):
            out[f"workspace_for/{name}/precision{prec}"] = [int(L.rlppo_minibatch_workspace_bytes_for(p, len(pol) - 1, v, len(val) - 1, mb, prec)), ""]
            out[f"workspace_critic/{name}/precision{prec}"] = [int(L.rlppo_minibatch_workspace_bytes_critic(p, len(pol) - 1, v, len(val) - 1, mb, prec)), ""]
    out["workspace/null_dims"] = [int(L.rlppo_minibatch_workspace_bytes(None, 3, None, 3, 300)), ""]


def answers():
    """case -> [return value, error text ("" where the call succeeds: the text is then the previous call's)]."""
    L, out = N.lib(), {}
    before = int(L.rlppo_get_update_precision())
    L.rlppo_set_update_precision(0)   # the process default the precision-0 cases resolve to
    try:
        for part in (_pass_answers, _gae_answers, _optimizer_answers, _gate_answers, _workspace_answers):
            part(L, out)
    finally:
        L.rlppo_set_update_precision(before)
    return out


def test_entry_layer_answers_are_the_recorded_ones():
    want = json.load(open(GOLDEN))
    got = answers()
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, (len(wrong), sorted(wrong.items())[:5])
    # the table covers what it is meant to: no pass got as far as a launch, and each layer of the ladder gave its name to a text
    passes = {k: v for k, v in want.items() if k.split("/")[0] in ("plain", "nvec", "diag", "ex", "critic", "vnorm")}
    assert len(passes) > 800 and all(rc == 1001 for rc, _ in passes.values())
    reached_slot = [k for k, (_, msg) in passes.items() if f"slot {SLOT_BEYOND}" in msg]
    assert {k.split("/")[0] for k in reached_slot} == {"plain", "nvec", "diag", "ex", "critic", "vnorm"}
    for who in ("ppo_minibatch_ex", "ppo_minibatch_critic", "ppo_minibatch_vnorm", "ppo_minibatch_diag"):
        assert any(msg == f"{who}: scratch must be 8-byte aligned" for _, msg in want.values()), who
    for text in ("gae: bad argument", "gae_boot: bad argument", "gae_norm: bad argument", "kl_gate: host_words missing",
                 "kl_gate_lr: phases 1 and 2 need the exchange words", "clip_adam_pack2_lr: a rate must be 8-byte aligned"):
        assert any(msg == text for _, msg in want.values()), text
    assert want["gae_norm/no_rews/boot1/scale0"][1] == "gae_boot: bad argument"   # no scale: the call is rlppo_gae_boot
