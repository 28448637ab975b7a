"""The critic's own observations on the GPU (asymmetric actor-critic; include/rlppo.h "[critic rows]"): the two-matrix gather launch,
one update pass through rlppo_ppo_minibatch_critic in every form, PPOLearner.learn on a buffer with critic_states and the Learner loop
with critic_observations=True through the three collect paths of the vector manager.

Two kinds of claim.  Where the critic's matrix is a copy of the policy's, everything must equal the symmetric run BIT FOR BIT (same
launches on the same numbers).  Where the widths differ (policy 13, critic 29) the pass is held to float64 under the project's rule,
err(HIP, fp64) <= max(1e-5, 1.5 x err(float32 yardstick, fp64)): tanh / ELU against tests/ppo_yardstick.py; ReLU, whose two
chains are independent, bit for bit against two symmetric passes (one per matrix, with a dummy partner) and per network through
tests/fp64_gate.py under the pass's own ReLU decisions."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets  # noqa: E402
import critic_obs_env as CE  # noqa: E402
import fp64_gate  # noqa: E402
import ppo_yardstick as A  # noqa: E402
from diag_gaussian_yardstick import assert_clear_of_clip_edges  # noqa: E402
from hip_pass import L, P, check, dev, run_pass, stream  # noqa: E402,F401

CLIP, ENT = 0.2, 0.005
OBS, COBS = CE.OBS, CE.CRITIC_OBS
C_PASS, C_PAIRED, C_FUSED, C_GROUP, C_CRITIC = 2, 3, 4, 5, 15   # 15 = rlppo_dbg_counter: passes with separate critic rows


def counters(L, *keys):
    return [int(L.rlppo_dbg_counter(k)) for k in keys]


@contextlib.contextmanager
def switches(L, **kv):
    """rlppo_dbg_set(key, value) for the block; the defaults (26: 1, 37: 1, 29: 1) afterwards."""
    try:
        for k, v in kv.items():
            check(L, L.rlppo_dbg_set(int(k[1:]), v))
        yield
    finally:
        for k in kv:
            check(L, L.rlppo_dbg_set(int(k[1:]), 1))


# ------------------------------------------------------------------------------------------------ 1. the gather launch
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("n", [1, 300])
def test_gather_rows2_equals_numpy_indexing(L, n, ring):
    """Policy width 12 (3 chunks) + critic width 16 (4 chunks): 7 chunks per row, so a 256-thread block straddles rows and the boundary
    between the two sources; source lds larger than the widths; 37 source rows, as a ring with base 29 (rows wrap) or plain; the
    destinations and the scalars sit inside guard bands that must come back untouched; zero_n is zeroed."""
    from rlgym_ppo_amd import _native as N
    rs = np.random.RandomState(7 + n)
    rows, wp, wc, ldp, ldc, k, G, S = 37, 12, 16, 20, 24, 2, 64, -777.0
    src_p, src_c = rs.randn(rows, ldp).astype(np.float32), rs.randn(rows, ldc).astype(np.float32)
    acts, old, adv, tgt = rs.randn(rows, k).astype(np.float32), rs.randn(rows).astype(np.float32), rs.randn(rows).astype(np.float32), rs.randn(rows).astype(np.float32)
    idx = rs.randint(0, rows, n).astype(np.int64)
    base, cap = (29, rows) if ring else (0, 0)
    phys = (idx + base) % rows if ring else idx
    band = lambda m: torch.full((G + m + G,), S, device="cuda")
    out = dict(p=band(n * wp), c=band(n * wc), act=band(n * k), old=band(n), adv=band(n), tgt=band(n), zero=band(n))
    inner = lambda t: ctypes.c_void_p(t.data_ptr() + 4 * G)
    keep = [dev(x) for x in (src_p, src_c, acts, old, adv, tgt)] + [dev(idx, torch.int64)]
    g = N.Gather2Args()
    g.src, g.ld_src, g.dst, g.width = keep[0].data_ptr(), ldp, inner(out["p"]), wp
    g.critic_src, g.critic_ld_src, g.critic_dst, g.critic_width = keep[1].data_ptr(), ldc, inner(out["c"]), wc
    g.idx, g.n, g.ring_base, g.ring_cap = keep[6].data_ptr(), n, base, cap
    g.actions, g.old_logp, g.advantages, g.targets, g.act_dim = keep[2].data_ptr(), keep[3].data_ptr(), keep[4].data_ptr(), keep[5].data_ptr(), k
    g.g_act, g.g_old, g.g_adv, g.g_tgt, g.zero_n = inner(out["act"]), inner(out["old"]), inner(out["adv"]), inner(out["tgt"]), inner(out["zero"])
    check(L, L.rlppo_gather_rows2(stream(), ctypes.byref(g)))
    torch.cuda.synchronize()
    want = dict(p=src_p[phys, :wp], c=src_c[phys, :wc], act=acts[phys], old=old[phys], adv=adv[phys], tgt=tgt[phys], zero=np.zeros(n, np.float32))
    for name, t in out.items():
        got = t.cpu().numpy()
        assert (got[:G] == S).all() and (got[-G:] == S).all(), f"{name}: a guard band was written"
        assert np.array_equal(got[G:-G].view(np.uint32), np.ascontiguousarray(want[name]).reshape(-1).view(np.uint32)), name
    # without the scalars: the rows alone, nothing else touched
    for name in ("p", "c"):
        out[name].fill_(S)
    g.actions = g.old_logp = g.advantages = g.targets = g.g_act = g.g_old = g.g_adv = g.g_tgt = g.zero_n = None
    before = {name: out[name].clone() for name in ("act", "old", "adv", "tgt", "zero")}
    check(L, L.rlppo_gather_rows2(stream(), ctypes.byref(g)))
    torch.cuda.synchronize()
    assert np.array_equal(out["p"].cpu().numpy()[G:-G], src_p[phys, :wp].reshape(-1)) and np.array_equal(out["c"].cpu().numpy()[G:-G], src_c[phys, :wc].reshape(-1))
    assert all(torch.equal(out[name], t) for name, t in before.items())


# ------------------------------------------------------------------------------------------------ 2. alias, bit for bit
def make_case(head, seed, act, pol_hidden=(64, 128), val_hidden=(32, 64), n=420, critic_width=OBS, masked=True):
    """tests/test_gpu_hidden_activation.py::make_case with a critic matrix: critic_width == OBS: a copy of the policy's rows (the alias
    case); else the rows ++ (critic_width - OBS) further features, and a critic built on that width.  masked: the discrete head with an action mask."""
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    n_out = {"discrete": 6, "diag": 3}[head]
    pol, val = nets.init_mlp(OBS, pol_hidden, n_out), nets.init_mlp(critic_width, val_hidden, 1)
    obs = np.clip(rs.randn(n, OBS), -5, 5).astype(np.float32)
    cobs = obs.copy() if critic_width == OBS else np.concatenate([obs, np.clip(rs.randn(n, critic_width - OBS) * 2 + 0.5, -5, 5).astype(np.float32)], 1)
    hk, log_std, mask = {}, None, None
    if head == "discrete":
        act_ = rs.randint(0, n_out, n).astype(np.float32)
    if head == "discrete" and masked:
        mask = rs.rand(n, n_out) < 0.7
        mask[np.arange(n), act_.astype(int)] = True   # stored actions are valid
        mask[3::5] = True
    if head == "diag":
        log_std = rs.uniform(-1.0, 0.5, n_out).astype(np.float32)
        act_ = (A.forward64(pol, obs, act) + np.exp(log_std.astype(np.float64)) * rs.randn(n, n_out)).astype(np.float32)
    z = torch.as_tensor(A.forward64(pol, obs, act))
    if mask is not None:
        z = z.masked_fill(~torch.as_tensor(mask), float("-inf"))
    ls64 = None if log_std is None else torch.as_tensor(log_std, dtype=torch.float64)
    logp = A.head_terms(head, z, torch.as_tensor(act_, dtype=torch.float64), log_std=ls64)[0].numpy()
    cls = np.arange(n) % 3
    off = 0.05 * rs.randn(n) + np.where(cls == 1, -0.5, 0.0) + np.where(cls == 2, 0.5, 0.0)
    return dict(head=head, pol=pol, val=val, obs=obs, cobs=cobs, act=act_, log_std=log_std, mask=mask, act_name=act,
                old=(logp + off).astype(np.float32), adv=rs.randn(n).astype(np.float32), tgt=rs.randn(n).astype(np.float32), rs=rs)


def run(L, c, idx, entry, mb_ratio=1.0, **kw):
    kw.setdefault("pol", c["pol"])
    kw.setdefault("val", c["val"])
    kw.setdefault("obs_all", c["obs"])
    kw.setdefault("cobs_all", c["cobs"])
    pol, val, obs_all, cobs_all = (kw.pop(k) for k in ("pol", "val", "obs_all", "cobs_all"))
    kw.setdefault("precision", "fp32")
    return run_pass(L, pol, val, obs_all, c["act"], c["old"], c["tgt"], c["adv"], idx, head=c["head"], entry=entry, pol_act=c["act_name"],
                    val_act=c["act_name"], clip=CLIP, ent=ENT, mb_ratio=mb_ratio, cobs=cobs_all, log_std=c["log_std"], mask=c["mask"],
                    raise_rc=False, **kw)


def same(a, b):
    return torch.equal(a["gp"], b["gp"]) and torch.equal(a["gv"], b["gv"]) and np.array_equal(a["stats"], b["stats"])


FORMS = {   # name -> (hidden activation, policy hidden, critic hidden, switches, precision, gather-fused?)
    "default": ("relu", (64, 128), (32, 64), {}, "fp32", False),
    "gather_fused": ("relu", (128, 128), (128, 64), {"k26": 2}, "fp32", True),   # (first layers of 128: the widths that form takes)
    "plain_tanh": ("tanh", (64, 128), (32, 64), {}, "fp32", False),
    "x3": ("relu", (256, 256), (256, 256), {}, "x3", False),                     # (256-wide layers: the widths the split kernels take)
}


@pytest.mark.parametrize("head", ["discrete", "diag"])
@pytest.mark.parametrize("form", list(FORMS))
def test_alias_pass_is_the_symmetric_pass_bit_for_bit(L, form, head):
    """mb = 300 of a 420-row ring-mapped buffer (base 137), accumulating into non-zero gradients: the critic's matrix a separate copy
    of `states` at another leading dimension.  Gradient arenas and statistics equal rlppo_ppo_minibatch_ex's on the one matrix, bit
    for bit; counter 15 shows which path ran; critic == NULL and critic->states == NULL are the old path."""
    act, ph, vh, sw, prec, fused = FORMS[form]
    c = make_case(head, 61 + len(form), act, ph, vh)
    idx = c["rs"].permutation(len(c["obs"]))[:300]
    g = torch.Generator().manual_seed(5)
    n_pol = int(nets.flatten(c["pol"]).numel()) + (3 if head == "diag" else 0)
    gp0, gv0 = torch.randn(n_pol, generator=g).cuda(), torch.randn(int(nets.flatten(c["val"]).numel()), generator=g).cuda()
    grads = lambda: (gp0.clone(), gv0.clone())
    kw = dict(ring=137, precision=prec, mb_ratio=0.5)
    with switches(L, **sw):
        c0 = counters(L, C_PASS, C_PAIRED, C_FUSED, C_CRITIC)
        sym = run(L, c, idx, "ex", grads=grads(), **kw)
        c1 = counters(L, C_PASS, C_PAIRED, C_FUSED, C_CRITIC)
        asym = run(L, c, idx, "critic", grads=grads(), critic_ld=24, **kw)     # (padded width 16; 24 is another leading dimension)
        c2 = counters(L, C_PASS, C_PAIRED, C_FUSED, C_CRITIC)
        nulls = [run(L, c, idx, e, grads=grads(), **kw) for e in ("critic_null", "critic_null_states")]
        c3 = counters(L, C_PASS, C_PAIRED, C_FUSED, C_CRITIC)
    assert sym["rc"] == 0 and asym["rc"] == 0 and all(r["rc"] == 0 for r in nulls), (sym["msg"], asym["msg"])
    assert [b - a for a, b in zip(c0, c1)] == [1, 0, int(fused), 0]
    assert [b - a for a, b in zip(c1, c2)] == [1, 0, int(fused), 1]
    assert [b - a for a, b in zip(c2, c3)] == [2, 0, 2 * int(fused), 0]
    assert same(asym, sym) and all(same(r, sym) for r in nulls)
    assert not torch.equal(sym["gp"], gp0) and not torch.equal(sym["gv"], gv0) and torch.isfinite(sym["gp"]).all() and torch.isfinite(sym["gv"]).all()


def test_alias_pass_never_pairs(L):
    """Pairing forced "always" (switch 29 = 2) on twin networks: the symmetric pass pairs, the pass with separate critic rows does not
    (a paired layer 0 shares one A operand) and still computes the same gradients up to the summation order of the forms."""
    c = make_case("discrete", 67, "relu", (128, 128), (128, 128))
    idx = c["rs"].permutation(len(c["obs"]))[:300]
    with switches(L, k29=2):
        c0 = counters(L, C_PAIRED, C_CRITIC)
        sym = run(L, c, idx, "ex")
        c1 = counters(L, C_PAIRED, C_CRITIC)
        asym = run(L, c, idx, "critic")
        c2 = counters(L, C_PAIRED, C_CRITIC)
    assert sym["rc"] == 0 and asym["rc"] == 0
    assert [b - a for a, b in zip(c0, c1)] == [1, 0] and [b - a for a, b in zip(c1, c2)] == [0, 1]
    assert A.err(A.tensors(asym), A.tensors(sym)) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. two widths, no discrete decision
@pytest.mark.parametrize("act", ["tanh", "elu"])
@pytest.mark.parametrize("head", ["discrete", "diag"])
def test_two_widths_against_float64(L, head, act):
    """Policy width 13, critic width 29, tanh / ELU (no hidden decision is discrete: ppo_yardstick's docstring); also from a
    ring-mapped buffer and with n_rows == 0, bit-identical."""
    c = make_case(head, 71, act, critic_width=COBS, masked=False)
    idx = c["rs"].permutation(len(c["obs"]))[:300]
    args = (c["pol"], c["val"], c["obs"][idx], c["act"][idx], c["old"][idx], c["adv"][idx], c["tgt"][idx], CLIP, ENT, 0.5)
    r64, r32 = (A.minibatch(dt, head, *args, pol_act=c["act_name"], val_act=c["act_name"], cobs=c["cobs"][idx], log_std=c["log_std"])
                for dt in (torch.float64, torch.float32))
    assert_clear_of_clip_edges(r64["ratio"], CLIP)
    c0 = counters(L, C_PASS, C_PAIRED, C_FUSED, C_CRITIC)
    got = run(L, c, idx, "critic", mb_ratio=0.5)
    assert got["rc"] == 0, got["msg"]
    assert [b - a for a, b in zip(c0, counters(L, C_PASS, C_PAIRED, C_FUSED, C_CRITIC))] == [1, 0, 0, 1]
    A.gate(got, r64, r32, f"[act fp64 gate] critic rows 13 / 29, {head} {act}")
    for kw in (dict(ring=137), dict(n_rows=0)):
        other = run(L, c, idx, "critic", mb_ratio=0.5, **kw)
        assert other["rc"] == 0 and same(other, got), kw


# ------------------------------------------------------------------------------------------------ 4. two widths, ReLU
def test_two_widths_relu_chains_are_independent(L):
    """Policy (13, 128, 128, 6) on its matrix, critic (29, 128, 64, 1) on its own.  Grouped dW off and the gather pass forced: each
    network's gradient is, bit for bit, that of a SYMMETRIC pass on its matrix with a dummy partner (the chains are independent and
    take the same launches), and so are its statistics.  Then the default form and the forced gather-fused form: the forward-only
    statistics bit-identical to that run, the gradients held to float64 per network under the pass's own ReLU decisions."""
    c = make_case("discrete", 73, "relu", (128, 128), (128, 64), critic_width=COBS, masked=False)   # (fp64_gate restates the unmasked head)
    torch.manual_seed(74)
    dummy_val, dummy_pol = nets.init_mlp(OBS, (128, 64), 1), nets.init_mlp(COBS, (128, 128), 6)
    idx = c["rs"].permutation(len(c["obs"]))[:300]
    runs = {}
    for name, sw in (("separate", dict(k37=0, k26=0)), ("default", {}), ("gather_fused", dict(k26=2))):
        with switches(L, **sw):
            c0 = counters(L, C_FUSED, C_GROUP, C_CRITIC)
            asym = run(L, c, idx, "critic")
            moved = [b - a for a, b in zip(c0, counters(L, C_FUSED, C_GROUP, C_CRITIC))]
            on_pol = run(L, c, idx, "ex", val=dummy_val)                               # the policy with a dummy critic, on the policy's matrix
            on_crit = run(L, c, idx, "ex", pol=dummy_pol, obs_all=c["cobs"])           # a dummy policy with the critic, on the critic's matrix
        assert asym["rc"] == 0 and on_pol["rc"] == 0 and on_crit["rc"] == 0, (asym["msg"], on_pol["msg"], on_crit["msg"])
        assert moved == [int(name == "gather_fused"), int(name != "separate"), 1], (name, moved)
        runs[name] = (asym, on_pol, on_crit)
    asym, on_pol, on_crit = runs["separate"]
    assert torch.equal(asym["gp"], on_pol["gp"]) and torch.equal(asym["gv"], on_crit["gv"])
    assert np.array_equal(asym["stats"][[0, 1, 3, 4]], on_pol["stats"][[0, 1, 3, 4]]) and asym["stats"][2] == on_crit["stats"][2]
    assert float(asym["gp"].abs().max()) > 0 and float(asym["gv"].abs().max()) > 0
    rows = lambda x: np.asarray(x)[idx]
    for name in ("default", "gather_fused"):
        a_f, p_f, v_f = runs[name]
        assert np.array_equal(a_f["stats"][:5], asym["stats"][:5]), name          # forward-only: the same numbers in every form
        common = (rows(c["act"]), rows(c["old"]), rows(c["adv"]), rows(c["tgt"]), CLIP, ENT, 1.0)
        fp64_gate.gate(L, "discrete", c["pol"], dummy_val, rows(c["obs"]), *common, (a_f["grad_policy"], p_f["grad_value"], None),
                       label=f"critic rows, {name}: policy")
        fp64_gate.gate(L, "discrete", dummy_pol, c["val"], rows(c["cobs"]), *common, (v_f["grad_policy"], a_f["grad_value"], None),
                       label=f"critic rows, {name}: critic")


# ------------------------------------------------------------------------------------------------ 5. refusals at the C boundary
def test_refusals_launch_nothing(L):
    """bf16 precision and a workspace sized with the old function: the error code with a message, no pass counted, the gradient
    arenas untouched.  (ld_states too small: tests/test_critic_obs_host.py -- no matrix of that shape can be built here.)"""
    c = make_case("discrete", 79, "relu", critic_width=COBS, masked=False)
    idx = c["rs"].permutation(len(c["obs"]))[:300]
    c0 = counters(L, C_PASS, C_CRITIC)
    r = run(L, c, idx, "critic", precision="bf16")
    assert r["rc"] == 1001 and "bf16" in r["msg"] and "separate critic rows" in r["msg"], r["msg"]
    assert float(r["gp"].abs().max()) == 0 and float(r["gv"].abs().max()) == 0
    r = run(L, c, idx, "critic", ws_fn=L.rlppo_minibatch_workspace_bytes_for)
    assert r["rc"] not in (0, 1001) and "rlppo_minibatch_workspace_bytes_critic" in r["msg"], r["msg"]
    assert float(r["gp"].abs().max()) == 0 and float(r["gv"].abs().max()) == 0
    r = run(L, c, idx, "critic_null")                 # two widths without a matrix: the old refusal
    assert r["rc"] == 1001 and "observe different sizes" in r["msg"]
    assert counters(L, C_PASS, C_CRITIC) == c0


# ------------------------------------------------------------------------------------------------ 6. PPOLearner.learn
LEARN_SEED = 23
N_ROWS, B, MB, EPOCHS, LR = 1024, 512, 128, 2, 3e-4


def learn_inputs(act, critic_width, seed=LEARN_SEED):
    """Initial parameters (the learner's own, checked) and an experience dict made on the CPU alone: stored log-probabilities are the
    float64 yardstick's + N(0, 0.1)."""
    torch.manual_seed(seed)
    pol, val = nets.init_mlp(OBS, (32, 32), 6), nets.init_mlp(critic_width, (32, 32), 1)
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(N_ROWS, OBS), -5, 5).astype(np.float32)
    cobs = np.concatenate([obs, np.clip(rs.randn(N_ROWS, critic_width - OBS) * 2 + 0.5, -5, 5).astype(np.float32)], 1) if critic_width != OBS else obs.copy()
    acts = rs.randint(0, 6, N_ROWS).astype(np.float32)
    z = torch.as_tensor(A.forward64(pol, obs, act))
    logp = A.head_terms("discrete", z, torch.as_tensor(acts, dtype=torch.float64))[0].numpy()
    exp = dict(states=obs, critic_states=cobs, actions=acts, log_probs=(logp + 0.1 * rs.randn(N_ROWS)).astype(np.float32),
               values=rs.randn(N_ROWS).astype(np.float32), advantages=rs.randn(N_ROWS).astype(np.float32))
    return pol, val, exp


def build_learner(act, critic_width, seed=LEARN_SEED):
    from rlgym_ppo_amd.ppo import LayerSizes, ObsSizes, PPOLearner
    torch.manual_seed(seed)
    sizes = LayerSizes((32, 32), act)
    obs_size = OBS if critic_width is None else ObsSizes(OBS, critic_width)
    with contextlib.redirect_stdout(io.StringIO()):
        return PPOLearner(obs_size, 6, 0, sizes, sizes, (0.1, 1.0), B, EPOCHS, LR, LR, CLIP, ENT, MB, "cuda:0")


def buffer_of(exp, critic, seed=LEARN_SEED):
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    buf = ExperienceBuffer(N_ROWS, seed, "cpu")
    z = np.zeros(N_ROWS, np.float32)
    extra = dict(critic_states=exp["critic_states"]) if critic else {}
    buf.submit_experience(exp["states"], exp["actions"], exp["log_probs"], z, exp["states"], z, z, exp["values"], exp["advantages"], **extra)
    return buf


def params_cpu(module):
    return [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in module.arena.linears]


def flats(learner):
    return learner.policy.arena.flat.cpu().numpy().astype(np.float64), learner.value_net.arena.flat.cpu().numpy().astype(np.float64)


def test_learn_with_alias_critic_states_is_learn_without_them(L):
    """A buffer whose critic_states are a copy of its states leaves the same parameters and the same report as the buffer without them,
    bit for bit -- through the new entry point (counter 15) against the old one; the FIFO carries the field like `states`."""
    _, _, exp = learn_inputs("relu", OBS)
    plain, twin = build_learner("relu", None), build_learner("relu", None)
    assert torch.equal(plain.policy.arena.flat, twin.policy.arena.flat)
    c0 = counters(L, C_PASS, C_CRITIC)
    r0 = plain.learn(buffer_of(exp, False))
    c1 = counters(L, C_PASS, C_CRITIC)
    buf = buffer_of(exp, True)
    assert buf.critic_width == OBS and torch.equal(buf.critic_states, buf.states) and buf.ring()[0]["critic_states"].shape == buf.ring()[0]["states"].shape
    r1 = twin.learn(buf)
    c2 = counters(L, C_PASS, C_CRITIC)
    assert c1[0] > c0[0] and c1[1] == c0[1] and c2[0] - c1[0] == c1[0] - c0[0] == c2[1] - c1[1]
    assert torch.equal(plain.policy.arena.flat, twin.policy.arena.flat) and torch.equal(plain.value_net.arena.flat, twin.value_net.arena.flat)
    assert {k: v for k, v in r0.items() if "Time" not in k} == {k: v for k, v in r1.items() if "Time" not in k}
    # the ring: a second submit wraps both matrices alike; clear() forgets the field
    half = {k: v[:N_ROWS // 2] for k, v in exp.items()}
    z = np.zeros(N_ROWS // 2, np.float32)
    buf.submit_experience(half["states"], half["actions"], half["log_probs"], z, half["states"], z, z, half["values"], half["advantages"],
                          critic_states=half["critic_states"])
    assert buf.ring()[1] == N_ROWS // 2 and torch.equal(buf.critic_states, buf.states) and len(buf) == N_ROWS
    buf.clear()
    assert buf.critic_states is None and buf.critic_width is None


def test_learn_refuses_mismatched_buffers(L):
    _, _, exp = learn_inputs("relu", COBS)
    wide = build_learner("relu", COBS)
    flat0 = wide.value_net.arena.flat.clone()
    assert wide.critic_obs_space_size == COBS and wide.value_net.arena.d_in == COBS and wide.policy.arena.d_in == OBS
    assert torch.equal(wide.policy.arena.flat, build_learner("relu", None).policy.arena.flat)   # construction order: the policy's weights as without it
    c0 = counters(L, C_PASS)
    with pytest.raises(ValueError, match="holds no critic_states"):
        wide.learn(buffer_of(exp, False))
    narrow = build_learner("relu", None)
    with pytest.raises(ValueError, match="critic_states have 29 features, the critic observes 13"):
        narrow.learn(buffer_of(exp, True))
    wide.update_precision = "bf16"
    with pytest.raises(ValueError, match="update_precision='bf16' with separate critic observations"):
        wide.learn(buffer_of(exp, True))
    assert counters(L, C_PASS) == c0 and torch.equal(wide.value_net.arena.flat, flat0)


_YARD = {}


def learn_yardstick(pol, val, exp):
    """The float64 and float32 yardsticks of the width-29 tanh learn(): computed once, shared, left unchanged."""
    if "tanh" not in _YARD:
        weakest = {}
        run_ = lambda dt, **kw: A.learn(dt, "discrete", "tanh", pol, val, exp, B, MB, EPOCHS, CLIP, ENT, LR, LR, np.random.RandomState(LEARN_SEED), **kw)
        t = run_(torch.float64, weakest=weakest)
        _YARD["tanh"] = (t[0], t[1], *run_(torch.float32), weakest)
    return _YARD["tanh"]


def learn_errs(p_, v_, yard_):
    """tests/test_gpu_hidden_activation.py::learn_errs (that file's cap and bound): (err over the well-conditioned parameters, worst
    ill-conditioned one as a fraction of its derived bound steps x lr x min(1, 1e-5 / w_i))."""
    t_pol, t_val, _, _, weakest = yard_
    steps = EPOCHS * (N_ROWS // B)
    good = frac = 0.0
    for x, tr, weak in ((p_, t_pol, weakest["pol"]), (v_, t_val, weakest["val"])):
        dlt, bad = np.abs(np.asarray(x, np.float64) - tr), weak < 1e-4
        good = max(good, float(dlt[~bad].max() / np.abs(tr).max()))
        if bad.any():
            bound = steps * LR * np.minimum(1.0, 1e-5 / np.maximum(weak[bad], 1e-300))
            frac = max(frac, float((dlt[bad] / bound).max()))
    return good, frac


def yardstick_for(learner):
    pol, val, exp = learn_inputs("tanh", COBS)
    for mine, theirs in ((pol, params_cpu(learner.policy)), (val, params_cpu(learner.value_net))):   # the CPU-made inputs ARE the learner's
        assert all(torch.equal(w, w2) and torch.equal(b, b2) for (w, b), (w2, b2) in zip(mine, theirs))
    yard_ = learn_yardstick(pol, val, exp)
    t_pol, t_val, f_pol, f_val, weakest = yard_
    n_ill = int((weakest["pol"] < 1e-4).sum() + (weakest["val"] < 1e-4).sum())
    assert n_ill <= 0.05 * (t_pol.size + t_val.size), n_ill          # the cap, from float64 alone, before the GPU result is looked at
    e_32 = learn_errs(f_pol, f_val, yard_)
    assert e_32[1] <= 1.0, e_32                                       # (the seed was chosen on the CPU so that the float32 yardstick stays inside)
    return exp, yard_, e_32, n_ill


def test_learn_two_widths_against_the_float64_yardstick(L):
    """Policy 13, critic 29, tanh, (32, 32) networks, 1024 rows, B 512, MB 128, 2 epochs, lr 3e-4, in the manner of
    tests/test_gpu_hidden_activation.py::test_learn_against_the_float64_yardstick (its cap on ill-conditioned Adam entries, 5 %)."""
    learner = build_learner("tanh", COBS)
    exp, yard_, e_32, n_ill = yardstick_for(learner)
    c0 = counters(L, C_PASS, C_CRITIC)
    report = learner.learn(buffer_of(exp, True))
    c1 = counters(L, C_PASS, C_CRITIC)
    assert report["Cumulative Model Updates"] == EPOCHS * (N_ROWS // B) and c1[0] > c0[0] and c1[1] - c0[1] == c1[0] - c0[0]
    assert all(np.isfinite(float(v)) for v in report.values())
    e_hip = learn_errs(*flats(learner), yard_)
    print(f"[critic rows fp64 gate] learn() 13 / 29 tanh: err(HIP, fp64)={e_hip[0]:.2e}  err(float32 yardstick, fp64)={e_32[0]:.2e}; {n_ill} ill-conditioned "
          f"parameters: HIP at {e_hip[1]:.3f} of the derived bound, float32 yardstick {e_32[1]:.3f}")
    assert e_hip[0] <= max(1e-5, 1.5 * e_32[0]) and e_hip[1] <= 1.0, (e_hip, e_32)


def test_two_virtual_ranks_sum_the_one_rank_gradient():
    """dp.run_virtual_ranks with critic_states: the replicas end bit-identical to each other and within the same rule of the yardstick."""
    from rlgym_ppo_amd import dp
    reps = [build_learner("tanh", COBS) for _ in range(2)]
    exp, yard_, e_32, _ = yardstick_for(reps[0])
    dp.run_virtual_ranks(reps, [buffer_of(exp, True) for _ in range(2)])
    assert torch.equal(reps[0].policy.arena.flat, reps[1].policy.arena.flat) and torch.equal(reps[0].value_net.arena.flat, reps[1].value_net.arena.flat)
    good, frac = learn_errs(*flats(reps[0]), yard_)
    print(f"[critic rows fp64 gate] learn(), two ranks: err(HIP, fp64)={good:.2e}  err(float32 yardstick, fp64)={e_32[0]:.2e}; ill-conditioned at {frac:.3f}")
    assert good <= max(1e-5, 1.5 * e_32[0]) and frac <= 1.0, (good, e_32, frac)


# ------------------------------------------------------------------------------------------------ 7. Learner, vector mode
NA, T, ITERS = 8, 16, 3
PATHS = ("fused", "chain", "device")


def make_learner(tmp_path, path, alias, critic, start=0, iters=ITERS, **kw):
    from rlgym_ppo_amd import Learner
    cfg = dict(vector_env=True, n_proc=1, timestep_limit=iters * NA * T, exp_buffer_size=2 * NA * T, ts_per_iteration=NA * T, ppo_epochs=1,
               ppo_batch_size=NA * T, ppo_minibatch_size=NA * T // 2, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32),
               checkpoints_save_folder=str(tmp_path), add_unix_timestamp=False, checkpoint_load_folder=None, save_every_ts=10 ** 12,
               log_to_wandb=False, random_seed=5, critic_observations=critic)
    cfg.update(kw)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = Learner(CE.make(alias, device=path == "device", start=start, n_agents=NA), **cfg)
    if path == "chain":
        learner.ppo_learner.policy.fused_step = False
    return learner


def run_learner(learner, keep_rows=False):
    rows = []
    plain = learner.add_new_experience

    def spy(experience):
        if keep_rows:
            rows.append(learner.agent.critic_value_input_rows.clone())
        return plain(experience)
    learner.add_new_experience = spy
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            learner._learn()
        p_ = learner.ppo_learner
        state = dict(pol=p_.policy.arena.flat.clone(), val=p_.value_net.arena.flat.clone(), m=p_.policy_optimizer.exp_avg.clone(),
                     vm=p_.value_optimizer.exp_avg.clone(), book=learner.agent.cumulative_timesteps, epoch=learner.epoch,
                     obs_stats=None if learner.agent.obs_stats is None else json_of(learner.agent.obs_stats),
                     critic_stats=None if learner.agent.critic_obs_stats is None else json_of(learner.agent.critic_obs_stats))
        return state, rows
    finally:
        learner.agent.cleanup()


def json_of(stat):
    import json
    return json.loads(json.dumps(stat.to_json()))


def same_state(a, b, keys=None):
    for k in keys or a:
        ok = torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k]
        assert ok, k


@pytest.mark.parametrize("path", PATHS)
def test_alias_environment_is_the_run_without_critic_observations(L, tmp_path, path):
    """critic_observations() == the observation: 3 iterations of 8 agents x 16 steps leave the parameters, the Adam moments and the
    observation statistics of the run without the option, bit for bit; the critic's statistics are the observation's."""
    c0 = counters(L, C_CRITIC)[0]
    off, _ = run_learner(make_learner(tmp_path / "off", path, True, False))
    assert counters(L, C_CRITIC)[0] == c0 and off["critic_stats"] is None       # off: the old entry point, the environment never asked
    on, rows = run_learner(make_learner(tmp_path / "on", path, True, True), keep_rows=True)
    assert counters(L, C_CRITIC)[0] > c0 and on["epoch"] == ITERS and len(rows) == ITERS
    same_state(on, off, ("pol", "val", "m", "vm", "book", "epoch", "obs_stats"))
    assert on["critic_stats"] == on["obs_stats"]


def numpy_rows(iters, per_feature=False):
    """The standardisation cadence restated on the host: the reset answer enters the statistics and is acted on RAW; the answer of every
    step is standardised with the statistics as they stand BEFORE that step's increment (scalars of feature 0: quirk Q5; or per
    feature), clipped to +-5; the statistics move when more than steps_per_obs_stats_increment (5) steps have passed since the last
    move.  -> per collect [N + 1, d_c] trajectory-major rows ++ the last next-state row, and the statistics."""
    from rlgym_ppo_amd.util import WelfordRunningStat
    env = CE.CriticVectorEnv(n_agents=NA)
    st = WelfordRunningStat(COBS)
    x = env.critic_obs_at(0)
    st.increment(x, NA)
    cur, since, t, out = x.copy(), 0, 0, []
    for _ in range(iters):
        CS = np.empty((T + 1, NA, COBS), np.float32)
        CS[0] = cur
        for s in range(T):
            t += 1
            x = env.critic_obs_at(t)
            mean, std = (st.mean.astype(np.float32), st.std.astype(np.float32)) if per_feature else (np.float32(st.mean[0]), np.float32(st.std[0]))
            if since > 5:
                st.increment(x, NA)
                since = 0
            else:
                since += 1
            CS[s + 1] = np.clip((x - mean) / std, np.float32(-5), np.float32(5))
        cur = CS[T]
        out.append(np.concatenate([CS[:T].transpose(1, 0, 2).reshape(NA * T, COBS), CS[T][NA - 1:NA]], 0))
    return out, st


@pytest.mark.parametrize("per_feature", [False, True])
def test_critic_rows_are_the_same_through_the_three_collect_paths(tmp_path, per_feature):
    """Width 29: critic_value_input_rows of every collect, bit for bit the same through the fused, the chain and the device path, equal
    to the numpy restatement of the cadence (rtol 1e-6 / atol 1e-7: the tolerance tests/test_gpu_vector_rollout.py holds the policy's
    rows to, one float32 division per element), padded with zeros; and critic_obs_stats the restatement's."""
    got = {}
    for path in PATHS:
        state, rows = run_learner(make_learner(tmp_path / path, path, False, True, per_feature_obs_standardization=per_feature), keep_rows=True)
        got[path] = (state, [r.cpu().numpy() for r in rows])
    for path in PATHS[1:]:
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[path][1], got["fused"][1])), path
        same_state(got[path][0], got["fused"][0])
    want, st = numpy_rows(ITERS, per_feature)
    for r, w in zip(got["fused"][1], want):
        assert r.shape == (NA * T + 1, 32) and (r[:, COBS:] == 0).all()
        np.testing.assert_allclose(r[:, :COBS], w, rtol=1e-6, atol=1e-7)
    assert got["fused"][0]["critic_stats"] == json_of(st)
    assert got["fused"][0]["critic_stats"] != got["fused"][0]["obs_stats"]


def test_save_load_continue_equals_the_uninterrupted_run(tmp_path):
    """Three iterations against two + a second Learner that loads "latest" and runs the third, bit for bit, in the manner of
    tests/test_gpu_hidden_activation.py's test of the same name: vector mode, the environment restarted at the step the first run
    reached, the host generators carried over, a buffer of one collect (a buffer is not checkpoint state) and standardize_obs=False
    (a fresh manager acts on RAW rows in its first collect).  With standardisation on, what the book holds comes back exactly:
    critic_obs_stats beside obs_stats."""
    kw = dict(standardize_obs=False, standardize_returns=False, exp_buffer_size=NA * T)
    whole, _ = run_learner(make_learner(tmp_path / "whole", "fused", False, True, **kw))
    first = make_learner(tmp_path / "ck", "fused", False, True, iters=2, save_every_ts=NA * T, **kw)
    s1, _ = run_learner(first)
    rng = torch.get_rng_state(), np.random.get_state(), first.experience_buffer.rng.get_state()
    assert s1["book"] == 2 * NA * T and whole["book"] == 3 * NA * T and not torch.equal(s1["val"], whole["val"])
    second = make_learner(tmp_path / "ck", "fused", False, True, start=2 * T, checkpoint_load_folder="latest", random_seed=9, **kw)
    try:
        assert second.agent.cumulative_timesteps == 2 * NA * T
        assert torch.equal(second.ppo_learner.value_net.arena.flat, s1["val"]) and torch.equal(second.ppo_learner.policy.arena.flat, s1["pol"])
        torch.set_rng_state(rng[0])
        np.random.set_state(rng[1])
        second.experience_buffer.rng.set_state(rng[2])
    except BaseException:
        second.agent.cleanup()
        raise
    resumed, _ = run_learner(second)
    same_state(resumed, whole, ("pol", "val", "m", "vm", "book"))   # (the book's epoch is written before the loop counts the iteration)
    # standardisation on: the statistics in the book
    sa, _ = run_learner(make_learner(tmp_path / "st", "fused", False, True, iters=1, save_every_ts=NA * T))
    b = make_learner(tmp_path / "st", "fused", False, True, checkpoint_load_folder="latest", random_seed=9)
    try:
        assert json_of(b.agent.critic_obs_stats) == sa["critic_stats"] and json_of(b.agent.obs_stats) == sa["obs_stats"]
        assert b.agent.critic_obs_stats.count == sa["critic_stats"]["count"] > NA
    finally:
        b.agent.cleanup()
