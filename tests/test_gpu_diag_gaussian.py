"""The diagonal-Gaussian head with a learnable log_std on the GPU (include/rlppo.h, "[diag]"): rollout step, loss and gradient,
optimiser tail, PPOLearner.learn and the Learner loop, against the float64 yardstick of tests/diag_gaussian_yardstick.py under the
tolerance rule of tests/fp64_gate.py: err(HIP, float64) <= max(1e-5, 1.5 x err(float32 yardstick, float64)).

Inputs are built on the CPU and checked there, from float64 alone, BEFORE anything runs on the GPU: no ratio near a clip edge, and
-- where a network has hidden layers -- no hidden pre-activation within its float32 rounding bound of 0 (the seeds below were
picked so; a seed that trips the assertion is replaced, the tolerance never widened)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets  # noqa: E402
import diag_gaussian_env as E  # noqa: E402
import diag_gaussian_yardstick as Y  # noqa: E402
import ppo_yardstick as PY  # noqa: E402
from hip_pass import L, Net, P, check, dev, run_pass, stream  # noqa: E402,F401

U32 = 2.0 ** -24
CLIP, ENT = 0.2, 0.005


# ------------------------------------------------------------------------------------------------ inputs (CPU)
def make_case(seed, n, d, k, hidden=(), noise=True):
    """Policy [d, hidden.., k] + log_std + critic [d, hidden.., 1] and an n-row buffer whose actions the float64 yardstick drew from
    the policy itself.  Old log-probabilities: a third of the rows inside the clip range (ratio exp(0.05 z)), a third above it
    (ratio ~ e^0.5), a third below (~ e^-0.5); advantages and targets N(0, 1): both signs."""
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    pol, val = nets.init_mlp(d, hidden, k), nets.init_mlp(d, hidden, 1)
    log_std = rs.uniform(-1.0, 0.5, k).astype(np.float32)
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    eps = rs.randn(n, k).astype(np.float32)
    _, act, _ = Y.sample64(pol, log_std, obs, eps)
    act = act.astype(np.float32)
    logp = Y.logp_terms(torch.as_tensor(act, dtype=torch.float64), torch.as_tensor(Y.sample64(pol, log_std, obs, eps)[0]),
                        torch.as_tensor(log_std, dtype=torch.float64)).sum(-1).numpy()
    cls = np.arange(n) % 3
    off = 0.05 * rs.randn(n) + np.where(cls == 1, -0.5, 0.0) + np.where(cls == 2, 0.5, 0.0)
    old = (logp + (off if noise else 0.0)).astype(np.float32)
    adv, tgt = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    return dict(pol=pol, val=val, log_std=log_std, obs=obs, eps=eps, act=act, old=old, adv=adv, tgt=tgt, rs=rs, k=k)


def yard(c, idx, mb_ratio, **opt):
    """(float64, float32) yardstick results on rows idx, after the CPU assertions on the float64 one."""
    args = ("diag", c["pol"], c["val"], c["obs"][idx], c["act"][idx], c["old"][idx], c["adv"][idx], c["tgt"][idx], CLIP, ENT, mb_ratio)
    opt = dict(opt, log_std=c["log_std"])
    r64 = PY.minibatch(torch.float64, *args, **opt)
    Y.assert_clear_of_clip_edges(r64["ratio"], CLIP)
    if len(c["pol"]) > 1:
        Y.assert_relu_clear(c["pol"], c["obs"][idx], "policy")
        Y.assert_relu_clear(c["val"], c["obs"][idx], "critic")
    return r64, PY.minibatch(torch.float32, *args, **opt)


def hip(L, c, idx, mb_ratio, precision="fp32", **kw):
    return run_pass(L, c["pol"], c["val"], c["obs"], c["act"], c["old"], c["tgt"], c["adv"], idx, head="diag", entry="diag", log_std=c["log_std"],
                    clip=CLIP, ent=ENT, mb_ratio=mb_ratio, precision=precision, **kw)


def got_tensors(r):
    return PY.tensors(r)


# ------------------------------------------------------------------------------------------------ 1. rollout step
# seeds per (n, k): picked on the CPU so that no hidden pre-activation of [13, 32, 32, k] lies within float32 rounding of 0
ROLLOUT_SEEDS = {(255, 3): 1889, (255, 32): 1918, (257, 32): 1932}   # (every other case: 100 + 7 n + k)


def rollout_case(n, k):
    c = make_case(ROLLOUT_SEEDS.get((n, k), 100 + 7 * n + k), n, 13, k, hidden=(32, 32))
    c["log_std"][0], c["eps"][0, 0] = 0.5, 3.0   # a sample far outside [-1, 1] in every case (row 0: |sigma eps| = 4.9)
    return c


def act_diag(L, net, c, n, opts=None, log_std=None):
    k = c["k"]
    act = torch.full((n, k), float("nan"), device="cuda")
    logp = torch.full((n,), float("nan"), device="cuda")
    w, rows = net.ws(n), net.pad(c["obs"][:n])
    ls = dev(c["log_std"] if log_std is None else log_std)
    check(L, L.rlppo_diag_gaussian_act(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, P(dev(c["eps"][:n])), P(ls), P(act), P(logp),
                                       P(w), w.numel(), opts))
    from rlgym_ppo_amd import _native as N
    mu = torch.empty(n, net.ld_out, device="cuda")   # the chain's own output, in the call's precision (no completion words of its own)
    fwd = None if opts is None else N.ActOpts(opts.precision, 0, None)
    check(L, L.rlppo_mlp_forward(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, 0, P(mu), net.ld_out, P(w), w.numel(), fwd))
    torch.cuda.synchronize()
    return act.cpu().numpy(), logp.cpu().numpy(), mu[:, :k].cpu().numpy()


def check_actions(act, mu_hip, c, n):
    """a = mu + exp(log_std) eps formed in float64 from the forward's OWN output, within 4 u (|mu| + |sigma eps|) per entry."""
    mu, se = mu_hip.astype(np.float64), np.exp(c["log_std"].astype(np.float64))[None, :] * c["eps"][:n].astype(np.float64)
    assert (np.abs(act.astype(np.float64) - (mu + se)) <= 4 * U32 * (np.abs(mu) + np.abs(se))).all()
    assert abs(act[0, 0]) > 1.5   # not clamped (row 0: |sigma eps| >= 3 e^-0.25)
    return mu + se


def check_logp(logp, act, mean64, c, label, mean32=None):
    """log p AT THE RETURNED ACTIONS under the tolerance rule: float64 head math on the float64 mean against the kernel's; the
    float32 yardstick is the same head math in float32 on the float32 torch forward."""
    a = torch.as_tensor(act)
    want = Y.logp_terms(a.double(), torch.as_tensor(mean64, dtype=torch.float64), torch.as_tensor(c["log_std"]).double()).sum(-1).numpy()
    if mean32 is None:
        mean32 = PY.mlp(c["pol"], torch.as_tensor(c["obs"][:len(act)]))
    f32 = Y.logp_terms(a, mean32, torch.as_tensor(c["log_std"])).sum(-1).numpy()
    e_hip, e_32 = PY.rel(logp, want), PY.rel(f32, want)
    print(f"[diag fp64 gate] {label}: logp err(HIP, fp64)={e_hip:.2e}  err(float32 yardstick, fp64)={e_32:.2e}")
    assert e_hip <= max(1e-5, 1.5 * e_32), (label, e_hip, e_32)


@pytest.mark.parametrize("k", [1, 3, 32, 33])
@pytest.mark.parametrize("n", [1, 16, 255, 257])
def test_rollout_step(L, n, k):
    from rlgym_ppo_amd import _native as N
    c = rollout_case(n, k)
    Y.assert_relu_clear(c["pol"], c["obs"], "policy")
    mean64 = Y.sample64(c["pol"], c["log_std"], c["obs"], c["eps"])[0]
    net = Net(L, c["pol"])
    act, logp, mu = act_diag(L, net, c, n)
    assert PY.rel(mu, mean64) <= 1e-5
    check_actions(act, mu, c, n)
    check_logp(logp, act, mean64, c, f"rollout n={n} k={k}")
    # a changed log_std is seen by the next call
    ls2 = c["log_std"] - 0.75
    act2, logp2, _ = act_diag(L, net, c, n, log_std=ls2)
    c2 = dict(c, log_std=ls2.astype(np.float32))
    check_actions(act2, mu, c2, n)
    check_logp(logp2, act2, mean64, c2, f"rollout n={n} k={k}, log_std - 0.75")
    # completion words arrive, from the sampling kernel
    nw = int(L.rlppo_act_done_words(n))
    done = torch.zeros(nw, dtype=torch.int32).pin_memory()
    act3, logp3, _ = act_diag(L, net, c, n, opts=N.ActOpts(N.PRECISION_DEFAULT, 77, done.data_ptr()))
    assert (done.numpy() == 77).all() and np.array_equal(act3, act) and np.array_equal(logp3, logp)
    # bf16 inference precision: the fp32 head math applied to the bf16 chain's output
    act16, logp16, mu16 = act_diag(L, net, c, n, opts=N.ActOpts(N.PRECISION_BF16, 0, None))
    assert 1e-7 < np.abs(mu16 - mean64).max() < 0.05   # another arithmetic in the layers ...
    check_actions(act16, mu16, c, n)          # ... the same head
    check_logp(logp16, act16, mu16, c, f"rollout n={n} k={k}, bf16 chain", mean32=torch.as_tensor(mu16))


def test_policy_class_rollout_paths_follow_log_std():
    """DiagGaussianPolicy: log_std is the tail of the arena (params() order, state dict, no generator use), the eager path and the
    graph-replayed small call give the same numbers and both follow a log_std overwritten in the arena; deterministic = the mean,
    row by row."""
    from rlgym_ppo_amd.ppo import DiagGaussianPolicy
    k, d = 3, 13
    torch.manual_seed(21)
    pol = DiagGaussianPolicy(d, k, (32, 32), "cuda:0", log_std_init=-0.25)
    after = torch.get_rng_state()
    torch.manual_seed(21)
    params = nets.init_mlp(d, (32, 32), k)
    assert torch.equal(after, torch.get_rng_state())   # the log_std fill consumed nothing from the CPU generator
    a = pol.arena
    assert a.n_tail == k and a.n_flat == a.n_net + k and a.grad.numel() == a.n_flat
    assert pol.log_std.data_ptr() == a.flat.data_ptr() + 4 * a.n_net and pol.log_std.grad.data_ptr() == a.grad.data_ptr() + 4 * a.n_net
    assert list(a.params())[-1] is pol.log_std and a.is_bound()
    assert sorted(pol.state_dict().keys()) == sorted([f"model.{i}.{w}" for i in (0, 2, 4) for w in ("weight", "bias")] + ["log_std"])
    for (w, b), lin in zip(params, a.linears):
        assert torch.equal(w, lin.weight.cpu()) and torch.equal(b, lin.bias.cpu())
    assert torch.equal(pol.log_std.cpu(), torch.full((k,), -0.25))
    rs = np.random.RandomState(2)
    obs = np.clip(rs.randn(40, d), -5, 5).astype(np.float32)
    eps = torch.as_tensor(rs.randn(40, k).astype(np.float32))

    def both(ls):
        pol.act_graphs = True
        ag, lg = pol.get_action(obs, noise=eps)           # one graph replay
        n_graphs = len(pol._graphs)
        pol.act_graphs = False
        ae, le = pol.get_action(obs, noise=eps)           # the eager path
        assert torch.equal(ag, ae) and torch.equal(lg, le) and n_graphs == 1
        mean64, act64, logp64 = Y.sample64(params, ls, obs, eps.numpy())
        assert PY.rel(ag, act64) <= 1e-5 and PY.rel(lg, logp64) <= 1e-5
        return ag

    a1 = both(np.full(k, -0.25))
    graph = next(iter(pol._graphs.values()))
    with torch.no_grad():
        pol.log_std.copy_(torch.tensor([0.5, -1.0, 0.0]))   # written in place, into the arena
    a2 = both(np.array([0.5, -1.0, 0.0]))
    assert next(iter(pol._graphs.values())) is graph and not torch.equal(a1, a2)   # the SAME captured call saw the new parameter
    assert a2.abs().max() > 1.0                                                    # nothing is clamped
    det, zero = pol.get_action(obs, deterministic=True)
    mean64 = Y.sample64(params, np.zeros(k), obs, np.zeros((40, k)))[0]
    assert zero == 0 and det.shape == (40, k) and PY.rel(det, mean64) <= 1e-5 and not torch.equal(det[0], det[1])
    mean, std = pol.get_output(obs)
    assert torch.equal(mean.cpu(), det) and torch.allclose(std.cpu(), torch.tensor([0.5, -1.0, 0.0]).exp())
    with pytest.raises(ValueError, match="Gaussian"):
        pol.get_action(obs, action_mask=np.ones((40, k), bool))
    # the stock-torch accessor agrees with the kernels
    lp, ent = pol.get_backprop_data(obs, a2)
    assert PY.rel(lp.detach().cpu(), Y.sample64(params, [0.5, -1.0, 0.0], obs, eps.numpy())[2]) <= 1e-5
    assert abs(ent.item() - (3 * Y.ENT_C - 0.5)) < 1e-5
    # a state dict round trip keeps the parameter where the kernels read it
    other = DiagGaussianPolicy(d, k, (32, 32), "cuda:0")
    other.load_state_dict(pol.state_dict())
    assert other.arena.is_bound() and torch.equal(other.arena.flat, a.flat)
    other.act_graphs = False
    assert torch.equal(other.get_action(obs, noise=eps)[0], a2)


# ------------------------------------------------------------------------------------------------ 2. loss and gradient
@pytest.mark.parametrize("k", [1, 3, 32, 33])
@pytest.mark.parametrize("mb", [1, 255, 256, 257, 1000])
def test_minibatch_against_float64(L, mb, k):
    """One-layer policy and critic (no ReLU decision anywhere): every gradient -- weights, biases, log_std -- and the five statistics
    under the tolerance rule; two runs bit-identical over the whole gradient arena, tail included.  mb = the block boundaries of the
    thread-per-row grid (1, 1, 1, 2 and 4 partial sums per dimension)."""
    c = make_case(1000 * k + mb, mb + 9, 13, k)
    idx = c["rs"].permutation(mb + 9)[:mb]
    r64, r32 = yard(c, idx, 0.5)
    if mb >= 255:
        assert (r64["ratio"] < 0.8).sum() > 20 and (r64["ratio"] > 1.2).sum() > 20 and ((r64["ratio"] > 0.8) & (r64["ratio"] < 1.2)).sum() > 20
        assert (c["adv"][idx] > 0).sum() > 20 and (c["adv"][idx] < 0).sum() > 20
    got = hip(L, c, idx, 0.5)
    PY.gate(got, r64, r32, f"[diag fp64 gate] one-layer mb={mb} k={k}")
    assert got["stats"][5:].tolist() == [0.0, 0.0, 0.0]
    again = hip(L, c, idx, 0.5)
    assert torch.equal(got["gp"], again["gp"]) and torch.equal(got["gv"], again["gv"])
    assert np.isfinite(got["gp"].cpu().numpy()).all() and np.abs(got["grad_log_std"]).max() > 0


def test_minibatch_ring_repeats_empty_and_accumulation(L):
    c = make_case(5, 700, 13, 3)
    rs = c["rs"]
    idx = rs.randint(0, 700, 600)   # drawn with repeats
    idx[:3] = [699, 0, 699]
    r64, r32 = yard(c, idx, 0.5)
    # a ring-mapped buffer with ring_base != 0 gives the plain buffer's bits; so does n_rows == 0 (rows gathered into the workspace)
    plain = hip(L, c, idx, 0.5)
    ring = hip(L, c, idx, 0.5, ring=123)
    PY.gate(ring, r64, r32, "[diag fp64 gate] ring_base=123, repeated rows")
    assert torch.equal(plain["gp"], ring["gp"]) and torch.equal(plain["gv"], ring["gv"])
    unknown = hip(L, c, idx, 0.5, n_rows=0)
    assert torch.equal(plain["gp"], unknown["gp"]) and torch.equal(plain["gv"], unknown["gv"])
    # two passes into one arena give the sum: one add per element and launch
    idx_b = rs.permutation(700)[:300]
    yard(c, idx_b, 0.25)
    b = hip(L, c, idx_b, 0.25)
    arena = (plain["gp"].clone(), plain["gv"].clone())
    ab = hip(L, c, idx_b, 0.25, grads=arena)
    n_net = plain["gp"].numel() - 3
    assert torch.equal(ab["gp"][n_net:], plain["gp"][n_net:] + b["gp"][n_net:])
    for x, p_, q_ in ((ab["gp"], plain["gp"], b["gp"]), (ab["gv"], plain["gv"], b["gv"])):
        assert PY.rel(x.cpu(), (p_.double() + q_.double()).cpu()) <= 1e-6
    # an empty pass launches nothing and touches nothing
    from rlgym_ppo_amd import _native as N
    a = N.MinibatchArgs()
    pc, vc = N.dims_array([13, 3]), N.dims_array([13, 1])
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.mb = 3, 1, 1, 3, 0
    a.pol_dims, a.val_dims = ctypes.cast(pc, ctypes.POINTER(ctypes.c_int32)), ctypes.cast(vc, ctypes.POINTER(ctypes.c_int32))
    check(L, L.rlppo_ppo_minibatch_diag(stream(), ctypes.byref(a), None, None, None, 0))


def test_minibatch_options(L):
    """adv_norm, value_clip, armed kl_slots and a set stop word (which adds nothing to `stats`)."""
    c = make_case(6, 900, 13, 3)
    idx = c["rs"].permutation(900)[:700]
    an = Y.adv_stats(c["adv"][idx])
    vclip = 0.3
    # (CPU, float64: no |v - v_old| at the clamp's boundary for float32 to decide otherwise)
    v = c["obs"][idx].astype(np.float64) @ c["val"][0][0].numpy().astype(np.float64).T + c["val"][0][1].numpy().astype(np.float64)
    dv = np.abs(v[:, 0] - (c["tgt"][idx].astype(np.float64) - c["adv"][idx].astype(np.float64)))
    assert np.abs(dv - vclip).min() > 1e-5 and (dv < vclip).sum() > 20 and (dv > vclip).sum() > 20
    r64, r32 = yard(c, idx, 0.5, adv_norm=an, value_clip=vclip)
    got = hip(L, c, idx, 0.5, adv_norm=an, value_clip=vclip, kl_slots=True)
    PY.gate(got, r64, r32, "[diag fp64 gate] adv_norm + value_clip + kl_slots")
    grid = (700 + 255) // 256
    assert got["kl"][0] == grid and got["kl"][1] == 0.5
    assert abs(got["kl"][2:2 + grid].sum() - got["stats"][1]) <= 1e-12 * abs(got["stats"][1])
    stopped = hip(L, c, idx, 0.5, adv_norm=an, value_clip=vclip, stop=3)
    assert (stopped["stats"] == 0).all()
    assert torch.equal(stopped["gp"], got["gp"]) and torch.equal(stopped["gv"], got["gv"])
    running = hip(L, c, idx, 0.5, adv_norm=an, value_clip=vclip, stop=0)
    assert np.array_equal(running["stats"], got["stats"])


HIDDEN_SEED, HIDDEN_SEED_K1, HIDDEN_ROWS = 57, 82, 96   # (picked on the CPU: assert_relu_clear holds for both networks on these rows; at 300 rows of
#                                       2 x 256 hidden units no seed in 300 clears the worst-case rounding bound)


HIDDEN_SEEDS = {3: HIDDEN_SEED, 1: HIDDEN_SEED_K1}


def hidden_case(k=3):
    c = make_case(HIDDEN_SEEDS[k], HIDDEN_ROWS + 30, 13, k, hidden=(128, 128))
    return c, c["rs"].permutation(HIDDEN_ROWS + 30)[:HIDDEN_ROWS]


@pytest.mark.parametrize("k", [3, 1])
def test_three_layer_pass_in_the_paired_launch_form(L, k):
    """Policy [13, 128, 128, k] + critic [13, 128, 128, 1], 96 rows: the paired-launch form,
    which only starts at 262,144 rows, forced with rlppo_dbg_set(29, 2) as the existing tests force it; under the tolerance rule and
    bit-identical to the two-chain form.  k = 1: a one-output head behind hidden layers on the POLICY chain (the critic's shape, its
    matrix-vector kernels, but no folded head)."""
    c, idx = hidden_case(k)
    r64, r32 = yard(c, idx, 1.0)
    two_chains = hip(L, c, idx, 1.0)
    check(L, L.rlppo_dbg_set(29, 2))
    try:
        n_paired = L.rlppo_dbg_counter(3)
        paired = hip(L, c, idx, 1.0)
        assert L.rlppo_dbg_counter(3) == n_paired + 1
    finally:
        check(L, L.rlppo_dbg_set(29, 1))
    PY.gate(paired, r64, r32, "[diag fp64 gate] three layers, paired launches")
    PY.gate(two_chains, r64, r32, "[diag fp64 gate] three layers, two chains")
    # (the policy's arena, tail included, bit for bit; the critic's one-output head may be summed in another order by the form)
    assert torch.equal(paired["gp"], two_chains["gp"]) and PY.rel(paired["gv"].cpu(), two_chains["gv"].cpu()) <= 2e-6
    # one stream instead of two: the same bits
    check(L, L.rlppo_dbg_set(4, 0))
    try:
        one_stream = hip(L, c, idx, 1.0)
    finally:
        check(L, L.rlppo_dbg_set(4, 1))
    assert torch.equal(one_stream["gp"], two_chains["gp"]) and PY.rel(one_stream["gv"].cpu(), two_chains["gv"].cpu()) <= 2e-6


@pytest.mark.parametrize("precision", ["bf16", "x3"])
def test_other_update_precisions(L, precision):
    """The pass runs and is bit-reproducible in the bf16 and the split-bf16 update precision; the head math is fp32 on whatever the
    forward produced.  bf16 is another arithmetic in the layers: it is held to the margins
    tests/test_gpu_cfg5.py::test_bf16_update_precision_against_its_restatement applies to the reference Gaussian head in that
    precision, against the same CPU restatement (this file's yardstick in float32 under oracle.nets.bf16_operands(); its
    summation-order floor: the restatement against itself under oracle.nets.sum64()), on EVERY gradient tensor, log_std's included:
        `assert e_ref <= max(1e-3, 3.0 * floor), (e_ref, floor)`
        `assert 1e-4 < e_true < 0.5 and abs(e_true - e_ref_true) < 0.1 * e_ref_true + 3.0 * floor + 2e-3`
    and its statistics lines.  (The lower bound 1e-4 shows that the bf16 arithmetic ran.)  x3 keeps the fp32 meaning and is held
    to the float64 gate of the fp32 pass, as tests/test_gpu_kernels.py::test_minibatch_x3_precision_cfg2_shape holds it."""
    c, idx = hidden_case()
    r64, r32 = yard(c, idx, 1.0)
    got = hip(L, c, idx, 1.0, precision=precision)
    again = hip(L, c, idx, 1.0, precision=precision)
    assert torch.equal(got["gp"], again["gp"]) and torch.equal(got["gv"], again["gv"])
    assert np.isfinite(got["gp"].cpu().numpy()).all() and np.isfinite(got["stats"]).all()
    if precision == "x3":
        PY.gate(got, r64, r32, "[diag fp64 gate] three layers, x3")
        return
    args = ("diag", c["pol"], c["val"], c["obs"][idx], c["act"][idx], c["old"][idx], c["adv"][idx], c["tgt"][idx], CLIP, ENT, 1.0)
    with nets.bf16_operands():
        ref = PY.minibatch(torch.float32, *args, log_std=c["log_std"])
    with nets.bf16_operands(), nets.sum64():
        ref2 = PY.minibatch(torch.float32, *args, log_std=c["log_std"])
    floor = PY.err(PY.tensors(ref2), PY.tensors(ref))
    e_ref, e_true, e_ref_true = PY.err(got_tensors(got), PY.tensors(ref)), PY.err(got_tensors(got), PY.tensors(r64)), PY.err(PY.tensors(ref), PY.tensors(r64))
    ls_ref, ls_true = PY.rel(got["grad_log_std"], ref["grad_log_std"]), PY.rel(got["grad_log_std"], r64["grad_log_std"])
    print(f"[diag bf16 update] err(HIP bf16, CPU bf16 restatement)={e_ref:.2e}  summation-order floor of the restatement itself={floor:.2e}  "
          f"distance from float64 truth of the fp32 function: HIP {e_true:.2e}, restatement {e_ref_true:.2e}; log_std gradient alone: "
          f"against the restatement {ls_ref:.2e}, against float64 {ls_true:.2e}")
    assert e_ref <= max(1e-3, 3.0 * floor), (e_ref, floor)
    assert 1e-4 < e_true < 0.5 and abs(e_true - e_ref_true) < 0.1 * e_ref_true + 3.0 * floor + 2e-3
    for name, k_ in (("entropy", 0), ("kl", 1), ("value_loss", 2), ("policy_loss", 4)):
        tol = max(2e-4, 3.0 * abs(ref2[name] - ref[name]) / max(abs(ref[name]), 1e-2))
        assert abs(got["stats"][k_] - ref[name]) <= tol * max(abs(ref[name]), 1e-2), (name, got["stats"][k_], ref[name], ref2[name])
    assert abs(got["stats"][0] - r64["entropy"]) <= 1e-5 * abs(r64["entropy"])   # the entropy does not depend on the layers at all


# ------------------------------------------------------------------------------------------------ 3. optimiser tail
@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch_grid_barrier", "three_operations"])
def test_optimiser_tail_equals_clip_adam_plus_pack(L, one_launch):
    """rlppo_clip_adam_pack2_tail against rlppo_clip_adam over n_net + k elements followed by rlppo_net_pack: parameters, both
    moments and the WHOLE packed image bit for bit (a tail element written into `packed` would land in the last bias slot's
    padding), gradients zero, gnorm2 includes the tail; a max-norm small enough that the clip bites, then one that does not; a set
    skip_word leaves everything, the tail included, untouched."""
    from rlgym_ppo_amd import _native as N
    torch.manual_seed(4)
    shapes = [([13, 32, 1], 0), ([13, 32, 32, 3], 3), ([13, 5], 5)]   # (dims, tail): the critic, a policy + log_std, a one-layer net
    for pair in ((0, 1), (2, 1)):
        state = []
        for dims, tail in (shapes[pair[0]], shapes[pair[1]]):
            dc, nl = N.dims_array(dims), len(dims) - 1
            n_net, npk = int(L.rlppo_flat_floats(dc, nl)), int(L.rlppo_packed_floats(dc, nl))
            flat = torch.randn(n_net + tail, device="cuda") * 0.1
            st = dict(dc=dc, nl=nl, n=n_net + tail, n_net=n_net, tail=tail)
            for tag in ("a", "b"):
                st[tag] = dict(p=flat.clone(), m=torch.zeros(n_net + tail, device="cuda"), v=torch.zeros(n_net + tail, device="cuda"),
                               packed=torch.zeros(npk, device="cuda"), gn=torch.zeros(1, dtype=torch.float64, device="cuda"))
                check(L, L.rlppo_net_pack(stream(), dc, nl, P(st[tag]["p"]), P(st[tag]["packed"])))
            state.append(st)
        sync = torch.zeros(N.OPT_SYNC_BYTES // 4, dtype=torch.int32, device="cuda") if one_launch else None
        skip = torch.zeros(1, dtype=torch.int32, device="cuda")

        def descs_for(step, max_norm, grads, skip_word=None):
            out = []
            for st, g in zip(state, grads):
                b = st["b"]
                d = N.OptNet()
                d.dims, d.n_layers = ctypes.cast(st["dc"], ctypes.POINTER(ctypes.c_int32)), st["nl"]
                d.params, d.grads, d.exp_avg, d.exp_avg_sq = b["p"].data_ptr(), g.data_ptr(), b["m"].data_ptr(), b["v"].data_ptr()
                d.packed, d.gnorm2 = b["packed"].data_ptr(), b["gn"].data_ptr()
                d.max_norm, d.lr, d.beta1, d.beta2, d.eps, d.step = max_norm, 3e-4, 0.9, 0.999, 1e-8, step
                if skip_word is not None:
                    d.skip_word = skip_word.data_ptr()
                out.append(d)
            return out

        for step, (scale, max_norm) in enumerate([(1.0, 0.01), (1e-4, 0.5), (3.0, 0.5)], start=1):
            grads = []
            for st in state:
                g = torch.randn(st["n"], device="cuda") * scale
                if st["tail"]:
                    g[st["n_net"]:] *= 50.0   # the tail carries most of the norm: a norm without it would clip differently
                ga, gb = g.clone(), g.clone()
                a = st["a"]
                check(L, L.rlppo_clip_adam(stream(), P(a["p"]), P(ga), P(a["m"]), P(a["v"]), st["n"], max_norm, 3e-4, 0.9, 0.999, 1e-8, step, P(a["gn"])))
                check(L, L.rlppo_net_pack(stream(), st["dc"], st["nl"], P(a["p"]), P(a["packed"])))
                st["g64"] = float((g.double() ** 2).sum().item())
                grads.append(gb)
            d = descs_for(step, max_norm, grads)
            check(L, L.rlppo_clip_adam_pack2_tail(stream(), ctypes.byref(d[0]), ctypes.byref(d[1]), P(sync), state[0]["tail"], state[1]["tail"]))
            torch.cuda.synchronize()
            for st, gb in zip(state, grads):
                a, b = st["a"], st["b"]
                for key in ("p", "m", "v", "packed"):
                    assert torch.equal(a[key], b[key]), (pair, step, key)
                assert (gb == 0).all()
                assert abs(b["gn"].item() - st["g64"]) <= 1e-12 * st["g64"] and abs(a["gn"].item() - b["gn"].item()) <= 1e-12 * st["g64"]
                if step == 1:
                    assert max_norm / np.sqrt(st["g64"]) < 0.1   # the clip bites
        # a set skip word: nothing of either network moves, tail included, and the gradients stay
        skip.fill_(1)
        keep = [{k_: v_.clone() for k_, v_ in st["b"].items()} for st in state]
        grads = [torch.randn(st["n"], device="cuda") for st in state]
        gkeep = [g.clone() for g in grads]
        d = descs_for(4, 0.5, grads, skip)
        check(L, L.rlppo_clip_adam_pack2_tail(stream(), ctypes.byref(d[0]), ctypes.byref(d[1]), P(sync), state[0]["tail"], state[1]["tail"]))
        torch.cuda.synchronize()
        for st, kept, g, gk in zip(state, keep, grads, gkeep):
            for key in ("p", "m", "v", "packed"):
                assert torch.equal(st["b"][key], kept[key]), (pair, "skip", key)
            assert torch.equal(g, gk)
        if one_launch:
            assert sync.cpu().numpy()[2] == 0   # no barrier wait gave up


# ------------------------------------------------------------------------------------------------ 4. PPOLearner.learn
LEARN_SEED = 19   # (picked on the CPU: the initial networks clear assert_relu_clear on all 1024 rows)
OBS, K, N_ROWS, B, MB, EPOCHS, LR = 13, 3, 1024, 512, 128, 2, 3e-4


def build_learner(seed=LEARN_SEED, **kw):
    """PPOLearner(policy_type 3) and a 1024-row buffer the policy itself sampled (log_std 0: samples beyond +-1 are common)."""
    from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner
    torch.manual_seed(seed)
    np.random.seed(seed)
    learner = PPOLearner(OBS, K, 3, (32, 32), (32, 32), (0.1, 1.0), B, EPOCHS, LR, LR, CLIP, ENT, MB, "cuda:0", **kw)
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(N_ROWS, OBS), -5, 5).astype(np.float32)
    act, logp = learner.policy.get_action(obs, noise=torch.as_tensor(rs.randn(N_ROWS, K).astype(np.float32)))
    exp = dict(states=obs, actions=act.numpy(), log_probs=logp.numpy() + 0.1 * rs.randn(N_ROWS).astype(np.float32),
               values=rs.randn(N_ROWS).astype(np.float32), advantages=rs.randn(N_ROWS).astype(np.float32))
    return learner, exp


def buffer_of(exp, seed=LEARN_SEED):
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    buf = ExperienceBuffer(N_ROWS, seed, "cpu")
    z = np.zeros(N_ROWS, np.float32)
    buf.submit_experience(exp["states"], exp["actions"], exp["log_probs"], z, exp["states"], z, z, exp["values"], exp["advantages"])
    return buf


def params_of(learner):
    a = learner.policy.arena
    pol = [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in a.linears]
    val = [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in learner.value_net.arena.linears]
    return pol, learner.policy.log_std.detach().cpu().clone(), val


_LEARN_YARD = {}


def learn_yardstick(pol, ls, val, exp):
    """The float64 and the float32 yardstick of the learn() every test of this section runs (same initial parameters, same buffer):
    computed once, shared, left unchanged.  -> (t_pol, t_val, f_pol, f_val, weakest)."""
    if not _LEARN_YARD:
        weakest = {}
        t_pol, t_val = PY.learn(torch.float64, "diag", "relu", pol, val, exp, B, MB, EPOCHS, CLIP, ENT, LR, LR, np.random.RandomState(LEARN_SEED), log_std=ls, weakest=weakest)
        f_pol, f_val = PY.learn(torch.float32, "diag", "relu", pol, val, exp, B, MB, EPOCHS, CLIP, ENT, LR, LR, np.random.RandomState(LEARN_SEED), log_std=ls)
        _LEARN_YARD["r"] = (t_pol, t_val, f_pol, f_val, weakest)
        _LEARN_YARD["p0"] = np.concatenate([t.numpy().ravel() for wb in pol for t in wb])
    assert np.array_equal(_LEARN_YARD["p0"], np.concatenate([t.numpy().ravel() for wb in pol for t in wb]))   # the same learn()
    return _LEARN_YARD["r"]


def learn_errs(p_, v_, yard_):
    """Parameters after learn() against the float64 yardstick's, split as tests/test_gpu_learner.py splits them:
    -> (err over the well-conditioned parameters, relative to max|truth|; worst ill-conditioned one as a fraction of its derived
    bound (steps) lr min(1, 1e-5 / w_i))."""
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


def flats(learner):
    return learner.policy.arena.flat.cpu().numpy(), learner.value_net.arena.flat.cpu().numpy()


def test_learn_against_the_float64_yardstick():
    """Two epochs of two optimiser steps (B 512, MB 128: four minibatches per step, fused into one pass): the policy's parameters
    INCLUDING log_std, and the critic's, against the float64 yardstick's; the allowance per parameter is the one
    tests/test_gpu_learner.py::test_learn_matches_reference_fixture derives -- the plain tolerance rule where Adam's step is well
    conditioned (|g_i| >= 1e-4 max|g| in every step), (steps) lr min(1, 1e-5 / w_i) where it is not -- for the HIP result and for
    the float32 yardstick alike."""
    learner, exp = build_learner()
    assert learner.policy_type == 3 and learner._act_dim == K and learner.policy.arena.n_tail == K
    assert np.abs(exp["actions"]).max() > 1.0
    pol, ls, val = params_of(learner)
    Y.assert_relu_clear(pol, exp["states"], "policy")
    Y.assert_relu_clear(val, exp["states"], "critic")
    yard_ = learn_yardstick(pol, ls, val, exp)
    t_pol, t_val, f_pol, f_val, weakest = yard_
    report = learner.learn(buffer_of(exp))
    steps = EPOCHS * (N_ROWS // B)
    assert report["Cumulative Model Updates"] == steps
    got = (learner.policy.arena.flat.cpu().numpy().astype(np.float64), learner.value_net.arena.flat.cpu().numpy().astype(np.float64))
    assert got[0].size == t_pol.size
    errs = {}
    for who, (p_, v_) in (("hip", got), ("f32", (f_pol, f_val))):
        good, frac = learn_errs(p_, v_, yard_)
        errs[who] = (good, 0.0, frac)
    n_ill = int((weakest["pol"] < 1e-4).sum() + (weakest["val"] < 1e-4).sum())
    e_ls = (float(np.abs(got[0][-K:] - t_pol[-K:]).max()), float(np.abs(f_pol[-K:] - t_pol[-K:]).max()))
    print(f"[diag fp64 gate] learn(): err(HIP, fp64)={errs['hip'][0]:.2e}  err(float32 yardstick, fp64)={errs['f32'][0]:.2e}; {n_ill} ill-conditioned "
          f"parameters: HIP at {errs['hip'][2]:.3f} of the derived bound, float32 yardstick {errs['f32'][2]:.3f}; log_std: |HIP - fp64| {e_ls[0]:.2e}, "
          f"|float32 - fp64| {e_ls[1]:.2e}, moved by {np.abs(t_pol[-K:]).max():.2e}")
    assert errs["hip"][0] <= max(1e-5, 1.5 * errs["f32"][0]), errs
    assert errs["hip"][2] <= 1.0 and n_ill <= 0.05 * (t_pol.size + t_val.size), (errs, n_ill)
    assert np.abs(t_pol[-K:]).max() > 0.5 * LR   # log_std moved (and is among the parameters held to the rule above)
    assert abs(report["Policy Entropy"] - K * Y.ENT_C) < 4 * steps * LR * K   # entropy = sum_j (c + log_std_j), log_std within steps x lr of 0
    # the optimiser state has the stock layout, log_std last
    osd = learner.policy_optimizer.state_dict()
    assert len(osd["state"]) == 7 and tuple(osd["state"][6]["exp_avg"].shape) == (K,)
    assert torch.equal(osd["state"][6]["exp_avg"], learner.policy_optimizer.exp_avg[-K:]) and float(osd["state"][6]["step"]) == steps


def test_learn_target_kl_stops_log_std_and_checkpoints_round_trip(tmp_path):
    learner, exp = build_learner(target_kl=1e-9)
    ls0, flat0 = learner.policy.log_std.detach().clone(), learner.policy.arena.flat.clone()
    report = learner.learn(buffer_of(exp))
    # batch 0 runs at ratio != 1 (the stored log-probabilities carry noise): its KL is far above 1.5e-9, so no step is applied
    assert report["KL Early Stopped"] == 1.0 and report["PPO Optimizer Steps"] == 0
    assert torch.equal(learner.policy.log_std.detach(), ls0) and torch.equal(learner.policy.arena.flat, flat0)
    assert (learner.policy.arena.grad == 0).all() and learner.policy_optimizer.step_count == 0
    # without the gate log_std moves; save -> load -> continue equals the uninterrupted run bit for bit, log_std and its moments included
    a, exp = build_learner()
    a.n_epochs = 1
    a.learn(buffer_of(exp))
    assert not torch.equal(a.policy.log_std.detach(), ls0)
    a.save_to(str(tmp_path))
    assert "log_std" in torch.load(str(tmp_path / "PPO_POLICY.pt"))
    b, _ = build_learner(seed=LEARN_SEED + 1)   # other initial weights: everything must come from the files
    b.n_epochs = 1
    b.load_from(str(tmp_path))
    assert torch.equal(b.policy.arena.flat, a.policy.arena.flat) and b.policy.arena.is_bound()
    assert torch.equal(b.policy_optimizer.exp_avg, a.policy_optimizer.exp_avg) and torch.equal(b.policy_optimizer.exp_avg_sq, a.policy_optimizer.exp_avg_sq)
    assert b.policy_optimizer.step_count == a.policy_optimizer.step_count == 2
    buf_a, buf_b = buffer_of(exp), buffer_of(exp)
    a.learn(buf_a)
    b.learn(buf_b)
    for x, y in ((a.policy.arena.flat, b.policy.arena.flat), (a.value_net.arena.flat, b.value_net.arena.flat),
                 (a.policy_optimizer.exp_avg, b.policy_optimizer.exp_avg), (a.policy_optimizer.exp_avg_sq, b.policy_optimizer.exp_avg_sq)):
        assert torch.equal(x, y)
    # the reference's own optimiser class reads the file
    ref_opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros_like(p)) for p in a.policy.arena.params()], lr=1.0)
    ref_opt.load_state_dict(torch.load(str(tmp_path / "PPO_POLICY_OPTIMIZER.pt")))


def test_two_virtual_ranks_share_the_log_std_gradient():
    """Two data-parallel ranks (dp.run_virtual_ranks): the log_std gradient is inside the ONE exchanged tensor, so the replicas end
    bit-identical to each other, and within the tolerance of one rank (the same sums in another order)."""
    from rlgym_ppo_amd import dp
    one, exp = build_learner()
    pol, ls, val = params_of(one)
    one.learn(buffer_of(exp))
    reps = [build_learner()[0] for _ in range(2)]
    probes = []
    reps[0].grad_probe = lambda g: probes.append(g.clone())
    pa = reps[0].policy.arena
    assert reps[0]._grad_all.numel() == pa.n_flat + reps[0].value_net.arena.n_flat and pa.grad.data_ptr() == reps[0]._grad_all.data_ptr()
    dp.run_virtual_ranks(reps, [buffer_of(exp) for _ in range(2)])
    assert torch.equal(reps[0].policy.arena.flat, reps[1].policy.arena.flat) and torch.equal(reps[0].value_net.arena.flat, reps[1].value_net.arena.flat)
    assert torch.equal(reps[0].policy_optimizer.exp_avg, reps[1].policy_optimizer.exp_avg)
    assert float(probes[0][pa.n_net:pa.n_flat].abs().max()) > 0   # the summed log_std gradient, in the exchanged arena
    # "within tolerance of one rank": both results are held to the float64 yardstick of the same learn() by the rule
    # test_learn_against_the_float64_yardstick applies -- the tolerance rule on the well-conditioned parameters, the derived bound
    # on the ill-conditioned ones -- so they lie within twice that of each other
    yard_ = learn_yardstick(pol, ls, val, exp)
    e_32, _ = learn_errs(yard_[2], yard_[3], yard_)
    for who, l_ in (("one rank", one), ("two ranks", reps[0])):
        good, frac = learn_errs(*flats(l_), yard_)
        print(f"[diag fp64 gate] learn(), {who}: err(HIP, fp64)={good:.2e}  err(float32 yardstick, fp64)={e_32:.2e}; ill-conditioned at {frac:.3f} of the bound")
        assert good <= max(1e-5, 1.5 * e_32) and frac <= 1.0, (who, good, e_32, frac)


# ------------------------------------------------------------------------------------------------ 5. Learner end to end
def run_loop(tmp_path, mode, **kw):
    from rlgym_ppo_amd import Learner
    vector = mode == "vector"
    cfg = dict(n_proc=1, min_inference_size=2, timestep_limit=700, exp_buffer_size=1024, ts_per_iteration=384, ppo_epochs=1, ppo_batch_size=384,
               ppo_minibatch_size=192, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32), checkpoints_save_folder=str(tmp_path / "ckpt"),
               add_unix_timestamp=False, save_every_ts=10_000_000, checkpoint_load_folder=None, random_seed=3, vector_env=vector,
               continuous_head="diag")
    cfg.update(kw)
    learner = Learner(E.make_echo_vector_env if vector else E.make_echo_env, **cfg)
    if mode == "process_python":
        learner.agent.native_collect = False
    reports = []
    plain = learner.ppo_learner.learn
    learner.ppo_learner.learn = lambda exp: reports.append(plain(exp)) or reports[-1]
    try:
        learner._learn()
    except BaseException:
        learner.agent.cleanup()
        raise
    return learner, reports


@pytest.mark.parametrize("mode", ["vector", "process_native", "process_python"])
def test_learner_loop_clips_for_the_environment_only(tmp_path, mode):
    from rlgym_ppo_amd.ppo import DiagGaussianPolicy
    learner, reports = run_loop(tmp_path, mode, continuous_log_std_init=0.25)
    try:
        assert learner.epoch == 2 and len(reports) == 2 and all(np.isfinite(float(v)) for r in reports for v in r.values())
        pol = learner.ppo_learner.policy
        assert isinstance(pol, DiagGaussianPolicy) and learner.ppo_learner.policy_type == 3 and learner.continuous_action_clip == (-1.0, 1.0)
        buf = learner.experience_buffer
        acts, rews = buf.actions.cpu().numpy(), buf.rewards.cpu().numpy()
        assert acts.shape[1] == E.K and np.abs(acts).max() > 1.5      # the buffer holds the samples as drawn ...
        assert rews.max() <= 1.0 and rews.max() == 1.0 and rews.min() >= 0.0   # ... the environment saw them clipped to [-1, 1] (its reward echoes max |a|)
        ls = pol.log_std.detach().cpu().numpy()
        assert np.abs(ls - 0.25).max() > 0 and np.abs(ls - 0.25).max() < 0.01   # started at the init, moved by the optimiser
        assert abs(reports[0]["Policy Entropy"] - E.K * (Y.ENT_C + 0.25)) < 1e-4   # the first pass saw log_std = 0.25 in every dimension
    finally:
        learner.agent.cleanup()


def test_learner_save_load_continue_equals_the_uninterrupted_run(tmp_path):
    """Through Learner.save and the constructor's load: a run of one iteration that checkpoints, then a SECOND Learner that loads
    "latest" and runs the second iteration, against ONE Learner that runs both -- policy (log_std included), critic, both Adam
    moments and step counts, the book-keeping and the buffer's rows bit for bit.
    What a checkpoint does not hold is carried over by the test, so that the restored state is all that can differ: the environment
    (CounterVectorEnv: its whole state is a step counter, the second Learner's starts where the first one's stopped), the host
    generators (torch's, which draws the sampling noise; numpy's) and the buffer's shuffle generator; the buffer holds exactly one
    iteration (384 rows), so the rows of the first iteration are gone in both runs.  Observation and return standardisation are
    off: their statistics come back from JSON as float64 (the reference's behaviour), which is not the float32 state of a run
    that was never interrupted.  The second Learner is built with another seed and another continuous_log_std_init: everything
    must come from the files."""
    import functools
    from rlgym_ppo_amd import Learner
    kw = dict(vector_env=True, n_proc=1, min_inference_size=2, exp_buffer_size=384, ts_per_iteration=384, ppo_epochs=1, ppo_batch_size=384,
              ppo_minibatch_size=192, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32), add_unix_timestamp=False, save_every_ts=300,
              standardize_obs=False, standardize_returns=False, continuous_head="diag")

    def state(l_):
        p_ = l_.ppo_learner
        return dict(pol=p_.policy.arena.flat.clone(), val=p_.value_net.arena.flat.clone(), m=p_.policy_optimizer.exp_avg.clone(),
                    v=p_.policy_optimizer.exp_avg_sq.clone(), vm=p_.value_optimizer.exp_avg.clone(), vv=p_.value_optimizer.exp_avg_sq.clone(),
                    steps=(p_.policy_optimizer.step_count, p_.value_optimizer.step_count, p_.cumulative_model_updates),
                    book=l_.agent.cumulative_timesteps, acts=l_.experience_buffer.actions.clone(),
                    rews=l_.experience_buffer.rewards.clone(), logp=l_.experience_buffer.log_probs.clone())

    def run(l_):
        try:
            l_._learn()
            return state(l_), int(l_.agent.env.t), torch.get_rng_state(), np.random.get_state(), l_.experience_buffer.rng.get_state()
        finally:
            l_.agent.cleanup()

    whole, t_end, _, _, _ = run(Learner(functools.partial(E.CounterVectorEnv, 0), timestep_limit=700, checkpoint_load_folder=None, random_seed=3,
                                        continuous_log_std_init=0.25, checkpoints_save_folder=str(tmp_path / "whole"), **kw))
    first, t_mid, rng_torch, rng_numpy, rng_buffer = run(Learner(functools.partial(E.CounterVectorEnv, 0), timestep_limit=300, checkpoint_load_folder=None,
                                                                 random_seed=3, continuous_log_std_init=0.25, checkpoints_save_folder=str(tmp_path / "ck"), **kw))
    assert first["book"] == 384 and whole["book"] == 768 and (t_mid, t_end) == (24, 48) and first["steps"] == (1, 1, 1)
    assert not torch.equal(first["pol"], whole["pol"]) and float(first["v"][-E.K:].max()) > 0
    second = Learner(functools.partial(E.CounterVectorEnv, t_mid), timestep_limit=700, checkpoint_load_folder="latest", random_seed=9,
                     continuous_log_std_init=-1.0, checkpoints_save_folder=str(tmp_path / "ck"), **kw)
    try:
        restored = state(second)
        for key in ("pol", "val", "m", "v", "vm", "vv", "steps", "book"):
            same = torch.equal(restored[key], first[key]) if isinstance(first[key], torch.Tensor) else restored[key] == first[key]
            assert same, ("restored", key)
        assert torch.equal(second.ppo_learner.policy.log_std.detach(), first["pol"][-E.K:]) and second.ppo_learner.policy.arena.is_bound()
        torch.set_rng_state(rng_torch)
        np.random.set_state(rng_numpy)
        second.experience_buffer.rng.set_state(rng_buffer)
    except BaseException:
        second.agent.cleanup()
        raise
    resumed, t_res, _, _, _ = run(second)
    assert t_res == t_end
    for key, want in whole.items():
        same = torch.equal(resumed[key], want) if isinstance(want, torch.Tensor) else resumed[key] == want
        assert same, ("continued", key)
    assert float(resumed["acts"].abs().max()) > 1.5 and float(resumed["rews"].max()) == 1.0   # unclipped in the buffer, clipped for the environment


def test_learner_reference_head_is_the_default(tmp_path):
    """continuous_head="reference" next to it: ContinuousPolicy, no parameter tail, the caller's environment function unwrapped, the
    head's own clamp, the plain optimiser entry point -- and "reference" is what an omitted option means.  (That the reference head
    still computes what it computed is NOT shown here -- both runs take this tree's code: the guard for that are the existing
    tests, unchanged, against the reference's recorded fixtures: tests/test_gpu_learner.py::test_learn_matches_reference_fixture
    [g9_learn_continuous], tests/test_gpu_kernels.py::test_g9_gaussian_and_multidiscrete_act, tests/test_gpu_cfg5.py.)"""
    from rlgym_ppo_amd.ppo import ContinuousPolicy
    a, ra = run_loop(tmp_path / "a", "vector", continuous_head="reference")
    env_a = type(a.agent.env).__name__
    a.agent.cleanup()
    cfg = dict(n_proc=1, min_inference_size=2, timestep_limit=700, exp_buffer_size=1024, ts_per_iteration=384, ppo_epochs=1, ppo_batch_size=384,
               ppo_minibatch_size=192, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32), checkpoints_save_folder=str(tmp_path / "c"),
               add_unix_timestamp=False, save_every_ts=10_000_000, checkpoint_load_folder=None, random_seed=3, vector_env=True)
    from rlgym_ppo_amd import Learner
    c = Learner(E.make_echo_vector_env, **cfg)   # no continuous_* argument at all
    try:
        c._learn()
    finally:
        c.agent.cleanup()
    pa = a.ppo_learner.policy
    assert isinstance(pa, ContinuousPolicy) and a.ppo_learner.policy_type == 2 and pa.arena.n_tail == 0 and a.continuous_action_clip is None
    assert env_a == "EchoVectorEnv"
    assert float(a.experience_buffer.actions.abs().max()) <= 1.0
    assert torch.equal(pa.arena.flat, c.ppo_learner.policy.arena.flat) and torch.equal(a.ppo_learner.value_net.arena.flat, c.ppo_learner.value_net.arena.flat)
