"""Invalid-action masking of the discrete head on the device, from the rollout to the update (include/rlppo.h, ABI 8):
all-valid is off bit for bit; sampling picks the first arg-max over VALID actions of pc / q and never an invalid action; the masked
loss and its gradient against float64 truth under the HIP's own ReLU decisions (no row excluded: the inputs keep every ratio
>= 5e-4 away from the clip edges by construction); a column-constant mask is the narrower network; every form of the pass sees the
right rows of a wrapped ring; the Learner loop on a vectorised environment with action_masks()."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_gate  # noqa: E402
import ppo_yardstick as PY  # noqa: E402
import synthetic_env  # noqa: E402
from hip_pass import L, P, run_pass, stream, triple  # noqa: E402,F401
from oracle import nets, ppo  # noqa: E402

D = 107
CLIP, ENT = PY.CLIP, PY.ENT


def knob(L, key, value):
    assert L.rlppo_dbg_set(key, value) == 0


def rand_mask(rs, n, A, p=0.66):
    """Random masks: every row >= 1 valid action, every 7th row exactly one, every 5th row all valid."""
    m = rs.rand(n, A) < p
    m[np.arange(n), rs.randint(0, A, n)] = True
    one = np.arange(0, n, 7)
    m[one] = False
    m[one, rs.randint(0, A, len(one))] = True
    m[np.arange(3, n, 5)] = True
    return m


def softmax64(z, m):
    z = np.where(m, np.asarray(z, np.float64), -np.inf)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def logits64(params, obs):
    p64 = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in params]
    return ppo._fwd64(p64, np.asarray(obs, np.float64))[0][-1]


def params(net):
    return [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in net.arena.linears]


def policy(A, hidden, seed=0):
    from rlgym_ppo_amd.ppo.discrete_policy import DiscreteFF
    torch.manual_seed(seed)
    return DiscreteFF(D, A, hidden, "cuda:0")


def raw_act(L, pol, rows, q, words, want_probs=True):
    """rlppo_discrete_act with probs_out: (actions, logp, probs) on the device; which kernel ran is read off the counters."""
    from rlgym_ppo_amd import _native as N
    a = pol.arena
    n = rows.shape[0]
    a.ensure_packed()
    act = torch.empty(n, dtype=torch.int64, device="cuda")
    lp = torch.empty(n, dtype=torch.float32, device="cuda")
    pr = torch.full((n, pol.n_actions), float("nan"), device="cuda") if want_probs else None
    ws = a.forward_ws(n)
    opts = None
    if words is not None:
        opts = N.ActOpts()
        opts.action_mask, opts.mask_words = words.data_ptr(), words.shape[1]
    N.check(L.rlppo_discrete_act(stream(), a.dims_c, a.n_layers, P(a.packed), P(rows), rows.shape[1], n, P(q), P(act), P(lp), P(pr),
                                 P(ws), ws.numel(), ctypes.byref(opts) if opts is not None else None))
    torch.cuda.synchronize()
    return act, lp, pr


# ------------------------------------------------------------------------------------------------ 3: all-valid is off
TYPE_DISCRETE = 0


def build(B=2048, MB=1024, epochs=2, seed=5, hid=(128, 128), A=90, **opts):
    from rlgym_ppo_amd.ppo import PPOLearner
    torch.manual_seed(seed)
    return PPOLearner(D, A, TYPE_DISCRETE, hid, hid, (0.1, 1.0), B, epochs, 3e-4, 3e-4, CLIP, ENT, MB, "cuda:0", **opts)


def state(learner):
    torch.cuda.synchronize()
    po, vo = learner.policy_optimizer, learner.value_optimizer
    return [t.detach().clone() for t in (learner.policy.arena.flat, learner.value_net.arena.flat, po.exp_avg, po.exp_avg_sq, vo.exp_avg,
                                         vo.exp_avg_sq)] + [po.step_count, vo.step_count, learner.cumulative_model_updates]


def same_state(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y), (what, i)


def same_report(a, b, what):
    keys = set(a) - {"PPO Batch Consumption Time"}
    assert keys == set(b) - {"PPO Batch Consumption Time"}, what
    for k in keys:
        assert a[k] == b[k], (what, k, a[k], b[k])


@pytest.mark.parametrize("hidden", [(128, 128), (128, 96)])
def test_all_valid_mask_is_the_unmasked_rollout_bit_for_bit(L, hidden):
    """(128, 128): the one-launch kernel; (128, 96): the layer chain (a network the fused kernel does not cover)."""
    A = 90
    pol = policy(A, hidden)
    rs = np.random.RandomState(1)
    for n in (37, 1500):
        obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
        ones = np.ones((n, A), bool)
        out = []
        for mask in (None, ones, torch.ones(n, A, device="cuda")):
            torch.manual_seed(77)
            c = (int(L.rlppo_dbg_counter(0)), int(L.rlppo_dbg_counter(1)))
            act, lp = pol.get_action(obs) if mask is None else pol.get_action(obs, action_mask=mask)
            c = (int(L.rlppo_dbg_counter(0)) - c[0], int(L.rlppo_dbg_counter(1)) - c[1])
            if mask is not None:   # (the unmasked small call may be a graph replay: nothing counted)
                assert (c[0] > 0, c[1] > 0) == ((True, False) if hidden == (128, 128) else (False, True)), (hidden, c)
            out.append((torch.as_tensor(act).clone(), torch.as_tensor(lp).clone(), torch.get_rng_state().clone()))
        for o in out[1:]:
            assert torch.equal(o[0], out[0][0]) and torch.equal(o[1], out[0][1]) and torch.equal(o[2], out[0][2]), (hidden, n)
        rows = pol.arena.stage_obs(obs)
        q = torch.empty(n, A).exponential_(1)
        a0, l0 = pol.act_padded(rows, q)
        a1, l1 = pol.act_padded(rows, q, action_mask=ones)
        assert torch.equal(a0, a1) and torch.equal(l0, l1)
        assert torch.equal(pol.get_output(obs), pol.get_output(obs, action_mask=ones))
        d0, d1 = pol.get_action(obs, deterministic=True), pol.get_action(obs, deterministic=True, action_mask=ones)
        assert d0[0] == d1[0] and d0[1] == d1[1] == 0
        r0, r1 = raw_act(L, pol, rows, q.cuda(), None), raw_act(L, pol, rows, q.cuda(), pol._mask_opts(ones, n)[1])
        assert all(torch.equal(x, y) for x, y in zip(r0, r1))


def make_exp(learner, n, seed, mask=None):
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    torch.manual_seed(seed)
    act, logp = learner.policy.get_action(obs) if mask is None else learner.policy.get_action(obs, action_mask=mask)
    act = np.asarray(torch.as_tensor(act).cpu(), np.float32).reshape(n)
    old = (np.asarray(torch.as_tensor(logp).cpu(), np.float32).reshape(n) + 0.1 * rs.randn(n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    return (obs, act, old, z, obs, z, z, rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32))


def buffer(exp, masks=None, seed=9, size=None):
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    buf = ExperienceBuffer(size or exp[0].shape[0], seed, "cpu")
    if masks is None:
        buf.submit_experience(*exp)
    else:
        buf.submit_experience(*exp, action_masks=masks)
    return buf


@pytest.mark.parametrize("paired", [1, 2])
def test_all_valid_mask_is_the_unmasked_update_bit_for_bit(L, paired):
    knob(L, 29, paired)
    try:
        out = []
        for masked in (False, True):
            learner = build()
            exp = make_exp(learner, 4096, 1)
            c3 = int(L.rlppo_dbg_counter(3))
            report = learner.learn(buffer(exp, np.ones((4096, 90), bool) if masked else None))
            assert (int(L.rlppo_dbg_counter(3)) > c3) == (paired == 2)
            out.append((state(learner), report))
    finally:
        knob(L, 29, 1)
    same_state(out[0][0], out[1][0], "all-valid is off")
    same_report(out[0][1], out[1][1], "all-valid is off")
    assert out[0][0][6] == 4


# ------------------------------------------------------------------------------------------------------- 4: sampling
def check_sampling(L, pol, n, seed, fused, label):
    A = pol.n_actions
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(n, D) * 1.5, -5, 5).astype(np.float32)
    m = rand_mask(rs, n, A)
    rows = pol.arena.stage_obs(obs)
    words = pol._mask_opts(m, n)[1]
    q = torch.empty(n, A).exponential_(1, generator=torch.Generator().manual_seed(seed))
    q[1::2] = torch.where(torch.from_numpy(m[1::2]), q[1::2], torch.full_like(q[1::2], 1e-30))   # tiny q on invalid actions
    c = (int(L.rlppo_dbg_counter(0)), int(L.rlppo_dbg_counter(1)))
    act, lp, pr = raw_act(L, pol, rows, q.cuda(), words)
    c = (int(L.rlppo_dbg_counter(0)) - c[0], int(L.rlppo_dbg_counter(1)) - c[1])
    assert c == ((1, 0) if fused else (0, 1)), (label, c)
    pr_h, act_h = pr.cpu().numpy(), act.cpu().numpy()
    assert np.isfinite(pr_h).all() and (pr_h[~m] == 0.0).all(), label
    want = softmax64(logits64(params(pol), obs), m)
    err = np.abs(pr_h - want)[m].max() / want.max()
    v = np.where(m, pr_h / q.numpy(), -np.inf).astype(np.float32)    # float32 division of the kernel's own probabilities
    first = v.argmax(1)                                              # first index of the maximum
    lp_want = torch.log(pr.gather(1, act.view(-1, 1))).view(-1)
    print(f"[mask sampling] {label}: n={n} A={A} max|p - p64|/max p64 = {err:.2e}; actions differing from first arg-max: "
          f"{int((act_h != first).sum())}; max|logp - log pc| = {float((lp - lp_want).abs().max()):.1e}")
    assert err <= 1e-5, (label, err)
    assert np.array_equal(act_h, first), label
    assert m[np.arange(n), act_h].all(), label
    assert torch.equal(lp, lp_want), label
    return act, lp, pr


@pytest.mark.parametrize("A", [3, 33, 90, 128])
def test_masked_sampling_one_launch(L, A):
    check_sampling(L, policy(A, (128, 128), seed=A), 4099, A, True, f"one launch A={A}")


@pytest.mark.parametrize("A", [90, 200, 600])
def test_masked_sampling_chain(L, A):
    check_sampling(L, policy(A, (128, 96), seed=A), 4099, A, False, f"chain A={A}")


def test_one_launch_and_chain_agree_and_no_invalid_action_in_a_million_rows(L):
    pol = policy(90, (128, 128), seed=2)
    a = check_sampling(L, pol, 4099, 11, True, "both forms, one launch")
    knob(L, 27, 0)
    try:
        b = check_sampling(L, pol, 4099, 11, False, "both forms, chain")
    finally:
        knob(L, 27, 1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # >= 10^6 sampled rows, half of every call with q tiny on the invalid actions (where the clamp's 1e-11 floor would win)
    total = 0
    rs = np.random.RandomState(3)
    for n, calls in ((8192, 64), (65536, 8)):   # the one-launch kernel (<= 8192 rows) and the chain
        obs = torch.from_numpy(np.clip(rs.randn(n, D), -5, 5).astype(np.float32))
        rows = pol.arena.stage_obs(obs)
        for k in range(calls):
            m = torch.from_numpy(rand_mask(rs, n, 90, p=0.3 + 0.05 * (k % 8))).cuda()
            q = torch.empty(n, 90, device="cuda").exponential_(1)
            q[: n // 2] = torch.where(m[: n // 2], q[: n // 2], torch.full_like(q[: n // 2], 1e-30))
            c = (int(L.rlppo_dbg_counter(0)), int(L.rlppo_dbg_counter(1)))
            act, lp = pol.act_padded(rows, q, action_mask=m)          # device masks: packed on the device
            c = (int(L.rlppo_dbg_counter(0)) - c[0], int(L.rlppo_dbg_counter(1)) - c[1])
            assert c == ((1, 0) if n <= 8192 else (0, 1))
            assert bool(m.gather(1, act.view(-1, 1)).all()) and bool(torch.isfinite(lp).all())
            total += n
    assert total >= 10 ** 6
    # a device row without a valid action is treated as all-valid
    n = 64
    rows = pol.arena.stage_obs(np.zeros((n, D), np.float32) + 0.1)
    m = torch.ones(n, 90, device="cuda")
    m[5] = 0
    q = torch.empty(n, 90).exponential_(1)
    a0, l0 = pol.act_padded(rows, q)
    a1, l1 = pol.act_padded(rows, q, action_mask=m)
    assert torch.equal(a0, a1) and torch.equal(l0, l1)
    with pytest.raises(ValueError, match="row 5"):
        pol.act_padded(rows, q, action_mask=m.cpu().numpy())


# ----------------------------------------------------------------------------- 5: loss and gradient against float64 truth
def make_problem(pol, val, n, A, seed):
    """Observations, random per-row masks, valid stored actions, and old log-probabilities that keep every ratio >= 5e-4 away from
    both clip edges (old = float64 masked log p of the action - d, d ~ N(0, 0.1^2) redrawn while |exp(d) - (1 +/- clip)| < 1e-3)."""
    rs = np.random.RandomState(seed)
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    m = rand_mask(rs, n, A)
    acts = np.array([rs.choice(np.flatnonzero(r)) for r in m], np.float32)
    p = np.clip(softmax64(logits64(pol, obs), m), 1e-11, 1.0)
    logp = np.log(p[np.arange(n), acts.astype(int)])
    d = 0.1 * rs.randn(n)
    redrawn = 0
    while True:
        bad = np.minimum(np.abs(np.exp(d) - (1 - CLIP)), np.abs(np.exp(d) - (1 + CLIP))) < 1e-3
        if not bad.any():
            break
        redrawn += int(bad.sum())
        d[bad] = 0.1 * rs.randn(int(bad.sum()))
    old = (logp - d).astype(np.float32)
    ratio = np.exp(logp - old.astype(np.float64))
    assert np.minimum(np.abs(ratio - (1 - CLIP)), np.abs(ratio - (1 + CLIP))).min() >= 5e-4   # float64 side alone, no GPU
    outside = float(((ratio < 1 - CLIP) | (ratio > 1 + CLIP)).mean())
    assert 0.02 < outside < 0.15, outside                                                      # both surrogate branches are exercised
    return dict(obs=obs, mask=m, acts=acts, old=old, adv=rs.randn(n).astype(np.float32), tgt=rs.randn(n).astype(np.float32),
                redrawn=redrawn, outside=outside)


def rows_of(pr):
    """A problem as hip_pass.run_pass takes it: (the five row arrays, keywords: rlppo_ppo_minibatch, fp32, under the problem's mask)."""
    return (pr["obs"], pr["acts"], pr["old"], pr["tgt"], pr["adv"]), dict(head="discrete", clip=CLIP, ent=ENT, mask=pr["mask"])


@pytest.mark.parametrize("hidden,A", [((128, 128), 90), ((256, 256, 256), 90), ((128, 128), 200)])
def test_masked_loss_and_gradient_against_float64(L, hidden, A):
    """4096 rows through rlppo_ppo_minibatch directly; A = 200: the wave-per-row loss kernel."""
    torch.manual_seed(A + len(hidden))
    pol, val = nets.init_mlp(D, hidden, A), nets.init_mlp(D, hidden, 1)
    n = 4096
    pr = make_problem(pol, val, n, A, seed=A)
    rows, kw = rows_of(pr)
    got = triple(run_pass(L, pol, val, *rows, np.random.RandomState(1).permutation(n), **kw))
    PY.masked_gate(L, "discrete", pol, val, pr, got, f"[masked fp64 gate] {D} -> {hidden} -> {A}")
    # a stored action its own mask marks invalid (a caller error) stays finite
    pr2 = dict(pr)
    pr2["mask"] = pr["mask"].copy()
    pr2["mask"][np.arange(0, n, 9), pr["acts"][::9].astype(int)] = False
    pr2["mask"][np.arange(0, n, 9), (pr["acts"][::9].astype(int) + 1) % A] = True
    rows, kw = rows_of(pr2)
    gp, gv, st = triple(run_pass(L, pol, val, *rows, np.arange(n), **kw))
    assert all(bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all()) for w, b in gp) and np.isfinite(st).all()


# --------------------------------------------------------------------------- 6: column-constant mask = the narrower network
def test_column_constant_mask_is_the_narrower_network(L):
    A, hidden, n = 90, (128, 128), 4096
    torch.manual_seed(6)
    pol, val = nets.init_mlp(D, hidden, A), nets.init_mlp(D, hidden, 1)
    rs = np.random.RandomState(6)
    S = np.sort(rs.permutation(A)[:60])
    out_S = np.setdiff1d(np.arange(A), S)
    m = np.zeros((n, A), bool)
    m[:, S] = True
    obs = np.clip(rs.randn(n, D), -5, 5).astype(np.float32)
    narrow = [(w.clone(), b.clone()) for w, b in pol[:-1]] + [(pol[-1][0][S].clone(), pol[-1][1][S].clone())]
    p = np.clip(softmax64(logits64(narrow, obs), np.ones((n, len(S)), bool)), 1e-11, 1)
    acts_S = rs.randint(0, len(S), n)
    old = (np.log(p[np.arange(n), acts_S]) + 0.1 * rs.randn(n)).astype(np.float32)
    pr = dict(obs=obs, mask=m, acts=S[acts_S].astype(np.float32), old=old, adv=rs.randn(n).astype(np.float32),
              tgt=rs.randn(n).astype(np.float32))
    rows, kw = rows_of(pr)
    gp, gv, stats = triple(run_pass(L, pol, val, *rows, rs.permutation(n), **kw))
    hw, hb = gp[-1]
    assert bool((hw[out_S] == 0.0).all()) and bool((hb[out_S] == 0.0).all())            # exactly zero outside S
    gp_S = list(gp[:-1]) + [(hw[S], hb[S])]
    fp64_gate.gate(L, "discrete", narrow, val, obs, acts_S.astype(np.float32), old, pr["adv"], pr["tgt"], CLIP, ENT, 1.0, (gp_S, gv, stats),
                   label="column-constant mask against the narrower network")
    # a 2-epoch learn(): the head's parameters outside S do not move, in every update precision
    for prec in ("fp32", "bf16", "x3"):
        learner = build(B=2048, MB=1024, epochs=2, seed=8)
        learner.update_precision = prec
        exp = make_exp(learner, n, 2, mask=m)
        head = learner.policy.arena.linears[-1]
        w0, b0 = head.weight.detach().clone(), head.bias.detach().clone()
        report = learner.learn(buffer(exp, m))
        torch.cuda.synchronize()
        assert torch.equal(head.weight.detach()[out_S], w0[out_S]) and torch.equal(head.bias.detach()[out_S], b0[out_S]), prec
        assert not torch.equal(head.weight.detach()[S], w0[S]) and np.isfinite(report["Mean KL Divergence"]), prec
        assert (np.isin(exp[1].astype(int), S)).all()


# ------------------------------------------------------------------------------- 7: every pass form sees the right rows
def obs_mask(obs, A):
    """A mask that is a known function of the row's own observation."""
    o = np.asarray(obs)[:, :D]
    m = o[:, np.arange(A) % D] + 0.5 * o[:, (3 * np.arange(A) + 1) % D] > -0.4
    m[:, 0] |= ~m.any(1)
    return m


def first_gradient(learner, buf):
    got = []
    learner.grad_probe = lambda g: got.append(g.detach().clone()) if not got else None
    report = learner.learn(buf)
    learner.grad_probe = None
    return got[0].cpu(), report


def split(flat, ps):
    out, o = [], 0
    for w, b in ps:
        gw = flat[o:o + w.numel()].view(w.shape)
        o += w.numel()
        out.append((gw, flat[o:o + b.numel()]))
        o += b.numel()
    return out, o


def wrapped_buffer(pr, size, chunks, extra_seed=0):
    """Submits `extra` older rows and then the problem's rows in uneven chunks, so the ring wraps (ring_base != 0) and ends up
    holding exactly the problem's rows in logical order."""
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    n = pr["obs"].shape[0]
    assert n == size
    rs = np.random.RandomState(100 + extra_seed)
    extra = 1234
    eo = np.clip(rs.randn(extra, D), -5, 5).astype(np.float32)
    ez = np.zeros(extra, np.float32)
    allf = dict(obs=np.concatenate([eo, pr["obs"]]), acts=np.concatenate([ez, pr["acts"]]), old=np.concatenate([ez, pr["old"]]),
                tgt=np.concatenate([ez, pr["tgt"]]), adv=np.concatenate([ez, pr["adv"]]),
                mask=np.concatenate([obs_mask(eo, pr["mask"].shape[1]), pr["mask"]]))
    buf = ExperienceBuffer(size, 9, "cpu")
    o = 0
    for c in chunks:
        s = slice(o, o + c)
        z = np.zeros(c, np.float32)
        buf.submit_experience(allf["obs"][s], allf["acts"][s], allf["old"][s], z, allf["obs"][s], z, z, allf["tgt"][s], allf["adv"][s],
                              action_masks=allf["mask"][s])
        o += c
    assert o == extra + n
    return buf


def ring_problem(learner, n, A, seed):
    pol, val = params(learner.policy), params(learner.value_net)
    pr = make_problem(pol, val, n, A, seed)
    # the masks become a function of the row's own observation; actions and old log-probabilities are redone under them
    rs = np.random.RandomState(seed + 1)
    pr["mask"] = m = obs_mask(pr["obs"], A)
    pr["acts"] = np.array([rs.choice(np.flatnonzero(r)) for r in m], np.float32)
    p = np.clip(softmax64(logits64(pol, pr["obs"]), m), 1e-11, 1.0)
    logp = np.log(p[np.arange(n), pr["acts"].astype(int)])
    d = 0.1 * rs.randn(n)
    while True:
        bad = np.minimum(np.abs(np.exp(d) - (1 - CLIP)), np.abs(np.exp(d) - (1 + CLIP))) < 1e-3
        if not bad.any():
            break
        d[bad] = 0.1 * rs.randn(int(bad.sum()))
    pr["old"] = (logp - d).astype(np.float32)
    ratio = np.exp(logp - pr["old"].astype(np.float64))
    assert np.minimum(np.abs(ratio - (1 - CLIP)), np.abs(ratio - (1 + CLIP))).min() >= 5e-4
    return pol, val, pr


def test_every_pass_form_sees_the_right_rows_of_a_wrapped_ring(L):
    from rlgym_ppo_amd import dp
    n, A = 4096, 90
    chunks = (700, 1500, 333, 1200, 997, 600)
    grads = {}
    for form, (k26, k29, slots, MB) in dict(separate=(0, 1, 1, 4096), rowtab=(2, 1, 1, 4096), paired=(1, 2, 1, 4096),
                                            slots2=(1, 1, 2, 2048)).items():
        knob(L, 26, k26)
        knob(L, 29, k29)
        try:
            learner = build(B=n, MB=MB, epochs=1, seed=5)
            learner.n_slots = slots
            pol, val, pr = ring_problem(learner, n, A, seed=21)
            buf = wrapped_buffer(pr, n, chunks)
            store, base, cap = buf.ring()
            assert base != 0 and cap == n and "action_masks" in store and store["action_masks"].dtype == torch.int32
            assert np.array_equal(buf.action_masks.cpu().numpy(), pr["mask"])                 # logical order
            assert np.array_equal(buf.states.cpu().numpy(), pr["obs"])
            c = (int(L.rlppo_dbg_counter(3)), int(L.rlppo_dbg_counter(4)))
            g, report = first_gradient(learner, buf)
            c = (int(L.rlppo_dbg_counter(3)) - c[0], int(L.rlppo_dbg_counter(4)) - c[1])
            if form == "separate":
                assert c[1] == 0
            if form == "rowtab":
                assert c[1] > 0
            if form == "paired":
                assert c[0] > 0
        finally:
            knob(L, 26, 1)
            knob(L, 29, 1)
        grads[form] = g
        gp, o = split(g, pol)
        gv, _ = split(g[o:], val)
        if form in ("paired", "slots2"):
            PY.masked_gate(L, "discrete", pol, val, pr, (gp, gv, None), f"[masked fp64 gate] wrapped ring, {form}")
    # the two gather forms: bit for bit where the unmasked pass is
    unmasked = {}
    for form, k26 in (("separate", 0), ("rowtab", 2)):
        knob(L, 26, k26)
        try:
            learner = build(B=n, MB=4096, epochs=1, seed=5)
            unmasked[form] = first_gradient(learner, buffer(make_exp(learner, n, 4)))[0]
        finally:
            knob(L, 26, 1)
    if torch.equal(unmasked["separate"], unmasked["rowtab"]):
        assert torch.equal(grads["separate"], grads["rowtab"])
    else:
        print("[mask ring] the unmasked separate-gather and row-table gradients differ themselves: "
              f"{fp64_gate._rel(unmasked['separate'], unmasked['rowtab']):.1e}")
        assert fp64_gate._rel(grads["separate"], grads["rowtab"]) < 1e-5
    # mixing masked and unmasked submits raises; clear() resets that
    buf = buffer(make_exp(learner, 512, 3), size=2048)
    with pytest.raises(ValueError, match="masked or not"):
        buf.submit_experience(*make_exp(learner, 512, 3), action_masks=np.ones((512, A), bool))
    buf.clear()
    buf.submit_experience(*make_exp(learner, 512, 3), action_masks=np.ones((512, A), bool))
    with pytest.raises(ValueError, match="masked or not"):
        buf.submit_experience(*make_exp(learner, 512, 3))
    assert buf.action_masks.shape == (512, A)
    # 2 virtual ranks end a masked learn() bit-identical to each other
    reps = [build(B=n, MB=512, epochs=2, seed=5) for _ in range(2)]
    pol, val, pr = ring_problem(reps[0], n, A, seed=22)
    dp.run_virtual_ranks(reps, [wrapped_buffer(pr, n, chunks) for _ in range(2)])
    same_state(state(reps[0])[:6], state(reps[1])[:6], "2 virtual ranks")
    assert not torch.equal(reps[0].policy.arena.flat, build(B=n, MB=512, epochs=2, seed=5).policy.arena.flat)
    # a non-discrete learner refuses a masked buffer
    from rlgym_ppo_amd.ppo import PPOLearner
    torch.manual_seed(1)
    gl = PPOLearner(D, 8, 2, (64, 64), (64, 64), (0.1, 1.0), 512, 1, 3e-4, 3e-4, CLIP, ENT, 512, "cuda:0")
    z = np.zeros(512, np.float32)
    gb = buffer((pr["obs"][:512], np.zeros((512, 8), np.float32), z, z, pr["obs"][:512], z, z, z, z), np.ones((512, 8), bool))
    with pytest.raises(ValueError, match="discrete head"):
        gl.learn(gb)


# ------------------------------------------------------------------------------------------------------ 8: end to end
class MaskedVectorEnv(synthetic_env.SyntheticVectorEnv):
    """action_masks(): a deterministic function of the observation the agents act on next."""

    def _obs(self):
        self.last = super()._obs()
        return self.last

    def action_masks(self):
        return obs_mask(self.last, 90)


class RecordingEnv(MaskedVectorEnv):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []   # (mask the agents acted under, actions)

    def step(self, actions):
        self.log.append((obs_mask(self.last, 90), np.asarray(actions).reshape(-1).astype(int).copy()))
        return super().step(actions)


def run_learner(env_cls, fused, iters=3):
    import contextlib, io
    from rlgym_ppo_amd import Learner
    na, T = 64, 8
    envs = []

    def mk():
        envs.append(env_cls(n_agents=na, seed=4))
        return envs[-1]
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = Learner(mk, vector_env=True, n_proc=1, timestep_limit=10 ** 9, exp_buffer_size=na * T, ts_per_iteration=na * T,
                          ppo_epochs=2, ppo_batch_size=na * T, ppo_minibatch_size=na * T // 2, policy_layer_sizes=(64, 64),
                          critic_layer_sizes=(64, 64), checkpoints_save_folder=None, checkpoint_load_folder=None, save_every_ts=10 ** 12,
                          log_to_wandb=False, random_seed=5, standardize_obs=False)
    out = []
    try:
        if not fused:
            learner.ppo_learner.policy.fused_step = False
        for it in range(iters):
            exp, _, n_col, _ = learner.agent.collect_timesteps(na * T)
            masks = learner.agent.action_masks
            with contextlib.redirect_stdout(io.StringIO()):
                learner.add_new_experience(exp)
                report = learner.ppo_learner.learn(learner.experience_buffer)
            bm = learner.experience_buffer.action_masks
            out.append(dict(actions=exp[1].cpu().numpy().reshape(-1).astype(int), logp=exp[2].cpu().numpy().copy(),
                            masks=None if masks is None else masks.cpu().numpy(), buf=None if bm is None else bm.cpu().numpy(),
                            report=report, flat=learner.ppo_learner.policy.arena.flat.detach().cpu().clone()))
    finally:
        learner.agent.cleanup()
    return out, envs[0], na, T


def test_learner_loop_with_action_masks_end_to_end():
    runs = {}
    for fused in (True, False):
        out, env, na, T = run_learner(RecordingEnv, fused)
        runs[fused] = out
        for it, o in enumerate(out):
            log = env.log[it * T:(it + 1) * T]
            m_tm = np.stack([m for m, _ in log])                          # [T, na, A]: the masks the environment gave, step by step
            a_tm = np.stack([a for _, a in log])
            want = m_tm.transpose(1, 0, 2).reshape(na * T, 90)            # trajectory-major
            assert np.array_equal(o["actions"], a_tm.T.reshape(-1))
            assert want[np.arange(na * T), o["actions"]].all(), ("an invalid action was collected", fused, it)
            assert np.array_equal(o["masks"], want) and np.array_equal(o["buf"], want), (fused, it)
            assert all(np.isfinite(v) for v in o["report"].values() if isinstance(v, float)), o["report"]
    for a, b in zip(runs[True], runs[False]):                             # fused and chain collection agree bit for bit
        assert np.array_equal(a["actions"], b["actions"]) and np.array_equal(a["logp"], b["logp"]) and torch.equal(a["flat"], b["flat"])
    # the same environment without the method: no masks anywhere, and not the masked run's actions
    plain, _, _, _ = run_learner(synthetic_env.SyntheticVectorEnv, True, iters=2)
    assert plain[0]["masks"] is None and plain[0]["buf"] is None
    assert not np.array_equal(plain[0]["actions"], runs[True][0]["actions"])
