"""Invalid-action masking of the multi-discrete head on the GPU (include/rlppo.h, "[nvec, masked]"): rlppo_multidiscrete_act_nvec_masked
and rlppo_ppo_minibatch_nvec with a mask of one bit per logit, against float64 restated in tests/masked_multidiscrete_yardstick.py;
all-valid is the unmasked general kernels bit for bit; a column-constant mask is the narrower policy; every pass form and a rotated
ring see the right mask rows; MultiDiscreteFF and the Learner loop on a vector environment with action_masks()."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets  # noqa: E402
import fp64_gate  # noqa: E402
import masked_multidiscrete_yardstick as M  # noqa: E402
import multidiscrete_env as E  # noqa: E402
import multidiscrete_nvec_yardstick as Y  # noqa: E402
import ppo_yardstick as PY  # noqa: E402
from hip_pass import L, Net, check, run_pass, triple  # noqa: E402,F401

BINS = (2, 7, 3, 11, 2)


def finite(grads):
    return all(bool(torch.isfinite(w).all()) and bool(torch.isfinite(b).all()) for w, b in grads)


# ------------------------------------------------------------------------------------------------ 1. all-valid is off
@pytest.mark.parametrize("bins", [BINS, (30, 64, 5)])
def test_all_valid_mask_is_the_unmasked_general_kernels_bit_for_bit(L, bins):
    S, H = sum(bins), len(bins)
    pol, val, pr, rs = M.make_problem(bins, 11 + H, 5000)
    net = Net(L, pol)
    n = 603
    q = nets.draw_exp_noise(n * H, max(bins))
    rows = net.pad(pr["obs"][:n])
    a0, l0 = M.act_nvec(L, net, bins, rows, n, q)                      # (act_nvec asserts counter 6 advances by one per call)
    a1, l1 = M.act_nvec(L, net, bins, rows, n, q, mask=np.ones((n, S), bool))
    assert np.array_equal(a0, a1) and np.array_equal(l0, l1)
    idx = rs.randint(0, 5000, 1500)
    out = []
    for mask in (None, np.ones((5000, S), bool)):
        c6 = L.rlppo_dbg_counter(6)
        rows, kw = M.pass_args(pr, bins, mask=mask)
        out.append(triple(run_pass(L, pol, val, *rows, idx, mb_ratio=0.5, **kw)))
        assert L.rlppo_dbg_counter(6) == c6 + 1
    (gp0, gv0, st0, dz0), (gp1, gv1, st1, dz1) = out
    for (x, y), (u, v) in zip(gp0 + gv0, gp1 + gv1):
        assert torch.equal(x, u) and torch.equal(y, v)
    assert np.array_equal(st0, st1) and np.array_equal(dz0, dz1)
    Y.check_output_gradient(dz1, gp1, S)


# ------------------------------------------------------------------------------------------------ 2. sampling
# (bins, rows, observation width, hidden layers, seed).  The seeds were picked on the CPU, from the float64 reference alone, so that
# the inputs hold at most 2 near-ties (M.check_sampled asserts that first).
SAMPLING_CASES = {
    "one_word": (BINS, 613, 107, (64, 64), 1),
    "head_across_a_word_boundary": ((20, 20, 20), 601, 40, (64, 64), 1),
    "64_bin_head_over_three_words": ((30, 64, 5), 607, 64, (64, 64), 1),
    "S_past_64": ((33, 2, 31), 599, 64, (64, 64), 1),
    "H_at_cap": ((2,) * 64, 593, 107, (128, 128), 1),
    "S_at_cap": ((64,) * 8, 589, 72, (64, 64), 1),
    "one_bin_head": ((1, 4), 577, 33, (64, 64), 1),
    "reference_bins": (Y.REFERENCE_BINS, 611, 107, (64, 64), 1),
}


def sampling_inputs(name):
    bins, n, d, hidden, seed = SAMPLING_CASES[name]
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    pol = nets.init_mlp(d, hidden, sum(bins))
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    q = nets.draw_exp_noise(n * len(bins), max(bins))
    mask = M.rand_mask(rs, n, bins)
    return bins, pol, obs, q, mask


@pytest.mark.parametrize("name", list(SAMPLING_CASES))
def test_masked_act_nvec_against_float64(L, name):
    bins, pol, obs, q, mask = sampling_inputs(name)
    v3 = M.head_valid(mask, bins)
    assert mask[3].all() and (v3[0].sum(-1) == 1).all() and mask[0, sum(bins) - 1]   # all valid; one bin per head, the last of the last
    net = Net(L, pol)
    n = obs.shape[0]
    qn = q.numpy().copy()
    qn.reshape(n, len(bins), max(bins))[1::2][~v3[1::2]] = 1e-30     # tiny noise on invalid (and padded) bins: never read
    act, logp = M.act_nvec(L, net, bins, net.pad(obs), n, qn, mask=mask)
    M.check_sampled(act, logp, Y.logits64(pol, obs), bins, q.numpy(), mask)


def test_no_invalid_action_in_262144_rows(L):
    bins, n, d = BINS, 262144, 20
    S, H = sum(bins), len(bins)
    torch.manual_seed(2)
    net = Net(L, nets.init_mlp(d, (64, 64), S))
    g = torch.Generator(device="cuda").manual_seed(5)
    obs = torch.randn(n, d, device="cuda", generator=g).clamp_(-5, 5)
    mask = torch.rand(n, S, device="cuda", generator=g) < 0.6
    for s, b in zip(M.starts(bins), bins):   # one bin forced valid per head
        mask[torch.arange(n, device="cuda"), s + torch.randint(0, b, (n,), device="cuda", generator=g)] = True
    q = torch.empty(n * H, max(bins), device="cuda").exponential_(1, generator=g)
    act, logp = M.act_nvec(L, net, bins, net.pad(obs.cpu().numpy()), n, q, mask=mask)
    assert np.isfinite(logp).all()
    v3 = M.head_valid(mask.cpu().numpy(), bins)
    assert np.take_along_axis(v3, act[..., None], -1).all()


# ------------------------------------------------------------------------------------------------ 3. the update
UPDATE_CASES = {
    "ragged_1500_of_5000": (BINS, 5000, 1500, False),
    "three_words_1300_of_1800": ((30, 64, 5), 1800, 1300, False),
    "saturated_2999_of_3500": ((33, 2, 31), 3500, 2999, True),
    "one_bin_head": ((1, 4), 1400, 1100, False),
}


@pytest.mark.parametrize("name", list(UPDATE_CASES))
def test_masked_minibatch_nvec_against_float64(L, monkeypatch, name):
    """The masked pass through ppo_yardstick.masked_gate: err(HIP, fp64 under the HIP's ReLU decisions) <= max(1e-5, 1.5 x err(float32 torch
    restatement, fp64 under its own)), statistics likewise; dz exactly 0 on invalid logits and on columns >= S, finite everywhere."""
    bins, n, mb, saturate = UPDATE_CASES[name]
    S = sum(bins)
    pol, val, pr, rs = M.make_problem(bins, 50 + len(bins), n, saturate=saturate)
    if name == "ragged_1500_of_5000":
        idx = rs.randint(0, n, mb)   # drawn with repeats
        idx[:3] = [n - 1, 0, n - 1]
    else:
        idx = rs.permutation(n)[:mb]
    if saturate:
        assert 25 < np.abs(Y.logits64(pol, pr["obs"])).max() <= 30.001
    ratio = np.exp(pr["logp"][idx] - pr["old"][idx].astype(np.float64))
    assert (ratio < 0.8).sum() > 10 and (ratio > 1.2).sum() > 10                        # both clip edges are crossed ...
    assert np.minimum(np.abs(ratio - 0.8), np.abs(ratio - 1.2)).min() >= 5e-4           # ... and no row sits on one
    c6 = L.rlppo_dbg_counter(6)
    rows, kw = M.pass_args(pr, bins)
    gp, gv, st, dz = triple(run_pass(L, pol, val, *rows, idx, mb_ratio=0.5, **kw))
    assert L.rlppo_dbg_counter(6) == c6 + 1
    Y.check_output_gradient(dz, gp, S)
    m = pr["mask"][idx]
    assert (dz[:, :S][~m] == 0).all() and np.isfinite(dz).all() and (dz[:, :S][m] != 0).any()
    if 1 in bins:   # a head of one bin: zero gradient in its column
        assert (dz[:, M.starts(bins)[bins.index(1)]] == 0).all()
    one = M.head_valid(m, bins).sum(-1) == 1   # heads with exactly one valid bin: zero gradient on it too
    for h, (s, b) in enumerate(zip(M.starts(bins), bins)):
        assert (dz[one[:, h], s:s + b] == 0).all(), h
    Y.patch_oracle(monkeypatch, bins)
    PY.masked_gate(L, "nvec", pol, val, M.rows(pr, idx), (gp, gv, st), f"[masked nvec fp64 gate] masked multi-discrete {name}, {mb} rows", 0.5, bins)
    # stored actions their own masks mark invalid, on every ninth row (a caller error): everything stays finite
    bad = dict(pr)
    bad["mask"] = pr["mask"].copy()
    r = np.arange(0, n, 9)
    for h, (s, b) in enumerate(zip(M.starts(bins), bins)):
        if b > 1:
            a = pr["acts"][r, h].astype(int)
            bad["mask"][r, s + a] = False
            bad["mask"][r, s + (a + 1) % b] = True
    rows, kw = M.pass_args(bad, bins)
    gp, gv, st, dz = triple(run_pass(L, pol, val, *rows, np.arange(n), mb_ratio=1.0, **kw))
    assert finite(gp) and finite(gv) and np.isfinite(st).all() and np.isfinite(dz).all() and (dz[:, :S][~bad["mask"]] == 0).all()


# ------------------------------------------------------------------------------------------------ 4. column-constant mask
KEPT = ((0, 1), (0, 2, 3, 6), (1,), (0, 1, 4, 5, 7, 10), (0,))   # the bins every row keeps, per head of BINS
REDUCED = tuple(len(k) for k in KEPT)


def test_column_constant_mask_is_the_narrower_policy(L, monkeypatch):
    bins, n, d, hidden = BINS, 2000, 107, (128, 128)
    S, H, B, Br = sum(bins), len(bins), max(bins), max(REDUCED)
    cols = np.concatenate([s + np.asarray(k) for s, k in zip(M.starts(bins), KEPT)])      # kept logits, in order
    gone = np.setdiff1d(np.arange(S), cols)
    torch.manual_seed(6)
    rs = np.random.RandomState(6)
    pol, val = nets.init_mlp(d, hidden, S), nets.init_mlp(d, hidden, 1)
    narrow = [(w.clone(), b.clone()) for w, b in pol[:-1]] + [(pol[-1][0][cols].clone(), pol[-1][1][cols].clone())]
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    mask = np.zeros((n, S), bool)
    mask[:, cols] = True
    # ---- sampling: identical actions after index remapping, identical log-probabilities
    ns = 601
    q = nets.draw_exp_noise(ns * H, B).numpy().reshape(ns, H, B)
    qr = np.ones((ns, H, Br), np.float32)
    for h, k in enumerate(KEPT):
        qr[:, h, :len(k)] = q[:, h, list(k)]
    full, small = Net(L, pol), Net(L, narrow)
    act, logp = M.act_nvec(L, full, bins, full.pad(obs[:ns]), ns, q.reshape(ns * H, B), mask=mask[:ns])
    act_r, logp_r = M.act_nvec(L, small, REDUCED, small.pad(obs[:ns]), ns, qr.reshape(ns * H, Br))
    for h, k in enumerate(KEPT):
        assert np.array_equal(act[:, h], np.asarray(k)[act_r[:, h]]), h
    assert np.array_equal(logp, logp_r)
    # ---- the update: actions and old log-probabilities drawn from the narrower policy by the float64 yardstick
    z = Y.logits64(narrow, obs)
    a_r, lp, _, _ = Y.sample64(z, REDUCED, nets.draw_exp_noise(n * H, Br).numpy())
    a_full = np.stack([np.asarray(k)[a_r[:, h]] for h, k in enumerate(KEPT)], 1).astype(np.float32)
    old = (lp + 0.2 * rs.randn(n)).astype(np.float32)
    tgt, adv = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    idx = rs.permutation(n)[:1500]
    pr = dict(obs=obs, acts=a_full, old=old, tgt=tgt, adv=adv, mask=mask)
    rows, kw = M.pass_args(pr, bins)
    gp, gv, st, dz = triple(run_pass(L, pol, val, *rows, idx, mb_ratio=0.5, **kw))
    gpr, gvr, str_, dzr = triple(run_pass(L, narrow, val, obs, a_r.astype(np.float32), old, tgt, adv, idx, head="nvec", entry="nvec",
                                          bins=REDUCED, clip=0.2, ent=0.005, mb_ratio=0.5, dz=True))
    assert np.array_equal(dz[:, cols], dzr[:, :len(cols)]) and (dz[:, gone] == 0).all() and (dz[:, S:] == 0).all()
    hw, hb = gp[-1]
    assert bool((hw[gone] == 0).all()) and bool((hb[gone] == 0).all())
    Y.patch_oracle(monkeypatch, REDUCED)
    gp_r = list(gp[:-1]) + [(hw[cols], hb[cols])]
    fp64_gate.gate(L, "multidiscrete", narrow, val, obs[idx], a_r[idx].astype(np.float32), old[idx], adv[idx], tgt[idx], 0.2, 0.005, 0.5,
                   (gp_r, gv, st), label="column-constant mask against the narrower multi-discrete policy")
    # ---- a 2-epoch learn(): the head's rows of removed bins do not move, in every update precision
    from rlgym_ppo_amd.ppo import ExperienceBuffer, PPOLearner
    nl = 1024
    for prec in ("fp32", "bf16", "x3"):
        torch.manual_seed(8)
        learner = PPOLearner(d, bins, 1, hidden, hidden, (0.1, 1.0), 512, 2, 3e-4, 3e-4, 0.2, 0.005, 256, "cuda:0")
        learner.update_precision = prec
        torch.manual_seed(9)
        a, lp = learner.policy.get_action(obs[:nl], action_mask=mask[:nl])
        a = a.numpy()
        for h, k in enumerate(KEPT):
            assert np.isin(a[:, h], k).all(), (prec, h)
        buf = ExperienceBuffer(nl, 3, "cpu")
        zero = np.zeros(nl, np.float32)
        buf.submit_experience(obs[:nl], a.astype(np.float32), lp.numpy() + 0.1 * rs.randn(nl).astype(np.float32), zero, obs[:nl], zero, zero,
                              tgt[:nl], adv[:nl], action_masks=mask[:nl])
        head = learner.policy.arena.linears[-1]
        w0, b0 = head.weight.detach().clone(), head.bias.detach().clone()
        report = learner.learn(buf)
        torch.cuda.synchronize()
        assert torch.equal(head.weight.detach()[gone], w0[gone]) and torch.equal(head.bias.detach()[gone], b0[gone]), prec
        assert not torch.equal(head.weight.detach()[cols], w0[cols]) and np.isfinite(report["Mean KL Divergence"]), prec


# ------------------------------------------------------------------------------------------------ 5. pass forms and ring
def obs_mask(obs, bins, d):
    """A mask that is a known function of the row's own observation (every head keeps a valid bin: its first, where none is)."""
    o = np.asarray(obs)[:, :d]
    c = np.arange(sum(bins))
    m = o[:, c % d] + 0.5 * o[:, (3 * c + 1) % d] > -0.4
    for s, b in zip(M.starts(bins), bins):
        m[:, s] |= ~m[:, s:s + b].any(1)
    return m


def test_masked_launch_forms_and_ring(L, monkeypatch):
    """The knob sets of tests/test_gpu_multidiscrete_nvec.py::test_launch_forms_and_ring_for_nvec (26, 29, 32, 33) on 256 x 3 nets:
    fused / separate gather / two chains / stacked pairs give bit-identical gradients, a ring-rotated buffer the plain buffer's, and
    the result passes the masked float64 gate."""
    bins, n, base, d = BINS, 5000, 3777, 107
    pol, val, pr, rs = M.make_problem(bins, 77, n, hidden=(256, 256, 256), mask_fn=lambda o: obs_mask(o, bins, d))
    assert 0.2 < pr["mask"].mean() < 0.9
    idx = rs.randint(0, n, 1500)
    idx[:4] = [n - base - 1, n - base, 0, n - 1]
    forms = dict(fused=(2, 2, 0, 1), separate_gather=(0, 2, 0, 1), two_chains=(2, 0, 0, 1), stacked_pairs=(2, 2, 0, 0))
    runs, paired = {}, {}
    for key, (k26, k29, k32, k33) in forms.items():
        for knob, v in ((26, k26), (29, k29), (32, k32), (33, k33)):
            check(L, L.rlppo_dbg_set(knob, v))
        try:
            c3 = L.rlppo_dbg_counter(3)
            rows, kw = M.pass_args(pr, bins)
            runs[key] = triple(run_pass(L, pol, val, *rows, idx, mb_ratio=0.25, **kw))
            paired[key] = L.rlppo_dbg_counter(3) - c3
            if key == "fused":
                rows, kw = M.pass_args(pr, bins)
                runs["ring"] = triple(run_pass(L, pol, val, *rows, idx, mb_ratio=0.25, ring=base, **kw))
        finally:
            for knob in (26, 29, 32, 33):
                check(L, L.rlppo_dbg_set(knob, 1))
    assert paired["fused"] == 1 and paired["two_chains"] == 0 and paired["stacked_pairs"] == 1
    gp0, gv0, st0, _ = runs["fused"]
    for key, (gp, gv, st, _) in runs.items():
        for (x, y), (u, v) in zip(gp0 + gv0, gp + gv):
            assert torch.equal(x, u) and torch.equal(y, v), key
        np.testing.assert_allclose(st0, st, rtol=1e-12, atol=0, err_msg=key)
    # (a pass that read another row's mask words would not be this one: the unmasked pass differs)
    rows, kw = M.pass_args(pr, bins, mask=None)
    plain = triple(run_pass(L, pol, val, *rows, idx, mb_ratio=0.25, **kw))
    assert not torch.equal(plain[0][-1][0], gp0[-1][0])
    Y.patch_oracle(monkeypatch, bins)
    PY.masked_gate(L, "nvec", pol, val, M.rows(pr, idx), runs["fused"][:3], "[masked nvec fp64 gate] masked multi-discrete, launch forms, 1500 rows", 0.25,
                   bins)


# ------------------------------------------------------------------------------------------------ 6. policy class, learner loop
def params(policy):
    return [(l.weight.detach().cpu().clone(), l.bias.detach().cpu().clone()) for l in policy.arena.linears]


def test_policy_class_takes_a_mask(L):
    from rlgym_ppo_amd.ppo import ExperienceBuffer, MultiDiscreteFF, PPOLearner
    torch.manual_seed(4)
    pol = MultiDiscreteFF(E.OBS_DIM, (64, 64), "cuda:0", bins=BINS)
    rs = np.random.RandomState(4)
    n, S, H = 300, sum(BINS), len(BINS)
    obs = np.clip(rs.randn(n, E.OBS_DIM), -5, 5).astype(np.float32)
    mask = M.rand_mask(rs, n, BINS)
    z64 = Y.logits64(params(pol), obs)
    for form in (mask, torch.from_numpy(mask).cuda()):
        torch.manual_seed(21)
        c6 = L.rlppo_dbg_counter(6)
        act, logp = pol.get_action(obs, action_mask=form)      # a small host batch: the general path, not the graph replay
        assert L.rlppo_dbg_counter(6) == c6 + 1
        state = torch.get_rng_state()
        torch.manual_seed(21)
        q = torch.empty(n * H, max(BINS)).exponential_(1)
        assert torch.equal(state, torch.get_rng_state())        # the noise draw is the unmasked call's
        assert act.dtype == torch.int64 and tuple(act.shape) == (n, H)
        M.check_sampled(act.numpy(), logp.numpy(), z64, BINS, q.numpy(), mask)
    det, _ = pol.get_action(obs, deterministic=True, action_mask=mask)
    zz = np.where(mask, z64, -np.inf)
    want = np.stack([zz[:, s:s + b].argmax(-1) for s, b in zip(M.starts(BINS), BINS)])
    assert det.shape == (H, n) and (det != want).sum() <= 2
    assert np.take_along_axis(M.head_valid(mask, BINS), det.T[..., None], -1).all()
    # get_backprop_data: the masked log-probabilities
    lp_bp, ent = pol.get_backprop_data(obs, act.cuda(), action_mask=mask)
    assert np.abs(lp_bp.detach().cpu().numpy() - logp.numpy()).max() < 1e-4 and np.isfinite(float(ent.detach()))
    # host masks are held to the per-head rule; get_output keeps refusing
    broken = mask.copy()
    broken[5, 2:9] = False
    with pytest.raises(ValueError, match="row 5, head 1"):
        pol.get_action(obs, action_mask=broken)
    with pytest.raises(ValueError, match="multi-discrete"):
        pol.get_output(obs, action_mask=mask)
    with pytest.raises(ValueError, match="shape"):
        pol.get_action(obs, action_mask=np.ones((n, S + 1), bool))
    # the reference's bins with a mask: the general kernels, through rollout and update
    torch.manual_seed(5)
    learner = PPOLearner(E.OBS_DIM, 8, 1, (64, 64), (64, 64), (0.1, 1.0), 256, 1, 3e-4, 3e-4, 0.2, 0.005, 128, "cuda:0")
    ref = learner.policy
    assert ref.md_nvec is None
    mref = M.rand_mask(rs, n, Y.REFERENCE_BINS)
    torch.manual_seed(22)
    c6 = L.rlppo_dbg_counter(6)
    ref.act_graphs = False
    a0, _ = ref.get_action(obs)
    assert L.rlppo_dbg_counter(6) == c6                         # unmasked: the fixed kernel
    torch.manual_seed(22)
    a1, lp1 = ref.get_action(obs, action_mask=mref)
    assert L.rlppo_dbg_counter(6) == c6 + 1                     # masked: the general kernel
    assert np.take_along_axis(M.head_valid(mref, Y.REFERENCE_BINS), a1.numpy()[..., None], -1).all() and not torch.equal(a0, a1)
    torch.manual_seed(22)
    a2, lp2 = ref.get_action(obs, action_mask=np.ones_like(mref))
    assert torch.equal(a0, a2)                                  # all-valid on the general kernel: the fixed kernel's actions
    buf = ExperienceBuffer(n, 1, "cpu")
    zero = np.zeros(n, np.float32)
    buf.submit_experience(obs, a1.numpy().astype(np.float32), lp1.numpy(), zero, obs, zero, zero, rs.randn(n).astype(np.float32),
                          rs.randn(n).astype(np.float32), action_masks=mref)
    assert tuple(buf.action_masks.shape) == (n, 21) and tuple(buf.actions.shape) == (n, 8)
    c6 = L.rlppo_dbg_counter(6)
    report = learner.learn(buf)
    assert L.rlppo_dbg_counter(6) > c6 and all(np.isfinite(float(v)) for v in report.values())
    # the Gaussian head keeps its refusal
    torch.manual_seed(1)
    gl = PPOLearner(E.OBS_DIM, 8, 2, (64, 64), (64, 64), (0.1, 1.0), 256, 1, 3e-4, 3e-4, 0.2, 0.005, 128, "cuda:0")
    gb = ExperienceBuffer(n, 1, "cpu")
    gb.submit_experience(obs, np.zeros((n, 8), np.float32), zero, zero, obs, zero, zero, zero, zero, action_masks=np.ones((n, 8), bool))
    with pytest.raises(ValueError, match="policy_type 2"):
        gl.learn(gb)


class MaskedNvecEnv(E.NvecVectorEnv):
    """action_masks(): a deterministic function of the observation the agents act on next; step() records the mask the agents acted
    under next to their actions."""
    all_valid = False

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.log = []

    def _obs(self):
        self.last = super()._obs()
        return self.last

    def _mask(self):
        m = obs_mask(self.last, BINS, E.OBS_DIM)
        return np.ones_like(m) if self.all_valid else m

    def action_masks(self):
        return self._mask()

    def step(self, actions):
        self.log.append((self._mask(), np.asarray(actions).reshape(self.n_agents, -1).astype(int).copy()))
        return super().step(actions)


class AllValidEnv(MaskedNvecEnv):
    all_valid = True


class WrongWidthEnv(MaskedNvecEnv):
    def action_masks(self):
        return np.ones((self.n_agents, len(BINS)), bool)   # one entry per component instead of one per bin


def run_learner(env_cls, iters=3):
    import contextlib
    import io
    from rlgym_ppo_amd import Learner
    T = 16
    envs = []

    def mk():
        envs.append(env_cls(seed=4))
        return envs[-1]
    na = 12
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = Learner(mk, vector_env=True, n_proc=1, timestep_limit=10 ** 9, exp_buffer_size=na * T, ts_per_iteration=na * T,
                          ppo_epochs=2, ppo_batch_size=na * T, ppo_minibatch_size=na * T // 2, policy_layer_sizes=(64, 64),
                          critic_layer_sizes=(64, 64), checkpoints_save_folder=None, checkpoint_load_folder=None, save_every_ts=10 ** 12,
                          log_to_wandb=False, random_seed=5, standardize_obs=False, multi_discrete_bins=BINS)
    out = []
    try:
        for it in range(iters):
            exp, _, n_col, _ = learner.agent.collect_timesteps(na * T)
            with contextlib.redirect_stdout(io.StringIO()):
                learner.add_new_experience(exp)
                report = learner.ppo_learner.learn(learner.experience_buffer)
            bm = learner.experience_buffer.action_masks
            out.append(dict(actions=exp[1].cpu().numpy().astype(int), buf=None if bm is None else bm.cpu().numpy(), report=report,
                            flat=learner.ppo_learner.policy.arena.flat.detach().cpu().clone()))
    finally:
        learner.agent.cleanup()
    return out, envs[0], na, T


def test_learner_loop_on_a_vector_environment_with_action_masks(L):
    from test_gpu_action_mask import same_report
    S, H = sum(BINS), len(BINS)
    c6 = L.rlppo_dbg_counter(6)
    out, env, na, T = run_learner(MaskedNvecEnv)
    assert L.rlppo_dbg_counter(6) > c6 and env.out_of_range_steps == 0
    for it, o in enumerate(out):
        log = env.log[it * T:(it + 1) * T]
        m_tm = np.stack([m for m, _ in log])                          # [T, na, S]: the masks the environment gave, step by step
        a_tm = np.stack([a for _, a in log])                          # [T, na, H]
        want = m_tm.transpose(1, 0, 2).reshape(na * T, S)             # trajectory-major
        assert np.array_equal(o["actions"], a_tm.transpose(1, 0, 2).reshape(na * T, H))
        v3 = M.head_valid(m_tm.reshape(T * na, S), BINS)
        assert np.take_along_axis(v3, a_tm.reshape(T * na, H)[..., None], -1).all(), ("an invalid action reached step()", it)
        assert np.array_equal(o["buf"], want), it
        assert all(np.isfinite(v) for v in o["report"].values() if isinstance(v, float)), o["report"]
    assert not want.all() and 0.2 < want.mean() < 0.9
    # an all-valid mask: the unmasked run bit for bit, parameters and report
    valid, _, _, _ = run_learner(AllValidEnv, iters=2)
    plain, penv, _, _ = run_learner(E.NvecVectorEnv, iters=2)
    assert plain[0]["buf"] is None and valid[0]["buf"] is not None and valid[0]["buf"].all()
    for a, b in zip(valid, plain):
        assert np.array_equal(a["actions"], b["actions"]) and torch.equal(a["flat"], b["flat"])
        same_report(a["report"], b["report"], "all-valid is off")
    assert not np.array_equal(plain[0]["actions"], out[0]["actions"])
    with pytest.raises(ValueError, match=r"5.*25|25.*5"):
        run_learner(WrongWidthEnv, iters=1)
