"""The general multi-discrete head on the GPU: rlppo_multidiscrete_act_nvec and rlppo_ppo_minibatch with md_nvec, against float64
restated in tests/multidiscrete_nvec_yardstick.py (there is no reference fixture for other bins: the reference's are literals), and
against the reference's own fixtures where the bins are the reference's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets  # noqa: E402
import fp64_gate  # noqa: E402
import multidiscrete_nvec_yardstick as Y  # noqa: E402
from hip_pass import L, Net, P, check, dev, run_pass, stream, triple  # noqa: E402,F401

# ------------------------------------------------------------------------------------------------ 1. sampling
# (bins, rows, observation width, hidden layers, seed).  The seeds were picked on the CPU, from the float64 reference alone, so that
# the inputs hold at most 2 near-ties (check_sampled asserts that first).
NVEC = dict(head="nvec", entry="nvec", dz=True)   # hip_pass.run_pass: rlppo_ppo_minibatch_nvec, the output gradient returned
SAMPLING_CASES = {
    "one_head_of_5": ((5,), 601, 20, (64, 64), 1),
    "one_bin_head": ((1, 4), 577, 33, (64, 64), 1),
    "ragged_5_heads": ((2, 7, 3, 11, 2), 613, 107, (64, 64), 1),
    "S_past_64": ((33, 2, 31), 599, 64, (64, 64), 1),
    "17_heads": ((4,) * 17, 607, 45, (128, 128), 12),
    "H_at_cap": ((2,) * 64, 593, 107, (128, 128), 1),
    "S_at_cap": ((64,) * 8, 589, 72, (64, 64), 1),
    "reference_bins": (Y.REFERENCE_BINS, 611, 107, (64, 64), 1),
}


def sampling_inputs(name):
    bins, n, d, hidden, seed = SAMPLING_CASES[name]
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    pol = nets.init_mlp(d, hidden, sum(bins))
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    q = nets.draw_exp_noise(n * len(bins), max(bins))
    return bins, pol, obs, q


def act_nvec(L, net, bins, rows, n, q, opts=None):
    act = torch.full((n, len(bins)), -7, dtype=torch.int64, device="cuda")
    logp = torch.empty(n, device="cuda")
    w = net.ws(n)
    qd = dev(q)
    c6 = L.rlppo_dbg_counter(6)
    check(L, L.rlppo_multidiscrete_act_nvec(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, n, P(qd), P(act), P(logp), P(w),
                                            w.numel(), opts, Y.nvec_array(bins), len(bins)))
    torch.cuda.synchronize()
    assert L.rlppo_dbg_counter(6) == c6 + 1   # the general kernel ran
    return act.cpu().numpy(), logp.cpu().numpy()


@pytest.mark.parametrize("name", list(SAMPLING_CASES))
def test_act_nvec_against_float64(L, golden, name):
    bins, pol, obs, q = sampling_inputs(name)
    net = Net(L, pol)
    n = obs.shape[0]
    act, logp = act_nvec(L, net, bins, net.pad(obs), n, q)
    Y.check_sampled(act, logp, Y.logits64(pol, obs), bins, q.numpy())
    if name == "reference_bins":
        # ... and the general kernel on the reference's own fixture, at the tolerances test_g9_gaussian_and_multidiscrete_act applies
        # to the fixed kernel
        g = golden("g9_multidiscrete")
        net = Net(L, nets.params_from_state(g, "p."))
        act, logp = act_nvec(L, net, bins, net.pad(g["obs"]), 72, torch.as_tensor(g["q"]))
        assert np.array_equal(act, g["act"])
        np.testing.assert_allclose(logp, g["logp"], rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ 2. the update
def update_case(bins, seed, n, d=107, hidden=(128, 128), noise=0.2, saturate=False):
    """Policy + critic and an n-row buffer whose actions / old log-probabilities the float64 yardstick drew from the policy itself
    (ratios exp(+-noise randn): both clip edges crossed).  saturate: logits scaled to +-30; a third of the rows carry uniformly drawn
    actions with old log-probabilities 0.5 off either way (tests/test_gpu_heads.py::test_multidiscrete_saturated_logits)."""
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    H, S = len(bins), sum(bins)
    pol, val = nets.init_mlp(d, hidden, S), nets.init_mlp(d, hidden, 1)
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    if saturate:
        with torch.no_grad():
            s = 30.0 / nets.mlp(pol, obs).abs().max().item()
        pol = pol[:-1] + [(pol[-1][0] * s, pol[-1][1] * s)]
    z = Y.logits64(pol, obs)
    act, logp, _, _ = Y.sample64(z, bins, nets.draw_exp_noise(n * H, max(bins)).numpy())
    off = noise * rs.randn(n)
    if saturate:
        third = n // 3
        act[:third] = (rs.rand(third, H) * np.asarray(bins)).astype(np.int64)
        ls = Y.head_log_softmax64(z, bins)
        logp = sum(ls[h][np.arange(n), act[:, h]] for h in range(H))
        off[:third] = np.where(rs.rand(third) < 0.5, -0.5, 0.5)
    old = (logp + off).astype(np.float32)
    tgt, adv = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    return pol, val, obs, act.astype(np.float32), old, tgt, adv, rs, logp


def gate_rows(L, pol, val, obs, acts, old, tgt, adv, idx, mb_ratio, got, label):
    return fp64_gate.gate(L, "multidiscrete", pol, val, obs[idx], acts[idx], old[idx], adv[idx], tgt[idx], 0.2, 0.005, mb_ratio, got,
                          label=label)


UPDATE_CASES = {
    "ragged_1500_of_5000": ((2, 7, 3, 11, 2), 5000, 1500, False),
    "17_heads": ((4,) * 17, 1800, 1300, False),
    "saturated_2999": ((33, 2, 31), 3500, 2999, True),
    "one_bin_head": ((1, 4), 1400, 1100, False),
}


@pytest.mark.parametrize("name", list(UPDATE_CASES))
def test_minibatch_nvec_against_float64(L, monkeypatch, name):
    """rlppo_ppo_minibatch with md_nvec through tests/fp64_gate.gate, unmodified, under the patched oracle: error against float64
    <= max(1e-5, 1.5 x the float32 torch leg's on the same rows), statistics at 1e-5; columns >= S of the output gradient exactly 0."""
    bins, n, mb, saturate = UPDATE_CASES[name]
    Y.patch_oracle(monkeypatch, bins)
    pol, val, obs, acts, old, tgt, adv, rs, logp = update_case(bins, 50 + len(bins), n, saturate=saturate)
    if name == "ragged_1500_of_5000":
        idx = rs.randint(0, n, mb)   # drawn with repeats
        idx[:3] = [n - 1, 0, n - 1]
    else:
        idx = rs.permutation(n)[:mb]
    if saturate:
        assert 25 < np.abs(Y.logits64(pol, obs)).max() <= 30.001
        for h, b in enumerate(bins):
            assert set(np.unique(acts[idx, h]).astype(int)) == set(range(b)), h   # every bin of every head occurs
        assert logp[idx].min() < -50
    ratio = np.exp(logp[idx] - old[idx])
    assert (ratio < 0.8).sum() > 10 and (ratio > 1.2).sum() > 10
    c6 = L.rlppo_dbg_counter(6)
    gp, gv, st, dz = triple(run_pass(L, pol, val, obs, acts, old, tgt, adv, idx, bins=bins, clip=0.2, ent=0.005, mb_ratio=0.5, **NVEC))
    assert L.rlppo_dbg_counter(6) == c6 + 1
    Y.check_output_gradient(dz, gp, sum(bins))
    if 1 in bins:   # a head of one bin: zero gradient in its column
        s = int(np.cumsum((0,) + tuple(bins))[bins.index(1)])
        assert (dz[:, s] == 0).all()
    gate_rows(L, pol, val, obs, acts, old, tgt, adv, idx, 0.5, (gp, gv, st), f"multi-discrete nvec {name}, {mb} rows")


def test_general_kernel_on_the_reference_bins(L, golden, monkeypatch):
    """The general loss kernel forced onto the reference's bins: the G9 minibatch through the float64 gate next to the fixed kernel's
    result, and the reference's learn() fixture g9_learn_multidiscrete at the tolerances of the existing test (which runs here
    unmodified, on a learner whose policy takes the general kernels)."""
    g = golden("g9_multidiscrete")
    pol, val = nets.params_from_state(g, "p."), nets.params_from_state(g, "v.")
    n = g["obs"].shape[0]
    acts, idx = g["act"].astype(np.float32), np.arange(n)
    args = (L, pol, val, g["obs"], acts, g["old_logp"], g["targets"], g["adv"], idx)
    kw = dict(NVEC, bins=Y.REFERENCE_BINS, clip=0.2, ent=0.005, mb_ratio=0.5)
    c6 = L.rlppo_dbg_counter(6)
    fixed = triple(run_pass(*args, general=False, **kw))
    assert L.rlppo_dbg_counter(6) == c6
    general = triple(run_pass(*args, **kw))
    assert L.rlppo_dbg_counter(6) == c6 + 1
    Y.check_output_gradient(general[3], general[0], 21)
    fp64_gate.gate(L, "multidiscrete", pol, val, g["obs"], acts, g["old_logp"], g["adv"], g["targets"], 0.2, 0.005, 0.5, general[:3],
                   label="G9 multidiscrete, general kernel")
    fp64_gate.gate(L, "multidiscrete", pol, val, g["obs"], acts, g["old_logp"], g["adv"], g["targets"], 0.2, 0.005, 0.5, fixed[:3],
                   label="G9 multidiscrete, fixed kernel (md_nvec NULL)")

    import test_gpu_learner as T
    plain = T.make_learner

    def forced(cfg):
        learner = plain(cfg)
        learner.policy._force_general = True
        return learner
    monkeypatch.setattr(T, "make_learner", forced)
    c6 = L.rlppo_dbg_counter(6)
    T.test_learn_matches_reference_fixture(golden, "g9_learn_multidiscrete")
    assert L.rlppo_dbg_counter(6) > c6


# ------------------------------------------------------------------------------------------------ 3. launch forms
def test_launch_forms_and_ring_for_nvec(L, monkeypatch):
    """Bins (2, 7, 3, 11, 2) through the forms tests/test_gpu_heads.py::test_launch_forms_for_every_head sets (knobs 26, 29, 32, 33):
    fused / separate gather / two chains / stacked pairs give bit-identical gradients (256 x 3 nets: the paired pass applies); a
    ring-rotated buffer gives the plain buffer's gradients."""
    bins = (2, 7, 3, 11, 2)
    n, base = 5000, 3777
    pol, val, obs, acts, old, tgt, adv, rs, _ = update_case(bins, 77, n, hidden=(256, 256, 256))
    idx = rs.randint(0, n, 1500)
    idx[:4] = [n - base - 1, n - base, 0, n - 1]
    forms = dict(fused=(2, 2, 0, 1), separate_gather=(0, 2, 0, 1), two_chains=(2, 0, 0, 1), stacked_pairs=(2, 2, 0, 0))
    runs, paired = {}, {}
    for key, (k26, k29, k32, k33) in forms.items():
        for knob, v in ((26, k26), (29, k29), (32, k32), (33, k33)):
            check(L, L.rlppo_dbg_set(knob, v))
        try:
            c3 = L.rlppo_dbg_counter(3)
            runs[key] = triple(run_pass(L, pol, val, obs, acts, old, tgt, adv, idx, bins=bins, clip=0.2, ent=0.005, mb_ratio=0.25, **NVEC))
            paired[key] = L.rlppo_dbg_counter(3) - c3
            if key == "fused":
                runs["ring"] = triple(run_pass(L, pol, val, obs, acts, old, tgt, adv, idx, bins=bins, clip=0.2, ent=0.005, mb_ratio=0.25, ring=base, **NVEC))
        finally:
            for knob in (26, 29, 32, 33):
                check(L, L.rlppo_dbg_set(knob, 1))
    assert paired["fused"] == 1 and paired["two_chains"] == 0 and paired["stacked_pairs"] == 1
    gp0, gv0, st0, _ = runs["fused"]
    for key, (gp, gv, st, _) in runs.items():
        for (x, y), (u, v) in zip(gp0 + gv0, gp + gv):
            assert torch.equal(x, u) and torch.equal(y, v), key
        np.testing.assert_allclose(st0, st, rtol=1e-12, atol=0, err_msg=key)
    Y.patch_oracle(monkeypatch, bins)
    gate_rows(L, pol, val, obs, acts, old, tgt, adv, idx, 0.25, runs["fused"][:3], "multi-discrete nvec, launch forms, ragged 1500 rows")
