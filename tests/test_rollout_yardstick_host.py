"""tests/rollout_yardstick.py on the CPU: its rules are reachable (a float32 restatement of every head, and the project's float32
oracle, stay inside every allowance on every maker), they separate right from wrong (every mutant breaks at least one check), and
the makers keep the undecided rows under the cap -- all before a GPU is asked anything."""
import numpy as np
import pytest
import torch

import rollout_yardstick as R
from oracle import nets

WIDTHS = (5, 90, 600, 2048)
SPANS = (1, 30, 100)
N = 263
MD_CASES = {"reference_bins": (3, 3, 3, 3, 3, 2, 2, 2), "S_past_64": (33, 2, 31), "H_at_cap": (2,) * 64, "one_bin_head": (1, 4)}


def discrete_cases():
    for A in WIDTHS:
        for span in SPANS:
            for masked in (False, True):
                yield A, span, masked


def case(A, span, masked):
    z, mask, rs = R.logit_case(N, A, span, seed=span, masked=masked)
    q = R.noise_case(z.astype(np.float64), mask, rs)
    T = R.discrete_truth(z, q, mask)
    return z, mask, q, T


def discrete_worst(out, T):
    act, logp, pc, p = out
    c = R.choice_check(act, T["score"], T["m"], T["valid"])
    return max(R.logp_worst(logp, act, T), R.probs_worst(pc, T, True), R.probs_worst(p, T, False), np.inf if len(c["bad"]) else 0.0)


@pytest.fixture(scope="module")
def cases():
    return {key: case(*key) for key in discrete_cases()}


def test_makers_hold_what_they_promise(cases):
    for (A, span, masked), (z, mask, q, T) in cases.items():
        und = R.assert_inputs(T, (A, span, masked))
        assert und <= R.UNDECIDED_CAP * N
        mx = z.astype(np.float64).max(1)
        assert np.abs(np.diff(mx)).max() > 60                                     # neighbouring maxima more than 60 apart
        spread = z.max(1) - z.min(1)
        assert spread[4::5].max() < 0.01 * span * 2.1 and spread.max() > 0.9 * span   # nearly uniform rows next to peaked ones
        chosen = T["p"][np.arange(N), T["score"].argmax(1)]
        if span >= 30 and A >= 90:
            assert (chosen < R.FLOOR / 2).any() and ((chosen > 2 * R.FLOOR) & (chosen < 1e-6)).any()   # both sides of the clamp are CHOSEN
            assert T["firm"].any()                                                # elements that must read 1e-11f bit for bit
        if A >= 4:
            tied = (T["score"][:, 1] == T["score"][:, A - 2]) & (T["score"].argmax(1) == 1)
            assert tied.any()                                                     # an exact tie that wins


def test_float32_restatement_stays_inside_every_allowance(cases):
    worst = {}
    for key, (z, mask, q, T) in cases.items():
        worst[key] = discrete_worst(R.discrete32(z, q, mask), T)
    for A in WIDTHS:
        print(f"[rollout yardstick] float32 restatement, A={A}: worst ratio per span {[max(worst[(A, s, m)] for m in (False, True)) for s in SPANS]}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutant", R.DISCRETE_MUTANTS)
def test_every_discrete_mutant_breaks_a_check(cases, mutant):
    worst = {key: discrete_worst(R.discrete32(z, q, mask, mutant=mutant, n_pad=(-z.shape[1]) % 32 or 32), T) for key, (z, mask, q, T) in cases.items()}
    best = max(worst, key=worst.get)
    print(f"[rollout yardstick] mutant {mutant}: worst ratio {worst[best]:.3g} on (A, span, masked) = {best}; cases failed "
          f"{sum(v > 1 for v in worst.values())} of {len(worst)}")
    assert worst[best] > 1.0, worst


def md_case(bins, masked, span=30, n=N):
    rs = np.random.RandomState(len(bins) * 13 + sum(bins))
    S, H, B = sum(bins), len(bins), max(bins)
    z = rs.randn(n, S)
    z *= span / np.abs(z).max()
    z = (z * R.row_scales(n)[:, None]).astype(np.float32)
    q = np.maximum(rs.exponential(1.0, (n * H, B)), 1e-6).astype(np.float32)
    mask = None
    if masked:
        from masked_multidiscrete_yardstick import rand_mask
        mask = rand_mask(rs, n, bins)
    return z, q, mask, R.md_truth(z, bins, q, mask)


@pytest.mark.parametrize("name", list(MD_CASES))
@pytest.mark.parametrize("masked", [False, True])
def test_multidiscrete_restatement_and_mutant(name, masked):
    bins = MD_CASES[name]
    z, q, mask, T = md_case(bins, masked)
    assert R.md_undecided(T) <= R.UNDECIDED_CAP * T["n"] * T["H"]
    for float_sum in (False, True):
        act, logp = R.md32(z, bins, q, mask, float_sum=float_sum)
        assert R.md_hold(f"float32 restatement {name} masked={masked} float_sum={float_sum}", act, logp, T) <= 1.0
    if len(set(bins)) > 1:   # (a padding slot exists only where the heads differ in width)
        act, logp = R.md32(z, bins, q, mask, mutant="nvec_padding_candidate")
        assert R.md_hold(f"mutant nvec_padding_candidate {name}", act, logp, T) > 1.0


def gauss_case(k, n=N):
    rs = np.random.RandomState(100 + k)
    y = np.tanh(rs.randn(n, 2 * k) * 1.5).astype(np.float32)
    y[:, k] = -1.0                                   # a saturated sd unit: sd == var_min
    if k > 1:
        y[:, k + 1] = 1.0
    eps = rs.randn(n, k).astype(np.float32)
    eps[: n // 4] *= 4.0
    return y, eps


@pytest.mark.parametrize("k", [1, 17, 33])
def test_gaussian_restatement_and_mutants(k):
    vm, vb = nets.var_map(0.1, 1.0)
    y, eps = gauss_case(k)
    T = R.gauss_truth(y, eps, vm, vb)
    assert (np.abs(T["act"]) == 1).sum() > 10        # the clamp is active
    act, logp = R.gauss32(y, eps, vm, vb)
    assert R.gauss_hold(f"float32 restatement k={k}", act, logp, T) <= 1.0
    for mutant in ("gauss_logp_unclamped", "gauss_no_var_b"):
        act, logp = R.gauss32(y, eps, vm, vb, mutant=mutant)
        assert R.gauss_hold(f"mutant {mutant} k={k}", act, logp, T) > 1.0
    # the project's float32 oracle, on the same tanh outputs
    yt = torch.as_tensor(y)
    oact, ologp = nets.gauss_sample(yt[:, :k], yt[:, k:] * vm + vb, torch.as_tensor(eps))
    assert R.gauss_hold(f"oracle/nets.py gauss_sample k={k}", oact.numpy(), ologp.numpy(), T) <= 1.0


@pytest.mark.parametrize("k", [1, 33])
def test_diag_gaussian_restatement(k):
    rs = np.random.RandomState(200 + k)
    mu = (rs.randn(N, k) * 3).astype(np.float32)
    ls = rs.uniform(-2.5, 0.7, k).astype(np.float32)
    eps = rs.randn(N, k).astype(np.float32)
    T = R.diag_truth(mu, ls, eps)
    act, logp = R.diag32(mu, ls, eps)
    assert R.diag_hold(f"float32 restatement k={k}", act, logp, T) <= 1.0
    assert R.diag_hold(f"log p of a neighbouring row k={k}", act, np.roll(logp, 1), T) > 1.0


def test_the_float32_oracle_passes_discrete_and_multidiscrete():
    """oracle/nets.py (torch float32) on peaked networks: tier (i) on its own logits, tier (ii) from the observations."""
    d = 107
    for A, hidden, span in ((90, (64, 64), 30), (513, (128, 96), 100)):
        obs, rs = R.obs_case(N, d, seed=A)
        pol = R.peaked_policy(d, hidden, A, span, obs, seed=A)
        with torch.no_grad():
            z = nets.mlp(pol, obs).numpy()
        z64, e_z = R.logit_bound(pol, obs, dup=True)
        assert 0.99 * span < np.abs(z64).max() < 1.01 * span + 1
        mask = R.rand_mask(rs, N, A)
        q = R.noise_case(z64, mask, rs)
        with torch.no_grad():
            p = torch.clamp(torch.softmax(torch.as_tensor(z).masked_fill(~torch.as_tensor(mask), float("-inf")), -1), min=nets.PROB_MIN, max=1)
            act, logp = nets.discrete_sample(torch.where(torch.as_tensor(mask), p, torch.zeros_like(p)), torch.as_tensor(q))
        T64 = R.discrete_truth(z64, q, mask)
        R.assert_inputs(T64, ("oracle", A))                                       # from float64 alone
        T = R.discrete_truth(z, q, mask)
        assert R.discrete_hold(f"oracle/nets.py tier (i) A={A} span={span}", act.numpy(), logp.numpy(), T, probs=np.where(mask, p.numpy(), 0)) <= 1.0
        extra = R.extra_at(R.tier2_extra(T64, e_z), act.numpy())
        w = R.logp_worst(logp.numpy(), act.numpy(), T64, extra)
        lw = float((np.abs(z - z64) / e_z).max())
        print(f"[rollout yardstick] oracle/nets.py tier (ii) A={A} span={span}: logits {lw:.3g}, log p {w:.3g}")
        assert w <= 1.0 and lw <= 1.0
    bins = nets.MD_BINS
    obs, rs = R.obs_case(N, d, seed=21)
    pol = R.peaked_policy(d, (64, 64), 21, 30, obs, seed=21, dup=False)
    q = nets.draw_exp_noise(N * 8, 3)
    with torch.no_grad():
        z = nets.mlp(pol, obs).numpy()
        act, logp = nets.md_sample(*nets.md_dist(pol, obs), q)
    T = R.md_truth(z, bins, q.numpy())
    assert R.md_undecided(T) <= R.UNDECIDED_CAP * N * 8
    assert R.md_hold("oracle/nets.py md_sample, reference bins", act.numpy(), logp.numpy(), T) <= 1.0
