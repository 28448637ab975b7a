"""tests/optim_yardstick.py is neither too tight nor too loose -- shown on the CPU, before anything is held to it on a GPU.
Not too tight: torch's CPU float32 clip + Adam stays within every derived bound on every row of the table, element for element.
Not too loose: six wrong restatements of the step each exceed a bound by at least 10 x on some row.  Plus adv_stats64 against a
direct long-double mean / deviation and packed_image against the length the library reports."""
import math

import numpy as np
import pytest

import optim_yardstick as Y

KEYS = ("g", "m", "v", "p")


def case_args(case):
    _, n, step, kind, max_norm, (b1, b2) = case
    p, g, m, v = Y.adam_state(case)
    return (p, g, m, v), (max_norm, Y.LR, b1, b2, Y.EPS, step)


@pytest.fixture(scope="module")
def table():
    """Per row: the state, float64 truth and bounds, computed once and left unchanged."""
    out = {}
    for case in Y.ADAM_CASES:
        state, hyper = case_args(case)
        norm2 = Y.exact_sum_squares(state[1])
        truth, bound = Y.clip_adam64(*state, norm2, *hyper)
        out[case[0]] = (case, state, hyper, norm2, truth, bound)
    return out


def test_table_holds_small_steps_and_small_gradient_elements():
    steps = {c[2] for c in Y.ADAM_CASES}
    assert {1, 2, 7, 1000, 100000} <= steps
    assert {c[1] for c in Y.ADAM_CASES} >= {1, 255, 256, 257, 262144, 262145, 1100003}
    assert {c[4] for c in Y.ADAM_CASES} == {0.5, 1e-3, 1e9} and len({c[5] for c in Y.ADAM_CASES}) == 2
    assert {c[3] for c in Y.ADAM_CASES} == {"wide", "small", "big"}
    # small-gradient elements at small step counts: the elements on which eps and the bias corrections decide the update
    assert any(c[2] <= 2 and c[3] == "wide" and (np.abs(Y.adam_state(c)[1]) < 1e-7).any() for c in Y.ADAM_CASES)
    for c in Y.ADAM_CASES:
        p, g, m, v = Y.adam_state(c)
        assert all(x.dtype == np.float32 and x.shape == (c[1],) for x in (p, g, m, v))
        assert ((m == 0).all() and (v == 0).all()) == (c[2] == 1)


@pytest.mark.parametrize("case", Y.ADAM_CASES, ids=[c[0] for c in Y.ADAM_CASES])
def test_cpu_float32_adam_is_within_every_bound(table, case):
    _, state, hyper, exact, _, _ = table[case[0]]
    got, norm2 = Y.torch_adam32(*state, *hyper)
    # the oracle's own float32 norm: a float32 sum of n squares, (n - 1) u relative at the worst
    assert abs(norm2 - exact) <= case[1] * Y.U32 * exact
    truth, bound = Y.clip_adam64(*state, norm2, *hyper)
    worst = {k: Y.worst(got[k], truth[k], bound[k]) for k in KEYS}
    print(f"[fp64 gate] clip+Adam {case[0]}: CPU fp32 oracle max(err/bound) " + "  ".join(f"{k}' {worst[k]:.3f}" for k in KEYS))
    for k in KEYS:
        assert np.isfinite(truth[k]).all() and np.isfinite(bound[k]).all()
        assert (np.abs(got[k].astype(np.float64) - truth[k]) <= bound[k]).all(), (k, worst[k])


def _excess(table, mutant, rows=None):
    """max over the rows (and g', m', v', p') of |mutant - truth| / bound."""
    worst = {}
    for name, (case, state, hyper, norm2, truth, bound) in table.items():
        if rows is not None and name not in rows:
            continue
        wrong, _ = Y.clip_adam64(*state, norm2, *hyper, mutant=mutant)
        worst[name] = max(Y.worst(wrong[k], truth[k], bound[k]) for k in KEYS)
    return worst


@pytest.mark.parametrize("mutant", Y.MUTANTS)
def test_every_mutant_exceeds_a_bound_tenfold(table, mutant):
    worst = _excess(table, mutant)
    best = max(worst, key=worst.get)
    print(f"[fp64 gate] mutant {mutant}: max(err/bound) {worst[best]:.3g} on {best}")
    assert worst[best] >= 10.0, worst


def test_eps_mutants_are_invisible_at_step_100000():
    """Why the table needs its small steps and small gradients: at step 100000 bc2 == 1 in double, and the row's second moments
    (~900) dwarf eps -- both eps mutants stay inside the bound there.  Do not 'simplify' the table down to such rows."""
    rows = [c for c in Y.ADAM_CASES if c[2] == 100000]
    assert rows and 1.0 - 0.999 ** 100000 == 1.0
    for case in rows:
        state, hyper = case_args(case)
        norm2 = Y.exact_sum_squares(state[1])
        truth, bound = Y.clip_adam64(*state, norm2, *hyper)
        for mutant in Y.MUTANTS[:2]:
            wrong, _ = Y.clip_adam64(*state, norm2, *hyper, mutant=mutant)
            assert max(Y.worst(wrong[k], truth[k], bound[k]) for k in KEYS) <= 1.0, mutant


def test_lr_device_is_the_same_rate():
    state, hyper = case_args(Y.ADAM_CASES[1])
    norm2 = Y.exact_sum_squares(state[1])
    a, _ = Y.clip_adam64(*state, norm2, *hyper)
    b, _ = Y.clip_adam64(*state, norm2, hyper[0], 123.0, *hyper[2:], lr_device=Y.LR)
    assert all(np.array_equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize("n,kind,idx_kind,ring", Y.ADV_CASES, ids=[f"n{c[0]}_{c[1]}_{c[2]}_{'ring' if c[3] else 'plain'}" for c in Y.ADV_CASES])
def test_adv_stats64_against_long_double(n, kind, idx_kind, ring):
    adv, idx, base, cap = Y.adv_case(n, kind, idx_kind, ring)
    mean, scale, b_mean, b_scale = Y.adv_stats64(adv, idx, base, cap)
    rows = (idx + base) % cap if cap else idx
    if ring:
        assert rows.min() < idx.min() + base and (idx + base).max() >= cap   # the rows do wrap
    if n == 1:
        assert (mean, scale, b_mean, b_scale) == (0.0, 1.0, 0.0, 0.0)
        return
    a = adv[rows].astype(np.longdouble)
    want_mean = float(np.mean(a))
    want_scale = float(1.0 / (np.std(a, ddof=1) + np.longdouble(1e-8)))
    # float64 against a long-double evaluation of the textbook formulas: far inside what a float32 result can resolve
    assert abs(mean - want_mean) <= 1e-12 * max(abs(want_mean), float(np.abs(a - a[0]).max()))
    assert abs(scale - want_scale) <= 1e-9 * want_scale
    assert b_mean >= 0.5 * 2.0 ** -149 and b_scale >= 0.0 and math.isfinite(b_mean) and math.isfinite(b_scale)
    if kind == "constant":
        assert mean == float(adv[0]) and scale == 1e8


def test_kl_batch64():
    kl, bound = Y.kl_batch64([(0.5, [1.0, 2.0, 3.0]), (0.25, [4.0])])
    assert kl == 4.0 and bound == (3 + 2) * 2.0 ** -53 * 4.0


NETS = [[107, 256, 256, 90], [107, 256, 256, 1], [231, 512, 512, 512, 512, 16], [13, 1], [7, 33, 5], [300, 130, 257, 64, 1500]]


@pytest.mark.parametrize("dims", NETS, ids=["x".join(map(str, d)) for d in NETS])
def test_packed_image_length_and_placement(dims):
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    dc, nl = N.dims_array(dims), len(dims) - 1
    n_flat = int(L.rlppo_flat_floats(dc, nl))
    flat = np.arange(1, n_flat + 1, dtype=np.float32)
    img = Y.packed_image(dims, flat, L)
    assert img.size == int(L.rlppo_packed_floats(dc, nl)) and img.dtype == np.float32
    layers, total, nf = Y.packed_layout(dims, L)
    assert nf == n_flat and total == img.size
    # every parameter lands twice (W and W^T) or once (b), everything else is zero
    assert np.count_nonzero(img) == sum(2 * i * o + o for i, o, *_ in layers)
    i, o, pin, pout, off_w, off_wt, off_b, fw, fb = layers[-1]
    assert img[off_w + (o - 1) * pin + (i - 1)] == flat[fw + o * i - 1] == img[off_wt + (i - 1) * pout + (o - 1)]
    assert img[off_b + o - 1] == flat[fb + o - 1] == flat[-1]
