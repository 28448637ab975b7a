"""tests/gemm_yardstick.py is neither too tight nor too loose -- shown on the CPU, before any kernel is held to it on a GPU
(tests/test_gpu_products.py).  Not too tight: torch's CPU float32 products, the bf16 forms and a float32 restatement of the split-bf16
product stay within the allowance on EVERY element, for every maker and shape family the GPU file uses.  Not too loose: six wrong
restatements, each confined to the smallest-scale output row, exceed the allowance by at least MUTANT_FACTOR on the `scaled`
operands while the suite's old max-norm gate (< 2e-6) does not see them, and every one that changes a term breaks the bit equality on
`integers`.  Plus the guard bands and the integer makers' range asserts."""
import pytest
import torch

import gemm_yardstick as Y

OLD_GATE = 2e-6        # test_gemm_nt / test_gemm_tn: max|got - want| / max|want| < 2e-6
MUTANT_FACTOR = 5.0    # every mutant exceeds the allowance at least this much (the weakest, a row rounded to bf16 at K = 512, measures 6.07)

NT_SHAPES = [(1, 32, 16), (17, 96, 144), (130, 96, 48), (257, 128, 16), (257, 32, 64), (129, 256, 256), (1025, 64, 144), (513, 256, 96), (300, 256, 512)]
TN_SHAPES = [(1, 21, 32), (33, 90, 107), (65, 256, 256), (2081, 300, 130), (2081, 1, 64), (513, 128, 256)]   # (M, out, in)


def _nt_sets(M, N, K, epi, bf16=False):
    s = Y.scaled_nt(M, N, K, tanh=epi == 2, bf16=bf16)
    return [("scaled", s), ("cancelling", Y.cancelling_nt(s)), ("integers", Y.integers_nt(M, N, K, bf16=bf16))]


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_cpu_float32_nt_is_within_the_allowance_on_every_element(M, N, K):
    top = 0.0
    for epi in (0, 1, 2, 3):
        for name, o in _nt_sets(M, N, K, epi):
            want, pre, S = Y.nt_truth(o["A"], o["B"], o["bias"], epi, o["mask"], o["zero"])
            got = Y.nt_float32(o["A"], o["B"], o["bias"], epi, o["mask"])
            w = Y.worst(got, want, Y.nt_allow(S, K, want, tanh=epi == 2))
            top = max(top, w)
            assert w <= 1.0, (name, epi, w)
            if name == "integers" and epi != 2:
                assert torch.equal(got.double(), want), (epi, "integers are exact")
            if name == "cancelling" and epi != 2:
                assert (want[::3, ::2] == 0).all() and (S[::3, ::2] > 0).all()    # exact zeros the allowance still covers
    print(f"[gemm yardstick] NT {M}x{N}x{K}: CPU float32 max(err/allow) {top:.3f}")


@pytest.mark.parametrize("M,N,K", [(129, 128, 64), (257, 256, 128), (513, 32, 64)])
def test_cpu_bf16_forms_are_within_the_allowance(M, N, K):
    for name, o in _nt_sets(M, N, K, 1, bf16=True):
        want, pre, S = Y.nt_truth(o["A"], o["B"], o["bias"], 1, zero=o["zero"])
        got32 = Y.nt_float32(o["A"], o["B"], o["bias"], 1)
        assert Y.worst(got32, want, Y.nt_allow(S, K)) <= 1.0
        got = got32.bfloat16().float()                      # the hidden form's output rounding
        w = Y.worst(got, want, Y.nt_allow(S, K, want, bf16_out=True))   # against the UNROUNDED truth: one rounding, half an ulp
        assert w <= 1.0, (name, w)
        if name == "integers":
            assert torch.equal(got.double(), Y.bf16_round(want))


def test_three_pieces_hold_a_float32_exactly():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(200000, generator=g) * 2.0 ** torch.randint(-12, 13, (200000,), generator=g)
    h, m, l = Y.split3(x)
    assert torch.equal(h.double() + m.double() + l.double(), x.double())
    assert ((m.abs() <= 2.0 ** -8 * x.abs()) & (l.abs() <= 2.0 ** -17 * x.abs())).all()
    i = torch.randint(-256, 257, (1000,), generator=g).float()
    h, m, l = Y.split3(i)
    assert torch.equal(h, i) and not m.any() and not l.any()


@pytest.mark.parametrize("M,N,K", [(1, 256, 32), (129, 256, 96), (513, 256, 32), (130, 256, 256)])
def test_cpu_x3_restatement_is_within_its_derived_allowance(M, N, K):
    for mode in (0, 1):
        for name, o in _nt_sets(M, N, K, 1):
            want, pre, S = Y.nt_truth(o["A"], o["B"], o["bias"], 1 if mode == 0 else 3, o["mask"], o["zero"])
            got = Y.x3_float32(o["A"], o["B"], o["bias"], mode, o["mask"])
            w = Y.worst(got, want, Y.x3_allow(S, K))
            assert w <= 1.0, (name, mode, w)
            if name == "integers":
                assert torch.equal(got.double(), want)
    assert Y.x3_const(32) == 36 and Y.x3_const(96) == 102 and Y.x3_const(256) == 267       # below K + 8 up to K = 128, above from 160


@pytest.mark.parametrize("M,out,in_", TN_SHAPES)
def test_cpu_float32_tn_is_within_the_allowance_on_every_element(M, out, in_):
    s = Y.scaled_tn(M, out, in_)
    sets = [("scaled", s), ("cancelling", Y.cancelling_tn(s)), ("integers", Y.integers_tn(M, out, in_)),
            ("gathered", Y.scaled_tn(M, out, in_, seed=1, src_rows=3 * M + 7)), ("bf16", Y.scaled_tn(M, out, in_, seed=2, bf16=True))]
    top = 0.0
    for name, o in sets:
        wW, wb, SW, Sb = Y.tn_truth(o["dY"], o["X"], o["dW0"], o["db0"], o["rowtab"], o["zero"])
        gW, gb = Y.tn_float32(o["dY"], o["X"], o["dW0"], o["db0"], o["rowtab"])
        w = max(Y.worst(gW, wW, Y.tn_allow(SW, M, o["dW0"])), Y.worst(gb, wb, Y.tn_allow(Sb, M, o["db0"])))
        top = max(top, w)
        assert w <= 1.0, (name, w)
        if name == "integers":
            assert torch.equal(gW.double(), wW) and torch.equal(gb.double(), wb)
        if name == "cancelling":
            assert torch.equal(wW[::2, ::3], o["dW0"][::2, ::3].double()) and torch.equal(wb[::2], o["db0"][::2].double())
            assert M < 2 or (SW[::2, ::3] > 0).all()
        if name == "gathered":
            t = o["rowtab"]
            assert t[0] == 3 * M + 6 and (M == 1 or t[-1] == 0) and (M <= 3 or t[1] == t[2])
    print(f"[gemm yardstick] TN {M} rows, {out}x{in_}: CPU float32 max(err/allow) {top:.3f}")


# ------------------------------------------------------------------------------------------------ wrong restatements
def _nt_mutants(o, small_r, small_cols):
    """name -> (wrong float64 C (epilogue 0), changes a term).  Every mutant touches ONLY row small_r of C (the smallest-scale row
    of A); the bias and the swap touch only the smallest-scale columns of that row (small_cols: the columns by scale, ascending)."""
    A, B, bias = o["A"].double(), o["B"].double(), o["bias"].double()
    M, K = A.shape
    good = A @ B.T + bias
    r, c0 = small_r, small_cols[0]
    c1 = next(c for c in small_cols[1:] if good[r, c] != good[r, c0])   # (integers: two columns can hold the same value; a swap of those is no error)

    def with_row(row):
        C = good.clone()
        C[r] = row
        return C

    late = torch.cat([A[r, 4:], torch.zeros(4, dtype=torch.float64)])   # a stride off by 4 floats: the row read 4 floats late, its end from (zero) padding
    swapped = good[r].clone()
    swapped[c0], swapped[c1] = good[r, c1], good[r, c0]
    nobias = good[r].clone()
    nobias[c0] -= bias[c0]
    return {
        "dropped_last_k": (with_row(A[r, :K - 1] @ B[:, :K - 1].T + bias), True),
        "row_rounded_to_bf16": (with_row(o["A"][r].bfloat16().double() @ B.T + bias), False),   # small integers ARE bf16 numbers
        "missing_bias": (with_row(nobias), True),
        "column_pair_swapped": (with_row(swapped), True),
        "stride_off_by_4_floats": (with_row(late @ B.T + bias), True),
    }


def _tn_mutant_dropped_last_row(o, small_n):
    """dW whose row small_n (the smallest-scale column of dY) lacks the last row of the contraction."""
    dY, X = o["dY"].double(), o["X"].double()
    good = o["dW0"].double() + dY.T @ X
    wrong = good.clone()
    wrong[small_n] = o["dW0"][small_n].double() + dY[:-1, small_n] @ X[:-1]
    return wrong


@pytest.mark.parametrize("M,N,K", [(130, 96, 48), (257, 128, 16), (300, 256, 512)])
def test_wrong_restatements_exceed_the_allowance_where_the_max_norm_is_blind(M, N, K):
    o = Y.scaled_nt(M, N, K)
    r = int(o["ea"].argmin())
    cols = [int(c) for c in o["eb"].argsort()]                  # by scale, the smallest first
    assert o["ea"][r] == -12 and o["eb"][cols[0]] == -12
    want, pre, S = Y.nt_truth(o["A"], o["B"], o["bias"], 0)
    allow = Y.nt_allow(S, K)
    i = Y.integers_nt(M, N, K)
    iwant, _, _ = Y.nt_truth(i["A"], i["B"], i["bias"], 0)
    for (name, (wrong, changes)), (_, (iwrong, _)) in zip(_nt_mutants(o, r, cols).items(), _nt_mutants(i, r, cols).items()):
        excess, old = Y.worst(wrong, want, allow), Y.maxnorm(wrong, want)
        print(f"[gemm yardstick] mutant {name} at {M}x{N}x{K}: err/allow {excess:.3g}, old max-norm gate {old:.2e}")
        assert excess >= MUTANT_FACTOR, (name, excess)
        assert old < OLD_GATE, (name, old)                      # the old gate passes it
        # the integer equality does not -- unless the mutant only loses precision (integers have none to lose: why BOTH checks run)
        assert torch.equal(iwrong, iwant) == (not changes), name


@pytest.mark.parametrize("M,out,in_", [(33, 90, 107), (65, 256, 256), (2081, 300, 130)])
def test_dropped_contraction_row_exceeds_the_tn_allowance(M, out, in_):
    """One missing term of M weighs ~1 / M of sum|t| against an allowance of (M + 8) u sum|t|: the excess falls like 1 / (M^2 u) and is
    gone near M = 4096 -- no worst-case rounding bound can see ONE dropped row of thousands.  The integer equality sees it at any M."""
    o = Y.scaled_tn(M, out, in_)
    n = int(o["ey"].argmin())
    wW, _, SW, _ = Y.tn_truth(o["dY"], o["X"], o["dW0"], o["db0"])
    wrong = _tn_mutant_dropped_last_row(o, n)
    excess, old = Y.worst(wrong, wW, Y.tn_allow(SW, M, o["dW0"])), Y.maxnorm(wrong, wW)
    print(f"[gemm yardstick] mutant dropped_last_row at {M} rows {out}x{in_}: err/allow {excess:.3g}, old max-norm gate {old:.2e}")
    assert (excess >= MUTANT_FACTOR or M > 100) and excess > 1.0 and old < OLD_GATE
    i = Y.integers_tn(M, out, in_)
    iW, _, _, _ = Y.tn_truth(i["dY"], i["X"], i["dW0"], i["db0"])
    assert not torch.equal(_tn_mutant_dropped_last_row(i, n), iW)


# ------------------------------------------------------------------------------------------------ guard bands, range asserts
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_guard_bands_report_a_write_one_element_past_each_edge(dtype):
    rows, cols, ld, band = 5, 12, 16, 2

    def fresh(role="out"):
        b = Y.Guarded(rows, cols, dtype, ld=ld, band=band, role=role, values=torch.ones(rows, cols), name="C")
        assert b.violations() == [] and b.m.data_ptr() == b.raw.data_ptr() + (band * ld) * b.raw.element_size()
        return b

    flat_of = lambda b: b.raw.view(dtype).view(-1)
    first, last = band * ld, (band + rows - 1) * ld + cols - 1
    for where in (first - 1, first + cols, last + 1, (band + rows) * ld, 0, flat_of(fresh()).numel() - 1):
        b = fresh()
        flat_of(b)[where] = 3.0
        assert len(b.violations()) == 1 and "sentinel" in b.violations()[0], where
    for where in (first, first + cols - 1, last):        # the matrix itself is the caller's to write
        b = fresh()
        flat_of(b)[where] = 3.0
        assert b.violations() == []
    b = Y.Guarded(rows, cols, dtype, ld=ld, band=band, role="out", name="C")     # an output nobody wrote
    assert "NaN left" in b.violations()[0]
    b = fresh("in")
    b.m[1, 1] = 2.0
    assert "input changed" in b.violations()[0]
    v = Y.vec(10, torch.uint8, role="scratch", name="ws")
    assert v.violations() == [] and (v.m == 0xFF).all()
    v.raw.view(-1)[v.raw.shape[1] + 10] = 0
    assert "sentinel" in v.violations()[0]
    with pytest.raises(AssertionError, match="sentinel"):
        Y.assert_intact(fresh(), v, None)


def test_integer_makers_refuse_ranges_that_could_round():
    Y.integers_nt(4, 32, 512, r=8)                  # 64 . 512 + 64 = 32,832
    Y.integers_tn(65536, 4, 4, r=3)                 # 9 . 65,536 + 64
    Y.integers_tn(65536, 4, 4, r=15)                # 225 . 65,536 + 64 = 14,745,664 < 2^24
    with pytest.raises(AssertionError):
        Y.integers_tn(65536, 4, 4, r=16)            # 256 . 65,536 = 2^24
    with pytest.raises(AssertionError):
        Y.integers_nt(4, 32, 16, r=257)             # 257 is no bf16 number
    with pytest.raises(AssertionError):
        Y.integers_nt(4, 32, 512, r=8, r_bias=2 ** 24)
    assert Y.int_range_ok(3, 3, 1864127, 64) and not Y.int_range_ok(3, 3, 1864128, 64)    # 9 n + 64 < 2^24
