"""Every matrix product of the library, kernel by kernel through the C ABI, held to tests/gemm_yardstick.py: per ELEMENT within the
derived float32 allowance of the float64 product of the same operand values on `scaled` + `cancelling` operands (outputs span ~48
binades, some are exactly 0), BIT-EQUAL to float64 on `integers` (no rounding anywhere: a dropped, doubled or mis-addressed term cannot
hide), and every operand and output inside a guarded buffer (leading dimensions larger than the widths, NaN sentinels around every
input, sentinels around every output, workspaces NaN-filled and guarded behind their stated size).  No element is excluded anywhere.
The shapes are the smallest that cross each tile, stage, split and kernel-selection edge; the large ones (32-bit offsets, several rounds)
stay with tests/test_gpu_kernels.py.  Each test prints its family's worst error / allowance ("What the matrix products are held to", holds the table)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_yardstick as Y  # noqa: E402
from hip_pass import L, P, check, dev, stream  # noqa: E402,F401
from test_gpu_kernels import b16_tiles  # noqa: E402,F401

G = Y.Guarded


def gin(t, ld_pad, dtype=None, name="", band=2):
    """An input matrix in a guarded CUDA buffer, leading dimension = width + ld_pad."""
    dtype = dtype or t.dtype
    return G(t.shape[0], t.shape[1], dtype, "cuda", ld=t.shape[1] + ld_pad, band=band, role="in", values=t, name=name)


def gout(rows, cols, ld_pad, dtype=torch.float32, values=None, name=""):
    return G(rows, cols, dtype, "cuda", ld=cols + ld_pad, role="out", values=values, name=name)


def gvec(t, name, role="in"):
    return Y.vec(t.numel(), t.dtype, "cuda", role=role, values=t, name=name)


def gbytes(n, name, role="scratch", values=None):
    """n bytes (a bitmask, a workspace) 16-byte aligned, NaN-filled (0xFF) inside, sentinels behind and before."""
    return Y.vec(n, torch.uint8, "cuda", pad=16 + (-n) % 16, role=role, values=values, name=name)


def forms(L):
    """Launches so far by kernel form (rlppo_dbg_counter 8 .. 13): few-row NT, tiled NT, bf16 256 x 256 tiles, bf16 persistent, x3 persistent,
    gemv dW through fixed-order partials."""
    return [int(L.rlppo_dbg_counter(k)) for k in range(8, 14)]


def ran(L, before):
    return [a - b for a, b in zip(forms(L), before)]


def report(family, worst):
    print(f"[products] {family}: worst err / allowance {worst:.3f}")


# ReLU bitmask layout (csrc/gemm_detail.hpp, relu_bits): 128 x 128 tile (row tile, column tile) = 256 64-bit words, word tid = wave * 64 +
# q * 16 + r16 holds rows 32 wave + 16 i + r16, columns 16 j + 4 q + e at bit (8 i + j) * 4 + e.
_SHIFT = ((8 * np.arange(2)[:, None, None] + np.arange(8)[None, :, None]) * 4 + np.arange(4)[None, None, :]).astype(np.uint64)


def decode_bits(raw_bytes, M, N):
    rt, ct = (M + 127) // 128, N // 128
    w = raw_bytes.cpu().numpy().view(np.uint64).reshape(rt, ct, 4, 4, 16)
    b = (w[..., None, None, None] >> _SHIFT) & np.uint64(1)                   # rt ct wave q r16 i j e
    return torch.from_numpy(b.transpose(0, 2, 5, 4, 1, 6, 3, 7).reshape(rt * 128, N)[:M].astype(bool))


def encode_bits(on):
    """The bitmask of a boolean M x N pattern; rows past M (the ragged last tile) are set: a kernel that let them through would show."""
    M, N = on.shape
    rt, ct = (M + 127) // 128, N // 128
    full = np.ones((rt * 128, N), dtype=np.uint64)
    full[:M] = on.numpy()
    b = full.reshape(rt, 4, 2, 16, ct, 8, 4, 4).transpose(0, 4, 1, 6, 3, 2, 5, 7)  # rt ct wave q r16 i j e
    w = (b << _SHIFT).sum(axis=(5, 6, 7), dtype=np.uint64)
    return torch.from_numpy(w.reshape(-1).view(np.uint8).copy())


def test_bitmask_codec_round_trips():
    g = torch.Generator().manual_seed(0)
    on = torch.rand(257, 256, generator=g) > 0.5
    assert torch.equal(decode_bits(encode_bits(on), 257, 256), on)


# ------------------------------------------------------------------------------------------------ fp32 NT
def nt_sets(M, N, K, epi, seed=0, bf16=False):
    return [("scaled+cancelling", Y.cancelling_nt(Y.scaled_nt(M, N, K, seed=seed, tanh=epi == 2, bf16=bf16))),
            ("integers", Y.integers_nt(M, N, K, seed=seed, bf16=bf16))]


def run_nt(L, o, M, N, K, epi, pads):
    pa, pb, pc, pm = pads
    A, B = gin(o["A"], pa, name="A"), gin(o["B"], pb, name="B")
    bias = gvec(o["bias"], "bias") if epi != 3 else None
    mask = gin(o["mask"], pm, name="mask") if epi == 3 else None
    C = gout(M, N, pc, name="C")
    check(L, L.rlppo_dbg_gemm_nt(stream(), A.ptr, A.ld, B.ptr, B.ld, bias.ptr if bias else None, mask.ptr if mask else None,
                                 mask.ld if mask else N, C.ptr, C.ld, M, N, K, epi))
    torch.cuda.synchronize()
    Y.assert_intact(A, B, bias, mask, C)
    return C.host()


def hold_nt(name, got, o, K, epi, allow_fn=None):
    """The three checks' numerical half: allowance on every element, or bit equality for integers (tanh: the pre-activation is exact, the
    result is within the 4 u |f| of tanhf alone).  Returns the worst ratio."""
    want, pre, S = Y.nt_truth(o["A"], o["B"], o["bias"], epi, o["mask"], o["zero"])
    if name == "integers":
        if epi == 2:
            w = Y.worst(got, want, 4 * Y.U32 * want.abs())
            assert w <= 1.0, (name, epi, w)
            return 0.0
        assert torch.equal(got.double(), want), f"integers: {int((got.double() != want).sum())} of {want.numel()} elements differ from float64"
        return 0.0
    allow = allow_fn(S, want) if allow_fn else Y.nt_allow(S, K, want, tanh=epi == 2)
    w = Y.worst(got, want, allow)
    assert w <= 1.0, (name, epi, w)
    return w


@pytest.fixture
def tiled(L):
    """The 128-row-tile kernel at every row count (rlppo_dbg_set(40, 0)); the few-row form is restored afterwards."""
    check(L, L.rlppo_dbg_set(40, 0))
    try:
        yield
    finally:
        check(L, L.rlppo_dbg_set(40, 1))


ALL_PADS = (4, 8, 12, 20)     # lda > K, ldb > K, ldc > N, ld_mask > N, all together and all different
ONE_PAD = [(8, 0, 0, 0), (0, 8, 0, 0), (0, 0, 8, 0), (0, 0, 0, 8), (0, 0, 0, 0)]


@pytest.mark.parametrize("N", [32, 64, 96, 128, 256])
def test_gemm_nt_tiled(L, tiled, N):
    """gemm_nt_dma_kernel, every tile width: BK = 16 (and BK = 32 at N = 32, K % 32 == 0), every epilogue, row counts around the 128-row
    tile edge, strides larger than the widths all together -- and one at a time at M = 129."""
    top = 0.0
    for K in (16, 48, 64, 256):
        for epi in (0, 1, 2, 3):
            for M in (1, 127, 128, 129, 257):
                for pads in [ALL_PADS] + (ONE_PAD if M == 129 and K in (16, 64) else []):
                    for name, o in nt_sets(M, N, K, epi):
                        f0 = forms(L)
                        top = max(top, hold_nt(name, run_nt(L, o, M, N, K, epi, pads), o, K, epi))
                        assert ran(L, f0)[:2] == [0, 1]                      # the tiled kernel is the one that ran
    report(f"gemm_nt tiled N={N}", top)


@pytest.mark.parametrize("N", [32, 96, 128])
def test_gemm_nt_few_rows(L, N):
    """gemm_nt_skinny_kernel (the default up to 1024 rows): row counts around its 16-row blocks, widths that are no multiple of its
    64-column workgroup, K below, at and above its 8 tiles in flight; 1025 rows is the tiled kernel; at 1024 rows the two forms give the
    same bits."""
    top = 0.0
    for K in (16, 128, 144):
        for epi in (0, 1, 2):
            for M in (1, 15, 16, 17, 1024, 1025):
                for name, o in nt_sets(M, N, K, epi, seed=1):
                    f0 = forms(L)
                    got = run_nt(L, o, M, N, K, epi, ALL_PADS)
                    assert ran(L, f0)[:2] == ([1, 0] if M <= 1024 else [0, 1])   # the few-row kernel up to 1024 rows, the tiled one at 1025
                    top = max(top, hold_nt(name, got, o, K, epi))
                    if M == 1024:
                        check(L, L.rlppo_dbg_set(40, 0))
                        try:
                            other = run_nt(L, o, M, N, K, epi, ALL_PADS)
                        finally:
                            check(L, L.rlppo_dbg_set(40, 1))
                        assert ran(L, f0)[:2] == [1, 1]
                        assert torch.equal(got.view(torch.int32), other.view(torch.int32)), (K, epi, name)
    report(f"gemm_nt few rows N={N}", top)


@pytest.mark.parametrize("N", [128, 256])
def test_gemm_nt_bits(L, N):
    """The bitmask forms: forward C = relu(pre) within the allowance with bits == [C > 0] of the kernel's OWN C exactly; dX masked by a
    given bitmask; the bit buffer guarded behind rlppo_dbg_gemm_nt_bits_bytes."""
    top = 0.0
    for K in (16, 48):
        for M in (1, 127, 129, 257):
            nbytes = int(L.rlppo_dbg_gemm_nt_bits_bytes(M, N))
            assert nbytes == ((M + 127) // 128) * (N // 128) * 256 * 8
            for name, o in nt_sets(M, N, K, 1, seed=2):
                A, B, bias = gin(o["A"], 4, name="A"), gin(o["B"], 8, name="B"), gvec(o["bias"], "bias")
                C, bits = gout(M, N, 12, name="C"), gbytes(nbytes, "bits")
                check(L, L.rlppo_dbg_gemm_nt_bits(stream(), A.ptr, A.ld, B.ptr, B.ld, bias.ptr, C.ptr, C.ld, M, N, K, 1, bits.ptr))
                torch.cuda.synchronize()
                Y.assert_intact(A, B, bias, C, bits)
                got = C.host()
                top = max(top, hold_nt(name, got, o, K, 1))
                assert torch.equal(decode_bits(bits.host().view(-1), M, N), got > 0)
                # masked dX through a GIVEN bitmask (rows past M set in it): (A . B^T) where the bit is on, 0 elsewhere
                on = o["mask"] > 0
                mb = gbytes(nbytes, "mask bits", role="in", values=encode_bits(on))
                D = gout(M, N, 12, name="dX")
                check(L, L.rlppo_dbg_gemm_nt_bits(stream(), A.ptr, A.ld, B.ptr, B.ld, None, D.ptr, D.ld, M, N, K, 3, mb.ptr))
                torch.cuda.synchronize()
                Y.assert_intact(A, B, D, mb)
                top = max(top, hold_nt(name, D.host(), o, K, 3))
    report(f"gemm_nt bitmask forms N={N}", top)


# ------------------------------------------------------------------------------------------------ fp32 TN
TN_SHAPES = [(256, 256), (90, 256), (256, 107), (90, 107), (300, 130), (1, 64), (21, 32)]   # the three geometries and their ragged tiles


def tn_sets(M, out, in_, seed=0, src_rows=None, bf16=False):
    s = Y.scaled_tn(M, out, in_, seed=seed, src_rows=src_rows, bf16=bf16)
    return [("scaled+cancelling" if not src_rows else "scaled", Y.cancelling_tn(s) if not src_rows else s),
            ("integers", Y.integers_tn(M, out, in_, seed=seed, src_rows=src_rows, bf16=bf16))]


def padded_operand(t, valid, seed):
    """t with its columns widened to `valid`: the padded columns hold finite garbage (include/rlppo.h: they may, and reach no output)."""
    g = torch.Generator().manual_seed(seed)
    pad = (torch.randn(t.shape[0], valid - t.shape[1], generator=g) * 1e6).to(t.dtype)
    return torch.cat([t, pad], 1)


def hold_tn(name, dW, db, o, M, with_db=True):
    wW, wb, SW, Sb = Y.tn_truth(o["dY"], o["X"], o["dW0"], o["db0"], o["rowtab"], o["zero"])
    if name == "integers":
        assert torch.equal(dW.double(), wW), f"integers: {int((dW.double() != wW).sum())} of {wW.numel()} dW elements differ from float64"
        assert not with_db or torch.equal(db.double(), wb)
        return 0.0
    w = Y.worst(dW, wW, Y.tn_allow(SW, M, o["dW0"]))
    if with_db:
        w = max(w, Y.worst(db, wb, Y.tn_allow(Sb, M, o["db0"])))
    assert w <= 1.0, (name, w)
    return w


def tn_buffers(L, o, out, in_, seed):
    ny, kx = int(L.rlppo_padded_out(out)), int(L.rlppo_padded_out(in_))
    dY = gin(padded_operand(o["dY"], ny, seed), 8, name="dY")              # ldy > ny_valid, NaN beyond the valid columns
    X = gin(padded_operand(o["X"], kx, seed + 1), 12, name="X")
    dW = G(out, in_, torch.float32, "cuda", role="out", values=o["dW0"], name="dW")   # the arena's contiguous block: ld == in
    db = gvec(o["db0"], "db", role="out")
    return ny, kx, dY, X, dW, db


@pytest.mark.parametrize("out,in_", TN_SHAPES)
def test_gemm_tn(L, out, in_):
    """gemm_tn_dma_kernel + tn_reduce_kernel: one split of 1 .. 32 rows, two, three (the last of one row), 64-row splits (the last of 33
    rows); padded operand columns, accumulation on top of non-zero gradients, the partial-tile workspace NaN-filled and guarded."""
    top = 0.0
    for M in (1, 31, 32, 33, 65, 2081):
        for name, o in tn_sets(M, out, in_):
            ny, kx, dY, X, dW, db = tn_buffers(L, o, out, in_, M)
            ws = gbytes(int(L.rlppo_dbg_gemm_tn_workspace_bytes(out, in_, M)), "workspace")
            check(L, L.rlppo_dbg_gemm_tn(stream(), dY.ptr, dY.ld, ny, X.ptr, X.ld, kx, dW.ptr, db.ptr, out, in_, M, ws.ptr, ws.cols))
            torch.cuda.synchronize()
            Y.assert_intact(dY, X, dW, db, ws)
            top = max(top, hold_tn(name, dW.host(), db.host().view(-1), o, M))
    report(f"gemm_tn {out}x{in_}", top)


@pytest.mark.parametrize("budget", [0, 8], ids=["two_per_cu", "eight_workgroups"])
@pytest.mark.parametrize("shapes", [[(256, 107), (90, 256), (21, 32)], [(300, 130), (90, 107), (1, 64)], [(256, 256), (256, 107), (90, 256)]],
                         ids=["first_head_small", "ragged", "update"])
def test_gemm_tn_group(L, shapes, budget):
    """The grouped launch: three products, the first through a row table that repeats indices and names the first and the last source row,
    the last without a bias gradient; few rows and 2081; the library's grid and a grid of 8 workgroups (long splits)."""
    from rlgym_ppo_amd import _native as N
    top = 0.0
    for M in (33, 2081):
        for kind in (0, 1):
            prods = (N.TnProduct * len(shapes))()
            held = []
            for i, (out, in_) in enumerate(shapes):
                name, o = tn_sets(M, out, in_, seed=10 + i, src_rows=3 * M + 7 if i == 0 else None)[kind]
                ny, kx, dY, X, dW, db = tn_buffers(L, o, out, in_, M + i)
                rt = gvec(o["rowtab"], "row table") if i == 0 else None
                with_db = i != len(shapes) - 1
                q = prods[i]
                q.dY, q.ldy, q.ny_valid, q.X, q.ldx, q.kx_valid = dY.ptr, dY.ld, ny, X.ptr, X.ld, kx
                q.dW, q.db, q.out, q.in_ = dW.ptr, db.ptr if with_db else None, out, in_
                q.rowtab, q.src_rows = (rt.ptr, 3 * M + 7) if i == 0 else (None, 0)
                held.append((name, o, dY, X, dW, db, rt, with_db))
            check(L, L.rlppo_dbg_set(38, budget))
            try:
                ws = gbytes(int(L.rlppo_dbg_gemm_tn_group_workspace_bytes(prods, len(shapes), M)), "workspace")
                check(L, L.rlppo_dbg_gemm_tn_group(stream(), prods, len(shapes), M, ws.ptr, ws.cols))
                torch.cuda.synchronize()
            finally:
                check(L, L.rlppo_dbg_set(38, 0))
            for name, o, dY, X, dW, db, rt, with_db in held:
                Y.assert_intact(dY, X, dW, db, rt, ws)
                if not with_db:
                    assert torch.equal(db.host().view(-1), o["db0"])       # db == NULL: the caller's vector is not touched
                top = max(top, hold_tn(name, dW.host(), db.host().view(-1), o, M, with_db))
    report(f"gemm_tn_group {shapes} budget {budget}", top)


# ------------------------------------------------------------------------------------------------ bf16 in memory
B16_ROWS = (1, 129, 257, 513)


@pytest.mark.parametrize("N,K", [(32, 64), (64, 128), (128, 64)])
def test_gemm_nt_b16_output_layer(L, N, K):
    """hidden == 0: bf16 operands in memory, fp32 result (epilogues 0 and 2) at the smallest legal K and N and one step above."""
    top = 0.0
    for M in B16_ROWS:
        for epi in (0, 2):
            for name, o in nt_sets(M, N, K, epi, seed=3, bf16=True):
                A, B, bias = gin(o["A"], 8, name="A"), gin(o["B"], 16, name="B"), gvec(o["bias"], "bias")
                C = gout(M, N, 12, name="C")
                check(L, L.rlppo_dbg_gemm_nt_b16(stream(), A.ptr, A.ld, B.ptr, B.ld, bias.ptr, C.ptr, C.ld, None, 0, M, N, K, epi, 0, None))
                torch.cuda.synchronize()
                Y.assert_intact(A, B, bias, C)
                top = max(top, hold_nt(name, C.host(), o, K, epi))
    report(f"gemm_nt_b16 output layer N={N} K={K}", top)


def b16_hidden_and_dx(L, M, N, K, seed, with_c32, expect=None):
    """One hidden forward (with or without the fp32 copy C) and one masked dX at M x N x K on both operand sets; `expect`: the
    (256 x 256-tile, persistent) launches each of the two calls must add to the form counters.  Returns the worst ratio."""
    top = 0.0
    nbytes = int(L.rlppo_dbg_gemm_nt_bits_bytes(M, N))
    bf16_allow = lambda S_, w_: Y.nt_allow(S_, K, w_, bf16_out=True)
    for name, o in nt_sets(M, N, K, 1, seed=seed, bf16=True):
        A, B, bias = gin(o["A"], 8, name="A"), gin(o["B"], 16, name="B"), gvec(o["bias"], "bias")
        C = gout(M, N, 12, name="C") if with_c32 else None
        Cb, bits = gout(M, N, 8, torch.bfloat16, name="Cb"), gbytes(nbytes, "bits")
        f0 = forms(L)
        check(L, L.rlppo_dbg_gemm_nt_b16(stream(), A.ptr, A.ld, B.ptr, B.ld, bias.ptr, C.ptr if C else None, C.ld if C else 0, Cb.ptr, Cb.ld,
                                         M, N, K, 1, 1, bits.ptr))
        torch.cuda.synchronize()
        assert expect is None or ran(L, f0)[2:4] == list(expect[0]), (ran(L, f0), expect)
        Y.assert_intact(A, B, bias, C, Cb, bits)
        got = Cb.host().float()
        assert C is None or torch.equal(C.host(), got)                      # the fp32 copy IS the bf16 value
        assert torch.equal(decode_bits(bits.host().view(-1), M, N), got > 0)
        want, _, S = Y.nt_truth(o["A"], o["B"], o["bias"], 1, zero=o["zero"])
        if name == "integers":
            assert torch.equal(got.double(), Y.bf16_round(want))
        else:
            top = max(top, hold_nt(name, got, o, K, 1, allow_fn=bf16_allow))
        mb = gbytes(nbytes, "mask bits", role="in", values=encode_bits(o["mask"] > 0))
        D = gout(M, N, 8, torch.bfloat16, name="dX")
        f0 = forms(L)
        check(L, L.rlppo_dbg_gemm_nt_b16(stream(), A.ptr, A.ld, B.ptr, B.ld, None, None, 0, D.ptr, D.ld, M, N, K, 3, 2, mb.ptr))
        torch.cuda.synchronize()
        assert expect is None or ran(L, f0)[2:4] == list(expect[1]), (ran(L, f0), expect)
        Y.assert_intact(A, B, D, mb)
        want, _, S = Y.nt_truth(o["A"], o["B"], o["bias"], 3, o["mask"], o["zero"])
        if name == "integers":
            assert torch.equal(D.host().double(), Y.bf16_round(want))
        else:
            top = max(top, hold_nt(name, D.host().float(), o, K, 3, allow_fn=bf16_allow))
    return top


@pytest.mark.parametrize("N,K", [(128, 64), (256, 128)])
def test_gemm_nt_b16_hidden_and_dx(L, N, K):
    """hidden == 1: C (fp32) == Cb (bf16) = round_bf16(relu(pre)) within the product's allowance + half a bf16 ulp of the UNROUNDED
    float64 value, bits == [C > 0]; on integers the bf16 rounding of the exact sum, bit for bit.  hidden == 2: the masked, rounded dX.
    Below 1024 rows every form setting runs the 128 x 128-tile kernel (asserted), so this test takes no b16_tiles fixture."""
    top = max(b16_hidden_and_dx(L, M, N, K, 4, True, expect=((0, 0), (0, 0))) for M in B16_ROWS)
    report(f"gemm_nt_b16 hidden + dX N={N} K={K} (128 x 128 tiles)", top)


def test_gemm_nt_b16_hidden_and_dx_wide_tiles(L, b16_tiles):
    """From 1024 rows on a width that is a multiple of 256 takes the 256 x 256-tile kernels: one workgroup per tile, or persistent
    workgroups when the call asks for no fp32 copy (every dX, and the hidden forward of an update pass).  1024 rows: four whole row
    tiles; 1025: a fifth of one row.  The form counters prove which kernel each call ran under each b16_tiles setting."""
    N, K, top = 256, 128, 0.0
    wide, pers, small = (1, 0), (0, 1), (0, 0)
    for M in (1024, 1025):
        for with_c32 in (True, False):
            fwd = small if b16_tiles == 0 else pers if (b16_tiles == 2 and not with_c32) else wide
            dx = small if b16_tiles == 0 else pers if b16_tiles == 2 else wide
            top = max(top, b16_hidden_and_dx(L, M, N, K, 14, with_c32, expect=(fwd, dx)))
    report(f"gemm_nt_b16 hidden + dX N={N} K={K} from 1024 rows, tiles {b16_tiles}", top)


@pytest.mark.parametrize("pout,pin,out,in_", [(128, 128, 100, 107), (256, 128, 256, 128), (128, 256, 1, 231), (256, 256, 200, 256)])
def test_gemm_tn_b16(L, pout, pin, out, in_, b16_tiles):
    """The bf16 weight-gradient product per element: exact products, float32 accumulation over M rows, on top of non-zero gradients."""
    top = 0.0
    for M in B16_ROWS:
        for name, o in tn_sets(M, out, in_, seed=5, bf16=True):
            dY = gin(padded_operand(o["dY"], pout, M), 8, name="dY")
            X = gin(padded_operand(o["X"], pin, M + 1), 16, name="X")
            dW = G(out, in_, torch.float32, "cuda", role="out", values=o["dW0"], name="dW")
            db = gvec(o["db0"], "db", role="out")
            ws = gbytes(int(L.rlppo_dbg_gemm_tn_workspace_bytes(out, in_, M)), "workspace")
            check(L, L.rlppo_dbg_gemm_tn_b16(stream(), dY.ptr, dY.ld, X.ptr, X.ld, dW.ptr, db.ptr, pout, pin, out, in_, M, ws.ptr, ws.cols))
            torch.cuda.synchronize()
            Y.assert_intact(dY, X, dW, db, ws)
            top = max(top, hold_tn(name, dW.host(), db.host().view(-1), o, M))
    report(f"gemm_tn_b16 {out}x{in_} tiles {b16_tiles}", top)


@pytest.mark.parametrize("out,kp,in_", [(1, 128, 128), (21, 128, 100), (8, 256, 256), (32, 256, 231)])
def test_thin_head_b16(L, out, kp, in_):
    """The narrow head's two backward products: dxb = round_bf16(dY . W) masked by the bitmask (contraction over the `out` outputs:
    allowance (out + 8) u sum|dy||w| + half a bf16 ulp), dW += dY^T . hb and db += colsum(dY) per element over M rows."""
    top, top_w = 0.0, 0.0
    for M in B16_ROWS:
        nbytes = int(L.rlppo_dbg_gemm_nt_bits_bytes(M, kp))
        for kind in ("scaled", "integers"):
            g = torch.Generator().manual_seed(1000 * out + kp + M)
            if kind == "scaled":
                t = Y.cancelling_tn(Y.scaled_tn(M, out, kp, seed=6))
                hb = t["X"].clamp(min=0).bfloat16()
                W = (torch.randn(out, kp, generator=g) * 2.0 ** Y._exponents(kp, g)).bfloat16().float()
            else:
                t = Y.integers_tn(M, out, kp, seed=6, r=8)
                hb = t["X"].clamp(min=0).bfloat16()
                W = Y._nonzero_ints(8, (out, kp), g)
            on = hb.float() > 0
            # include/rlppo.h: dY is read over max(4, padded outputs) columns, those from `out` on may hold any finite values; W over `out` rows
            nout = max(4, 1 if out == 1 else (out + 7) // 8 * 8)
            dY, Wg, hbg = gin(padded_operand(t["dY"], nout, M), 8, name="dY"), gin(W, 4, name="W"), gin(hb, 8, name="hb")
            bits = gbytes(nbytes, "bits", role="in", values=encode_bits(on))
            dxb = G(M, kp, torch.bfloat16, "cuda", role="out", name="dxb")
            dW = G(out, in_, torch.float32, "cuda", role="out", values=t["dW0"][:, :in_], name="dW")
            db = gvec(t["db0"], "db", role="out")
            ws = gbytes(int(L.rlppo_dbg_thin_head_workspace_bytes(out, kp, M)), "workspace")
            check(L, L.rlppo_dbg_thin_head_b16(stream(), dY.ptr, dY.ld, out, Wg.ptr, Wg.ld, bits.ptr, hbg.ptr, hbg.ld, dxb.ptr, dW.ptr, db.ptr,
                                               in_, kp, M, ws.ptr, ws.cols))
            torch.cuda.synchronize()
            Y.assert_intact(dY, Wg, hbg, bits, dxb, dW, db, ws)
            o_dx = dict(A=t["dY"], B=W.T.contiguous(), bias=None, mask=on.float(), zero=None)
            o_dw = dict(dY=t["dY"], X=hb[:, :in_], dW0=t["dW0"][:, :in_], db0=t["db0"], rowtab=None,
                        zero=t["zero"][:, :in_] if kind == "scaled" and (hb.float() == t["X"].clamp(min=0)).all() else None)
            want, _, S = Y.nt_truth(o_dx["A"], o_dx["B"], None, 3, o_dx["mask"])
            if kind == "integers":
                assert torch.equal(dxb.host().double(), Y.bf16_round(want))
            else:
                top = max(top, hold_nt(kind, dxb.host().float(), o_dx, out, 3, allow_fn=lambda S_, w_: Y.nt_allow(S_, out, w_, bf16_out=True)))
            top_w = max(top_w, hold_tn(kind, dW.host(), db.host().view(-1), o_dw, M))
    report(f"thin_head_b16 out={out} kp={kp} dX (bf16 out)", top)
    report(f"thin_head_b16 out={out} kp={kp} dW, db", top_w)


# ------------------------------------------------------------------------------------------------ split-bf16 (x3)
def x3_case(L, o, name, M, N, K, modes=(0, 1)):
    """pack + forward (mode 0) and / or masked dX (mode 1) of one operand set; returns the worst ratio."""
    top = 0.0
    nbytes = int(L.rlppo_dbg_gemm_nt_bits_bytes(M, N))
    W = gin(o["B"], 8, name="W")
    planes = G(1, 3 * N * K, torch.bfloat16, "cuda", ld=3 * N * K + 16, band=1, role="out", name="planes")
    check(L, L.rlppo_dbg_pack_x3(stream(), W.ptr, W.ld, N, K, planes.ptr))
    A, bias = gin(o["A"], 4, name="A"), gvec(o["bias"], "bias")
    torch.cuda.synchronize()
    Y.assert_intact(W, planes)
    if 0 in modes:
        C, bits = gout(M, N, 12, name="C"), gbytes(nbytes, "bits")
        check(L, L.rlppo_dbg_gemm_nt_x3(stream(), A.ptr, A.ld, planes.ptr, bias.ptr, C.ptr, C.ld, M, N, K, 0, bits.ptr))
        torch.cuda.synchronize()
        Y.assert_intact(planes, A, bias, C, bits)
        got = C.host()
        top = max(top, hold_nt(name, got, o, K, 1, allow_fn=lambda S_, w_: Y.x3_allow(S_, K)))
        assert torch.equal(decode_bits(bits.host().view(-1), M, N), got > 0)
    if 1 in modes:
        mb = gbytes(nbytes, "mask bits", role="in", values=encode_bits(o["mask"] > 0))
        D = gout(M, N, 12, name="dX")
        check(L, L.rlppo_dbg_gemm_nt_x3(stream(), A.ptr, A.ld, planes.ptr, None, D.ptr, D.ld, M, N, K, 1, mb.ptr))
        torch.cuda.synchronize()
        Y.assert_intact(planes, A, D, mb)
        top = max(top, hold_nt(name, D.host(), o, K, 3, allow_fn=lambda S_, w_: Y.x3_allow(S_, K)))
    return top


@pytest.mark.parametrize("K", [32, 96])
def test_gemm_nt_x3(L, K):
    """The split-bf16 products (gemm_nt_split_kernel, one tile per workgroup: asserted), ALL rows against float64 with the allowance
    derived from the piece products gemm_split.hip keeps and drops ((K + K / 32 + 3) u (sum|a||b| + |bias|): below the fp32 constant at
    these K), not against the fp32 kernel; integers exact."""
    N, top, f0 = 256, 0.0, forms(L)
    for M in (1, 129, 513):
        for name, o in nt_sets(M, N, K, 1, seed=7):
            top = max(top, x3_case(L, o, name, M, N, K))
    assert ran(L, f0)[4] == 0
    report(f"gemm_nt_x3 K={K} one tile per workgroup", top)


def test_gemm_nt_x3_persistent(L):
    """gemm_nt_split_p_kernel, the form an update pass runs: the launcher takes it only from 2 x 8 x (CUs / 8) row tiles of 256 (512 tiles
    = 130,817 rows on 256 CUs) and an even K / 32, so this is the file's one large case: the smallest row count that reaches it, a ragged
    last tile of one row, K = 64.  Forward within the allowance on scaled + cancelling operands; forward and masked dX bit-equal to
    float64 on integers; guard bands on all; the form counter proves the persistent kernel ran all three launches."""
    N, K = 256, 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = (2 * max(cus // 8, 1) * 8 - 1) * 256 + 1
    rows, cols = torch.arange(M)[:, None], torch.arange(N)[None, :]
    mask = ((rows * 7 + cols * 3) % 5 - 2).float()                 # -2 .. 2, a fifth of it zeros: cheap at this size
    g = torch.Generator().manual_seed(11)
    ea, eb = Y._exponents(M, g), Y._exponents(N, g)
    s = dict(A=torch.randn(M, K, generator=g) * (2.0 ** ea)[:, None], B=torch.randn(N, K, generator=g) * (2.0 ** eb)[:, None],
             bias=torch.randn(N, generator=g) * 2.0 ** eb, mask=mask, zero=None)
    i = dict(A=Y._nonzero_ints(8, (M, K), g), B=Y._nonzero_ints(8, (N, K), g), bias=torch.randint(-64, 65, (N,), generator=g).float(),
             mask=mask, zero=None)
    assert Y.int_range_ok(8, 8, K, 64)
    f0 = forms(L)
    top = x3_case(L, Y.cancelling_nt(s), "scaled+cancelling", M, N, K, modes=(0,))
    x3_case(L, i, "integers", M, N, K)
    assert ran(L, f0)[4] == 3, "the persistent split-bf16 kernel did not run"
    report(f"gemm_nt_x3 K={K} persistent workgroups, {M} rows", top)


# ------------------------------------------------------------------------------------------------ the one-output head (gemv.hip)
@pytest.mark.parametrize("kp", [64, 256])
def test_gemv_one_output_head(L, kp):
    """The critic head's matrix-vector kernels alone (rlppo_dbg_gemv_*): forward (the padded output columns are zeros), dX by the saved
    activation and by the bitmask, dW / db through the fixed-order partials and through atomics; around the 256-row mark."""
    top = {"forward": 0.0, "dX": 0.0, "dW, db": 0.0}
    for M in (1, 255, 256, 257):
        for name, o in nt_sets(M, 32, kp, 0, seed=8):
            x, w, b = gin(o["A"], 8, name="x"), gvec(o["B"][0], "w"), gvec(o["bias"][:1], "b")
            y = gout(M, 32, 4, name="y")
            check(L, L.rlppo_dbg_gemv_fwd(stream(), x.ptr, x.ld, w.ptr, b.ptr, y.ptr, y.ld, M, kp, 32))
            torch.cuda.synchronize()
            Y.assert_intact(x, w, b, y)
            got = y.host()
            assert not got[:, 1:].any()
            o1 = dict(o, B=o["B"][:1], bias=o["bias"][:1], zero=o["zero"][:, :1] if o["zero"] is not None else None)
            top["forward"] = max(top["forward"], hold_nt(name, got[:, :1], o1, kp, 0))
        # backward: dy[m] in column 0 of a 32-wide buffer whose other columns are NaN (nothing but column 0 is the kernels' to read)
        for name, t in tn_sets(M, 1, kp, seed=9):
            in_ = kp - 3
            h = t["X"].clamp(min=0)                                          # the saved ReLU activation
            g = torch.Generator().manual_seed(kp + M)
            w_t = torch.randn(kp, generator=g) * 2.0 ** Y._exponents(kp, g) if name != "integers" else Y._nonzero_ints(8, (kp,), g)
            dy32 = torch.full((M, 32), float("nan"))
            dy32[:, 0] = t["dY"][:, 0]
            dy, w, hg = gin(dy32, 4, name="dy"), gvec(w_t, "w"), gin(h, 8, name="h")
            want_dx = t["dY"].double() * w_t.double() * (h > 0)
            outs = []
            if kp % 128 == 0:
                bits = gbytes(int(L.rlppo_dbg_gemm_nt_bits_bytes(M, kp)), "bits", role="in", values=encode_bits(h > 0))
                outs.append(bits)
            for b_ in outs + [None]:
                dx = gout(M, kp, 12, name="dx")
                check(L, L.rlppo_dbg_gemv_dx(stream(), dy.ptr, dy.ld, w.ptr, hg.ptr, hg.ld, b_.ptr if b_ else None, dx.ptr, dx.ld, kp, M))
                torch.cuda.synchronize()
                Y.assert_intact(dy, w, hg, dx, b_)
                # one product per element: one rounding, u |dy w|; integers exact
                r = Y.worst(dx.host(), want_dx, Y.U32 * want_dx.abs())
                assert r <= 1.0 and (name != "integers" or torch.equal(dx.host().double(), want_dx))
                top["dX"] = max(top["dX"], r)
            o_dw = dict(t, X=h[:, :in_], dW0=t["dW0"][:, :in_], zero=None)
            for fixed_order in (True, False):
                dW = G(1, in_, torch.float32, "cuda", role="out", values=o_dw["dW0"], name="dw")
                db = gvec(t["db0"], "db", role="out")
                ws = gbytes(int(L.rlppo_dbg_gemv_dw_workspace_bytes(kp, M)), "workspace") if fixed_order else None
                f0 = forms(L)
                check(L, L.rlppo_dbg_gemv_dw(stream(), dy.ptr, dy.ld, hg.ptr, hg.ld, dW.ptr, db.ptr, in_, kp, M, ws.ptr if ws else None,
                                             ws.cols if ws else 0))
                torch.cuda.synchronize()
                assert ran(L, f0)[5] == int(fixed_order)                     # the partials + reduction ran, or the atomics did
                Y.assert_intact(dy, hg, dW, db, ws)
                top["dW, db"] = max(top["dW, db"], hold_tn(name, dW.host(), db.host().view(-1), o_dw, M))
    for k, v in top.items():
        report(f"gemv one-output head kp={kp} {k}", v)
