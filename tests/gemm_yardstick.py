"""The yardstick of the matrix products (csrc/gemm.hip, gemm_b16.hip, gemm_split.hip, gemv.hip): float64 truth of the same operand
values, a PER-ELEMENT allowance, operand makers with fixed seeds, and guarded buffers.  Plain torch / numpy: it runs on the CPU
(tests/test_gemm_yardstick_host.py shows it is neither too tight nor too loose) and the GPU tests hold every kernel to it
(tests/test_gpu_products.py).

The allowance
-------------
u = 2^-24 (float32 unit roundoff).  A float32 sum of n terms t_1 .. t_n taken in ANY order and grouping has n - 1 additions, each
rounding its own partial sum, which is at most sum|t|: |fl(sum) - sum| <= (n - 1) u sum|t| to first order in u.  A product a b is
either fused into the addition (MFMA, fmaf: no rounding of its own) or rounded once (u |a b|, one more unit).  Hence

  NT   C[m][n] = sum_k a_k b_k + bias : K + 1 terms; the project's constant keeps 8 units of slack for the second-order terms, an
       unfused product and the epilogue:              allow = (K + 8) u (sum_k |a_k b_k| + |bias|)      (product_bound of
       tests/test_gpu_hidden_activation.py).  ReLU and the mask are 1-Lipschitz or exact: nothing is added and NO element is
       excluded, the ones whose float64 value is 0 included (there the allowance is the product's own, > 0).
  tanh f = tanh(pre) is 1-Lipschitz; tanhf is good to a few ulp:                 + 4 u |f|.
  TN   dW[n][k] = dW0 + sum_m dy_m x_m : the same with the contraction length M, whatever the splits, the two chains per split
       and the reduction tree do to the order; the sum is then added ON TOP of dW0 (one rounding of |dW0 + s| <= |dW0| + sum|t|):
                                                       allow = (M + 8) u sum_m |dy_m x_m| + 2 u |dW0|,  db alike with x = 1.
  bf16 operands: the values ARE bf16 numbers, their products are exact in float32 (8 x 8 bits), the accumulation is float32: the
       NT / TN allowance unchanged.  A bf16 OUTPUT rounds the float32 result once more: + half a bf16 ulp of the result (taken
       at |want| + allow, the largest magnitude the float32 result can have), measured against the UNROUNDED float64 value
       (against the rounded one it would be a whole ulp: the two can round apart).  On integers the float32 result is exact, so
       the output equals bf16_round(truth) bit for bit.
  x3   (split-bf16, gemm_split.hip) x = x_h + x_m + x_l, every piece rounded to nearest: the first residual is at most half a
       bf16 ulp, |x_m| <= 2^-8 |x|, the second |x_l| <= 2^-17 |x|, and the third piece is EXACT (a float32 has 24 bits, the
       first two pieces take 8 + 9 of them with their signs, 6 are left): the pieces add up to x.  Of the nine piece products the
       kernel keeps the six with index sum <= 2 and drops x_m w_l, x_l w_m, x_l w_l <= (2 . 2^-25 + 2^-34) |x||w| = 1.001 u |x||w|.
       Per 32-wide K block the large product x_h w_h is ONE MFMA into the accumulator (32 exact products: a float32 chain of K
       terms over the row, bias first) and the five small ones, <= (2 . 2^-8 + 3 . 2^-17) |x||w| together, are a chain of 160 terms
       from 0 (<= 160 u . 2^-6.99 sum|x||w| = 1.26 u sum|x||w|) that enters the accumulator with one addition (K / 32 more):
                                                       allow = (K + K / 32 + 3) u (sum_k |a_k b_k| + |bias|).
       This is BELOW the fp32 constant K + 8 up to K = 128 and above it from K = 160 on (K = 256: 267 against 264): the
       derivation is used as it stands, because the extra K / 32 additions are real.

Why integers are exact
----------------------
Operands that are small integers (|x| <= 256: bf16 numbers, so float32, bf16 and the three-piece split hold them exactly, with
x_m = x_l = 0) make every product an integer and every partial sum, in any order, an integer below 2^24 -- exactly representable
in float32.  No addition rounds, so a correct kernel equals the float64 product BIT FOR BIT whatever its summation order; a
dropped, doubled or mis-addressed term changes an integer and cannot hide.  The makers assert, from the shapes alone, that
r_a r_b n + r_0 < 2^24 (n the contraction length, r_0 the bound of bias / dW0) and that every range is within 256.

Buffers
-------
Guarded puts a rows x cols matrix inside a larger buffer: leading dimension > cols, a band of rows before and after.  Everything
outside the matrix holds a sentinel bit pattern that reads as NaN in float32 and bf16 (an input read beyond its contract poisons the
result; a store beyond an output's contract changes the pattern); an output is prefilled with NaN.  After the call violations()
names every changed sentinel, every NaN left in an output and every input that changed.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
SENT32 = 0x7FC5A5A5                                                         # a quiet NaN with a payload (int32 view)
SENT16 = 0x7FC5                                                             # the same in bf16 (int16 view)
SENT8 = 0xA5


# ---------------------------------------------------------------------------------------------------------------- truth
def bf16_round(x64):
    """float64 -> nearest bf16 (ties to even), returned as float64.  Exact for the magnitudes used here: float64 -> float32 is only
    inexact below 2^-24 relative, which moves a bf16 rounding decision for no value a float32 kernel can produce."""
    return x64.float().bfloat16().double()


def nt_truth(A, B, bias, epi, mask=None, zero=None):
    """(want, pre, S): float64 C = epi(A . B^T + bias) of the operand VALUES (float32 or bf16 tensors), the pre-activation and
    S = sum_k |a_k b_k| + |bias|.  epi: 0 bias, 1 bias + ReLU, 2 bias + tanh, 3 (A . B^T) masked by mask > 0 (no bias).
    zero: the elements whose product is 0 BY CONSTRUCTION (cancelling_nt): a float64 matmul leaves K 2^-53 sum|a||b| there, the exact
    value is 0 and that is what the truth holds."""
    A, B = A.double(), B.double()
    pre = A @ B.T
    if zero is not None:
        pre = pre.masked_fill(zero, 0.0)
    S = A.abs() @ B.abs().T
    if epi == 3:
        return pre * (mask > 0), pre, S
    pre = pre + bias.double()
    S = S + bias.double().abs()
    want = pre if epi == 0 else pre.clamp(min=0) if epi == 1 else torch.tanh(pre)
    return want, pre, S


def tn_truth(dY, X, dW0, db0, rowtab=None, zero=None):
    """(dW, db, SW, Sb) in float64: dW0 + dY^T . X[rowtab], db0 + colsum(dY), and the sums of absolute terms."""
    dY = dY.double()
    X = (X if rowtab is None else X[rowtab.long()]).double()
    P, s = dY.T @ X, dY.sum(0)
    if zero is not None:   # (cancelling_tn: products and column sums that are 0 by construction, not K 2^-53 sum|t|)
        P, s = P.masked_fill(zero, 0.0), s.masked_fill(zero.any(1), 0.0)
    return dW0.double() + P, db0.double() + s, dY.abs().T @ X.abs(), dY.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------- allowances
def half_ulp_bf16(x64):
    """Half a bf16 ulp (8 significant bits) at magnitude |x|: 2^(floor(log2 |x|) - 8); 0 at 0."""
    _, e = np.frexp(np.abs(x64.numpy()))
    return torch.from_numpy(np.where(x64.numpy() == 0, 0.0, np.ldexp(1.0, e - 9)))


def nt_allow(S, K, want=None, tanh=False, bf16_out=False):
    a = (K + 8) * U32 * S
    if tanh:
        a = a + 4 * U32 * want.abs()
    if bf16_out:
        a = a + half_ulp_bf16(want.abs() + a)
    return a


def x3_const(K):
    return K + K // 32 + 3


def x3_allow(S, K):
    return x3_const(K) * U32 * S


def tn_allow(S, M, base0):
    return (M + 8) * U32 * S + 2 * U32 * base0.double().abs()


def worst(got, want, allow):
    """max over ALL elements of |got - want| / allow; an element with allow == 0 must be exact (ratio 0 or inf)."""
    err = (got.double() - want).abs()
    r = torch.where(allow > 0, err / allow.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isnan(got.double()), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def maxnorm(got, want):
    """The suite's old gate: max|got - want| / max|want| (relerr of tests/test_gpu_kernels.py)."""
    return float((got.double() - want).abs().max() / want.abs().max().clamp(min=1e-30))


# ---------------------------------------------------------------------------------------------------------------- operand makers
def _exponents(n, g):
    """n integer exponents uniform in -12 .. 12; with n >= 2 both ends are present (entries 0 and 1 of a random order)."""
    e = torch.randint(-12, 13, (n,), generator=g)
    if n >= 2:
        p = torch.randperm(n, generator=g)
        e[p[0]], e[p[1]] = -12, 12
    return e


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def scaled_nt(M, N, K, seed=0, tanh=False, bf16=False):
    """randn with the rows of A and the rows of B (and its bias entry) scaled by 2^e, e in -12 .. 12: outputs span ~48 binades,
    every dot product stays as well conditioned relative to its own sum|a||b| as an unscaled one.  tanh: B and bias times
    1 / sqrt(K), so that with unit row scales the pre-activations are O(1).  Returns dict(A, B, bias, mask, ea, eb)."""
    g = _gen(1000003 * seed + 131 * M + 17 * N + K)
    ea, eb = _exponents(M, g), _exponents(N, g)
    A = torch.randn(M, K, generator=g) * (2.0 ** ea)[:, None]
    B = torch.randn(N, K, generator=g) * (2.0 ** eb)[:, None]
    bias = torch.randn(N, generator=g) * 2.0 ** eb
    if tanh:
        B, bias = B / K ** 0.5, bias / K ** 0.5
    mask = mask_values(M, N, g)
    if bf16:
        A, B = A.bfloat16(), B.bfloat16()
    return dict(A=A, B=B, bias=bias, mask=mask, ea=ea, eb=eb, zero=None)


def mask_values(M, N, g):
    """A saved-activation operand for the mask epilogue: randn with +0, -0 and the smallest positive / negative normals sprinkled in."""
    mask = torch.randn(M, N, generator=g)
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, -2.0 ** -126])
    pick = torch.randint(0, 8, (M, N), generator=g)
    for i in range(4):
        mask = torch.where(pick == i, special[i].expand(M, N), mask)
    return mask


def cancelling_nt(ops):
    """On top of an NT operand set: in every third row of A the second half of the contraction is MINUS the first half, in every
    second row of B it EQUALS the first half and the bias is 0 -- those outputs are exactly 0 in float64 while sum|a||b| is not."""
    A, B, bias = ops["A"].clone(), ops["B"].clone(), ops["bias"].clone()
    h = A.shape[1] // 2
    A[::3, h:2 * h] = -A[::3, :h]
    B[::2, h:2 * h] = B[::2, :h]
    bias[::2] = 0
    zero = torch.zeros(A.shape[0], B.shape[0], dtype=torch.bool)
    zero[::3, ::2] = 2 * h == A.shape[1]
    return dict(ops, A=A, B=B, bias=bias, zero=zero)


def int_range_ok(ra, rb, n, r0):
    return max(ra, rb, 1) <= 256 and r0 <= 2 ** 24 and ra * rb * n + r0 < 2 ** 24


def _nonzero_ints(r, shape, g):
    """Integers of magnitude 1 .. r, either sign: no entry is 0, so dropping ANY term of a product changes the result."""
    return (torch.randint(1, r + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def integers_nt(M, N, K, seed=0, r=8, r_bias=64, bf16=False):
    """Non-zero integer operands in [-r, r], non-zero integer bias in [-r_bias, r_bias]: every partial sum, in any order, is an integer of magnitude
    <= r r K + r_bias < 2^24 and every value is a bf16 number (asserted from the shapes alone)."""
    assert int_range_ok(r, r, K, r_bias), f"integers_nt: r={r} K={K} r_bias={r_bias}: a partial sum can reach 2^24 or an entry is no bf16 number"
    g = _gen(2000003 * seed + 131 * M + 17 * N + K)
    A = _nonzero_ints(r, (M, K), g)
    B = _nonzero_ints(r, (N, K), g)
    bias = _nonzero_ints(r_bias, (N,), g)
    mask = mask_values(M, N, g)
    if bf16:
        A, B = A.bfloat16(), B.bfloat16()
    return dict(A=A, B=B, bias=bias, mask=mask, zero=None)


def scaled_tn(M, out, in_, seed=0, bf16=False, src_rows=None):
    """The TN counterpart: the COLUMNS of dY and of X scaled by 2^e; dW0 / db0 take their element's scale.  src_rows: X has that many
    rows and a row table (repeats; the first and the last source row are named) picks the M of the contraction."""
    g = _gen(3000003 * seed + 131 * M + 17 * out + in_)
    ey, ex = _exponents(out, g), _exponents(in_, g)
    rows = src_rows or M
    dY = torch.randn(M, out, generator=g) * 2.0 ** ey
    X = torch.randn(rows, in_, generator=g) * 2.0 ** ex
    dW0 = torch.randn(out, in_, generator=g) * (2.0 ** ey)[:, None] * 2.0 ** ex
    db0 = torch.randn(out, generator=g) * 2.0 ** ey
    if bf16:
        dY, X = dY.bfloat16(), X.bfloat16()
    return dict(dY=dY, X=X, dW0=dW0, db0=db0, ey=ey, ex=ex, rowtab=row_table(M, rows, g) if src_rows else None, zero=None)


def row_table(M, rows, g):
    t = torch.randint(0, rows, (M,), generator=g).to(torch.int32)
    t[0] = rows - 1
    if M > 1:
        t[-1] = 0
    if M > 3:
        t[2] = t[1]
    return t


def cancelling_tn(ops):
    """On top of a TN operand set without a row table: rows M/2 .. 2 (M/2) - 1 repeat the first M/2, with every second column of
    dY negated and every third column of X equal -- dW[2 i][3 j] is exactly dW0 there (an odd last row is 0 in those columns)."""
    assert ops["rowtab"] is None
    dY, X = ops["dY"].clone(), ops["X"].clone()
    M = dY.shape[0]
    h = M // 2
    dY[h:2 * h, ::2] = -dY[:h, ::2]
    X[h:2 * h, ::3] = X[:h, ::3]
    if M % 2:
        dY[M - 1, ::2] = 0
    zero = torch.zeros(dY.shape[1], X.shape[1], dtype=torch.bool)
    zero[::2, ::3] = True
    return dict(ops, dY=dY, X=X, zero=zero)


def integers_tn(M, out, in_, seed=0, r=3, r0=64, bf16=False, src_rows=None):
    """Non-zero integer dY, X in [-r, r] and non-zero integer dW0, db0 in [-r0, r0]: r r M + r0 < 2^24 (asserted).  r = 3 fits M up to 1.8 million."""
    assert int_range_ok(r, r, M, r0), f"integers_tn: r={r} M={M} r0={r0}: a partial sum can reach 2^24 or an entry is no bf16 number"
    g = _gen(4000003 * seed + 131 * M + 17 * out + in_)
    rows = src_rows or M
    dY = _nonzero_ints(r, (M, out), g)
    X = _nonzero_ints(r, (rows, in_), g)
    dW0 = _nonzero_ints(r0, (out, in_), g)
    db0 = _nonzero_ints(r0, (out,), g)
    if bf16:
        dY, X = dY.bfloat16(), X.bfloat16()
    return dict(dY=dY, X=X, dW0=dW0, db0=db0, rowtab=row_table(M, rows, g) if src_rows else None, zero=None)


# ---------------------------------------------------------------------------------------------------------------- float32 restatements
def nt_float32(A, B, bias, epi, mask=None):
    """torch's float32 product of the operand values (bf16 operands: exact products, float32 accumulation -- the bf16 kernels' arithmetic)."""
    pre = A.float() @ B.float().T
    if epi == 3:
        return pre * (mask > 0)
    pre = pre + bias
    return pre if epi == 0 else pre.clamp(min=0) if epi == 1 else torch.tanh(pre)


def tn_float32(dY, X, dW0, db0, rowtab=None):
    X = X if rowtab is None else X[rowtab.long()]
    return dW0 + dY.float().T @ X.float(), db0 + dY.float().sum(0)


def split3(x):
    """The three bf16 pieces of a float32 tensor, as float32 (gemm_split.hip, split8)."""
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    l = (x - h - m).bfloat16().float()
    return h, m, l


def x3_float32(A, B, bias, mode, mask=None):
    """The split-bf16 product restated in float32: the large product + the five small ones summed apart, the piece x_l w_l etc. dropped."""
    (ah, am, al), (bh, bm, bl) = split3(A), split3(B)
    small = ah @ bm.T + am @ bh.T + am @ bm.T + ah @ bl.T + al @ bh.T
    pre = ah @ bh.T + small
    return (pre + bias).clamp(min=0) if mode == 0 else pre * (mask > 0)


# ---------------------------------------------------------------------------------------------------------------- guarded buffers
_INT = {torch.float32: (torch.int32, SENT32), torch.bfloat16: (torch.int16, SENT16), torch.uint8: (torch.uint8, SENT8),
        torch.int32: (torch.int32, SENT32)}


class Guarded:
    """rows x cols of `dtype` at leading dimension ld >= cols inside a (band + rows + band) x ld buffer of sentinels.
    role 'in': holds `values`, must come back unchanged.  role 'out': prefilled with NaN (or `values`: an accumulator), must come
    back without NaN.  role 'scratch' (a workspace inside its stated size): prefilled with NaN bytes, nothing is asked of it.
    .m is the strided view, .ptr its address, .ld the leading dimension in elements."""

    def __init__(self, rows, cols, dtype=torch.float32, device="cpu", ld=None, band=2, role="out", values=None, name=""):
        self.idt, self.sent = _INT[dtype]
        self.rows, self.cols, self.ld, self.band, self.role, self.name = rows, cols, ld or cols, band, role, name
        assert self.ld >= cols
        self.raw = torch.full((rows + 2 * band, self.ld), self.sent, dtype=self.idt, device=device)
        self.m = (self.raw if dtype == self.idt else self.raw.view(dtype))[band:band + rows, :cols]
        if values is not None:
            self.m.copy_(values.to(device=device, dtype=dtype).reshape(rows, cols))
        elif role == "scratch" or dtype in (torch.uint8, torch.int32):
            self.im.fill_(-1 if self.idt != torch.uint8 else 0xFF)
        else:
            self.m.fill_(float("nan"))
        self.before = self.im.clone() if role == "in" else None

    @property
    def im(self):
        return self.raw[self.band:self.band + self.rows, :self.cols]

    @property
    def ptr(self):
        return self.m.data_ptr()

    def violations(self):
        out = []
        outside = torch.ones_like(self.raw, dtype=torch.bool)
        outside[self.band:self.band + self.rows, :self.cols] = False
        bad = outside & (self.raw != self.sent)
        if bad.any():
            r, c = [int(v[0]) for v in torch.nonzero(bad, as_tuple=True)]
            out.append(f"{self.name}: {int(bad.sum())} sentinel(s) overwritten, the first at row {r - self.band} column {c} (rows x cols {self.rows} x {self.cols}, ld {self.ld})")
        if self.role == "out" and self.m.is_floating_point() and torch.isnan(self.m).any():
            out.append(f"{self.name}: {int(torch.isnan(self.m).sum())} NaN left in the output")
        if self.role == "in" and not torch.equal(self.im, self.before):
            out.append(f"{self.name}: an input changed")
        return out

    def host(self):
        return self.m.detach().cpu().clone()


def vec(n, dtype=torch.float32, device="cpu", pad=8, **kw):
    """A guarded vector (bias, db, a bitmask, a workspace): n elements with `pad` sentinels behind them in their own row."""
    return Guarded(1, n, dtype, device, ld=n + pad, band=1, **kw)


def assert_intact(*bufs):
    bad = [v for b in bufs if b is not None for v in b.violations()]
    assert not bad, "; ".join(bad)
