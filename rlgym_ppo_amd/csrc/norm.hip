// norm.hip -- parameter-free layer normalisation of a hidden activation, as two row kernels between the products of a layer chain
// (chain.hip): y = (h - mean(h)) * rsqrt(var(h) + 1e-5) over the TRUE width of the layer (torch's F.layer_norm without weight or
// bias: biased variance, eps inside the root), and its backward multiplied by the activation's derivative in the same launch.
//
// Design.  A row lives in the registers of the lanes that own it: LPR lanes per row (16 for padded widths up to 128 -- four rows per
// wave --, the whole wave from 256 on), lane i holding the 16-byte chunks i, i + LPR, ... of the row (consecutive lanes read
// consecutive chunks: every load and store instruction of a wave covers whole runs of a row).  A lane adds its own elements in
// column order, the lanes' sums meet in an xor butterfly of log2(LPR) shuffles -- every lane ends with the same bits, the order is
// fixed by the shape alone, so results are reproducible from run to run and the backward recomputes the forward's statistics
// exactly (row_stats is the one instruction sequence both kernels run; nothing but h is kept between them).  No LDS, no atomics, no
// allocation, no synchronisation: the forward is one read and one write of the matrix, the backward two reads and one write.
// The variance is centred (a second pass over the registers, never E[x^2] - mean^2), and the mean is refined once by the mean of
// the centred values, so a row of mean 1e3 and spread 1 keeps the precision of its spread.  Columns [width, padded width) are
// outside every sum and are STORED as exact zeros (the next layer's products and the dW product read them); rows at and beyond n
// are neither read nor written.  The outputs may alias an input (y == h, dx == dy): a lane stores only after its last load, and only
// the chunks it loaded.
// RowRegs / group_sum / row_stats / row_norm_bwd / act_bwd / the launch shape live in norm_rows.hpp: residual.hip's kernels are the same
// design on the same code.
#include "norm_rows.hpp"

namespace rlppo {

namespace {
// zeros (optional): zero_n floats that workgroup 0 clears -- the zero bias of the backward's plain dX products (chain.hip), written
// by the chain's first forward launch instead of a fill of its own
template <int LPR, int VPL>
__global__ __launch_bounds__(256) void row_norm_fwd_kernel(const float *h, int64_t ld, int64_t n, int width, int cpr, float *y, int64_t ld_y,
                                                           float *zeros, int zero_n) {
    if (zeros && blockIdx.x == 0)
        for (int i = threadIdx.x; i < zero_n; i += 256) zeros[i] = 0.f;
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int sub = threadIdx.x % LPR;
    const bool live = row < n;
    RowRegs<LPR, VPL> r;
    r.load(h + row * ld, sub, cpr, live);
    row_stats<LPR, VPL>(r, sub, width);
    r.store(y + row * ld_y, sub, cpr, live);
}

// dx = act'(h) * rstd * (dy - mean(dy) - y^ mean(dy y^)), the means over columns < width; ACT's derivative from the saved OUTPUT h
template <int LPR, int VPL, int ACT>
__global__ __launch_bounds__(256) void row_norm_bwd_kernel(const float *h, int64_t ld, const float *dy, int64_t ld_dy, int64_t n, int width,
                                                           int cpr, float *dx, int64_t ld_dx) {
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int sub = threadIdx.x % LPR;
    const bool live = row < n;
    RowRegs<LPR, VPL> a, yh, g;
    a.load(h + row * ld, sub, cpr, live);
    g.load(dy + row * ld_dy, sub, cpr, live);
    yh = a;
    const float rstd = row_stats<LPR, VPL>(yh, sub, width);
    row_norm_bwd<LPR, VPL>(g, yh, rstd, width, sub);
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) g.v[j][e] = 4 * (j * LPR + sub) + e < width ? act_bwd<ACT>(g.v[j][e], a.v[j][e]) : 0.f;
    g.store(dx + row * ld_dx, sub, cpr, live);
}

}  // namespace

int launch_row_norm_fwd(hipStream_t st, const float *h, int64_t ld, int64_t n, int width, int pout, float *y, int64_t ld_y, float *zeros, int zero_n) {
    if (n <= 0) return 0;
    if (int rc = norm_check("row_norm_fwd", h, ld, y, ld_y, zeros, ld, width, pout)) return rc;
    with_row_shape(pout, [&](auto L, auto V) {
        hipLaunchKernelGGL((row_norm_fwd_kernel<L.value, V.value>), row_grid<L.value>(n), dim3(256), 0, st, h, ld, n, width, pout / 4, y, ld_y, zeros, zero_n);
    });
    RLPPO_LAUNCH_CHECK();
    return 0;
}

int launch_row_norm_bwd(hipStream_t st, const float *h, int64_t ld, const float *dy, int64_t ld_dy, int64_t n, int width, int pout, int act,
                        float *dx, int64_t ld_dx) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(hidden_act_ok(act), "row_norm_bwd: act %d (0 = ReLU, 1 = tanh, 2 = ELU)", act);
    if (int rc = norm_check("row_norm_bwd", h, ld, dy, ld_dy, dx, ld_dx, width, pout)) return rc;
    with_hidden_act(act, [&](auto A) {
        with_row_shape(pout, [&](auto L, auto V) {
            hipLaunchKernelGGL((row_norm_bwd_kernel<L.value, V.value, A.value>), row_grid<L.value>(n), dim3(256), 0, st, h, ld, dy, ld_dy, n, width, pout / 4, dx,
                               ld_dx);
        });
    });
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo

using namespace rlppo;

extern "C" {

// the two launches on their own (the padded width is the library's: rlppo_padded_out(width))
int rlppo_row_norm_fwd(void *stream, const float *h, int64_t ld, int64_t n, int32_t width, float *y, int64_t ld_y) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && h && y && width >= 1, "row_norm_fwd: bad argument");
    return launch_row_norm_fwd((hipStream_t)stream, h, ld, n, width, (int)rlppo_padded_out(width), y, ld_y, nullptr, 0);
}
int rlppo_row_norm_bwd(void *stream, const float *h, int64_t ld, const float *dy, int64_t ld_dy, int64_t n, int32_t width, int32_t act, float *dx,
                       int64_t ld_dx) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && h && dy && dx && width >= 1, "row_norm_bwd: bad argument");
    return launch_row_norm_bwd((hipStream_t)stream, h, ld, dy, ld_dy, n, width, (int)rlppo_padded_out(width), act, dx, ld_dx);
}

}  // extern "C"
