// residual.hip -- the skip stream of residual hidden layers (common.hpp: HiddenSpec::res; include/rlppo.h, "[res]") as two row kernels between the
// products of a layer chain, beside norm.hip's and of the same design (norm_rows.hpp: a row in the registers of its 16 lanes or of a whole
// wave, 16-byte chunks interleaved over the lanes, shuffle butterflies in a fixed order, no LDS, no atomics, bit-reproducible; padded
// columns stored as exact zeros, rows at and beyond n neither read nor written).
//   row_res_fwd: s = s_prev + a and, under a norm, u = N(s) -- the unnormalised stream and the next layer's operand from ONE pass over
//                the registers: two reads and one or two writes of the matrix where an add and a separate normalisation would take three
//                reads and two writes.
//   row_res_bwd: everything of a hidden layer's backward that is not a product, in one launch: the normalisation's backward of the plain dX
//                product (statistics recomputed from the saved stream by row_stats, the forward's own sequence), plus the gradient
//                of the stream above, stored for the layer below, times the activation's derivative from its saved output.
#include "norm_rows.hpp"

namespace rlppo {

namespace {
// s may be s_prev.  zeros (optional): zero_n floats that workgroup 0 clears, as in row_norm_fwd
template <int LPR, int VPL, bool NORM>
__global__ __launch_bounds__(256) void row_res_fwd_kernel(const float *s_prev, int64_t ld_sp, const float *a, int64_t ld_a, int64_t n, int width,
                                                          int cpr, float *s, int64_t ld_s, float *u, int64_t ld_u, float *zeros, int zero_n) {
    if (zeros && blockIdx.x == 0)
        for (int i = threadIdx.x; i < zero_n; i += 256) zeros[i] = 0.f;
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int sub = threadIdx.x % LPR;
    const bool live = row < n;
    RowRegs<LPR, VPL> r, t;
    r.load(s_prev + row * ld_sp, sub, cpr, live);
    t.load(a + row * ld_a, sub, cpr, live);
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) r.v[j][e] = 4 * (j * LPR + sub) + e < width ? r.v[j][e] + t.v[j][e] : 0.f;
    r.store(s + row * ld_s, sub, cpr, live);
    if constexpr (NORM) {
        row_stats<LPR, VPL>(r, sub, width);
        r.store(u + row * ld_u, sub, cpr, live);
    }
}

// The whole non-GEMM part of a residual hidden layer's backward: g = (NORM ? the normalisation's backward of p at the saved stream s : p)
// + g_next (the gradient of the stream above; null for the last hidden layer), stored unless g_out is null (layer 0), and
// dz = g * act'(a) from the saved activation OUTPUT a.  Every load of a lane comes before its first store: dz may be p.
template <int LPR, int VPL, int ACT, bool NORM>
__global__ __launch_bounds__(256) void row_res_bwd_kernel(const float *a, int64_t ld_a, const float *s, int64_t ld_s, const float *p, int64_t ld_p,
                                                          const float *g_next, int64_t ld_gn, int64_t n, int width, int cpr, float *g_out,
                                                          int64_t ld_g, float *dz, int64_t ld_dz) {
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int sub = threadIdx.x % LPR;
    const bool live = row < n;
    RowRegs<LPR, VPL> av, g;
    av.load(a + row * ld_a, sub, cpr, live);
    g.load(p + row * ld_p, sub, cpr, live);
    if constexpr (NORM) {
        RowRegs<LPR, VPL> yh;
        yh.load(s + row * ld_s, sub, cpr, live);
        const float rstd = row_stats<LPR, VPL>(yh, sub, width);
        row_norm_bwd<LPR, VPL>(g, yh, rstd, width, sub);
    }
    if (g_next) {  // (the same for every lane of the launch)
        RowRegs<LPR, VPL> t;
        t.load(g_next + row * ld_gn, sub, cpr, live);
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) g.v[j][e] += t.v[j][e];
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) g.v[j][e] = 4 * (j * LPR + sub) + e < width ? g.v[j][e] : 0.f;
    if (g_out) g.store(g_out + row * ld_g, sub, cpr, live);
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) g.v[j][e] = 4 * (j * LPR + sub) + e < width ? act_bwd<ACT>(g.v[j][e], av.v[j][e]) : 0.f;
    g.store(dz + row * ld_dz, sub, cpr, live);
}

}  // namespace

int launch_row_res_fwd(hipStream_t st, const float *s_prev, int64_t ld_sp, const float *a, int64_t ld_a, int64_t n, int width, int pout, int norm,
                       float *s, int64_t ld_s, float *u, int64_t ld_u, float *zeros, int zero_n) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(s_prev && a && s && (!norm || u), "row_res_fwd: null matrix");
    if (int rc = norm_check("row_res_fwd", s_prev, ld_sp, a, ld_a, s, ld_s, width, pout)) return rc;
    if (norm)
        if (int rc = norm_check("row_res_fwd", u, ld_u, u, ld_u, u, ld_u, width, pout)) return rc;
    RLPPO_CHECK_ARG((reinterpret_cast<uintptr_t>(zeros) & 3) == 0, "row_res_fwd: the zero row must be a float pointer");
    with_row_shape(pout, [&](auto L, auto V) {
        const dim3 grid = row_grid<L.value>(n);
        if (norm)
            hipLaunchKernelGGL((row_res_fwd_kernel<L.value, V.value, true>), grid, dim3(256), 0, st, s_prev, ld_sp, a, ld_a, n, width, pout / 4, s, ld_s, u, ld_u,
                               zeros, zero_n);
        else
            hipLaunchKernelGGL((row_res_fwd_kernel<L.value, V.value, false>), grid, dim3(256), 0, st, s_prev, ld_sp, a, ld_a, n, width, pout / 4, s, ld_s, nullptr,
                               0, zeros, zero_n);
    });
    RLPPO_LAUNCH_CHECK();
    return 0;
}

int launch_row_res_bwd(hipStream_t st, const float *a, int64_t ld_a, const float *s, int64_t ld_s, const float *p, int64_t ld_p, const float *g_next,
                       int64_t ld_gn, int64_t n, int width, int pout, int act, int norm, float *g, int64_t ld_g, float *dz, int64_t ld_dz) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(hidden_act_ok(act), "row_res_bwd: act %d (0 = ReLU, 1 = tanh, 2 = ELU)", act);
    RLPPO_CHECK_ARG(a && p && dz && (!norm || s), "row_res_bwd: null matrix");
    if (int rc = norm_check("row_res_bwd", a, ld_a, p, ld_p, dz, ld_dz, width, pout)) return rc;
    if (int rc = norm_check("row_res_bwd", norm ? s : a, norm ? ld_s : ld_a, g_next ? g_next : a, g_next ? ld_gn : ld_a, g ? g : dz, g ? ld_g : ld_dz,
                            width, pout))
        return rc;
    if (!norm) s = nullptr;
    with_hidden_act(act, [&](auto A) {
        with_row_shape(pout, [&](auto L, auto V) {
            const dim3 grid = row_grid<L.value>(n);
            if (norm)
                hipLaunchKernelGGL((row_res_bwd_kernel<L.value, V.value, A.value, true>), grid, dim3(256), 0, st, a, ld_a, s, ld_s, p, ld_p, g_next, ld_gn, n, width,
                                   pout / 4, g, ld_g, dz, ld_dz);
            else
                hipLaunchKernelGGL((row_res_bwd_kernel<L.value, V.value, A.value, false>), grid, dim3(256), 0, st, a, ld_a, s, ld_s, p, ld_p, g_next, ld_gn, n, width,
                                   pout / 4, g, ld_g, dz, ld_dz);
        });
    });
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo

using namespace rlppo;

extern "C" {

// [res] the two launches of the residual stream on their own (norm != 0: with the normalisation; u / s may be NULL without it)
int rlppo_row_res_fwd(void *stream, const float *s_prev, int64_t ld_sp, const float *a, int64_t ld_a, int64_t n, int32_t width, int32_t norm, float *s,
                      int64_t ld_s, float *u, int64_t ld_u) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && s_prev && a && s && (!norm || u) && width >= 1, "row_res_fwd: bad argument");
    return launch_row_res_fwd((hipStream_t)stream, s_prev, ld_sp, a, ld_a, n, width, (int)rlppo_padded_out(width), norm != 0, s, ld_s, u, ld_u, nullptr, 0);
}
int rlppo_row_res_bwd(void *stream, const float *a, int64_t ld_a, const float *s, int64_t ld_s, const float *p, int64_t ld_p, const float *g_next,
                      int64_t ld_gn, int64_t n, int32_t width, int32_t act, int32_t norm, float *g, int64_t ld_g, float *dz, int64_t ld_dz) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && a && p && dz && (!norm || s) && width >= 1, "row_res_bwd: bad argument");
    return launch_row_res_bwd((hipStream_t)stream, a, ld_a, s, ld_s, p, ld_p, g_next, ld_gn, n, width, (int)rlppo_padded_out(width), act, norm != 0, g,
                              ld_g, dz, ld_dz);
}

}  // extern "C"
