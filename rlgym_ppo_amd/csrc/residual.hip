// residual.hip -- the skip stream of residual hidden layers (chain.hip: hidden_res; include/rlppo.h, "[res]") as two row kernels between the
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
        const float inv_w = 1.f / (float)width;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = 4 * (j * LPR + sub) + e < width ? g.v[j][e] : 0.f;
                g.v[j][e] = d;
                s1 += d;
                s2 += d * yh.v[j][e];
            }
        const float m1 = group_sum<LPR>(s1) * inv_w, m2 = group_sum<LPR>(s2) * inv_w;
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) g.v[j][e] = rstd * ((g.v[j][e] - m1) - yh.v[j][e] * m2);
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
        for (int e = 0; e < 4; ++e) {
            const float hv = av.v[j][e], gv = g.v[j][e];
            float o;
            if constexpr (ACT == ACT_TANH) o = gv * (1.f - hv * hv);
            else if constexpr (ACT == ACT_ELU) o = gv * (hv > 0.f ? 1.f : hv + 1.f);
            else o = hv > 0.f ? gv : 0.f;
            g.v[j][e] = 4 * (j * LPR + sub) + e < width ? o : 0.f;
        }
    g.store(dz + row * ld_dz, sub, cpr, live);
}

}  // namespace

// ---- [res]
int res_net_check(const char *who, const NetLayout &net) {
    RLPPO_CHECK_ARG(norm_width_ok(net), "%s: residual hidden layers (RLPPO_ACT_RES) of a layer wider than RLPPO_NORM_MAX_WIDTH = %d (padded): the row "
                    "kernels hold a row of the stream in registers", who, RLPPO_NORM_MAX_WIDTH);
    for (int l = 1; l + 1 < net.n_layers; ++l)
        RLPPO_CHECK_ARG(net.L[l].out == net.L[0].out, "%s: residual hidden layers (RLPPO_ACT_RES) need equal hidden widths: hidden layer %d has %d "
                        "outputs, hidden layer 0 has %d", who, l, net.L[l].out, net.L[0].out);
    return 0;
}

template <bool NORM>
static void launch_res_fwd(hipStream_t st, const NormShape sh, dim3 grid, const float *s_prev, int64_t ld_sp, const float *a, int64_t ld_a, int64_t n,
                           int width, int cpr, float *s, int64_t ld_s, float *u, int64_t ld_u, float *zeros, int zero_n) {
#define FWD(L, V) \
    hipLaunchKernelGGL((row_res_fwd_kernel<L, V, NORM>), grid, dim3(256), 0, st, s_prev, ld_sp, a, ld_a, n, width, cpr, s, ld_s, u, ld_u, zeros, zero_n)
    if (sh.lpr == 16) {
        if (sh.vpl == 1) FWD(16, 1); else FWD(16, 2);
    } else if (sh.vpl == 1) FWD(64, 1);
    else if (sh.vpl == 2) FWD(64, 2);
    else if (sh.vpl == 4) FWD(64, 4);
    else FWD(64, 8);
#undef FWD
}

int launch_row_res_fwd(hipStream_t st, const float *s_prev, int64_t ld_sp, const float *a, int64_t ld_a, int64_t n, int width, int pout, int norm,
                       float *s, int64_t ld_s, float *u, int64_t ld_u, float *zeros, int zero_n) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(s_prev && a && s && (!norm || u), "row_res_fwd: null matrix");
    if (int rc = norm_check("row_res_fwd", s_prev, ld_sp, a, ld_a, s, ld_s, width, pout)) return rc;
    if (norm)
        if (int rc = norm_check("row_res_fwd", u, ld_u, u, ld_u, u, ld_u, width, pout)) return rc;
    RLPPO_CHECK_ARG((reinterpret_cast<uintptr_t>(zeros) & 3) == 0, "row_res_fwd: the zero row must be a float pointer");
    const NormShape sh = norm_shape(pout);
    const dim3 grid((unsigned)cdiv(n, 256 / sh.lpr));
    if (norm) launch_res_fwd<true>(st, sh, grid, s_prev, ld_sp, a, ld_a, n, width, pout / 4, s, ld_s, u, ld_u, zeros, zero_n);
    else launch_res_fwd<false>(st, sh, grid, s_prev, ld_sp, a, ld_a, n, width, pout / 4, s, ld_s, nullptr, 0, zeros, zero_n);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

struct ResBwdArgs {
    const float *a, *s, *p, *g_next;
    int64_t ld_a, ld_s, ld_p, ld_gn, n;
    int width, cpr;
    float *g, *dz;
    int64_t ld_g, ld_dz;
};
template <int ACT, bool NORM>
static void launch_res_bwd(hipStream_t st, const NormShape sh, dim3 grid, const ResBwdArgs &q) {
#define BWD(L, V)                                                                                                                                  \
    hipLaunchKernelGGL((row_res_bwd_kernel<L, V, ACT, NORM>), grid, dim3(256), 0, st, q.a, q.ld_a, q.s, q.ld_s, q.p, q.ld_p, q.g_next, q.ld_gn, q.n, \
                       q.width, q.cpr, q.g, q.ld_g, q.dz, q.ld_dz)
    if (sh.lpr == 16) {
        if (sh.vpl == 1) BWD(16, 1); else BWD(16, 2);
    } else if (sh.vpl == 1) BWD(64, 1);
    else if (sh.vpl == 2) BWD(64, 2);
    else if (sh.vpl == 4) BWD(64, 4);
    else BWD(64, 8);
#undef BWD
}
template <int ACT>
static void launch_res_bwd(hipStream_t st, const NormShape sh, dim3 grid, const ResBwdArgs &q, int norm) {
    if (norm) launch_res_bwd<ACT, true>(st, sh, grid, q);
    else launch_res_bwd<ACT, false>(st, sh, grid, q);
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
    const NormShape sh = norm_shape(pout);
    const dim3 grid((unsigned)cdiv(n, 256 / sh.lpr));
    const ResBwdArgs q{a, norm ? s : nullptr, p, g_next, ld_a, ld_s, ld_p, ld_gn, n, width, pout / 4, g, dz, ld_g, ld_dz};
    if (act == ACT_TANH) launch_res_bwd<ACT_TANH>(st, sh, grid, q, norm);
    else if (act == ACT_ELU) launch_res_bwd<ACT_ELU>(st, sh, grid, q, norm);
    else launch_res_bwd<ACT_RELU>(st, sh, grid, q, norm);
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
