// norm_rows.hpp -- what the row kernels of norm.hip (layer normalisation) and residual.hip (the residual stream) share: a row in the registers of
// the lanes that own it, the fixed-order sums over those lanes, the statistics of a row, the normalisation's backward, the activation's
// derivative, the launch shape of a padded width and the argument checks.  One definition each: both files run the same instruction
// sequences (norm.hip's header describes the design).
#pragma once
#include <type_traits>

#include "common.hpp"

namespace rlppo {
namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float NORM_EPS = 1e-5f;

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {  // the sum over the LPR lanes of a row, in every one of them
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// A lane's share of one row: chunk j of the lane is columns 4 (j LPR + lane_in_row) .. + 3
template <int LPR, int VPL>
struct RowRegs {
    f32x4 v[VPL];
    __device__ __forceinline__ void load(const float *row, int sub, int cpr, bool live) {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = j * LPR + sub;
            v[j] = live && c < cpr ? *reinterpret_cast<const f32x4 *>(row + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __device__ __forceinline__ void store(float *row, int sub, int cpr, bool live) const {
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int c = j * LPR + sub;
            if (live && c < cpr) *reinterpret_cast<f32x4 *>(row + 4 * c) = v[j];
        }
    }
};

// mean and 1 / sqrt(var + eps) of the row whose share `h` is, over columns < width; on return h holds y^ = (h - mean) * rstd in
// the valid columns and 0 in the others.  The forward's result and the backward's recomputation are this one sequence.
template <int LPR, int VPL>
__device__ __forceinline__ float row_stats(RowRegs<LPR, VPL> &h, int sub, int width) {
    const float inv_w = 1.f / (float)width;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += 4 * (j * LPR + sub) + e < width ? h.v[j][e] : 0.f;
    const float mu0 = group_sum<LPR>(s) * inv_w;
    s = 0.f;  // the mean of the centred values: what rounding left of the mean (zero for a row that fp32 sums exactly)
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += 4 * (j * LPR + sub) + e < width ? h.v[j][e] - mu0 : 0.f;
    const float mu = mu0 + group_sum<LPR>(s) * inv_w;
    s = 0.f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = 4 * (j * LPR + sub) + e < width ? h.v[j][e] - mu : 0.f;
            h.v[j][e] = d;
            s += d * d;
        }
    const float rstd = 1.f / sqrtf(group_sum<LPR>(s) * inv_w + NORM_EPS);
#pragma unroll
    for (int j = 0; j < VPL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) h.v[j][e] *= rstd;
    return rstd;
}

// The normalisation's backward on a row: g (the gradient of y^, cleared beyond width on the way) becomes
// rstd * (g - mean(g) - y^ mean(g y^)), the means over columns < width; yh and rstd are row_stats' of the same row
template <int LPR, int VPL>
__device__ __forceinline__ void row_norm_bwd(RowRegs<LPR, VPL> &g, const RowRegs<LPR, VPL> &yh, float rstd, int width, int sub) {
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

// g times the derivative of the hidden activation ACT (HiddenAct), from the activation's saved OUTPUT h
template <int ACT>
__device__ __forceinline__ float act_bwd(float g, float h) {
    if constexpr (ACT == ACT_TANH) return g * (1.f - h * h);
    else if constexpr (ACT == ACT_ELU) return g * (h > 0.f ? 1.f : h + 1.f);
    else return h > 0.f ? g : 0.f;
}

// The launch shape of a padded width (a multiple of 32 up to RLPPO_NORM_MAX_WIDTH): LPR lanes per row (16 up to 128 columns, the whole
// wave beyond) and VPL 16-byte chunks per lane.  f(Int<LPR>, Int<VPL>) launches the caller's kernel of that shape on row_grid<LPR>(n):
// every launcher of norm.hip and residual.hip selects its instantiation here.
template <int N>
using Int = std::integral_constant<int, N>;
template <class F>
inline void with_row_shape(int pout, F &&f) {
    if (pout <= 64) f(Int<16>{}, Int<1>{});
    else if (pout <= 128) f(Int<16>{}, Int<2>{});
    else if (pout <= 256) f(Int<64>{}, Int<1>{});
    else if (pout <= 512) f(Int<64>{}, Int<2>{});
    else if (pout <= 1024) f(Int<64>{}, Int<4>{});
    else f(Int<64>{}, Int<8>{});
}
template <int LPR>
inline dim3 row_grid(int64_t n) { return dim3((unsigned)cdiv(n, 256 / LPR)); }
// ... and f(Int<ACT>) the instantiation of a hidden activation (hidden_act_ok holds)
template <class F>
inline void with_hidden_act(int act, F &&f) {
    if (act == ACT_TANH) f(Int<ACT_TANH>{});
    else if (act == ACT_ELU) f(Int<ACT_ELU>{});
    else f(Int<ACT_RELU>{});
}
inline int norm_check(const char *who, const void *a, int64_t lda, const void *b, int64_t ldb, const void *c, int64_t ldc, int width, int pout) {
    RLPPO_CHECK_ARG(width >= 1 && width <= pout && pout % 4 == 0, "%s: width=%d, padded width=%d", who, width, pout);
    RLPPO_CHECK_ARG(pout <= RLPPO_NORM_MAX_WIDTH, "%s: padded width %d: the row kernels hold a row of up to RLPPO_NORM_MAX_WIDTH = %d floats in registers",
                    who, pout, RLPPO_NORM_MAX_WIDTH);
    RLPPO_CHECK_ARG(lda >= pout && ldb >= pout && ldc >= pout && lda % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0,
                    "%s: leading dimensions %ld / %ld / %ld must be multiples of 4, at least the padded width %d", who, (long)lda, (long)ldb, (long)ldc, pout);
    RLPPO_CHECK_ARG(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0,
                    "%s: the matrices must be 16-byte aligned", who);
    return 0;
}
}  // namespace
}  // namespace rlppo
