// norm_rows.hpp -- what the row kernels of norm.hip (layer normalisation) and residual.hip (the residual stream) share: a row in the registers of
// the lanes that own it, the fixed-order sums over those lanes, the statistics of a row, the launch shape of a padded width and the
// argument checks.  One definition each: both files run the same instruction sequences (norm.hip's header describes the design).
#pragma once
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

// lanes per row and 16-byte chunks per lane of a padded width (a multiple of 32 up to RLPPO_NORM_MAX_WIDTH)
struct NormShape {
    int lpr, vpl;
};
inline NormShape norm_shape(int pout) {
    if (pout <= 64) return {16, 1};
    if (pout <= 128) return {16, 2};
    const int v = (int)cdiv(pout, 256);
    return {64, v <= 1 ? 1 : v <= 2 ? 2 : v <= 4 ? 4 : 8};
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
