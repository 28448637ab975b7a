// row_layout.hpp -- how a row of logits lies over the lanes of a wave, and the block-level accumulation of the report statistics: the
// pieces the row kernels of heads.hip (the policy heads) and value_bins.hip (the categorical critic) are written against.
#pragma once
#include "common.hpp"

namespace rlppo {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- 16 lanes per row: the reductions are 4 DPP steps inside a 16-lane row instead of 6 cross-lane shuffles of a whole wave
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// all-reduce over a 16-lane DPP row: xor 1, xor 2 (quad_perm), then half-row mirror and row mirror (every lane of a quad /
// half row already holds the same partial, so a mirror is as good as an xor)
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    return v;
}

// ------------------------------------------------------------------------------------------ row layouts
// How a discrete row lies over lanes.  The sampling, probability and loss kernels are written once against a layout, which supplies:
// EPL elements per lane and ROWS rows per block, the row a lane works on (`group`) and the lane that reports for it (`writer`), the
// column of element e, the row-wide sum and max, the load and store of a lane's logits, the valid actions of a row as bit e per
// element, and SHADOW: whether the idle groups of a block's last pass run along on the last row (storing nothing) or leave.
// A kernel's `in(e)` is "element e takes part": col(e) < A, or [ABI 8] its bit of valid_bits.

// One wave per row, 4 rows per block: lane l holds the EPL strided columns l + 64 e (any width up to 64 EPL).
template <int EPL_>
struct WaveRow {
    static constexpr int EPL = EPL_, ROWS = 4;
    static constexpr bool SHADOW = false;
    const int lane = threadIdx.x & 63, group = threadIdx.x >> 6;
    __device__ __forceinline__ bool writer() const { return lane == 0; }
    __device__ __forceinline__ int col(int e) const { return lane + 64 * e; }
    __device__ __forceinline__ static float sum(float v) { return wave_sum(v); }
    __device__ __forceinline__ static float max(float v) { return wave_max(v); }
    template <class In>
    __device__ __forceinline__ void load(const float *__restrict__ z, int64_t, float (&p)[EPL], In in) const {
#pragma unroll
        for (int e = 0; e < EPL; ++e) p[e] = in(e) ? z[col(e)] : -INFINITY;
    }
    __device__ __forceinline__ void store(float *__restrict__ z, int64_t ld, const float (&g)[EPL]) const {
#pragma unroll
        for (int e = 0; e < EPL; ++e)
            if (col(e) < ld) z[col(e)] = g[e];
    }
    // [ABI 8] element c = lane + 64 e sits in word c / 32 = (lane >> 5) + 2 e at bit lane & 31.  A row without a valid action is
    // all-valid (wave-uniform decision).
    __device__ __forceinline__ unsigned valid_bits(const unsigned *__restrict__ words, int A) const {
        unsigned bits = 0, in_row = 0;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            if (col(e) < A) {
                in_row |= 1u << e;
                bits |= ((words[(lane >> 5) + 2 * e] >> (lane & 31)) & 1u) << e;
            }
        }
        return __ballot(bits != 0) ? bits : in_row;
    }
};

// 16 lanes per row, 16 rows per block (padded width <= 128): a wave works on 4 rows at once and lane l of a row holds the 8
// CONSECUTIVE columns 8 l .. 8 l + 7, two 16-byte loads / stores.  The padded width is a multiple of 32, so a lane's 8 columns are
// all inside the row or all outside.  Only the summation order inside a row differs from WaveRow.
struct Lanes16 {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    static constexpr int EPL = 8, ROWS = 16;
    static constexpr bool SHADOW = true;
    const int l16 = threadIdx.x & 15, group = threadIdx.x >> 4;
    __device__ __forceinline__ bool writer() const { return l16 == 0; }
    __device__ __forceinline__ int col(int e) const { return l16 * 8 + e; }
    __device__ __forceinline__ static float sum(float v) { return row16_sum(v); }
    __device__ __forceinline__ static float max(float v) { return row16_max(v); }
    template <class In>
    __device__ __forceinline__ void load(const float *__restrict__ z, int64_t ld, float (&p)[8], In in) const {
        if (col(0) < ld) {
            const f32x4 z0 = *reinterpret_cast<const f32x4 *>(z + col(0)), z1 = *reinterpret_cast<const f32x4 *>(z + col(4));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                p[e] = z0[e];
                p[4 + e] = z1[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (!in(e)) p[e] = -INFINITY;
    }
    __device__ __forceinline__ void store(float *__restrict__ z, int64_t ld, const float (&g)[8]) const {
        if (col(0) < ld) {
            *reinterpret_cast<f32x4 *>(z + col(0)) = f32x4{g[0], g[1], g[2], g[3]};
            *reinterpret_cast<f32x4 *>(z + col(4)) = f32x4{g[4], g[5], g[6], g[7]};
        }
    }
    // [ABI 8] a lane's 8 consecutive actions are exactly byte l16 of the row's mask words (little-endian bit order)
    __device__ __forceinline__ unsigned valid_bits(const unsigned *__restrict__ words, int A) const {
        const int c0 = col(0);
        const unsigned in_bits = c0 + 8 <= A ? 0xffu : (c0 < A ? (1u << (A - c0)) - 1u : 0u);
        unsigned valid = 0;
        if (in_bits)  // (c0 < A: byte l16 lies inside the row's W = ceil(A / 32) words)
            valid = reinterpret_cast<const unsigned char *>(words)[l16] & in_bits;
        return row16_max(valid ? 1.f : 0.f) > 0.f ? valid : in_bits;  // a row without a valid action: all-valid
    }
};

// block-level accumulation of per-row statistics into the double accumulators.  [ABI 7] kl_slots (the policy loss launches of an
// armed pass): the workgroup's KL sum -- the value it adds to stats[KL] -- also lands in slot 2 + blockIdx.x, fixed for a given
// grid, so rlppo_kl_gate adds the same numbers in the same order every run; a set stop word keeps the launch out of the report.
__device__ __forceinline__ void block_stats_add(double *stats, const float (&v)[5], bool active, const LossCfg &c,
                                                double *kl_slots = nullptr) {
    __shared__ float red[5][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        float x = wave_sum(active ? v[k] : 0.f);
        if (lane == 0) red[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int k = threadIdx.x;
        const double s = (double)red[k][0] + (double)red[k][1] + (double)red[k][2] + (double)red[k][3];
        if (k == RLPPO_STAT_KL && kl_slots) {
            kl_slots[2 + blockIdx.x] = s;
            if (blockIdx.x == 0) {
                kl_slots[0] = (double)gridDim.x;
                kl_slots[1] = (double)c.mb_ratio;
            }
        }
        if (!(c.stop_word && *c.stop_word)) atomicAdd(stats + k, s);
    }
}

}  // namespace rlppo
