// reduce.hpp -- the reduction steps the parameter-side kernels (optim.hip, stats.hip) share, each written once: the sum of a
// 256-thread workgroup in double, and the ticketed sum of a pair of doubles over the workgroups of a launch.  Every order of
// additions here is fixed, so a result that goes through these helpers alone is the same bits every run.
#pragma once
#include "common.hpp"

namespace rlppo {

// How the four waves' sums meet.  The two differ in the last bit, and results are pinned to each: the kernels that add their
// workgroup's sum to an atomic accumulator (sqnorm_kernel, sqnorm2_kernel) have always combined left to right, every other pairwise.
enum class Combine { Pairwise, LeftToRight };

// v[0 .. N) summed over the 256 threads of the workgroup; the result is valid in THREAD 0 only.  Per value: the shuffle tree of a
// 64-lane wave (lane l + lane l ^ 32, then ^ 16, ...), one LDS word per wave, the combine.  Every thread of the workgroup calls it.
// A workgroup that calls it twice needs a __syncthreads() between thread 0's use of the first result and the second call.
template <int N, Combine C = Combine::Pairwise>
__device__ __forceinline__ void block_sum_256(double (&v)[N]) {
    __shared__ double red[4][N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v[k] += __shfl_xor(v[k], s);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < N; ++k)
        v[k] = C == Combine::Pairwise ? (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]) : red[0][k] + red[1][k] + red[2][k] + red[3][k];
}
template <Combine C = Combine::Pairwise>
__device__ __forceinline__ double block_sum_256(double x) {
    double v[1] = {x};
    block_sum_256<1, C>(v);
    return v[0];
}

// The workspace of a ticketed sum, `BLOCKS` the launch's largest grid.  The caller's memory: zeroed once by its owner, every
// completed launch leaves it armed (include/rlppo.h: tickets at byte 0, the slots from byte 16).
template <int BLOCKS>
struct TicketWs {
    unsigned tickets;
    unsigned pad[3];
    double partial[BLOCKS][2];
};

// The sum of s[0], s[1] over every thread of the launch (gridDim.x <= BLOCKS workgroups of 256 threads), without floating-point
// atomics: each workgroup parks its pair in its slot of `ws` and takes a ticket; the threads of the LAST arriver fetch the slots
// side by side (one thread walking 128 dependent loads took 19 of learn_report_kernel's 24 us) and its thread 0 adds them in slot
// order.  This is the only place these kernels synchronise across workgroups.
//
// ticket_pair_sum_together keeps the last arriver whole: it returns true in EVERY thread of the last-arriving workgroup (uniformly:
// a __syncthreads() behind it is legal) and false in every thread of every other; the totals are in s[] of its thread 0 alone.  For an
// epilogue with work for 256 threads (value_norm_update_popart_kernel's rescale); thread 0 ends with ticket_rearm(ws).
template <int BLOCKS>
__device__ __forceinline__ bool ticket_pair_sum_together(double (&s)[2], TicketWs<BLOCKS> *ws) {
    __shared__ int last;
    __shared__ double slots[BLOCKS][2];
    block_sum_256(s);
    if (threadIdx.x == 0) {
        ws->partial[blockIdx.x][0] = s[0];
        ws->partial[blockIdx.x][1] = s[1];
        __threadfence();
        last = atomicAdd(&ws->tickets, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return false;
    __threadfence();
    if (threadIdx.x < 2 * gridDim.x)
        slots[threadIdx.x >> 1][threadIdx.x & 1] = __hip_atomic_load(&ws->partial[threadIdx.x >> 1][threadIdx.x & 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x != 0) return true;
    s[0] = s[1] = 0.0;
    for (unsigned b = 0; b < gridDim.x; ++b) {
        s[0] += slots[b][0];
        s[1] += slots[b][1];
    }
    return true;
}
// ... and the form of an epilogue of one thread: true in thread 0 of the last-arriving workgroup ONLY, with the totals in s[]; every
// other thread is done (false).  That thread writes its outputs and ends with ticket_rearm(ws).
template <int BLOCKS>
__device__ __forceinline__ bool ticket_pair_sum(double (&s)[2], TicketWs<BLOCKS> *ws) {
    return ticket_pair_sum_together(s, ws) && threadIdx.x == 0;
}
template <int BLOCKS>
__device__ __forceinline__ void ticket_rearm(TicketWs<BLOCKS> *ws) {
    __hip_atomic_store(&ws->tickets, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace rlppo
