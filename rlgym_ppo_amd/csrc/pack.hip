// pack.hip -- the kernels' weight copies: the flat parameter arena -> tile-padded W / W^T / b per layer (fp32, and the bf16 image of
// the bf16 update precision), and the fp32 <-> bf16 hand-over of activation rows between layers that take different kernels.
#include "common.hpp"

namespace rlppo {

void fill_jobs(const NetLayout &net, PackJobs *jobs) {
    jobs->n = net.n_layers;
    int64_t tot = 0;
    for (int l = 0; l < net.n_layers; ++l) {
        const LayerLayout &L = net.L[l];
        jobs->j[l] = PackJob{L.in, L.out, L.pin, L.pout, L.off_w, L.off_wt, L.off_b, L.off_flat_w, L.off_flat_b, tot};
        tot += (int64_t)L.pin * L.pout;
    }
    jobs->total = tot;
}
static int pack_blocks(const PackJobs &jobs) { return (int)(cdiv(jobs.total, 256) < 2048 ? cdiv(jobs.total, 256) : 2048); }

// one work item per element of the padded W (pout*pin); the same thread also writes W^T and (row 0 items) b
__global__ __launch_bounds__(256) void pack_kernel(const float *__restrict__ flat, float *__restrict__ packed, PackJobs jobs) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < jobs.total; g += (int64_t)gridDim.x * blockDim.x) {
        int l = 0;
        while (l + 1 < jobs.n && g >= jobs.j[l + 1].first) ++l;
        const PackJob &J = jobs.j[l];
        const int64_t e = g - J.first;
        const int o = (int)(e / J.pin), i = (int)(e % J.pin);
        const float w = (o < J.out && i < J.in) ? flat[J.off_flat_w + (int64_t)o * J.in + i] : 0.f;
        packed[J.off_w + (int64_t)o * J.pin + i] = w;
        packed[J.off_wt + (int64_t)i * J.pout + o] = w;
        if (i == 0) packed[J.off_b + o] = o < J.out ? flat[J.off_flat_b + o] : 0.f;
    }
}

int launch_pack(hipStream_t st, const NetLayout &net, const float *flat, float *packed) {
    PackJobs jobs;
    fill_jobs(net, &jobs);
    hipLaunchKernelGGL(pack_kernel, dim3(pack_blocks(jobs)), dim3(256), 0, st, flat, packed, jobs);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// bf16 update precision: the fp32 master copy rounded to bf16 (round-to-nearest-even), once per optimiser step:
//   packed_r -- the packed image (W | W^T | b per layer) holding the ROUNDED weights as fp32 (the fp32 dX product and the
//               critic's matrix-vector head then multiply exactly what the bf16 forward multiplied); biases stay fp32;
//   wb16     -- the W[Pout][Pin] blocks alone as bf16, layer after layer (the B operand of the forward gemm_nt_b16_kernel),
//               followed by the W^T[Pin][Pout] blocks in the same order (the B operand of its dX form).
__global__ __launch_bounds__(256) void pack_bf16_kernel(const float *__restrict__ flat, float *__restrict__ packed_r,
                                                        unsigned short *__restrict__ wb16, PackJobs jobs) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < jobs.total; g += (int64_t)gridDim.x * blockDim.x) {
        int l = 0;
        while (l + 1 < jobs.n && g >= jobs.j[l + 1].first) ++l;
        const PackJob &J = jobs.j[l];
        const int64_t e = g - J.first;
        const int o = (int)(e / J.pin), i = (int)(e % J.pin);
        const float w = (o < J.out && i < J.in) ? flat[J.off_flat_w + (int64_t)o * J.in + i] : 0.f;
        const unsigned short h = bf16_bits(w);
        const float wr = __uint_as_float((unsigned)h << 16);
        packed_r[J.off_w + (int64_t)o * J.pin + i] = wr;
        packed_r[J.off_wt + (int64_t)i * J.pout + o] = wr;
        wb16[J.first + e] = h;  // J.first = sum of the previous layers' Pout * Pin
        wb16[jobs.total + J.first + (int64_t)i * J.pout + o] = h;
        if (i == 0) packed_r[J.off_b + o] = o < J.out ? flat[J.off_flat_b + o] : 0.f;
    }
}

int launch_pack_bf16(hipStream_t st, const NetLayout &net, const float *flat, float *packed_r, unsigned short *wb16) {
    PackJobs jobs;
    fill_jobs(net, &jobs);
    hipLaunchKernelGGL(pack_bf16_kernel, dim3(pack_blocks(jobs)), dim3(256), 0, st, flat, packed_r, wb16, jobs);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// x[r][0..width) -> rounded to bf16 in place (as fp32) + the bf16 copy xb[r][0..width): the hand-over of a layer that took the
// fp32 kernels in the bf16 update precision (shapes gemm_nt_b16_kernel does not cover).  4 elements per thread.
__global__ __launch_bounds__(256) void round_rows_kernel(float *__restrict__ x, unsigned short *__restrict__ xb, int64_t n4) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = reinterpret_cast<f32x4 *>(x)[g];
        u16x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float f = v[e];
            h[e] = bf16_bits(f);
            v[e] = __uint_as_float((unsigned)h[e] << 16);
        }
        reinterpret_cast<f32x4 *>(x)[g] = v;
        reinterpret_cast<u16x4 *>(xb)[g] = h;
    }
}

int launch_round_rows(hipStream_t st, float *x, unsigned short *xb, int64_t n_elems) {
    if (n_elems <= 0) return 0;
    RLPPO_CHECK_ARG(n_elems % 4 == 0, "round_rows: element count %ld is not a multiple of 4", (long)n_elems);
    const int64_t n4 = n_elems / 4;
    const int blocks = (int)(cdiv(n4, 256) < 8192 ? cdiv(n4, 256) : 8192);
    hipLaunchKernelGGL(round_rows_kernel, dim3(blocks), dim3(256), 0, st, x, xb, n4);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// xb (bf16) -> x (the same values as fp32): the hand-over from a bf16-in-memory kernel to a layer that takes the fp32 kernels.
__global__ __launch_bounds__(256) void expand_rows_kernel(const unsigned short *__restrict__ xb, float *__restrict__ x, int64_t n4) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += (int64_t)gridDim.x * blockDim.x) {
        const u16x4 h = reinterpret_cast<const u16x4 *>(xb)[g];
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __uint_as_float((unsigned)h[e] << 16);
        reinterpret_cast<f32x4 *>(x)[g] = v;
    }
}

int launch_expand_rows(hipStream_t st, const unsigned short *xb, float *x, int64_t n_elems) {
    if (n_elems <= 0) return 0;
    RLPPO_CHECK_ARG(n_elems % 4 == 0, "expand_rows: element count %ld is not a multiple of 4", (long)n_elems);
    const int64_t n4 = n_elems / 4;
    const int blocks = (int)(cdiv(n4, 256) < 8192 ? cdiv(n4, 256) : 8192);
    hipLaunchKernelGGL(expand_rows_kernel, dim3(blocks), dim3(256), 0, st, xb, x, n4);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo
