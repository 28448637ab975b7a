// rows.hip -- staging rows of observations and experience for the GEMM kernels: padding raw observations to the tile width (with the
// reference's standardisation), gathering a minibatch's rows and per-row scalars, the running observation statistics (Welford
// increment and merge), and the action indices as floats.
#include "common.hpp"

namespace rlppo {

// --------------------------------------------------------------------------------------------- pad rows
// dst[r][c] = stats(src[r][c], c) for c < d, 0 in the padding columns.  `Stats` is the standardisation of column c:
//   ScalarStats   np.clip((obs - mean) / std, -5, 5) with the float32 scalars of feature 0 for every feature
//                 (batched_agent_manager.py:313-315; quirk Q5), or the plain copy;
//   FeatureStats  the same with PER-FEATURE statistics, the form the reference's obs_stats were meant for, behind a flag.
struct ScalarStats {
    int standardize;
    float mean0, std0;
    __device__ __forceinline__ float operator()(float v, int64_t) const { return standardize ? fminf(fmaxf((v - mean0) / std0, -5.f), 5.f) : v; }
};
struct FeatureStats {
    const float *mean, *stdv;
    __device__ __forceinline__ float operator()(float v, int64_t c) const { return fminf(fmaxf((v - mean[c]) / stdv[c], -5.f), 5.f); }
};
template <typename T, typename Stats>
__global__ __launch_bounds__(256) void pad_rows_kernel(const T *__restrict__ src, int64_t n, int64_t d, int64_t ld_src,
                                                        float *__restrict__ dst, int64_t ld_dst, Stats stats) {
    const int64_t total = n * ld_dst;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = g / ld_dst, c = g % ld_dst;
        dst[g] = c < d ? stats((float)src[r * ld_src + c], c) : 0.f;
    }
}

template <typename Stats>
static int launch_pad(hipStream_t st, const void *src, int is_f64, int64_t n, int64_t d, int64_t ld_src, float *dst, int64_t ld_dst, Stats stats) {
    if (n <= 0) return 0;
    const int64_t total = n * ld_dst;
    const int blocks = (int)(cdiv(total, 256) < 4096 ? cdiv(total, 256) : 4096);
    if (is_f64)
        hipLaunchKernelGGL((pad_rows_kernel<double, Stats>), dim3(blocks), dim3(256), 0, st, (const double *)src, n, d, ld_src, dst, ld_dst, stats);
    else
        hipLaunchKernelGGL((pad_rows_kernel<float, Stats>), dim3(blocks), dim3(256), 0, st, (const float *)src, n, d, ld_src, dst, ld_dst, stats);
    RLPPO_LAUNCH_CHECK();
    return 0;
}
int launch_pad_rows(hipStream_t st, const void *src, int is_f64, int64_t n, int64_t d, int64_t ld_src, float *dst,
                    int64_t ld_dst, int standardize, float mean0, float std0) {
    return launch_pad(st, src, is_f64, n, d, ld_src, dst, ld_dst, ScalarStats{standardize, mean0, std0});
}
int launch_pad_rows_vec(hipStream_t st, const void *src, int is_f64, int64_t n, int64_t d, int64_t ld_src, float *dst,
                        int64_t ld_dst, const float *mean, const float *stdv) {
    return launch_pad(st, src, is_f64, n, d, ld_src, dst, ld_dst, FeatureStats{mean, stdv});
}

// ---------------------------------------------------------------------------------------------- gathers
// The per-row scalars of a minibatch (experience_buffer.py:82-87 gathers them with the states): actions[act_dim], old log-prob,
// advantage, value target of physical row `srow` -> row `row` of four contiguous arrays; zero_n (optional): the critic's folded
// value head accumulates into zeros, so it needs no fill launch of its own (23 us at 65,536 rows).
__device__ __forceinline__ void gather_meta_row(const GatherMeta &meta, int64_t row, int64_t srow) {
    const float old = meta.old_logp[srow], adv = meta.adv[srow], tgt = meta.targets[srow];  // (three independent loads, then the stores)
    meta.g_old[row] = old;
    meta.g_adv[row] = adv;
    meta.g_tgt[row] = tgt;
    for (int k = 0; k < meta.act_dim; ++k) meta.g_act[row * meta.act_dim + k] = meta.actions[srow * meta.act_dim + k];
    if (meta.zero_n) meta.zero_n[row] = 0.f;
}

// Minibatch gather (experience_buffer.py:82-87): dst[r][0..width) = src[idx[r]][0..width), 16 bytes per thread.  One pass
// per minibatch, shared by the policy and the critic: the four first-layer GEMMs (two forwards, two dW) then read
// contiguous rows through the LDS-DMA kernels instead of each chasing the index vector.
// [r5] `meta` (optional): the per-row scalars ride along -- the thread of a row's chunk 0 gathers them -- so a pass that gathers its
// rows (every pass below 262,144 rows) starts with ONE launch instead of two.
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ src, int64_t ld_src,
                                                          const int64_t *__restrict__ idx, float *__restrict__ dst,
                                                          int chunks_per_row, int64_t n, int64_t ring_base, int64_t ring_cap, GatherMeta meta) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t / chunks_per_row;
    const int c = (int)(t - row * chunks_per_row);
    if (row >= n) return;
    const int64_t srow = ring_row(idx[row], ring_base, ring_cap);
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(src + srow * ld_src) + c);
    reinterpret_cast<f32x4 *>(dst)[t] = v;
    if (c == 0 && meta.g_old) gather_meta_row(meta, row, srow);
}

int launch_gather_rows(hipStream_t st, const float *src, int64_t ld_src, const int64_t *idx, float *dst, int width,
                       int64_t n, int64_t ring_base, int64_t ring_cap, const GatherMeta *meta) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(width > 0 && width % 4 == 0 && ld_src >= width && ld_src % 4 == 0, "gather_rows: width=%d ld=%ld", width,
                    (long)ld_src);
    const int cpr = width / 4;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)cdiv(n * cpr, 256)), dim3(256), 0, st, src, ld_src, idx, dst, cpr, n, ring_base,
                       ring_cap, meta ? *meta : GatherMeta{});
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// [critic rows] The gather of a pass whose critic reads a matrix of its own (privileged observations): row idx[r] of BOTH matrices in
// one launch.  Thread t is 16-byte chunk t % (p.cpr + c.cpr) of row t / (p.cpr + c.cpr): the first p.cpr chunks of a row are the
// policy's, the others the critic's -- so a wave's lanes still read and write runs of consecutive 16-byte chunks (one run per
// matrix and row), and the pass still starts with one launch.  `meta` rides on chunk 0 of the policy part, as above.
__global__ __launch_bounds__(256) void gather_rows2_kernel(GatherSide p, GatherSide c, const int64_t *__restrict__ idx, int64_t n,
                                                           int64_t ring_base, int64_t ring_cap, GatherMeta meta) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int cpr = p.cpr + c.cpr;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t / cpr;
    const int k = (int)(t - row * cpr);
    if (row >= n) return;
    const int64_t srow = ring_row(idx[row], ring_base, ring_cap);
    const bool critic = k >= p.cpr;
    const float *src = critic ? c.src : p.src;
    float *dst = critic ? c.dst : p.dst;
    const int64_t ld = critic ? c.ld : p.ld, scpr = critic ? c.cpr : p.cpr;
    const int ck = critic ? k - p.cpr : k;
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(src + srow * ld) + ck);
    reinterpret_cast<f32x4 *>(dst)[row * scpr + ck] = v;
    if (k == 0 && meta.g_old) gather_meta_row(meta, row, srow);
}

int launch_gather_rows2(hipStream_t st, const float *src_p, int64_t ld_p, float *dst_p, int width_p, const float *src_c, int64_t ld_c,
                        float *dst_c, int width_c, const int64_t *idx, int64_t n, int64_t ring_base, int64_t ring_cap, const GatherMeta *meta) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(width_p > 0 && width_p % 4 == 0 && ld_p >= width_p && ld_p % 4 == 0 && width_c > 0 && width_c % 4 == 0 && ld_c >= width_c &&
                        ld_c % 4 == 0, "gather_rows2: width=%d ld=%ld, critic width=%d ld=%ld", width_p, (long)ld_p, width_c, (long)ld_c);
    const GatherSide p{src_p, ld_p, dst_p, width_p / 4}, c{src_c, ld_c, dst_c, width_c / 4};
    const int64_t blocks = cdiv(n * (p.cpr + c.cpr), 256);
    RLPPO_CHECK_ARG(blocks <= 0x7fffffff, "gather_rows2: %ld rows of %d + %d floats are too many for one launch", (long)n, width_p, width_c);
    hipLaunchKernelGGL(gather_rows2_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p, c, idx, n, ring_base, ring_cap, meta ? *meta : GatherMeta{});
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// The same gather for the bf16 update precision: the gathered observation rows are rounded to bf16 on the way -- written as
// fp32 (X operand of the first layer's fp32 weight gradient) and as bf16 (A operand of the first layer's bf16 forward).
__global__ __launch_bounds__(256) void gather_rows_round_kernel(const float *__restrict__ src, int64_t ld_src,
                                                                const int64_t *__restrict__ idx, float *__restrict__ dst,
                                                                unsigned short *__restrict__ dstb, int chunks_per_row, int64_t n,
                                                                int64_t ring_base, int64_t ring_cap) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t / chunks_per_row;
    const int c = (int)(t - row * chunks_per_row);
    if (row >= n) return;
    f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(src + ring_row(idx[row], ring_base, ring_cap) * ld_src) + c);
    u16x4 h;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float f = v[e];
        h[e] = bf16_bits(f);
        v[e] = __uint_as_float((unsigned)h[e] << 16);
    }
    if (dst) reinterpret_cast<f32x4 *>(dst)[t] = v;  // the fp32 form only when an fp32 kernel will read the rows
    reinterpret_cast<u16x4 *>(dstb)[t] = h;
}

int launch_gather_rows_round(hipStream_t st, const float *src, int64_t ld_src, const int64_t *idx, float *dst, unsigned short *dstb,
                             int width, int64_t n, int64_t ring_base, int64_t ring_cap) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(width > 0 && width % 4 == 0 && ld_src >= width && ld_src % 4 == 0, "gather_rows: width=%d ld=%ld", width,
                    (long)ld_src);
    const int cpr = width / 4;
    hipLaunchKernelGGL(gather_rows_round_kernel, dim3((unsigned)cdiv(n * cpr, 256)), dim3(256), 0, st, src, ld_src, idx, dst, dstb,
                       cpr, n, ring_base, ring_cap);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// The per-row scalars alone, for a pass whose GEMMs gather their state rows themselves.  One thread per row, so the dependent
// idx -> row loads of the whole minibatch are in flight together; the loss kernels then stream contiguous data instead of chasing
// the index inside their row loop (two dependent HBM round trips per row with 16 rows per lane group: 150 us per 524,288-row pass).
__global__ __launch_bounds__(256) void gather_meta_kernel(const int64_t *__restrict__ idx, GatherMeta meta, int64_t n, int64_t ring_base,
                                                          int64_t ring_cap, unsigned *__restrict__ rowtab) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t src = ring_row(idx[r], ring_base, ring_cap);
    if (rowtab) rowtab[r] = (unsigned)src;  // [r3] the row table of the fused state gather (gemm.hip, GATHER)
    gather_meta_row(meta, r, src);
}

int launch_gather_meta(hipStream_t st, const int64_t *idx, const float *actions, int act_dim, const float *old_logp,
                       const float *adv, const float *targets, float *g_act, float *g_old, float *g_adv, float *g_tgt, int64_t n,
                       int64_t ring_base, int64_t ring_cap, unsigned *rowtab, float *zero_n) {
    if (n <= 0) return 0;
    GatherMeta meta;
    meta.actions = actions; meta.old_logp = old_logp; meta.adv = adv; meta.targets = targets;
    meta.g_act = g_act; meta.g_old = g_old; meta.g_adv = g_adv; meta.g_tgt = g_tgt; meta.zero_n = zero_n;
    meta.act_dim = act_dim;
    hipLaunchKernelGGL(gather_meta_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, idx, meta, n, ring_base, ring_cap, rowtab);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// action indices as floats (the experience buffer's encoding, experience_buffer.py:72) -- the launch-by-launch form of
// rlppo_discrete_step; the fused kernel writes them itself
__global__ __launch_bounds__(256) void i64_to_f32_kernel(const int64_t *__restrict__ src, float *__restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}
int launch_i64_to_f32(hipStream_t st, const int64_t *src, float *dst, int64_t n) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(i64_to_f32_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, src, dst, n);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------ running statistics
// WelfordRunningStat.increment (running_stats.py:28-46) for n samples of d features: the reference updates sample by
// sample in float32, and each feature's recurrence is independent of the others -- so one thread per feature walking the
// samples in order reproduces it BIT FOR BIT (IEEE division, no contraction), while the d threads read the sample rows
// coalesced.  4096 samples take ~0.1 ms on the stream instead of ~10 ms of Python on the host.
// T = the dtype of the running state: float32 as constructed, float64 after WelfordRunningStat.from_json (np.asarray of
// Python floats; the reference then updates in float64: float32 sample - float64 mean -> float64).
template <typename T>
__global__ __launch_bounds__(128) void welford_kernel(const float *__restrict__ x, int64_t ld, int64_t n, int d,
                                                      T *__restrict__ mean, T *__restrict__ m2, long long count0) {
    const int f = blockIdx.x * 128 + threadIdx.x;
    if (f >= d) return;
    T mu = mean[f], v = m2[f];
    // the recurrence is serial in mu / v, the loads are not: 16 samples are requested together ([r3]: with one dependent load
    // per iteration 4096 samples took 0.86 ms, a third of a 4096-agent collect; the chain of IEEE divisions alone is ~0.1 ms)
    constexpr int PF = 16;
    int64_t i = 0;
    for (; i + PF <= n; i += PF) {
        float xs[PF];
#pragma unroll
        for (int u = 0; u < PF; ++u) xs[u] = x[(i + u) * ld + f];
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const long long prev = count0 + i + u;
            const T cnt = (T)(prev + 1);
            const T delta = (T)xs[u] - mu;            // delta   = sample - running_mean
            const T dn = delta / cnt;                 // delta_n = delta / count
            mu += dn;                                 // running_mean += delta_n
            v += (delta * dn) * (T)prev;              // running_variance += delta * delta_n * (count - 1)
        }
    }
    for (; i < n; ++i) {
        const long long prev = count0 + i;
        const T cnt = (T)(prev + 1);
        const T delta = (T)x[i * ld + f] - mu;
        const T dn = delta / cnt;
        mu += dn;
        v += (delta * dn) * (T)prev;
    }
    mean[f] = mu;
    m2[f] = v;
}

int launch_welford(hipStream_t st, const float *x, int64_t ld, int64_t n, int d, void *mean, void *m2, long long count0,
                   int state_f64) {
    if (n <= 0 || d <= 0) return 0;
    if (state_f64)
        hipLaunchKernelGGL(welford_kernel<double>, dim3((unsigned)cdiv(d, 128)), dim3(128), 0, st, x, ld, n, d, (double *)mean,
                           (double *)m2, count0);
    else
        hipLaunchKernelGGL(welford_kernel<float>, dim3((unsigned)cdiv(d, 128)), dim3(128), 0, st, x, ld, n, d, (float *)mean,
                           (float *)m2, count0);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// WelfordRunningStat.increment_from_serialized_other (running_stats.py:71-98): Chan's parallel combination of two running
// statistics, elementwise over the d features, in the state's dtype and in the reference's operation order:
//   delta = other_mean - mean;  mean' = (count*mean + other_count*other_mean) / total
//   m2'   = m2 + other_m2 + ((delta*delta)*count)*other_count / total
template <typename T>
__global__ __launch_bounds__(128) void welford_merge_kernel(int d, T *__restrict__ mean, T *__restrict__ m2, long long count,
                                                            const float *__restrict__ omean, const float *__restrict__ om2,
                                                            long long ocount) {
    const int f = blockIdx.x * 128 + threadIdx.x;
    if (f >= d) return;
    const T c = (T)count, oc = (T)ocount, tot = (T)(count + ocount);
    const T mu = mean[f], om = (T)omean[f];
    const T delta = om - mu;
    const T dsq = delta * delta;
    // `other_count * other_mean` is int x float32-array = a float32 product whatever the state's dtype (the reference casts
    // the serialised list to float32, running_stats.py:79-80); only then does it meet the (possibly float64) state
    const T oterm = (T)((float)ocount * omean[f]);
    mean[f] = (c * mu + oterm) / tot;
    m2[f] = (m2[f] + (T)om2[f]) + ((dsq * c) * oc) / tot;
}

int launch_welford_merge(hipStream_t st, int d, void *mean, void *m2, long long count, const float *omean, const float *om2,
                         long long ocount, int state_f64) {
    if (d <= 0 || ocount == 0) return 0;
    if (state_f64)
        hipLaunchKernelGGL(welford_merge_kernel<double>, dim3((unsigned)cdiv(d, 128)), dim3(128), 0, st, d, (double *)mean,
                           (double *)m2, count, omean, om2, ocount);
    else
        hipLaunchKernelGGL(welford_merge_kernel<float>, dim3((unsigned)cdiv(d, 128)), dim3(128), 0, st, d, (float *)mean,
                           (float *)m2, count, omean, om2, ocount);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo
