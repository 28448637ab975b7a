// stats.hip -- the small statistics launches around an optimiser step: the report of a learn(), the advantage statistics of a batch,
// the running statistic of the value targets, the target-KL gate with its rate rule, and the completion words of a call.  The first
// three are a grid-stride accumulation of two doubles, ticket_pair_sum (reduce.hpp), and an epilogue of one thread.
#include "reduce.hpp"

namespace rlppo {

// ------------------------------------------------------------------------------------------------ the report of a learn() [r6]
// ppo_learner.py:213-234 in one launch: REPORT_BLOCKS workgroups sum (before - now)^2 over both flat arenas (float32 differences,
// double squares); the last arriver writes the statistics, the two norms and the give-up words into the caller's pinned `out`, zeroes
// the device accumulators for the next learn(), re-arms the ticket counter and releases the completion word at system scope.
constexpr int REPORT_BLOCKS = 64;
using ReportWs = TicketWs<REPORT_BLOCKS>;
static_assert(sizeof(ReportWs) <= RLPPO_REPORT_WS_BYTES, "report workspace");

__global__ __launch_bounds__(256) void learn_report_kernel(rlppo_report_args r) {
    ReportWs *const ws = reinterpret_cast<ReportWs *>(r.ws);
    const int64_t stride = (int64_t)gridDim.x * 256;
    double s[2] = {0.0, 0.0};
    for (int k = 0; k < 2; ++k) {
        const float *b = k ? r.val_before : r.pol_before, *a = k ? r.val_now : r.pol_now;
        const int64_t n = k ? r.n_val : r.n_pol;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            const float d = b[i] - a[i];
            s[k] += (double)d * (double)d;
        }
    }
    if (!ticket_pair_sum(s, ws)) return;
    r.stats[RLPPO_STAT_PASSES] += r.add_passes;
    for (int k = 0; k < RLPPO_N_STATS; ++k) {
        r.out[k] = r.stats[k];
        r.stats[k] = 0.0;
    }
    r.out[RLPPO_N_STATS] = sqrt(s[0]);
    r.out[RLPPO_N_STATS + 1] = sqrt(s[1]);
    const double own = r.timeout_word ? (double)__hip_atomic_load(r.timeout_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    r.out[RLPPO_N_STATS + 2] = own;
    r.out[RLPPO_N_STATS + 3] = r.extra ? *r.extra : own;
    ticket_rearm(ws);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_store(r.done_word, r.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

int launch_learn_report(hipStream_t st, const rlppo_report_args &r) {
    hipLaunchKernelGGL(learn_report_kernel, dim3(REPORT_BLOCKS), dim3(256), 0, st, r);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------- [ABI 7] options beyond the reference
// Advantage statistics of one batch (rlppo_adv_stats).  Every workgroup sums (A - A_first) and (A - A_first)^2 in double over its
// grid-stride share of the batch's rows (shifted sums: no cancellation, and a constant batch gives exactly zero).
constexpr int ADV_BLOCKS = 128;
using AdvWs = TicketWs<ADV_BLOCKS>;
static_assert(sizeof(AdvWs) <= RLPPO_ADV_STATS_WS_BYTES, "adv stats workspace");

__global__ __launch_bounds__(256) void adv_stats_kernel(const int64_t *__restrict__ idx, int64_t n, const float *__restrict__ adv,
                                                        int64_t ring_base, int64_t ring_cap, float *__restrict__ out, AdvWs *__restrict__ ws) {
    const double k0 = (double)adv[ring_row(idx[0], ring_base, ring_cap)];
    double s[2] = {0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double d = (double)adv[ring_row(idx[i], ring_base, ring_cap)] - k0;
        s[0] += d;
        s[1] += d * d;
    }
    if (!ticket_pair_sum(s, ws)) return;
    float mean = 0.f, scale = 1.f;  // one row: used as it is
    if (n > 1) {
        const double m = s[0] / (double)n;
        double var = (s[1] - s[0] * m) / (double)(n - 1);
        var = var > 0.0 ? var : 0.0;
        mean = (float)(k0 + m);
        scale = (float)(1.0 / (sqrt(var) + 1e-8));
    }
    out[0] = mean;
    out[1] = scale;
    ticket_rearm(ws);
}

// the grid of the two batch statistics: the row gathers are latency-bound, so they are spread; beyond 65,536 rows the workgroups stride
static unsigned batch_stat_blocks(int64_t n) {
    const int64_t blocks = cdiv(n, 256 * 2) < ADV_BLOCKS ? cdiv(n, 256 * 2) : ADV_BLOCKS;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

int launch_adv_stats(hipStream_t st, const int64_t *idx, int64_t n, const float *adv, int64_t ring_base, int64_t ring_cap, float *out,
                     void *ws) {
    hipLaunchKernelGGL(adv_stats_kernel, dim3(batch_stat_blocks(n)), dim3(256), 0, st, idx, n, adv, ring_base, ring_cap, out,
                       reinterpret_cast<AdvWs *>(ws));
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------------- [vnorm] value normalisation
// The running statistic of the value targets (rlppo_value_norm_update): adv_stats_kernel's sums on a contiguous array.  The last
// arriver forms the batch's n_b, mean_b, M2_b and merges them into state = {count, mean, M2, rejected} with Chan's formula, then
// publishes scale = {mu, 1/sigma, sigma, 0} with sigma = sqrt(M2 / count + 1e-5) (population variance and epsilon of rl_games'
// RunningMeanStd), computed in double, rounded once.  A batch whose sums are not finite (a NaN or infinite target) changes nothing
// but state[3], the count of rejected batches.  No floating-point atomics, no spin-wait: the same state and batch give the same
// bits every run.
using VnormWs = TicketWs<ADV_BLOCKS>;  // (batch_stat_blocks: the same grid)
static_assert(sizeof(VnormWs) <= RLPPO_VALUE_NORM_WS_BYTES, "value norm workspace");

// every thread's share of the batch's shifted sums: s = {sum (x - x_0), sum (x - x_0)^2}; returns the pivot x_0
__device__ __forceinline__ double value_norm_sums(const float *__restrict__ x, int64_t n, double (&s)[2]) {
    const double k0 = (double)x[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double d = (double)x[i] - k0;
        s[0] += d;
        s[1] += d * d;
    }
    return k0;
}

// the one thread that holds the batch's totals: merge and publish.  False for a rejected batch, which moves state[3] alone.
__device__ __forceinline__ bool value_norm_merge(const double (&s)[2], double k0, int64_t n, double *__restrict__ state,
                                                 float *__restrict__ scale) {
    // (a NaN / infinite target makes k0 or a sum non-finite: x - x = NaN covers an infinite pivot)
    if (!(fabs(s[0]) < INFINITY && fabs(s[1]) < INFINITY && fabs(k0) < INFINITY)) {
        state[3] += 1.0;
        return false;
    }
    const double nb = (double)n;
    const double m = s[0] / nb;
    const double mean_b = k0 + m;
    double m2_b = s[1] - s[0] * m;
    m2_b = m2_b > 0.0 ? m2_b : 0.0;
    const double count = state[0], mean = state[1], m2 = state[2];
    const double delta = mean_b - mean, tot = count + nb;
    const double mean_new = mean + delta * nb / tot;
    const double m2_new = m2 + (m2_b + delta * delta * count * nb / tot);
    state[0] = tot;
    state[1] = mean_new;
    state[2] = m2_new;
    const double sd = sqrt(m2_new / tot + 1e-5);
    scale[0] = (float)mean_new;
    scale[1] = (float)(1.0 / sd);
    scale[2] = (float)sd;
    scale[3] = 0.f;
    return true;
}

__global__ __launch_bounds__(256) void value_norm_update_kernel(const float *__restrict__ x, int64_t n, double *__restrict__ state,
                                                                float *__restrict__ scale, VnormWs *__restrict__ ws) {
    double s[2] = {0.0, 0.0};
    const double k0 = value_norm_sums(x, n, s);
    if (!ticket_pair_sum(s, ws)) return;
    value_norm_merge(s, k0, n, state, scale);
    ticket_rearm(ws);
}

int launch_value_norm_update(hipStream_t st, const float *targets, int64_t n, double *state, float *scale, void *ws) {
    hipLaunchKernelGGL(value_norm_update_kernel, dim3(batch_stat_blocks(n)), dim3(256), 0, st, targets, n, state, scale,
                       reinterpret_cast<VnormWs *>(ws));
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// The same update with PopArt's weight-preserving step (rlppo_value_norm_update_popart; the arithmetic is the contract in
// include/rlppo.h): the critic's last layer, n_w weights w and one bias b, is rescaled in the launch that moves the statistic, so that
// sigma_1 v^' + mu_1 = sigma_0 v^ + mu_0 for every input.  The last arriver stays whole (ticket_pair_sum_together): its thread 0
// reads {mu_0, sigma_0} as PUBLISHED -- the floats the last scan and loss read --, merges, and parks r = sigma_0 / sigma_1, sigma_0,
// mu_0 - mu_1 and sigma_1 (doubles of the published floats) in LDS; behind one __syncthreads() the 256 threads rescale w
// grid-stride-wise with scalar loads and stores (w is only 4-byte aligned inside its arena) and thread 0 writes b.  Every operation
// is spelled out (__dmul_rn, fma, __ddiv_rn): no contraction setting can change a bit.  A rejected batch stores nothing into w or b.
__global__ __launch_bounds__(256) void value_norm_update_popart_kernel(const float *__restrict__ x, int64_t n, double *__restrict__ state,
                                                                       float *__restrict__ scale, VnormWs *__restrict__ ws,
                                                                       float *__restrict__ w, int64_t n_w, float *__restrict__ b) {
    __shared__ double park[4];   // r, sigma_0, mu_0 - mu_1, sigma_1
    __shared__ int moved;
    double s[2] = {0.0, 0.0};
    const double k0 = value_norm_sums(x, n, s);
    if (!ticket_pair_sum_together(s, ws)) return;
    if (threadIdx.x == 0) {
        const double mu0 = (double)scale[0], sd0 = (double)scale[2];
        moved = value_norm_merge(s, k0, n, state, scale);
        if (moved) {
            const double mu1 = (double)scale[0], sd1 = (double)scale[2];   // (as published: this thread's own stores, rounded once)
            park[0] = __ddiv_rn(sd0, sd1);
            park[1] = sd0;
            park[2] = __dsub_rn(mu0, mu1);
            park[3] = sd1;
        }
        ticket_rearm(ws);
    }
    __syncthreads();
    if (!moved) return;
    const double r = park[0];
    for (int64_t i = threadIdx.x; i < n_w; i += 256) w[i] = (float)__dmul_rn((double)w[i], r);
    if (threadIdx.x == 0) b[0] = (float)__ddiv_rn(fma((double)b[0], park[1], park[2]), park[3]);
}

int launch_value_norm_update_popart(hipStream_t st, const float *targets, int64_t n, double *state, float *scale, void *ws, float *w_last,
                                    int64_t n_w, float *b_last) {
    hipLaunchKernelGGL(value_norm_update_popart_kernel, dim3(batch_stat_blocks(n)), dim3(256), 0, st, targets, n, state, scale,
                       reinterpret_cast<VnormWs *>(ws), w_last, n_w, b_last);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ the target-KL gate
// rlppo_kl_gate and rlppo_kl_gate_lr (include/rlppo.h, "[lr]"): one workgroup, one kernel.  Thread t adds slots t, t + 256, ... of
// every pass region in order, the fixed sum of the workgroup follows, the pass totals are weighted by their mb_ratio in pass order.
// Then thread 0 alone: the stop decision first -- a gate that stops the run moves no rate --, then every rate on its own, in double.
// The stop word, the rates and the host words are each optional (rlppo_kl_gate: no rates; api.hip insists on its stop and host
// words); without host words the launch writes device memory only.  Plain vector stores of thread 0; the optimiser launch behind it
// on the stream reads them.
__global__ __launch_bounds__(256) void kl_gate_lr_kernel(rlppo_kl_gate_args g, rlppo_lr_adapt_args l) {
    double kl = 0.0;
    for (int p = 0; p < g.n_passes; ++p) {
        const double *r = g.kl_slots + (int64_t)p * g.slot_stride;
        const int nw = (int)r[0];
        double a = 0.0;
        for (int w = threadIdx.x; w < nw; w += 256) a += r[2 + w];
        kl += r[1] * block_sum_256(a);  // (meaningful in thread 0 alone)
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (g.phase == 1) {  // this rank's share travels in the tail of the exchanged gradient tensor
        const float hi = (float)kl;
        g.exchange[0] = hi;
        g.exchange[1] = (float)(kl - (double)hi);
        return;
    }
    if (g.phase == 2) kl = (double)g.exchange[0] + (double)g.exchange[1];
    unsigned stop = 0;
    if (g.stop_word) {
        stop = *g.stop_word;
        if (stop == 0 && kl > g.threshold) {
            stop = g.batch + 1;
            *g.stop_word = stop;
        }
    }
    if (l.kl_out) *l.kl_out = kl;
    if (stop == 0) {
        const double hi_kl = 2.0 * l.desired_kl, lo_kl = l.desired_kl / 2.0;
        for (int i = 0; i < l.n_lr; ++i) {
            const double lr = l.lr[i];
            if (kl > hi_kl) {
                const double v = lr / l.factor;
                l.lr[i] = v < l.lr_min ? l.lr_min : v;
            } else if (kl > 0.0 && kl < lo_kl) {
                const double v = lr * l.factor;
                l.lr[i] = v > l.lr_max ? l.lr_max : v;
            }
        }
    }
    if (g.host_words) {
        __hip_atomic_store(g.host_words, stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __hip_atomic_store(g.host_words + 1, g.done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

int launch_kl_gate_lr(hipStream_t st, const rlppo_kl_gate_args &a, const rlppo_lr_adapt_args &l) {
    hipLaunchKernelGGL(kl_gate_lr_kernel, dim3(1), dim3(256), 0, st, a, l);
    RLPPO_LAUNCH_CHECK();
    return 0;
}
int launch_kl_gate(hipStream_t st, const rlppo_kl_gate_args &a) { return launch_kl_gate_lr(st, a, rlppo_lr_adapt_args{}); }

// ------------------------------------------------------------------------------------------------ completion words
// [r5] rlppo_act_opts.done_words for the calls whose last kernel does not write them itself: stream order puts this launch behind
// every output of the call; the words are stored with release semantics at system scope (visible to a polling host)
__global__ void signal_words_kernel(unsigned *__restrict__ words, int count, unsigned value) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    for (int i = threadIdx.x; i < count; i += blockDim.x) __hip_atomic_store(words + i, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int launch_signal_words(hipStream_t st, unsigned *words, int count, unsigned value) {
    if (count <= 0) return 0;
    hipLaunchKernelGGL(signal_words_kernel, dim3(1), dim3(64), 0, st, words, count, value);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo
