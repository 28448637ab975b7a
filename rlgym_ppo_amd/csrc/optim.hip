// optim.hip -- gradient-norm clip + Adam on the flat parameter arenas, in three forms: one arena (rlppo_clip_adam); both networks'
// arenas as three stream operations (fill, squared norms, update + re-pack); and the same in ONE launch with a grid barrier.  The
// element update (adam_math, adam_one), the clip coefficient and the workgroup sums (reduce.hpp) are each written once.
#include <atomic>

#include "reduce.hpp"

namespace rlppo {

// coef = min(1, max_norm / (||g|| + 1e-6)) of clip_grad_norm_, from the squared norm the reductions below leave in double
__device__ __forceinline__ float clip_coef(float max_norm, double gnorm2) {
    const float total = (float)sqrt(gnorm2);
    const float coef = max_norm / (total + 1e-6f);
    return coef > 1.f ? 1.f : coef;
}

// torch.optim.Adam single-tensor math (lerp / mul+addcmul / sqrt,div,add / addcdiv) on one element, gi the CLIPPED gradient: the
// moments are updated in place, the new parameter is returned.  No contraction (-ffp-contract=off): tests/optim_yardstick.py counts
// the roundings.
__device__ __forceinline__ float adam_math(float gi, float &mi, float &vi, float p0, float step_size, float bc2_sqrt, float omb1,
                                           float beta2, float omb2, float eps) {
    mi = mi + omb1 * (gi - mi);             // exp_avg.lerp_(grad, 1 - beta1)
    vi = vi * beta2 + (omb2 * gi) * gi;       // mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    return p0 + (-step_size * mi) / denom;
}

// ------------------------------------------------------------------------------------------ one arena
__global__ __launch_bounds__(256) void sqnorm_kernel(const float *__restrict__ g, int64_t n, double *__restrict__ out) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = (double)g[i];
        acc += v * v;
    }
    acc = block_sum_256<Combine::LeftToRight>(acc);
    if (threadIdx.x == 0) atomicAdd(out, acc);
}

__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                    float *__restrict__ v, int64_t n, const double *__restrict__ gnorm2,
                                                    float max_norm, float step_size, float bc2_sqrt, float omb1,
                                                    float beta2, float omb2, float eps) {
    const float coef = clip_coef(max_norm, *gnorm2);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * coef;
        g[i] = gi;  // clip_grad_norm_ scales .grad in place
        float mi = m[i], vi = v[i];
        p[i] = adam_math(gi, mi, vi, p[i], step_size, bc2_sqrt, omb1, beta2, omb2, eps);
        m[i] = mi;
        v[i] = vi;
    }
}

int launch_clip_adam(hipStream_t st, float *p, float *g, float *m, float *v, int64_t n, float max_norm, float step_size,
                     float bc2_sqrt, float omb1, float beta2, float omb2, float eps, double *gnorm2) {
    if (n <= 0) return 0;
    RLPPO_HIP(hipMemsetAsync(gnorm2, 0, sizeof(double), st));
    const int blocks = (int)(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024);
    hipLaunchKernelGGL(sqnorm_kernel, dim3(blocks), dim3(256), 0, st, g, n, gnorm2);
    RLPPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, st, p, g, m, v, n, gnorm2, max_norm, step_size, bc2_sqrt,
                       omb1, beta2, omb2, eps);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------- one optimiser step of BOTH networks, fused
// PPOLearner.learn's tail per batch is value_optimizer.step(); policy_optimizer.step() after two clip_grad_norm_ calls
// (ppo_learner.py:187-193), followed here by the re-packing of the kernels' weight copy and, at the next batch, by
// zero_grad.  As separate launches that is 2 memsets + 2 norms + 2 Adam + 2 packs + 1 fill = 9 dependent stream operations
// of 5-10 us each: ~60 us, 4-5 % of the 1.3 ms a rank of an 8-rank job spends per optimiser step.  Here: one memset, one
// launch for both squared norms, one launch that does clip + Adam for both arenas, writes every updated parameter straight
// into its W / W^T / b slots of the packed copy (the zero padding of the packed copy is never touched) and leaves the
// gradient arena zeroed for the next batch.  Same arithmetic, element by element, as adam_kernel / pack_kernel.
struct OptNet {
    float *p, *g, *m, *v, *packed;
    double *gnorm2;
    int64_t n;
    int64_t n_net;  // elements [n_net, n) are a parameter tail behind the network's layers: clipped, updated and zeroed like the rest, never packed
    float max_norm, step_size, bc2_sqrt, omb1, beta2, omb2, eps;
    PackJobs jobs;
    const unsigned *skip;  // [ABI 7] rlppo_opt_net.skip_word: non-zero = leave this network as it is (NULL: never)
    const double *lr;      // [lr] rlppo_clip_adam_pack2_lr: the rate in device memory (NULL: step_size above, formed on the host)
    double bc1;            //      1 - beta1^step, the host's double
};
__device__ __forceinline__ bool opt_skipped(const OptNet &N) { return N.skip && *N.skip; }
// [lr] the host's step_size = (float)(lr / bc1) for the rate an earlier launch of the stream left in *N.lr: IEEE double division and
// one rounding to float, so a rate in memory and the same rate in the descriptor give the same bits
__device__ __forceinline__ float opt_step_size(const OptNet &N) { return N.lr ? (float)(*N.lr / N.bc1) : N.step_size; }
struct OptPair {
    OptNet net[2];
};

// One element of a network of the pair: clip, Adam, the updated parameter written to the arena AND straight into its W / W^T / b
// slots of the packed copy (the zero padding of the packed copy is never touched), the gradient zeroed for the next batch.
__device__ __forceinline__ void adam_one(const OptNet &N, int64_t i, float gi, float mi, float vi, float p0, float coef, float step_size) {
    const float pi = adam_math(gi * coef, mi, vi, p0, step_size, N.bc2_sqrt, N.omb1, N.beta2, N.omb2, N.eps);
    N.p[i] = pi;
    N.m[i] = mi;
    N.v[i] = vi;
    N.g[i] = 0.f;  // zero_grad of the next batch (the clipped gradient is not observable inside learn())
    if (i >= N.n_net) return;  // a tail parameter has no slot in `packed`
    int l = 0;     // flat order: W0[out][in], b0, W1, b1, ...
    while (l + 1 < N.jobs.n && i >= N.jobs.j[l + 1].off_flat_w) ++l;
    const PackJob &J = N.jobs.j[l];
    if (i < J.off_flat_b) {
        const int64_t e = i - J.off_flat_w;
        const int r = (int)(e / J.in), c = (int)(e % J.in);
        N.packed[J.off_w + (int64_t)r * J.pin + c] = pi;
        N.packed[J.off_wt + (int64_t)c * J.pout + r] = pi;
    } else {
        N.packed[J.off_b + (i - J.off_flat_b)] = pi;
    }
}

__global__ __launch_bounds__(256) void sqnorm2_kernel(OptPair o) {
    const int k = blockIdx.y;
    if (opt_skipped(o.net[k])) return;
    const float *g = o.net[k].g;
    const int64_t n = o.net[k].n;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = (double)g[i];
        acc += v * v;
    }
    acc = block_sum_256<Combine::LeftToRight>(acc);
    if (threadIdx.x == 0) atomicAdd(o.net[k].gnorm2, acc);
}

__global__ __launch_bounds__(256) void adam_pack2_kernel(OptPair o) {
    const OptNet &N = o.net[blockIdx.y];
    if (opt_skipped(N)) return;
    const float coef = clip_coef(N.max_norm, *N.gnorm2), step_size = opt_step_size(N);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N.n; i += (int64_t)gridDim.x * blockDim.x)
        adam_one(N, i, N.g[i], N.m[i], N.v[i], N.p[i], coef, step_size);
}

// ---- the same update in ONE launch: squared norms -> grid barrier -> clip + Adam + re-pack + zero_grad.
// The three-operation form above costs, per optimiser step of an 8-rank job (profiles/r03_rank_share_step_gaps_before.txt): a
// 6 us fill of the two accumulators, 19 us for sqnorm2 (2048 workgroups queueing on two double-precision atomics) and 9 us for
// adam_pack2, each behind a launch boundary with the chip idle.  Here every workgroup writes its partial sum of squares into a
// slot of its own in the caller's sync block and arrives at a counter; the LAST workgroup to arrive adds the slots of both
// networks IN A FIXED ORDER (so the norm -- and with it every replica of a data-parallel job -- is bit-reproducible, which two
// atomically accumulated doubles are not), publishes the totals to the nets' gnorm2 outputs, re-arms the counter and opens the
// barrier (generation word).  While they wait the others already hold the Adam operands of their first elements in registers.
// Agent-scope atomics only on the words that cross workgroups (cdna_hip_programming.md Guideline 16); the block needs no
// per-launch memset: it is zeroed ONCE by its owner and every completed launch leaves it armed.  All workgroups must be
// co-resident: the grid is clamped per device to (occupancy x CUs - one workgroup per CU of margin) / 2 per network and to
// FUSED_MAX_BLOCKS (launch_clip_adam_pack2; below one workgroup the three-operation form runs instead).
// [r4] A wait that gives up is ALL OR NOTHING and leaves no NaN behind: opening the barrier and giving up are both compare-and-swaps
// on the generation word (g0 -> g0 + 1 | g0 -> FUSED_DEAD), so exactly one of them happens; after FUSED_DEAD every workgroup of this
// launch -- waiting, arriving late, or the last arriver itself -- skips its update: parameters, moments and gradients of BOTH
// networks stay as they were, the block's timeout word counts the event, and every later launch on that block skips at once
// until its owner has zeroed it again.  (Round 3 poisoned the step with NaN, which could not be recovered from: advisor finding.)
struct FusedSync {
    unsigned count, gen, timeouts, counted_seq, pad[12];  // 64-byte header; counted_seq: the last launch that added itself to `timeouts`
    double slot[2][512];                     // per network, per workgroup: partial sum of squares of this launch
};
static_assert(sizeof(FusedSync) <= RLPPO_OPT_SYNC_BYTES, "RLPPO_OPT_SYNC_BYTES");
constexpr int FUSED_EPT = 6;                    // elements per thread whose operands are fetched before the barrier
constexpr int FUSED_MAX_BLOCKS = 128;           // per network: 256 workgroups per launch, so that even 8 processes sharing one GPU (the
                                                // gloo tests) keep every launch's grid co-resident (2048 workgroup slots of 256 threads)
constexpr unsigned FUSED_SPIN_LIMIT = 1u << 22;  // x (s_sleep 8 + one L2 round trip) ~ seconds
constexpr unsigned FUSED_DEAD = 0xFFFFFFFFu;     // generation word of a block whose barrier was given up (sticky until re-zeroed)
static unsigned g_fused_spin_limit = FUSED_SPIN_LIMIT;  // rlppo_dbg_set(34, v): tests force the give-up path with 0
void set_fused_spin_limit(int v) { g_fused_spin_limit = v < 0 ? FUSED_SPIN_LIMIT : (unsigned)v; }
static int g_fused_test_hold = 0;  // rlppo_dbg_set(35, 1): test hook -- workgroup (0, 0) never arrives (a grid that is not co-resident)
void set_fused_test_hold(int v) { g_fused_test_hold = v; }

// `timeouts` counts SKIPPED OPTIMISER STEPS (the host rewinds Adam's step count by it), so a launch adds itself at most once:
// the waiter that wins the give-up and workgroup (0, 0) finding the block dead can be the same launch (a late-dispatched (0, 0)
// on a grid that was not co-resident -- exactly the give-up case); whoever swaps the launch's sequence number in first counts.
__device__ __forceinline__ void count_skipped_once(FusedSync *sy, unsigned seq) {
    if (__hip_atomic_exchange(&sy->counted_seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != seq)
        __hip_atomic_fetch_add(&sy->timeouts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void adam_fused_kernel(OptPair o, FusedSync *__restrict__ sy, const unsigned spin_limit, const int test_hold, const unsigned seq) {
    const int k = blockIdx.y, tid = threadIdx.x;
    const OptNet &N = o.net[k];
    const unsigned nblocks = gridDim.x * gridDim.y;
    const int64_t stride = (int64_t)gridDim.x * 256, i0 = (int64_t)blockIdx.x * 256 + tid;
    // ---- phase 1: this workgroup's share of ||g||^2, in double (as sqnorm2_kernel); the first FUSED_EPT elements stay in registers
    float g[FUSED_EPT], m[FUSED_EPT], v[FUSED_EPT], p[FUSED_EPT];
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < FUSED_EPT; ++e) {
        const int64_t i = i0 + e * stride;
        g[e] = i < N.n ? N.g[i] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < FUSED_EPT; ++e) {  // requested now, needed after the barrier
        const int64_t i = i0 + e * stride;
        m[e] = i < N.n ? N.m[i] : 0.f;
        v[e] = i < N.n ? N.v[i] : 0.f;
        p[e] = i < N.n ? N.p[i] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < FUSED_EPT; ++e) acc += (double)g[e] * (double)g[e];
    for (int64_t i = i0 + FUSED_EPT * stride; i < N.n; i += stride) {
        const double x = (double)N.g[i];
        acc += x * x;
    }
    __shared__ float s_coef, s_step;
    __shared__ int s_last, s_ok;
    __shared__ unsigned s_g0;
    acc = block_sum_256(acc);
    if (tid == 0) {
        int ok = 1, last = 0;
        const unsigned g0 = __hip_atomic_load(&sy->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // read BEFORE arriving
        s_g0 = g0;
        if (g0 == FUSED_DEAD) {  // an earlier launch on this block gave up and its owner has not re-zeroed it: nothing to wait for
            ok = 0;
            if (blockIdx.x == 0 && k == 0) count_skipped_once(sy, seq);
        } else if (test_hold && blockIdx.x == 0 && k == 0) {
            // test hook: this workgroup behaves like one that was never scheduled while the others wait -- it does not arrive; it
            // only watches the generation word until the waiters have given up, so that the launch ends
            while (__hip_atomic_load(&sy->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == g0) __builtin_amdgcn_s_sleep(8);
            ok = 0;
        } else {
            __hip_atomic_store(&sy->slot[k][blockIdx.x], acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // arrival: the release half orders our slot before the count, the acquire half lets the last arriver see everybody's
            const unsigned old = __hip_atomic_fetch_add(&sy->count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            last = old == nblocks - 1;
            if (!last) {
                unsigned spins = 0, cur;
                while ((cur = __hip_atomic_load(&sy->gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == g0) {
                    __builtin_amdgcn_s_sleep(8);
                    if (++spins > spin_limit) {
                        // give up -- unless the barrier opens in this very moment: ONE compare-and-swap decides for the whole launch
                        unsigned expect = g0;
                        if (__hip_atomic_compare_exchange_strong(&sy->gen, &expect, FUSED_DEAD, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                                 __HIP_MEMORY_SCOPE_AGENT)) {
                            count_skipped_once(sy, seq);
                            cur = FUSED_DEAD;
                        } else {
                            cur = expect;  // somebody else decided first: opened (g0 + 1) or dead
                        }
                        break;
                    }
                }
                ok = cur != FUSED_DEAD;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
        }
        s_last = last;
        s_ok = ok;
    }
    __syncthreads();
    if (s_last) {  // the whole workgroup adds the slots: thread t takes slots t, t + 256 of each network; fixed tree afterwards
        double a[2] = {0.0, 0.0};
        for (int j = 0; j < 2; ++j)
            for (int b = tid; b < (int)gridDim.x; b += 256)
                a[j] += __hip_atomic_load(&sy->slot[j][b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        block_sum_256(a);
        if (tid == 0) {
            for (int j = 0; j < 2; ++j) __hip_atomic_store(o.net[j].gnorm2, a[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&sy->count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // opens the barrier -- unless a waiter gave up first (then nobody updates, this workgroup included)
            unsigned expect = s_g0;
            const unsigned next = s_g0 + 1 == FUSED_DEAD ? 0u : s_g0 + 1;
            s_ok = __hip_atomic_compare_exchange_strong(&sy->gen, &expect, next, __ATOMIC_RELEASE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (tid == 0) {
        const double t = __hip_atomic_load(N.gnorm2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_coef = clip_coef(N.max_norm, t);
        s_step = opt_step_size(N);  // [lr] behind the barrier: one read of the rate per workgroup
    }
    __syncthreads();
    if (!s_ok) return;  // given up: parameters, moments and gradients stay as they were (the timeout word says so)
    // [ABI 7] a skipped network still took part in the barrier (every workgroup arrives, whatever the other network does)
    if (opt_skipped(N)) return;
    // ---- phase 2: adam_pack2_kernel, element for element
    const float coef = s_coef, step_size = s_step;
#pragma unroll
    for (int e = 0; e < FUSED_EPT; ++e) {
        const int64_t i = i0 + e * stride;
        if (i < N.n) adam_one(N, i, g[e], m[e], v[e], p[e], coef, step_size);
    }
    for (int64_t i = i0 + FUSED_EPT * stride; i < N.n; i += stride) adam_one(N, i, N.g[i], N.m[i], N.v[i], N.p[i], coef, step_size);
}

int launch_clip_adam_pack2(hipStream_t st, const NetLayout *nets, float *const *p, float *const *g, float *const *m, float *const *v,
                           float *const *packed, double *const *gnorm2, const int64_t *n, const float *max_norm,
                           const float *step_size, const float *bc2_sqrt, const float *omb1, const float *beta2, const float *omb2,
                           const float *eps, void *sync_ws, const unsigned *const *skip, const int64_t *tail, const double *const *lr,
                           const double *bc1) {
    OptPair o;
    int64_t nmax = 0;
    for (int k = 0; k < 2; ++k) {
        OptNet &N = o.net[k];
        N.p = p[k]; N.g = g[k]; N.m = m[k]; N.v = v[k]; N.packed = packed[k]; N.gnorm2 = gnorm2[k]; N.n = n[k];
        N.max_norm = max_norm[k]; N.step_size = step_size[k]; N.bc2_sqrt = bc2_sqrt[k]; N.omb1 = omb1[k]; N.beta2 = beta2[k];
        N.omb2 = omb2[k]; N.eps = eps[k];
        N.skip = skip ? skip[k] : nullptr;
        N.n_net = n[k] - (tail ? tail[k] : 0);
        N.lr = lr ? lr[k] : nullptr;
        N.bc1 = bc1 ? bc1[k] : 1.0;
        fill_jobs(nets[k], &N.jobs);
        nmax = n[k] > nmax ? n[k] : nmax;
    }
    if (sync_ws) {  // one launch (the caller owns a zero-initialised sync block)
        RLPPO_CHECK_ARG(((uintptr_t)sync_ws & 15) == 0, "clip_adam_pack2: the sync block must be 16-byte aligned");
        // The grid barrier needs every workgroup of the launch resident at once: per device (queried once for each device id),
        // workgroups per network <= (occupancy x CUs - one workgroup per CU of margin for kernels of other streams) / 2.  On an
        // MI355X that is (8 x 256 - 256) / 2 = 896, far above FUSED_MAX_BLOCKS; a small or partitioned device gets a smaller
        // grid, and one that cannot hold a single workgroup per network the three-operation form below.
        static std::atomic<int> cap_by_dev[64];
        int dev = 0;
        RLPPO_HIP(hipGetDevice(&dev));
        RLPPO_CHECK_ARG(dev >= 0 && dev < 64, "clip_adam_pack2: device id %d", dev);
        int cap = cap_by_dev[dev].load(std::memory_order_acquire);
        if (cap == 0) {
            int per_cu = 0;
            hipDeviceProp_t prop;
            RLPPO_HIP(hipGetDeviceProperties(&prop, dev));
            RLPPO_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, adam_fused_kernel, 256, 0));
            per_cu = per_cu > 7 ? 7 : per_cu;  // (the occupancy API over-reports by one in the 8-per-CU regime: MI355X_MICROARCH.md)
            cap = (per_cu * prop.multiProcessorCount - prop.multiProcessorCount) / 2;
            cap = cap < 1 ? -1 : cap;
            cap_by_dev[dev].store(cap, std::memory_order_release);
        }
        if (cap >= 1) {
            int64_t blocks = cdiv(nmax, 256 * FUSED_EPT);
            blocks = blocks < 1 ? 1 : (blocks > FUSED_MAX_BLOCKS ? FUSED_MAX_BLOCKS : blocks);
            blocks = blocks > cap ? cap : blocks;
            static std::atomic<unsigned> launch_seq{0};  // per-launch sequence number, never 0 (a zeroed block's counted_seq)
            unsigned seq = launch_seq.fetch_add(1, std::memory_order_relaxed) + 1;
            if (seq == 0) seq = launch_seq.fetch_add(1, std::memory_order_relaxed) + 1;
            hipLaunchKernelGGL(adam_fused_kernel, dim3((unsigned)blocks, 2), dim3(256), 0, st, o, reinterpret_cast<FusedSync *>(sync_ws),
                               g_fused_spin_limit, g_fused_test_hold, seq);
            RLPPO_LAUNCH_CHECK();
            return 0;
        }
    }
    if (gnorm2[1] == gnorm2[0] + 1 || gnorm2[0] == gnorm2[1] + 1) {  // adjacent accumulators (PPOLearner's): one fill
        RLPPO_HIP(hipMemsetAsync(gnorm2[0] < gnorm2[1] ? gnorm2[0] : gnorm2[1], 0, 2 * sizeof(double), st));
    } else {
        for (int k = 0; k < 2; ++k) RLPPO_HIP(hipMemsetAsync(gnorm2[k], 0, sizeof(double), st));
    }
    const int blocks = (int)(cdiv(nmax, 256) < 1024 ? cdiv(nmax, 256) : 1024);
    hipLaunchKernelGGL(sqnorm2_kernel, dim3(blocks, 2), dim3(256), 0, st, o);
    RLPPO_LAUNCH_CHECK();
    hipLaunchKernelGGL(adam_pack2_kernel, dim3(blocks, 2), dim3(256), 0, st, o);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo
