// gae_vtrace.hip -- the V-trace form of the GAE scan (IMPALA's off-policy correction inside the advantage recurrence): one segmented
// reverse affine scan whose per-step decay is DATA.
//
//     ratio_t = exp(logp_new[t] - logp_old[t])                         (float32 expf, in the kernel)
//     rho_t   = min(rho_bar, ratio_t) ,  c_t = lambda * min(c_bar, ratio_t)
//     b_t     = rho_t * (clip(r_t/sigma) + gamma * Vnext_t * nd_t - V_t)
//     a_t     = gamma * c_t * nd_t * nt_t
//     A_t     = b_t + a_t * A_{t+1} ,  value_target_t = V_t + A_t
// with nd = 1 - done, nt = 1 - truncated and Vnext_t chosen as rlppo_gae_boot chooses it.  In gae.hip a_t is gamma*lambda or 0 and a
// step carries one BIT for it; here every step carries its own double, the composite of a run of steps is a general affine map
// (a, b): x -> a*x + b, and nothing about it is known before the two log-probability streams have arrived.  Only the advantage
// recurrence exists (the buffer's returns feed the running return statistics alone), so a carry is two doubles, not four.
//
// Split of the work: a lane owns VT_EPT = 8 consecutive steps (two 16-byte loads per input stream), composes them right to left in
// registers; a wave's 64 lane composites go through a fixed-order shuffle suffix scan (6 steps); the four wave totals of a workgroup
// meet in LDS.  Across workgroups: ONE pass over HBM with decoupled look-back -- a chunk publishes its aggregate map as soon as its own
// scan is done and composes the aggregates to its right, in order, until the composed map has a == 0 (a done or a trajectory end
// cuts the recurrence: normally inside the very next chunk) or the data ends.  Records are the {tag, 32-bit half} granules of
// gae.hip, written and read by relaxed agent-scope atomics: the data is its own flag.  No floating-point atomics anywhere, and no
// choice between records that depends on timing: every output is a fixed expression tree of its inputs, the same bits on every run.
// The wait is bounded; on give-up the carry is NaN (the chunk's outputs and those that chain through it) and workspace word 1 counts
// the event, exactly as in rlppo_gae.  Under stream capture, with rlppo_dbg_set(1, 0), or when the scan has more chunks than
// workgroups can be resident, the stateless two-launch form runs instead (summary, then apply): same per-step maps, same in-chunk scan.
// The two coefficient arrays are never materialised; the outputs leave lane-contiguous through an in-wave LDS transpose.
#include "common.hpp"

namespace rlppo {

constexpr int VT_THREADS = 256;
constexpr int VT_EPT = 8;                        // steps per lane
constexpr int VT_WAVE = 64 * VT_EPT;             // steps per wave (512)
constexpr int VT_BLOCK = VT_THREADS * VT_EPT;    // steps per workgroup (2048)
static_assert(VT_BLOCK == 2048, "the look-back records live in rlppo_gae's workspace: one 128-byte record per 2048 steps");

struct Aff {  // x -> a * x + b
    double a, b;
};
__device__ __forceinline__ Aff vt_identity() { return Aff{1.0, 0.0}; }
// left o right: the left run of steps is applied after the right one
__device__ __forceinline__ Aff vt_compose(const Aff &l, const Aff &r) { return Aff{l.a * r.a, l.b + l.a * r.b}; }
__device__ __forceinline__ Aff vt_shfl_down(const Aff &v, int off) { return Aff{__shfl_down(v.a, off), __shfl_down(v.b, off)}; }
// inclusive suffix scan over the wave, fixed order: lane l <- f_l o f_{l+1} o ... o f_63 (lane 0: the wave's total)
__device__ __forceinline__ Aff vt_wave_suffix(Aff v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const Aff o = vt_shfl_down(v, off);
        if (lane + off < 64) v = vt_compose(v, o);
    }
    return v;
}

struct VtParams {
    double gamma, gl, rho_bar, c_bar;  // gl = gamma * lambda
    float ret_std;
    int use_std;
};

// the per-step maps of a lane's VT_EPT steps, and the real-unit V_t the value target needs
struct VtSteps {
    double a[VT_EPT], b[VT_EPT];
    float v[VT_EPT];
};

typedef float f4 __attribute__((ext_vector_type(4)));

template <bool BOOT, bool NORM>
__device__ __forceinline__ void vt_load(const VtraceIO &io, const VtParams &p, int64_t t0, VtSteps &s) {
    float r[VT_EPT], d[VT_EPT], tr[VT_EPT], v[VT_EPT + 1], ln[VT_EPT], lo[VT_EPT], bv[VT_EPT];
    const int64_t n = io.n;
    if (t0 + VT_EPT <= n) {  // (values has n + 1 entries: values[t0 + VT_EPT] exists)
#pragma unroll
        for (int h = 0; h < VT_EPT / 4; ++h) {
            const f4 r4 = *reinterpret_cast<const f4 *>(io.rews + t0 + 4 * h);
            const f4 d4 = *reinterpret_cast<const f4 *>(io.dones + t0 + 4 * h);
            const f4 t4 = *reinterpret_cast<const f4 *>(io.trunc + t0 + 4 * h);
            const f4 v4 = *reinterpret_cast<const f4 *>(io.values + t0 + 4 * h);
            const f4 n4 = *reinterpret_cast<const f4 *>(io.logp_new + t0 + 4 * h);
            const f4 o4 = *reinterpret_cast<const f4 *>(io.logp_old + t0 + 4 * h);
            f4 b4 = f4{0.f, 0.f, 0.f, 0.f};
            if constexpr (BOOT) b4 = *reinterpret_cast<const f4 *>(io.boot + t0 + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r[4 * h + e] = r4[e];
                d[4 * h + e] = d4[e];
                tr[4 * h + e] = t4[e];
                v[4 * h + e] = v4[e];
                ln[4 * h + e] = n4[e];
                lo[4 * h + e] = o4[e];
                bv[4 * h + e] = b4[e];
            }
        }
        v[VT_EPT] = io.values[t0 + VT_EPT];
    } else {
#pragma unroll
        for (int e = 0; e < VT_EPT; ++e) {
            const bool ok = t0 + e < n;
            r[e] = ok ? io.rews[t0 + e] : 0.f;
            d[e] = ok ? io.dones[t0 + e] : 0.f;
            tr[e] = ok ? io.trunc[t0 + e] : 0.f;
            v[e] = ok ? io.values[t0 + e] : 0.f;
            ln[e] = ok ? io.logp_new[t0 + e] : 0.f;
            lo[e] = ok ? io.logp_old[t0 + e] : 0.f;
            bv[e] = 0.f;
            if constexpr (BOOT) bv[e] = ok ? io.boot[t0 + e] : 0.f;
        }
        v[VT_EPT] = 0.f;
#pragma unroll
        for (int e = 0; e < VT_EPT; ++e)
            if (t0 + e + 1 <= n) v[e + 1] = io.values[t0 + e + 1];  // (values[n] = V of the last step's next state)
    }
    float mu = 0.f, sd = 1.f;
    if constexpr (NORM) {  // {mu, sigma}: uniform over the workgroup; one explicit float32 fma per value, as rlppo_gae_norm
        mu = io.vscale[0];
        sd = io.vscale[2];
#pragma unroll
        for (int e = 0; e <= VT_EPT; ++e) v[e] = fmaf(v[e], sd, mu);
        if constexpr (BOOT) {
#pragma unroll
            for (int e = 0; e < VT_EPT; ++e) bv[e] = fmaf(bv[e], sd, mu);
        }
    }
#pragma unroll
    for (int e = 0; e < VT_EPT; ++e) {
        // straight-line code with selects (a branch per step kept the sixteen doubles in scratch); a step past the end was loaded as
        // zeros and becomes the zero map: x = 0 beyond the last step
        const bool ok = t0 + e < n;
        s.v[e] = v[e];
        const float ndf = 1.0f - d[e], ntf = 1.0f - tr[e];
        const float rn = p.use_std ? fminf(fmaxf(r[e] / p.ret_std, -10.f), 10.f) : r[e];
        float v1 = v[e + 1];
        if constexpr (BOOT) v1 = tr[e] != 0.f && d[e] == 0.f ? bv[e] : v1;  // a select: an unused entry never reaches an output
        const double ratio = (double)expf(ln[e] - lo[e]);
        // (written so that a NaN ratio stays NaN instead of turning into the clip)
        const double rho = ratio > p.rho_bar ? p.rho_bar : ratio;
        const double c = ratio > p.c_bar ? p.c_bar : ratio;
        const double delta = rho * (((double)rn + p.gamma * (double)v1 * (double)ndf) - (double)v[e]);
        s.b[e] = ok ? delta : 0.0;
        s.a[e] = ok && ndf * ntf != 0.f ? p.gl * c : 0.0;
    }
}

__device__ __forceinline__ Aff vt_lane_composite(const VtSteps &s) {
    Aff c = vt_identity();
#pragma unroll
    for (int e = VT_EPT - 1; e >= 0; --e) {  // right to left: c <- step_e o c
        c.b = s.b[e] + s.a[e] * c.b;
        c.a = s.a[e] * c.a;
    }
    return c;
}

// In-chunk scan: returns this lane's inclusive suffix within its wave, leaves the four wave totals in wave_tot (behind a barrier).
__device__ __forceinline__ Aff vt_chunk_scan(const VtSteps &s, Aff *wave_tot) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Aff inc = vt_wave_suffix(vt_lane_composite(s), lane);
    if (lane == 0) wave_tot[wave] = inc;
    __syncthreads();
    return inc;
}
__device__ __forceinline__ Aff vt_chunk_total(const Aff *wave_tot) {
    return vt_compose(vt_compose(wave_tot[0], wave_tot[1]), vt_compose(wave_tot[2], wave_tot[3]));
}

// The outputs of a chunk once its carry-in (A at the first step of chunk + 1) is known.  o_lds: 2 * VT_WAVE floats per wave.
__device__ __forceinline__ void vt_emit(const VtraceIO &io, const VtSteps &s, const Aff &inc, const Aff *wave_tot, double carry, int chunk,
                                        float *o_lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = io.n;
    const int64_t t0 = ((int64_t)chunk * VT_THREADS + threadIdx.x) * VT_EPT;
    Aff after = vt_shfl_down(inc, 1);  // lanes lane + 1 .. 63 of this wave
    if (lane == 63) after = vt_identity();
    for (int w = wave + 1; w < VT_THREADS / 64; ++w) after = vt_compose(after, wave_tot[w]);
    double x = after.b + after.a * carry;  // A entering this lane's rightmost step
    const int64_t wbase = ((int64_t)chunk * VT_THREADS + wave * 64) * VT_EPT;
    const bool full_wave = wbase + VT_WAVE <= n;  // (wave-uniform)
    float *o = o_lds + wave * (2 * VT_WAVE);
#pragma unroll
    for (int h = VT_EPT / 4 - 1; h >= 0; --h) {
        f4 q_adv, q_vt;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const int e = 4 * h + j;
            x = s.b[e] + s.a[e] * x;
            q_adv[j] = (float)x;
            q_vt[j] = (float)((double)s.v[e] + x);
        }
        if (full_wave) {
            *reinterpret_cast<f4 *>(o + lane * VT_EPT + 4 * h) = q_adv;
            *reinterpret_cast<f4 *>(o + VT_WAVE + lane * VT_EPT + 4 * h) = q_vt;
        } else if (t0 + VT_EPT <= n) {
            *reinterpret_cast<f4 *>(io.adv + t0 + 4 * h) = q_adv;
            *reinterpret_cast<f4 *>(io.vt + t0 + 4 * h) = q_vt;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t0 + 4 * h + j < n) {
                    io.adv[t0 + 4 * h + j] = q_adv[j];
                    io.vt[t0 + 4 * h + j] = q_vt[j];
                }
        }
    }
    if (full_wave) {  // in-wave transpose: a wave's LDS operations execute in order, no workgroup barrier
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int h = 0; h < VT_EPT / 4; ++h) {
            const int k = h * 256 + lane * 4;  // 1 KiB of consecutive bytes per wave instruction
            *reinterpret_cast<f4 *>(io.adv + wbase + k) = *reinterpret_cast<const f4 *>(o + k);
            *reinterpret_cast<f4 *>(io.vt + wbase + k) = *reinterpret_cast<const f4 *>(o + VT_WAVE + k);
        }
    }
}

// ---- look-back records: 16 granules (128 B) per chunk as in gae.hip, of which [0, 4) hold the chunk's aggregate map.
// The carry of chunk k is DEFINED as the left-to-right composition agg_{k+1} o agg_{k+2} o ... applied to 0, cut at the first chunk
// where the composed a is 0 (a trajectory end; or the product of decays underflowing, which makes the rest irrelevant just the same).
// A chunk therefore publishes its aggregate and nothing else, and a walk reads aggregates only: no chunk ever waits for another
// chunk's CARRY, only for its local scan, and which records happen to be there when a walk passes cannot change a single bit -- the
// usual shortcut through a neighbour's inclusive value is left out because it rounds differently from the walk it replaces.  The
// stateless form evaluates the same definition in the same order: the two forms give the same bits.
typedef unsigned long long u64;
constexpr int VT_REC = 16, VT_AGG = 4;
__device__ __forceinline__ void vt_put(u64 *p, unsigned tag, double d) {
    const u64 bits = (u64)__double_as_longlong(d);
    __hip_atomic_store(p, ((u64)tag << 32) | (unsigned)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p + 1, ((u64)tag << 32) | (unsigned)(bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One launch.  Workgroup i takes chunk n_chunks - 1 - i: a chunk waits only on chunks to its right, i.e. on workgroups with lower ids,
// dispatched before it; the launcher gives every chunk a workgroup of its own and keeps the grid within what can be resident.
template <bool BOOT, bool NORM>
__global__ __launch_bounds__(VT_THREADS) void gae_vtrace_lookback_kernel(VtraceIO io, VtParams p, u64 *__restrict__ state, const unsigned tag,
                                                                          const unsigned spin_limit, unsigned *__restrict__ slow_word,
                                                                          int n_chunks) {
    __shared__ Aff wave_tot[VT_THREADS / 64];
    __shared__ double s_carry;
    __shared__ __attribute__((aligned(16))) float o_lds[(VT_THREADS / 64) * 2 * VT_WAVE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = n_chunks - 1 - (int)blockIdx.x;
    const int64_t t0 = ((int64_t)chunk * VT_THREADS + threadIdx.x) * VT_EPT;
    VtSteps s;
    vt_load<BOOT, NORM>(io, p, t0, s);
    const Aff inc = vt_chunk_scan(s, wave_tot);
    if (wave == 0) {
        if (lane == 0 && chunk > 0) {  // (nobody is to the left of chunk 0)
            const Aff agg = vt_chunk_total(wave_tot);
            u64 *rec = state + (size_t)chunk * VT_REC;
            vt_put(rec + 0, tag, agg.a);
            vt_put(rec + 2, tag, agg.b);
        }
        Aff acc = vt_identity();
        bool poisoned = false;
        unsigned spins = 0;
        for (int j = chunk + 1; j < n_chunks && !poisoned;) {
            u64 g = 0;  // lanes 0..3 read the four granules of chunk j's aggregate
            if (lane < VT_AGG) g = __hip_atomic_load(state + (size_t)j * VT_REC + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned rtag = (unsigned)(g >> 32), val = (unsigned)g;
            if (__ballot(lane < VT_AGG && rtag == tag) == 0xFull) {
                auto dbl = [&](int first) {
                    const unsigned lo = __shfl(val, first), hi = __shfl(val, first + 1);
                    return __longlong_as_double((long long)(((u64)hi << 32) | lo));
                };
                acc = vt_compose(acc, Aff{dbl(0), dbl(2)});
                if (acc.a == 0.0) break;  // nothing further to the right matters (wave-uniform)
                ++j;
                spins = 0;
            } else {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > spin_limit) {  // never a hang, never a silent wrong result: poison and count (include/rlppo.h)
                    if (lane == 0) atomicAdd(slow_word, 1u);
                    poisoned = true;
                }
            }
        }
        if (lane == 0) s_carry = poisoned ? __longlong_as_double(0x7ff8000000000000ll) : acc.b;  // (x = 0 beyond the last chunk)
    }
    __syncthreads();
    vt_emit(io, s, inc, wave_tot, s_carry, chunk, o_lds);
}

// ---- the stateless form: two launches, no waits (stream capture; more chunks than resident workgroups)
template <bool BOOT, bool NORM>
__global__ __launch_bounds__(VT_THREADS) void gae_vtrace_summary_kernel(VtraceIO io, VtParams p, Aff *__restrict__ summaries) {
    __shared__ Aff wave_tot[VT_THREADS / 64];
    const int64_t t0 = ((int64_t)blockIdx.x * VT_THREADS + threadIdx.x) * VT_EPT;
    VtSteps s;
    vt_load<BOOT, NORM>(io, p, t0, s);
    vt_chunk_scan(s, wave_tot);
    if (threadIdx.x == 0) summaries[blockIdx.x] = vt_chunk_total(wave_tot);
}

template <bool BOOT, bool NORM>
__global__ __launch_bounds__(VT_THREADS) void gae_vtrace_apply_kernel(VtraceIO io, VtParams p, const Aff *__restrict__ summaries, int n_chunks) {
    __shared__ Aff wave_tot[VT_THREADS / 64];
    __shared__ double s_carry;
    __shared__ __attribute__((aligned(16))) float o_lds[(VT_THREADS / 64) * 2 * VT_WAVE];
    const int chunk = blockIdx.x;
    const int64_t t0 = ((int64_t)chunk * VT_THREADS + threadIdx.x) * VT_EPT;
    VtSteps s;
    vt_load<BOOT, NORM>(io, p, t0, s);  // (issued first: the walk below overlaps with the loads)
    if (threadIdx.x == 0) {  // the carry's definition, in its order (uniform loads; normally one or two summaries)
        Aff acc = vt_identity();
        for (int j = chunk + 1; j < n_chunks; ++j) {
            acc = vt_compose(acc, summaries[j]);
            if (acc.a == 0.0) break;
        }
        s_carry = acc.b;
    }
    const Aff inc = vt_chunk_scan(s, wave_tot);  // (its barrier publishes s_carry too)
    vt_emit(io, s, inc, wave_tot, s_carry, chunk, o_lds);
}

// steps per lane / per wave / per workgroup (level 0 / 1 / 2): what rlppo_gae_vtrace_span reports
int gae_vtrace_span(int level) { return level == 0 ? VT_EPT : (level == 1 ? VT_WAVE : (level == 2 ? VT_BLOCK : -1)); }

template <bool BOOT, bool NORM>
static int launch_vtrace_form(hipStream_t st, const VtraceIO &io, const VtParams &p, void *ws) {
    const int nb = (int)cdiv(io.n, VT_BLOCK);
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st) RLPPO_HIP(hipStreamIsCapturing(st, &cap));
    if (gae_algo() >= 1 && cap == hipStreamCaptureStatusNone) {
        // workgroups of the look-back kernel that can be resident together, per device id (queried once each)
        static std::atomic<int> resident_by_dev[64];
        int dev = 0;
        RLPPO_HIP(hipGetDevice(&dev));
        RLPPO_CHECK_ARG(dev >= 0 && dev < 64, "gae_vtrace: device id %d", dev);
        int resident = resident_by_dev[dev].load(std::memory_order_acquire);
        if (resident == 0) {
            int per_cu = 0, cus = 0;
            if (const int rc = device_cu_count(&cus)) return rc;
            RLPPO_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gae_vtrace_lookback_kernel<BOOT, NORM>, VT_THREADS, 0));
            per_cu = per_cu > 6 ? 6 : (per_cu < 1 ? 1 : per_cu);
            resident = per_cu * cus;
            resident_by_dev[dev].store(resident, std::memory_order_release);
        }
        if (nb <= resident) {  // every chunk's workgroup is resident: a wait can only be for a workgroup that is running
            unsigned *hdr = reinterpret_cast<unsigned *>(ws);
            u64 *state = reinterpret_cast<u64 *>(reinterpret_cast<char *>(ws) + 16);
            hipLaunchKernelGGL((gae_vtrace_lookback_kernel<BOOT, NORM>), dim3(nb), dim3(VT_THREADS), 0, st, io, p, state, gae_next_tag(),
                               gae_spin_limit(), hdr + 1, nb);
            RLPPO_LAUNCH_CHECK();
            return 0;
        }
    }
    Aff *summ = reinterpret_cast<Aff *>(reinterpret_cast<char *>(ws) + 16);
    hipLaunchKernelGGL((gae_vtrace_summary_kernel<BOOT, NORM>), dim3(nb), dim3(VT_THREADS), 0, st, io, p, summ);
    RLPPO_LAUNCH_CHECK();
    hipLaunchKernelGGL((gae_vtrace_apply_kernel<BOOT, NORM>), dim3(nb), dim3(VT_THREADS), 0, st, io, p, summ, nb);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

int launch_gae_vtrace(hipStream_t st, const VtraceIO &io, double gamma, double lmbda, double rho_bar, double c_bar, float ret_std, void *ws,
                      size_t ws_bytes) {
    RLPPO_CHECK_ARG(((uintptr_t)io.rews | (uintptr_t)io.dones | (uintptr_t)io.trunc | (uintptr_t)io.values | (uintptr_t)io.logp_new |
                     (uintptr_t)io.logp_old | (uintptr_t)io.boot | (uintptr_t)io.vt | (uintptr_t)io.adv | (uintptr_t)ws) % 16 == 0,
                    "gae_vtrace: arrays and workspace must be 16-byte aligned");
    RLPPO_CHECK_ARG((uintptr_t)io.vscale % 16 == 0, "gae_vtrace: value_scale must be 16-byte aligned");
    if (ws_bytes < gae_workspace_bytes(io.n)) {
        set_error("gae_vtrace: workspace %zu < %zu bytes", ws_bytes, gae_workspace_bytes(io.n));
        return RLPPO_ERR_WORKSPACE;
    }
    VtParams p;
    p.gamma = gamma;
    p.gl = gamma * lmbda;
    p.rho_bar = rho_bar;
    p.c_bar = c_bar;
    p.use_std = !(ret_std != ret_std);  // NaN means "no scaling"
    p.ret_std = ret_std;
    if (io.vscale) return io.boot ? launch_vtrace_form<true, true>(st, io, p, ws) : launch_vtrace_form<false, true>(st, io, p, ws);
    return io.boot ? launch_vtrace_form<true, false>(st, io, p, ws) : launch_vtrace_form<false, false>(st, io, p, ws);
}

}  // namespace rlppo
