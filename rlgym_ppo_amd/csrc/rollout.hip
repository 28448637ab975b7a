// rollout.hip -- the per-step bookkeeping of a DEVICE-RESIDENT vector environment (batched_agents/vector_agent_manager.py,
// _DeviceEnv): what the host side (_HostEnv) keeps in numpy between two environment steps -- rewards / flags of the step, episode sums,
// the 0.9 / 0.1 episode-reward average, the standardisation scalars -- kept on the device, so that a collect never waits for it.
// Launches only: nothing in this file synchronises a stream, copies with the host or allocates.
#include "common.hpp"

namespace rlppo {

static std::atomic<long long> g_cnt_record{0};
long long rollout_record_count() { return g_cnt_record; }

// dtype codes of the environment's arrays (include/rlppo.h, RLPPO_DT_*)
__device__ __forceinline__ float load_as_f32(const void *p, int dt, int64_t i) {
    switch (dt) {
        case RLPPO_DT_F32: return static_cast<const float *>(p)[i];
        case RLPPO_DT_F64: return (float)static_cast<const double *>(p)[i];   // one rounding, as numpy's assignment into a float32 row
        default: return (float)static_cast<const unsigned char *>(p)[i];       // bool / uint8
    }
}

constexpr int REC_THREADS = 1024;
constexpr int REC_WAVES = REC_THREADS / 64;

// One workgroup walks the agents in chunks of 1024.  Everything per agent is independent except the average, which the reference
// folds in AGENT ORDER (batched_agent_manager.py:377-399 through _track_rewards): the ended agents of a chunk are compacted in agent
// order -- a ballot per wave, the population count of the lanes below, the waves' counts through LDS -- and thread 0 folds the
// compacted episode sums one after the other: avg = x for the first episode ever, else avg * 0.9 + x * 0.1 as two double
// multiplications and one addition (the intrinsics keep them apart whatever the contraction mode of the translation unit).
// state: int64[3] = { bits of the double average, has-value word, ended-episode counter }.
__global__ __launch_bounds__(REC_THREADS) void rollout_record_kernel(const void *__restrict__ rewards, int r_dt, const void *__restrict__ dones,
                                                                     int d_dt, const void *__restrict__ truncated, int t_dt, int64_t n, int64_t t,
                                                                     int64_t T, float *__restrict__ rdt, double *__restrict__ ep_sums,
                                                                     long long *__restrict__ state, float *__restrict__ patch) {
    __shared__ double s_x[REC_THREADS];
    __shared__ int s_cnt[REC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool flush = t == T - 1;
    float *r_out = rdt + (0 * T + t) * n, *d_out = rdt + (1 * T + t) * n, *t_out = rdt + (2 * T + t) * n;
    double avg = 0.0;
    long long has = 0, ended_total = 0;
    if (tid == 0) {
        avg = __longlong_as_double(state[0]);
        has = state[1];
        ended_total = state[2];
    }
    for (int64_t base = 0; base < n; base += REC_THREADS) {
        const int64_t a = base + tid;
        bool ended = false;
        double x = 0.0;
        if (a < n) {
            const float r = load_as_f32(rewards, r_dt, a);
            const bool d = load_as_f32(dones, d_dt, a) != 0.0f;
            const bool tr = truncated != nullptr && load_as_f32(truncated, t_dt, a) != 0.0f;
            ended = d || tr;                                    // the environment's own flags, before the flush rule
            x = __dadd_rn(ep_sums[a], (double)r);
            ep_sums[a] = ended ? 0.0 : x;
            r_out[a] = r;
            d_out[a] = d ? 1.0f : 0.0f;
            t_out[a] = flush ? (d ? 0.0f : 1.0f) : (tr ? 1.0f : 0.0f);   // quirk Q4 on what is STORED
            if (patch != nullptr) patch[a] = (tr && !d) ? 1.0f : 0.0f;
        }
        const unsigned long long votes = __ballot(ended);
        if (lane == 0) s_cnt[wave] = __popcll(votes);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < REC_WAVES; ++w) {
            const int c = s_cnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (ended) s_x[before + __popcll(votes & ((1ull << lane) - 1ull))] = x;
        __syncthreads();   // (s_cnt is rewritten only behind the NEXT chunk's first barrier, which thread 0 reaches after its fold)
        if (tid == 0) {
            for (int i = 0; i < total; ++i) {
                const double e = s_x[i];
                avg = has ? __dadd_rn(__dmul_rn(avg, 0.9), __dmul_rn(e, 0.1)) : e;
                has = 1;
            }
            ended_total += total;
        }
        __syncthreads();   // s_x is free again
    }
    if (tid == 0) {
        state[0] = __double_as_longlong(avg);
        state[1] = has;
        state[2] = ended_total;
    }
}

int launch_rollout_record(hipStream_t st, const void *rewards, int r_dt, const void *dones, int d_dt, const void *truncated, int t_dt,
                          int64_t n, int64_t t, int64_t T, float *rdt, double *ep_sums, void *state, float *patch) {
    hipLaunchKernelGGL(rollout_record_kernel, dim3(1), dim3(REC_THREADS), 0, st, rewards, r_dt, dones, d_dt, truncated, t_dt, n, t, T, rdt,
                       ep_sums, static_cast<long long *>(state), patch);
    RLPPO_LAUNCH_CHECK();
    ++g_cnt_record;
    return 0;
}

// WelfordRunningStat.mean / .std (running_stats.py:100-117) of the state as it stands, for the HOST-KNOWN count, as the float32
// vectors the standardising kernels read (mode 2 of rlppo_discrete_step, rlppo_pad_rows_per_feature): var = m2 / (count - 1) in the
// state's dtype (numpy: array / Python int), 1 where it is 0, the IEEE square root, then ONE rounding to float32 (none for a
// float32 state).  per_feature = 0: every entry holds feature 0's pair (quirk Q5).
template <typename T>
__device__ __forceinline__ T sqrt_rn(T v);
template <>
__device__ __forceinline__ float sqrt_rn<float>(float v) { return __fsqrt_rn(v); }
template <>
__device__ __forceinline__ double sqrt_rn<double>(double v) { return __dsqrt_rn(v); }
template <typename T>
__device__ __forceinline__ T div_rn(T a, T b);
template <>
__device__ __forceinline__ float div_rn<float>(float a, float b) { return __fdiv_rn(a, b); }
template <>
__device__ __forceinline__ double div_rn<double>(double a, double b) { return __ddiv_rn(a, b); }

template <typename T>
__global__ __launch_bounds__(128) void obs_scalars_kernel(const T *__restrict__ mean, const T *__restrict__ m2, long long count, int d,
                                                          int per_feature, float *__restrict__ mean_v, float *__restrict__ std_v) {
    const int f = blockIdx.x * 128 + threadIdx.x;
    if (f >= d) return;
    if (count < 2) {
        mean_v[f] = 0.0f;
        std_v[f] = 1.0f;
        return;
    }
    const int src = per_feature ? f : 0;
    T var = div_rn<T>(m2[src], (T)(count - 1));
    if (var == (T)0) var = (T)1;
    mean_v[f] = (float)mean[src];
    std_v[f] = (float)sqrt_rn<T>(var);
}

int launch_obs_scalars(hipStream_t st, const void *mean, const void *m2, int state_f64, long long count, int d, int per_feature,
                       float *mean_v, float *std_v) {
    const dim3 grid((unsigned)cdiv(d, 128));
    if (state_f64)
        hipLaunchKernelGGL(obs_scalars_kernel<double>, grid, dim3(128), 0, st, static_cast<const double *>(mean),
                           static_cast<const double *>(m2), count, d, per_feature, mean_v, std_v);
    else
        hipLaunchKernelGGL(obs_scalars_kernel<float>, grid, dim3(128), 0, st, static_cast<const float *>(mean),
                           static_cast<const float *>(m2), count, d, per_feature, mean_v, std_v);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// Time-major rollout storage -> the reference's trajectory-major arrays, once per collect and in one launch.  A thread moves 16
// bytes of one row S[t][a] (ld / 4 threads per row, rows in storage order: the reads are one contiguous stream) and stores them up
// to twice: as state row a * T + t (t < T) and as next-state row a * T + t - 1 (t >= 1) -- unless the step's patch entry is set, when
// the next-state row is the staged final observation instead.  The first thread of a row with t < T also moves the step's scalars.
__global__ __launch_bounds__(256) void to_trajectory_major_kernel(const float4 *__restrict__ S, const float *__restrict__ acts,
                                                                  const float *__restrict__ logp, const float *__restrict__ rdt, int64_t n,
                                                                  int64_t T, int ld4, int k, const float *__restrict__ patch,
                                                                  const float4 *__restrict__ final_rows, float4 *__restrict__ flat,
                                                                  float4 *__restrict__ nxt, float *__restrict__ actions,
                                                                  float *__restrict__ log_probs, float *__restrict__ rewards,
                                                                  float *__restrict__ dones, float *__restrict__ truncated) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rows = (T + 1) * n;
    if (i >= rows * ld4) return;
    const int64_t row = i / ld4;
    const int c = (int)(i - row * ld4);
    const int64_t t = row / n, a = row - t * n;
    const float4 v = S[i];
    if (t < T) {
        const int64_t o = a * T + t;
        flat[o * ld4 + c] = v;
        if (c == 0) {
            const int64_t s = t * n + a;
            for (int j = 0; j < k; ++j) actions[o * k + j] = acts[s * k + j];
            log_probs[o] = logp[s];
            rewards[o] = rdt[s];
            dones[o] = rdt[T * n + s];
            truncated[o] = rdt[2 * T * n + s];
        }
    } else if (a == n - 1) {
        flat[T * n * ld4 + c] = v;   // flat[N] = S[T][n - 1]: the row add_new_experience appends (learner.py:347)
    }
    if (t >= 1) {
        const int64_t s = (t - 1) * n + a;
        float4 w = v;
        if (patch != nullptr && patch[s] != 0.0f) w = final_rows[s * ld4 + c];
        nxt[(a * T + t - 1) * ld4 + c] = w;
    }
}

int launch_to_trajectory_major(hipStream_t st, const float *S, const float *acts, const float *logp, const float *rdt, int64_t n, int64_t T,
                               int ld, int k, const float *patch, const float *final_rows, float *flat, float *nxt, float *actions,
                               float *log_probs, float *rewards, float *dones, float *truncated) {
    const int ld4 = ld / 4;
    const int64_t lanes = (T + 1) * n * ld4;
    hipLaunchKernelGGL(to_trajectory_major_kernel, dim3((unsigned)cdiv(lanes, 256)), dim3(256), 0, st, reinterpret_cast<const float4 *>(S),
                       acts, logp, rdt, n, T, ld4, k, patch, reinterpret_cast<const float4 *>(final_rows), reinterpret_cast<float4 *>(flat),
                       reinterpret_cast<float4 *>(nxt), actions, log_probs, rewards, dones, truncated);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo
