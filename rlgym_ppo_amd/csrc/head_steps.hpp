// head_steps.hpp -- the steps the policy-head kernels of heads.hip and hybrid.hip share, each written once: the PPO surrogate of one
// row and its report statistics, the completion words of a sampling kernel, one term of the diagonal-Gaussian log-probability and the
// decoding of a stored multi-discrete index.
#pragma once
#include "common.hpp"

namespace rlppo {

// ------------------------------------------------------------------------------------ shared loss pieces
// d/d(ratio) of min(ratio*A, clamp(ratio)*A), divided by A
__device__ __forceinline__ float surrogate_weight(float ratio, float adv, const LossCfg &c, float &s_min) {
    const float s1 = ratio * adv;
    const float cl = fminf(fmaxf(ratio, c.clip_lo), c.clip_hi);
    const float s2 = cl * adv;
    const float inr = (ratio >= c.clip_lo && ratio <= c.clip_hi) ? 1.f : 0.f;
    s_min = fminf(s1, s2);
    return s1 < s2 ? 1.f : (s1 > s2 ? inr : 0.5f + 0.5f * inr);
}

// [ABI 7] the advantage the surrogate sees: the stored one, or (A - mean) * scale of the batch (rlppo_adv_stats)
__device__ __forceinline__ float surrogate_adv(float adv, const LossCfg &c) { return c.adv_norm ? (adv - c.adv_norm[0]) * c.adv_norm[1] : adv; }

// The PPO surrogate of one row, the tail of every policy loss kernel: from the row's log-probability, the stored one and the stored
// advantage to the log-ratio, the ratio, the surrogate min(s1, s2) and dL/d(log p)
struct Surrogate {
    float lr, ratio, smin, g_logp;
};
__device__ __forceinline__ Surrogate surrogate_row(float lp, float old_logp, float stored_adv, const LossCfg &c) {
    const float adv = surrogate_adv(stored_adv, c);
    Surrogate t;
    t.lr = lp - old_logp;
    t.ratio = expf(t.lr);
    const float w = surrogate_weight(t.ratio, adv, c, t.smin);
    t.g_logp = c.mb_ratio * (-(adv * w * t.ratio) * c.inv_mb);
    return t;
}
// ... and the row's share of the four report statistics of the policy loss; `entropy` is the row's term of the mean entropy
__device__ __forceinline__ void surrogate_stats_add(float (&st)[5], float entropy, const Surrogate &t, const LossCfg &c) {
    st[RLPPO_STAT_ENTROPY] += entropy;
    st[RLPPO_STAT_KL] += ((t.ratio - 1.f) - t.lr) * c.inv_mb;
    st[RLPPO_STAT_CLIPFRAC] += (fabsf(t.ratio - 1.f) > c.clip ? 1.f : 0.f) * c.inv_mb;
    st[RLPPO_STAT_PLOSS] += -t.smin * c.inv_mb;
}

// [r5] completion words of a sampling kernel that gives a block 256 whole rows = the 16 words 16 b .. 16 b + 15 (rlppo_act_opts.done_words):
// every thread releases its stores at system scope, a barrier, sixteen stores -- the words ride in the call's last kernel instead of
// a launch of their own behind it (one graph node fewer of the small call's eight)
__device__ __forceinline__ void block_done_words(unsigned *done_words, unsigned done_value, int64_t n) {
    if (!done_words) return;  // (uniform)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * 16 + threadIdx.x;
    if (threadIdx.x < 16 && w < (n + 15) / 16) __hip_atomic_store(done_words + w, done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr float DIAG_HALF_LOG_2PI = 0.9189385332046727f;  // log(sqrt(2 pi))
__device__ __forceinline__ float diag_logp_term(float d, float sd, float ls) { return -(d * d) / (2.f * (sd * sd)) - ls - DIAG_HALF_LOG_2PI; }
// the stored action of head h, float-encoded; clamped into [0, b) BEFORE it indexes anything (a value outside its head's range is a
// caller error: the row then trains on the nearest valid action, and no address outside the row is ever formed)
__device__ __forceinline__ int md_action(float a, int b) {
    const int i = (int)a;
    return i < 0 ? 0 : (i >= b ? b - 1 : i);
}

}  // namespace rlppo
