// heads.hip -- action-head kernels: sampling for rollout inference and the fused loss epilogue of the PPO update.
//
// Discrete head: a row's logits are held in registers, spread over lanes by a row layout (WaveRow: one wave per row, EPL strided
// logits per lane, wave-shuffle reductions; Lanes16, the loss up to 128 padded columns: 16 lanes per row, DPP reductions), and each
// kernel -- sampling, probabilities, loss -- is one body over a layout (max, sum-exp, entropy, the softmax-Jacobian dot product,
// arg-max of p/q).  The chain is the reference's literal softmax -> clamp(1e-11, 1) -> log (discrete_policy.py:52-54,70-78), NOT
// log_softmax, including the clamp's zero-gradient region and torch.min's tie rule.
// Gaussian / multi-discrete heads have 16 / 21 outputs per row: one thread per row, everything in registers.
// Every policy loss kernel ends in the same PPO surrogate (surrogate_row, surrogate_stats_add); dispatch_discrete picks a discrete
// kernel's instantiation from the row width and the presence of a mask.
// [nvec] The multi-discrete head for MultiDiscrete(nvec) of any nvec (up to 64 heads of up to 64 bins, 512 logits): a general
// sampling and a general loss kernel next to the fixed two, one thread per row, no per-row array (at the end of this file).
//
// [ABI 8] Invalid-action masking (discrete head): every discrete kernel has a MASKED instantiation (template parameter).  A row's
// mask is W = ceil(A / 32) words, bit c % 32 of word c / 32 = action c valid.  An invalid action's logit is -inf, as the padded columns c >= A always were: p = 0 exactly, no candidate of the arg-max, no term of
// the entropy, dL/dz = 0.  A row without a valid action counts as all-valid.  The loss kernels do NOT get the words through the
// minibatch gather: they read row idx[r]'s words straight from the buffer's mask field through the logical -> physical ring map
// (MaskRows below) -- the workspace plan and the gather launches of a pass are the same with and without a mask.
#include <type_traits>

#include "common.hpp"

namespace rlppo {

constexpr float PROB_MIN = 1e-11f;

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

// softmax + clamp of one row: p holds the lane's logits (-inf where !in(e)) and leaves as the probabilities, pc as the clamped ones
template <class L, class In>
__device__ __forceinline__ void softmax_clamp(float (&p)[L::EPL], float (&pc)[L::EPL], In in) {
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) mx = fmaxf(mx, p[e]);
    mx = L::max(mx);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) {
        p[e] = in(e) ? expf(p[e] - mx) : 0.f;
        s += p[e];
    }
    s = L::sum(s);
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) {
        p[e] = p[e] / s;
        pc[e] = fminf(fmaxf(p[e], PROB_MIN), 1.0f);
    }
}

// Width dispatch of the discrete kernels: widths up to 128 / 512 / 2048 take 2 / 8 / 32 elements per lane, and a mask selects the
// MASKED instantiations.  f(epl, masked) gets both as compile-time constants (std::integral_constant, std::bool_constant).
template <class F>
static int dispatch_discrete(int width, bool masked, F f) {
    const auto with_mask = [&](auto epl) {
        if (masked)
            f(epl, std::true_type{});
        else
            f(epl, std::false_type{});
    };
    if (width <= 128)
        with_mask(std::integral_constant<int, 2>{});
    else if (width <= 512)
        with_mask(std::integral_constant<int, 8>{});
    else if (width <= 2048)
        with_mask(std::integral_constant<int, 32>{});
    else {
        set_error("discrete head: n_actions=%d > 2048 unsupported", width);
        return RLPPO_ERR_ARG;
    }
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ----------------------------------------------------------------------------------- discrete: sampling
// action = argmax_c pc[c] / q[c] (first index wins ties), logp = log(pc[action]).  `from_probs`: the row already
// holds clamped probabilities (rlppo_categorical_select).  MASKED [ABI 8]: mask[n][W] words; only valid actions are candidates (the
// clamp's 1e-11 never makes an invalid one selectable), probs_out is 0 on invalid actions; the noise stays [n][A].
template <int EPL, bool FROM_PROBS, bool MASKED>
__global__ __launch_bounds__(256) void discrete_sample_kernel(const float *__restrict__ src, int64_t ld, int64_t n,
                                                               int A, const float *__restrict__ noise,
                                                               int64_t *__restrict__ actions, float *__restrict__ logp,
                                                               float *__restrict__ probs_out,
                                                               const unsigned *__restrict__ mask, int W) {
    typedef WaveRow<EPL> L;
    const L lay;
    const int64_t row = (int64_t)blockIdx.x * L::ROWS + lay.group;
    if (row >= n) return;
    float p[EPL], pc[EPL];
    const float *z = src + row * ld;
    unsigned valid = 0;
    if (MASKED) valid = lay.valid_bits(mask + row * W, A);
    const auto in = [&](int e) { return MASKED ? ((valid >> e) & 1u) != 0 : lay.col(e) < A; };
    if (FROM_PROBS) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) pc[e] = in(e) ? z[lay.col(e)] : 0.f;
    } else {
        lay.load(z, ld, p, in);
        softmax_clamp<L>(p, pc, in);
    }
    float best = -INFINITY;
    int besti = 0x7fffffff;
    float bestp = 1.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lay.col(e);
        const int64_t i = row * A + c;  // element c of the row in noise and probs_out, both [n][A]
        if (in(e)) {
            const float v = pc[e] / noise[i];  // IEEE fp32 division, as at::div
            if (v > best) {
                best = v;
                besti = c;
                bestp = pc[e];
            }
        }
        if (probs_out && c < A) probs_out[i] = in(e) ? pc[e] : 0.f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(besti, o);
        const float op = __shfl_xor(bestp, o);
        if (ov > best || (ov == best && oi < besti)) {
            best = ov;
            besti = oi;
            bestp = op;
        }
    }
    if (lay.writer()) {
        actions[row] = besti;
        logp[row] = logf(bestp);
    }
}

template <bool FROM_PROBS>
static int launch_discrete_sample(hipStream_t st, const float *src, int64_t ld, int64_t n, int A, const float *noise,
                                  int64_t *actions, float *logp, float *probs_out, const unsigned *mask = nullptr, int W = 0) {
    if (n <= 0) return 0;
    if (FROM_PROBS) mask = nullptr;
    RLPPO_CHECK_ARG(!mask || W == (A + 31) / 32, "discrete head: mask_words=%d, n_actions=%d needs %d", W, A, (A + 31) / 32);
    return dispatch_discrete(A, mask != nullptr, [&](auto epl, auto masked) {
        hipLaunchKernelGGL((discrete_sample_kernel<decltype(epl)::value, FROM_PROBS, !FROM_PROBS && decltype(masked)::value>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, src,
                           ld, n, A, noise, actions, logp, probs_out, mask, W);
    });
}

int launch_discrete_sample_logits(hipStream_t st, const float *logits, int64_t ld, int64_t n, int A, const float *noise,
                                  int64_t *actions, float *logp, float *probs_out, const unsigned *mask, int mask_words) {
    return launch_discrete_sample<false>(st, logits, ld, n, A, noise, actions, logp, probs_out, mask, mask_words);
}
int launch_categorical_select(hipStream_t st, const float *probs, int64_t ld, int64_t n, int A, const float *noise,
                              int64_t *actions, float *logp) {
    return launch_discrete_sample<true>(st, probs, ld, n, A, noise, actions, logp, nullptr);
}

// ---------------------------------------------------------------- discrete: probabilities / deterministic choice
// DiscreteFF.get_output (discrete_policy.py:34-42: softmax) and the deterministic branch of get_action (:52-57: clamp, then
// numpy's argmax over the FLATTENED [n, A] array -- quirk Q11: one index for the whole batch, first occurrence of the maximum).
// The flat arg-max is one 64-bit atomic max per row on key = (float bits of the row maximum << 32) | ~flat index: clamped
// probabilities are positive, so their bit patterns order like the values, and of equal values the smaller flat index wins.
// MASKED [ABI 8]: invalid actions read 0 (with and without the clamp) and are no candidates of the arg-max.
template <int EPL, bool MASKED>
__global__ __launch_bounds__(256) void discrete_probs_kernel(const float *__restrict__ logits, int64_t ld, int64_t n, int A,
                                                              int clamp, float *__restrict__ probs, int64_t ld_p,
                                                              unsigned long long *__restrict__ key,
                                                              const unsigned *__restrict__ mask, int W) {
    typedef WaveRow<EPL> L;
    const L lay;
    const int64_t row = (int64_t)blockIdx.x * L::ROWS + lay.group;
    if (row >= n) return;
    float p[EPL], pc[EPL];
    unsigned valid = 0;
    if (MASKED) valid = lay.valid_bits(mask + row * W, A);
    const auto in = [&](int e) { return MASKED ? ((valid >> e) & 1u) != 0 : lay.col(e) < A; };
    lay.load(logits + row * ld, ld, p, in);
    softmax_clamp<L>(p, pc, in);
    float best = -1.f;
    int besti = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int c = lay.col(e);
        if (probs && c < A) probs[row * ld_p + c] = in(e) ? (clamp ? pc[e] : p[e]) : 0.f;
        if (in(e) && pc[e] > best) {
            best = pc[e];
            besti = c;
        }
    }
    if (!key) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(besti, o);
        if (ov > best || (ov == best && oi < besti)) {
            best = ov;
            besti = oi;
        }
    }
    if (lay.writer()) {
        const unsigned long long flat = (unsigned long long)(row * A + besti);
        atomicMax(key, ((unsigned long long)__float_as_uint(best) << 32) | (0xffffffffull - flat));
    }
}
__global__ void decode_flat_argmax_kernel(unsigned long long *key) {
    *(long long *)key = (long long)(0xffffffffull - (*key & 0xffffffffull));
}

int launch_discrete_probs(hipStream_t st, const float *logits, int64_t ld, int64_t n, int A, int clamp, float *probs,
                          int64_t ld_p, int64_t *flat_argmax, const unsigned *mask, int W) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(!mask || W == (A + 31) / 32, "discrete head: mask_words=%d, n_actions=%d needs %d", W, A, (A + 31) / 32);
    if (flat_argmax && (unsigned long long)n * (unsigned long long)A > 0xffffffffull) {
        set_error("discrete_probs: n * n_actions exceeds the 32-bit flat index of the arg-max key");
        return RLPPO_ERR_ARG;
    }
    unsigned long long *key = (unsigned long long *)flat_argmax;
    if (key) RLPPO_HIP(hipMemsetAsync(key, 0, sizeof(*key), st));
    const int rc = dispatch_discrete(A, mask != nullptr, [&](auto epl, auto masked) {
        hipLaunchKernelGGL((discrete_probs_kernel<decltype(epl)::value, decltype(masked)::value>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, logits, ld, n, A, clamp, probs,
                           ld_p, key, mask, W);
    });
    if (rc) return rc;
    if (key) {
        hipLaunchKernelGGL(decode_flat_argmax_kernel, dim3(1), dim3(1), 0, st, key);
        RLPPO_LAUNCH_CHECK();
    }
    return 0;
}

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

// The grids of the policy loss launches: block b's KL sum lands in kl_slots[2 + b], so kl_slots_doubles sizes the slots from them.
constexpr int64_t DISCRETE_LOSS_MAX_BLOCKS = 2048;  // the discrete loss strides its grid over the rows
static unsigned discrete_loss_grid(int64_t mb, int rows_per_block) {
    const int64_t g = cdiv(mb, rows_per_block);
    return (unsigned)(g < DISCRETE_LOSS_MAX_BLOCKS ? g : DISCRETE_LOSS_MAX_BLOCKS);
}
static unsigned thread_per_row_grid(int64_t mb) { return (unsigned)cdiv(mb, 256); }  // gaussian / multi-discrete: one thread per row
int64_t kl_slots_doubles(int64_t mb) {
    const int64_t g = thread_per_row_grid(mb > 0 ? mb : 1);
    return 2 + (g > DISCRETE_LOSS_MAX_BLOCKS ? g : DISCRETE_LOSS_MAX_BLOCKS);
}

// value loss for one row: writes dL/dv in place, returns (v - t)^2.  [ABI 7] vclip > 0: Stable-Baselines3's clipped prediction
// v_pred = v_old + clamp(v - v_old, -c, c) around v_old = target - A (the buffer's target is V + A), loss (v_pred - t)^2, gradient
// where |v - v_old| <= c (torch.clamp passes it at its bounds)
// [vnorm] c.vnorm = {mu, 1/sigma, ...}: v is a NORMALISED value; the target becomes (target - mu) * (1/sigma) -- a float32 subtraction,
// then a float32 multiplication -- and under clipping so does v_old = target - A (rl_games: clipping in normalised units).  The rest
// of the row is the code it always was, on the normalised numbers.
__device__ __forceinline__ float value_row(float *vout_row, float target, float adv, const LossCfg &c) {
    const float v = vout_row[0];
    float v_old_n = 0.f;
    if (c.vnorm) {
        const float mu = c.vnorm[0], inv_sd = c.vnorm[1];
        if (c.vclip > 0.f) v_old_n = __fmul_rn(__fsub_rn(__fsub_rn(target, adv), mu), inv_sd);
        target = __fmul_rn(__fsub_rn(target, mu), inv_sd);
    }
    if (c.vclip > 0.f) {
        const float v_old = c.vnorm ? v_old_n : target - adv;
        const float dv = v - v_old;
        const float d = (v_old + fminf(fmaxf(dv, -c.vclip), c.vclip)) - target;
        vout_row[0] = fabsf(dv) <= c.vclip ? c.mb_ratio * (2.f * d * c.inv_mb) : 0.f;
        return d * d;
    }
    const float d = v - target;
    vout_row[0] = c.mb_ratio * (2.f * d * c.inv_mb);
    return d * d;
}

// ----------------------------------------------------------------------------------- discrete: loss + grad
// logits[row][0:A] is overwritten with dL/dlogits.  One body for both layouts (L = Lanes16 up to a padded width of 128, WaveRow<8> and
// WaveRow<32> above); the block strides over the rows and the statistics stay in registers, so a launch issues 5 atomics per BLOCK.
// MASKED [ABI 8]: the row's mask words come from the buffer's mask field at the physical row of idx[row] (MaskRows); invalid
// actions have p = 0, no entropy term and dL/dz = 0.  A stored action its own mask marks invalid (a caller error) takes the literal
// chain: pc_a = 1e-11 inside the clamp's zero-gradient region -- finite, no gradient.
template <class L, bool MASKED>
__global__ __launch_bounds__(256) void discrete_loss_kernel(float *__restrict__ logits, int64_t ld, int A,
                                                             const float *__restrict__ actions,
                                                             const float *__restrict__ old_logp,
                                                             const float *__restrict__ advantages, int64_t mb,
                                                             LossCfg cfg, double *__restrict__ stats, MaskRows mr) {
    constexpr int EPL = L::EPL;
    const L lay;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t base = (int64_t)blockIdx.x * L::ROWS; base < mb; base += (int64_t)gridDim.x * L::ROWS) {
        const bool live = base + lay.group < mb;
        if (!L::SHADOW && !live) break;
        const int64_t row = live ? base + lay.group : mb - 1;
        float *z = logits + row * ld;
        unsigned valid = 0;
        if (MASKED) valid = lay.valid_bits(mr.mask + ring_row(mr.idx[row], mr.ring_base, mr.ring_cap) * mr.W, A);
        const auto in = [&](int e) { return MASKED ? ((valid >> e) & 1u) != 0 : lay.col(e) < A; };
        float p[EPL], pc[EPL], lp[EPL];
        lay.load(z, ld, p, in);
        softmax_clamp<L>(p, pc, in);
        const int a = (int)actions[row];  // acts.long() of a float-encoded index (discrete_policy.py:71)
        float ent = 0.f, lpa = 0.f, pca = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            lp[e] = in(e) ? logf(pc[e]) : 0.f;
            if (in(e)) ent -= lp[e] * pc[e];
            if (lay.col(e) == a) {
                lpa = MASKED && !in(e) ? logf(pc[e]) : lp[e];
                pca = pc[e];
            }
        }
        ent = L::sum(ent);
        lpa = L::sum(lpa);  // exactly one lane holds a non-zero term
        pca = L::sum(pca);
        const Surrogate t = surrogate_row(lpa, old_logp[row], advantages[row], cfg);
        const float g_ent = cfg.mb_ratio * (cfg.ent_coef * cfg.inv_mb);
        float g[EPL];
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            g[e] = 0.f;
            if (in(e)) {
                g[e] = g_ent * (lp[e] + 1.f);
                if (lay.col(e) == a) g[e] += t.g_logp / pca;
                if (!(p[e] >= PROB_MIN)) g[e] = 0.f;  // clamp passes gradient on [1e-11, 1] only
            }
            dot += g[e] * p[e];
        }
        dot = L::sum(dot);
#pragma unroll
        for (int e = 0; e < EPL; ++e) g[e] = in(e) ? p[e] * (g[e] - dot) : 0.f;
        if (live) lay.store(z, ld, g);
        if (live && lay.writer()) surrogate_stats_add(st, ent * cfg.inv_mb, t, cfg);
    }
    block_stats_add(stats, st, true, cfg, cfg.kl_slots);
}

// Value loss on its own (value_estimator + ppo_learner.py:163-166: MSE(vals, target_values)): v -> d loss / d v in place,
// VLOSS statistic.  A separate launch so that the critic's launch chain never has to meet the policy's between the
// forward and the backward pass: the two chains only join at the end of the minibatch.
__global__ __launch_bounds__(256) void value_loss_kernel(float *__restrict__ vout, int64_t ldv, const float *__restrict__ targets,
                                                         const float *__restrict__ advantages, int64_t mb, LossCfg cfg,
                                                         double *__restrict__ stats) {
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < mb; row += (int64_t)gridDim.x * 256)
        st[RLPPO_STAT_VLOSS] += value_row(vout + row * ldv, targets[row], cfg.vclip > 0.f ? advantages[row] : 0.f, cfg) * cfg.inv_mb;
    block_stats_add(stats, st, true, cfg);
}

int launch_value_loss(hipStream_t st, float *vout, int64_t ldv, const float *targets, const float *adv, int64_t mb, const LossCfg &cfg,
                      double *stats) {
    if (mb <= 0) return 0;
    RLPPO_CHECK_ARG(!(cfg.vclip > 0.f) || adv, "value loss: clipping needs the advantages");
    dim3 grid((unsigned)(cdiv(mb, 256) < 1024 ? cdiv(mb, 256) : 1024));
    hipLaunchKernelGGL(value_loss_kernel, grid, dim3(256), 0, st, vout, ldv, targets, adv, mb, cfg, stats);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

int launch_discrete_loss(hipStream_t st, float *logits, int64_t ld, int A, const float *actions, const float *old_logp, const float *adv,
                         int64_t mb, const LossCfg &cfg, double *stats, const MaskRows *mr) {
    if (mb <= 0) return 0;
    RLPPO_CHECK_ARG(ld <= DISCRETE_LOSS_MAX_LD, "discrete head: padded width %ld too large", (long)ld);
    const bool masked = mr && mr->mask;
    RLPPO_CHECK_ARG(!masked || (mr->W == (A + 31) / 32 && mr->idx), "discrete head: mask_words=%d, n_actions=%d needs %d", mr->W, A, (A + 31) / 32);
    return dispatch_discrete((int)ld, masked, [&](auto epl, auto is_masked) {
        typedef std::conditional_t<decltype(epl)::value == 2, Lanes16, WaveRow<decltype(epl)::value>> L;  // padded width <= 128: 16 lanes per row
        hipLaunchKernelGGL((discrete_loss_kernel<L, decltype(is_masked)::value>), dim3(discrete_loss_grid(mb, L::ROWS)), dim3(256), 0, st, logits, ld, A, actions,
                           old_logp, adv, mb, cfg, stats, masked ? *mr : MaskRows{});
    });
}

// --------------------------------------------------------------------------------------------- gaussian
// Up to FLOAT_SUM_K action dimensions a row's log-probability (and entropy) is summed in float, in j order.  A serial float sum
// of more terms drifts past the reference's own float32 (torch sums over k with partial sums): at k = 64 the update's gradients
// miss float64 by 1.5e-5.  Wider heads therefore sum the same float terms in double and round once.
constexpr int FLOAT_SUM_K = 32;

__device__ __forceinline__ float gauss_logpdf(float x, float mean, float sd) {
    // the reference's four terms, in its order (continuous_policy.py:54-63)
    const float msq = mean * mean, ssq = sd * sd, xsq = x * x;
    const float t1 = -(msq / (2.f * ssq));
    const float t2 = (mean * x) / ssq;
    const float t3 = -(xsq / (2.f * ssq));
    const float t4 = logf(1.f / sqrtf((float)(2.0 * 3.14159265358979323846) * ssq));
    return t1 + t2 + t3 + t4;
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

// y[row][0:2k] holds tanh outputs.  action = clamp(mean + sd*eps, -1, 1); logp = sum logpdf(action)
__global__ __launch_bounds__(256) void gaussian_sample_kernel(const float *__restrict__ y, int64_t ld, int64_t n, int k,
                                                               const float *__restrict__ eps, float var_m, float var_b,
                                                               float *__restrict__ actions, float *__restrict__ logp,
                                                               unsigned *done_words, unsigned done_value) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row < n) {
        const float *yr = y + row * ld;
        float lp = 0.f;
        double lpd = 0.0;  // (k > FLOAT_SUM_K)
        for (int j = 0; j < k; ++j) {
            const float mean = yr[j];
            const float sd = yr[k + j] * var_m + var_b;
            float a = eps[row * k + j] * sd + mean;  // at::normal: output.mul_(std).add_(mean)
            a = fminf(fmaxf(a, -1.f), 1.f);
            actions[row * k + j] = a;
            if (k <= FLOAT_SUM_K)
                lp += gauss_logpdf(a, mean, sd);
            else
                lpd += (double)gauss_logpdf(a, mean, sd);
        }
        logp[row] = k <= FLOAT_SUM_K ? lp : (float)lpd;
    }
    block_done_words(done_words, done_value, n);
}

int launch_gaussian_sample(hipStream_t st, const float *y, int64_t ld, int64_t n, int k, const float *eps, float var_m,
                           float var_b, float *actions, float *logp, unsigned *done_words, unsigned done_value) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, y, ld, n, k, eps, var_m,
                       var_b, actions, logp, done_words, done_value);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// y[row][0:2k] (tanh outputs) is overwritten with dL/d(pre-tanh) ; entropy = mean over ALL mb*k elements (quirk Q8)
__global__ __launch_bounds__(256) void gaussian_loss_kernel(float *__restrict__ y, int64_t ld, int k,
                                                             const float *__restrict__ actions,
                                                             const float *__restrict__ old_logp,
                                                             const float *__restrict__ advantages, int64_t mb,
                                                             LossCfg cfg, double *__restrict__ stats) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = row < mb;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (active) {
        float *yr = y + row * ld;
        const float *xr = actions + row * k;
        float lp = 0.f, ent = 0.f;
        if (k <= FLOAT_SUM_K) {
#pragma unroll 4
            for (int j = 0; j < k; ++j) {
                const float mean = yr[j], sd = yr[k + j] * cfg.var_m + cfg.var_b;
                lp += gauss_logpdf(xr[j], mean, sd);
                ent += 1.4189385332046727f + logf(sd);  // 0.5 + 0.5*log(2*pi) + log(sd): Normal.entropy()
            }
        } else {  // the same terms, summed in double (FLOAT_SUM_K)
            double lpd = 0.0, entd = 0.0;
#pragma unroll 4
            for (int j = 0; j < k; ++j) {
                const float mean = yr[j], sd = yr[k + j] * cfg.var_m + cfg.var_b;
                lpd += (double)gauss_logpdf(xr[j], mean, sd);
                entd += (double)(1.4189385332046727f + logf(sd));
            }
            lp = (float)lpd;
            ent = (float)entd;
        }
        const Surrogate t = surrogate_row(lp, old_logp[row], advantages[row], cfg);
        const float g_ent = -cfg.mb_ratio * cfg.ent_coef * cfg.inv_mb / (float)k;  // d(-c_H * H)/d log sd
        // (no per-row arrays, so any k: the second pass re-reads mean / sd / x -- element j is overwritten only after its own reads)
#pragma unroll 4
        for (int j = 0; j < k; ++j) {
            const float ym = yr[j], ys = yr[k + j];
            const float sd = ys * cfg.var_m + cfg.var_b;
            const float d = xr[j] - ym;
            const float s2 = sd * sd;
            const float d_mu = t.g_logp * d / s2;
            const float d_sd = t.g_logp * (d * d / (s2 * sd) - 1.f / sd) + g_ent / sd;
            yr[j] = d_mu * (1.f - ym * ym);
            yr[k + j] = d_sd * cfg.var_m * (1.f - ys * ys);
        }
        surrogate_stats_add(st, ent * cfg.inv_mb / (float)k, t, cfg);
    }
    block_stats_add(stats, st, active, cfg, cfg.kl_slots);
}

int launch_gaussian_loss(hipStream_t st, float *y, int64_t ld, int k, const float *actions, const float *old_logp, const float *adv,
                         int64_t mb, const LossCfg &cfg, double *stats) {
    if (mb <= 0) return 0;
    RLPPO_CHECK_ARG(k >= 1, "gaussian head: action dim %d < 1", k);
    hipLaunchKernelGGL(gaussian_loss_kernel, dim3(thread_per_row_grid(mb)), dim3(256), 0, st, y, ld, k, actions, old_logp, adv, mb,
                       cfg, stats);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------- diagonal Gaussian [diag]
// RLPPO_HEAD_DIAG_GAUSSIAN (include/rlppo.h, "[diag]"): the head of Stable-Baselines3 / CleanRL / rl_games.  y[row][0:k] is the
// network's output as it is (no tanh) = the mean; sigma_j = exp(log_std_j) with log_std a k-float PARAMETER read from device memory
// at run time (a block keeps log_std and sigma in LDS).  Nothing is clamped; log p is Normal.log_prob's three terms in its order;
// the float terms are summed as the Gaussian head above sums its (FLOAT_SUM_K).  One thread per row, no per-row array.
constexpr float DIAG_HALF_LOG_2PI = 0.9189385332046727f;  // log(sqrt(2 pi))
__device__ __forceinline__ float diag_logp_term(float d, float sd, float ls) { return -(d * d) / (2.f * (sd * sd)) - ls - DIAG_HALF_LOG_2PI; }
// (every thread of the block, before anything diverges: the fill ends in a barrier)
__device__ __forceinline__ void diag_fill_lds(const float *__restrict__ log_std, int k, float *s_ls, float *s_sd) {
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const float ls = log_std[j];
        s_ls[j] = ls;
        s_sd[j] = expf(ls);
    }
    __syncthreads();
}

// action = mean + sigma * eps (NOT clamped), logp = sum_j log N(action_j; mean_j, sigma_j)
__global__ __launch_bounds__(256) void diag_gaussian_sample_kernel(const float *__restrict__ y, int64_t ld, int64_t n, int k,
                                                                    const float *__restrict__ eps, const float *__restrict__ log_std,
                                                                    float *__restrict__ actions, float *__restrict__ logp,
                                                                    unsigned *done_words, unsigned done_value) {
    __shared__ float s_ls[RLPPO_DIAG_MAX_K], s_sd[RLPPO_DIAG_MAX_K];
    diag_fill_lds(log_std, k, s_ls, s_sd);
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row < n) {  // (one barrier site behind it for the whole block: see multidiscrete_sample_kernel)
        const float *yr = y + row * ld;
        float lp = 0.f;
        double lpd = 0.0;  // (k > FLOAT_SUM_K)
        for (int j = 0; j < k; ++j) {
            const float mean = yr[j], sd = s_sd[j];
            const float a = eps[row * k + j] * sd + mean;  // at::normal: output.mul_(std).add_(mean)
            actions[row * k + j] = a;
            const float t = diag_logp_term(a - mean, sd, s_ls[j]);  // of the sample as stored: what the update will recompute
            if (k <= FLOAT_SUM_K)
                lp += t;
            else
                lpd += (double)t;
        }
        logp[row] = k <= FLOAT_SUM_K ? lp : (float)lpd;
    }
    block_done_words(done_words, done_value, n);
}

int launch_diag_gaussian_sample(hipStream_t st, const float *y, int64_t ld, int64_t n, int k, const float *eps, const float *log_std,
                                float *actions, float *logp, unsigned *done_words, unsigned done_value) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(k >= 1 && k <= RLPPO_DIAG_MAX_K && k <= ld, "diagonal-Gaussian head: k=%d not in [1, RLPPO_DIAG_MAX_K=%d] (rows of %ld)", k,
                    RLPPO_DIAG_MAX_K, (long)ld);
    hipLaunchKernelGGL(diag_gaussian_sample_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, y, ld, n, k, eps, log_std, actions,
                       logp, done_words, done_value);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// y[row][0:k] (the means) is overwritten with dL/dmean = g_logp (a - mean) / sigma^2.  A row's entropy is sum_j (1/2 + 1/2 log 2 pi +
// log_std_j): summed over the dimensions, NOT divided by k (unlike the Gaussian head above, quirk Q8), the same for every row.
// dL/dlog_std_j is a sum over ALL rows of the pass of g_logp ((a - mean)^2 / sigma^2 - 1) - mb_ratio ent_coef inv_mb: every thread's
// float term is widened to double, summed over the wave (shuffles, a fixed tree), the four waves' sums added in a fixed order, and
// the workgroup's k sums land in ITS row of `partials` [grid][k] -- no atomics; diag_logstd_finish_kernel adds the rows.
__global__ __launch_bounds__(256) void diag_gaussian_loss_kernel(float *__restrict__ y, int64_t ld, int k, const float *__restrict__ actions,
                                                                  const float *__restrict__ old_logp, const float *__restrict__ advantages,
                                                                  int64_t mb, LossCfg cfg, double *__restrict__ stats,
                                                                  const float *__restrict__ log_std, double *__restrict__ partials) {
    __shared__ float s_ls[RLPPO_DIAG_MAX_K], s_sd[RLPPO_DIAG_MAX_K];
    __shared__ double s_red[4][RLPPO_DIAG_MAX_K];
    diag_fill_lds(log_std, k, s_ls, s_sd);
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = row < mb;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    float *yr = y + (active ? row : 0) * ld;
    const float *xr = actions + (active ? row : 0) * k;
    Surrogate t = {};
    if (active) {
        float lp = 0.f, ent = 0.f;
        if (k <= FLOAT_SUM_K) {
#pragma unroll 4
            for (int j = 0; j < k; ++j) {
                lp += diag_logp_term(xr[j] - yr[j], s_sd[j], s_ls[j]);
                ent += 1.4189385332046727f + s_ls[j];  // Normal.entropy(): 0.5 + 0.5*log(2*pi) + log(sd)
            }
        } else {  // the same terms, summed in double (FLOAT_SUM_K)
            double lpd = 0.0, entd = 0.0;
#pragma unroll 4
            for (int j = 0; j < k; ++j) {
                lpd += (double)diag_logp_term(xr[j] - yr[j], s_sd[j], s_ls[j]);
                entd += (double)(1.4189385332046727f + s_ls[j]);
            }
            lp = (float)lpd;
            ent = (float)entd;
        }
        t = surrogate_row(lp, old_logp[row], advantages[row], cfg);
        surrogate_stats_add(st, ent * cfg.inv_mb, t, cfg);
    }
    const float g_ent = -cfg.mb_ratio * cfg.ent_coef * cfg.inv_mb;  // d(-c_H * H_row)/d log_std_j of one row
    // (the loop is uniform over the block: every lane takes part in the wave sums, rows beyond mb with a zero term)
    for (int j = 0; j < k; ++j) {
        float term = 0.f;
        if (active) {
            const float d = xr[j] - yr[j], sd = s_sd[j];
            const float s2 = sd * sd;
            yr[j] = t.g_logp * d / s2;
            term = t.g_logp * (d * d / s2 - 1.f) + g_ent;
        }
        double s = (double)term;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) s_red[wave][j] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x)
        partials[(int64_t)blockIdx.x * k + j] = (s_red[0][j] + s_red[1][j]) + (s_red[2][j] + s_red[3][j]);
    block_stats_add(stats, st, active, cfg, cfg.kl_slots);
}

// log_std_grad[j] += the sum over the workgroups' partial sums of dimension j, in a fixed order: one workgroup per dimension, thread t
// adds rows t, t + 256, ... of `partials`, then the fixed tree over the workgroup.  The one add per element and launch into the
// gradient arena is an atomic, as the weight gradients' is (passes of different slots meet there).
__global__ __launch_bounds__(256) void diag_logstd_finish_kernel(const double *__restrict__ partials, int nblocks, int k,
                                                                  float *__restrict__ grad) {
    const int j = blockIdx.x;
    double a = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 256) a += partials[(int64_t)b * k + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    __shared__ double red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(grad + j, (float)((red[0] + red[1]) + (red[2] + red[3])));
}

size_t diag_scratch_bytes(int64_t mb, int k) { return (size_t)thread_per_row_grid(mb > 0 ? mb : 1) * (size_t)(k > 0 ? k : 1) * sizeof(double); }

int launch_diag_gaussian_loss(hipStream_t st, float *y, int64_t ld, int k, const float *actions, const float *old_logp, const float *adv,
                              int64_t mb, const LossCfg &cfg, double *stats, const DiagHead &dg, int part) {
    if (mb <= 0) return 0;
    RLPPO_CHECK_ARG(k >= 1 && k <= RLPPO_DIAG_MAX_K && k <= ld, "diagonal-Gaussian head: k=%d not in [1, RLPPO_DIAG_MAX_K=%d] (rows of %ld)", k,
                    RLPPO_DIAG_MAX_K, (long)ld);
    RLPPO_CHECK_ARG(dg.log_std && dg.log_std_grad && dg.scratch && dg.scratch_bytes >= diag_scratch_bytes(mb, k),
                    "diagonal-Gaussian head: log_std / log_std_grad / scratch (%zu bytes, %zu needed)", dg.scratch_bytes, diag_scratch_bytes(mb, k));
    const unsigned grid = thread_per_row_grid(mb);
    if (part != 2) {  // (part: rlppo_dbg_diag_loss times the two launches apart; a pass runs both)
        hipLaunchKernelGGL(diag_gaussian_loss_kernel, dim3(grid), dim3(256), 0, st, y, ld, k, actions, old_logp, adv, mb, cfg, stats, dg.log_std,
                           dg.scratch);
        RLPPO_LAUNCH_CHECK();
    }
    if (part != 1) {
        hipLaunchKernelGGL(diag_logstd_finish_kernel, dim3((unsigned)k), dim3(256), 0, st, dg.scratch, (int)grid, k, dg.log_std_grad);
        RLPPO_LAUNCH_CHECK();
    }
    return 0;
}

// ---------------------------------------------------------------------------------------- multi-discrete
// 21 logits = 5 heads of 3 + 3 heads of 2 (multi_discrete_policy.py:20, torch_functions.py:101-113).
__device__ __forceinline__ int md_start(int h) { return h < 5 ? 3 * h : 15 + 2 * (h - 5); }
__device__ __forceinline__ int md_bins(int h) { return h < 5 ? 3 : 2; }

// Categorical(logits).sample() on the [n*8, 3] probability matrix == argmax(p / q) with q[n*8][3]; the padded third
// slot of a 2-way head has p = 0 and never wins.  logp = sum_h log_softmax(z_h)[a_h].
__global__ __launch_bounds__(256) void multidiscrete_sample_kernel(const float *__restrict__ logits, int64_t ld,
                                                                    int64_t n, const float *__restrict__ noise,
                                                                    int64_t *__restrict__ actions,
                                                                    float *__restrict__ logp, unsigned *done_words,
                                                                    unsigned done_value) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (one barrier site for the whole block: a wave whose lanes split at `row < n` would otherwise arrive at the barrier of
    // block_done_words twice -- and release it before its live lanes have stored)
    if (row < n) {
    const float *z = logits + row * ld;
    float lp = 0.f;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        const int s = md_start(h), b = md_bins(h);
        float mx = z[s];
        for (int c = 1; c < b; ++c) mx = fmaxf(mx, z[s + c]);
        float e[3], sum = 0.f;
        for (int c = 0; c < b; ++c) {
            e[c] = expf(z[s + c] - mx);
            sum += e[c];
        }
        const float lse = mx + logf(sum);
        float best = -INFINITY;
        int bi = 0;
        for (int c = 0; c < b; ++c) {
            const float v = (e[c] / sum) / noise[(row * 8 + h) * 3 + c];
            if (v > best) {
                best = v;
                bi = c;
            }
        }
        actions[row * 8 + h] = bi;
        lp += z[s + bi] - lse;
    }
    logp[row] = lp;
    }
    block_done_words(done_words, done_value, n);
}

int launch_multidiscrete_sample(hipStream_t st, const float *logits, int64_t ld, int64_t n, const float *noise,
                                int64_t *actions, float *logp, unsigned *done_words, unsigned done_value) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(multidiscrete_sample_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, logits, ld, n, noise,
                       actions, logp, done_words, done_value);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(256) void multidiscrete_loss_kernel(float *__restrict__ logits, int64_t ld,
                                                                  const float *__restrict__ actions,
                                                                  const float *__restrict__ old_logp,
                                                                  const float *__restrict__ advantages, int64_t mb,
                                                                  LossCfg cfg, double *__restrict__ stats) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = row < mb;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (active) {
        float *z = logits + row * ld;
        float ls[21], ph[21], eh[8];
        int act[8];
        float lp = 0.f, ent = 0.f;
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int s = md_start(h), b = md_bins(h);
            float mx = z[s];
            for (int c = 1; c < b; ++c) mx = fmaxf(mx, z[s + c]);
            float sum = 0.f;
            for (int c = 0; c < b; ++c) sum += expf(z[s + c] - mx);
            const float lse = mx + logf(sum);
            float e = 0.f;
            for (int c = 0; c < b; ++c) {
                ls[s + c] = z[s + c] - lse;
                ph[s + c] = expf(ls[s + c]);
                e -= ph[s + c] * ls[s + c];
            }
            eh[h] = e;
            ent += e;
            act[h] = (int)actions[row * 8 + h];
            lp += ls[s + act[h]];
        }
        const Surrogate t = surrogate_row(lp, old_logp[row], advantages[row], cfg);
        const float g_ent = -cfg.mb_ratio * cfg.ent_coef * cfg.inv_mb;  // coefficient of d(entropy_row)/dz
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int s = md_start(h), b = md_bins(h);
            for (int c = 0; c < b; ++c) {
                const float onehot = (c == act[h]) ? 1.f : 0.f;
                z[s + c] = t.g_logp * (onehot - ph[s + c]) + g_ent * (-ph[s + c] * (ls[s + c] + eh[h]));
            }
        }
        for (int c = 21; c < ld; ++c) z[c] = 0.f;
        surrogate_stats_add(st, ent * cfg.inv_mb, t, cfg);
    }
    block_stats_add(stats, st, active, cfg, cfg.kl_slots);
}

int launch_multidiscrete_loss(hipStream_t st, float *logits, int64_t ld, const float *actions, const float *old_logp, const float *adv,
                              int64_t mb, const LossCfg &cfg, double *stats) {
    if (mb <= 0) return 0;
    hipLaunchKernelGGL(multidiscrete_loss_kernel, dim3(thread_per_row_grid(mb)), dim3(256), 0, st, logits, ld, actions, old_logp,
                       adv, mb, cfg, stats);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------ multi-discrete, any nvec [nvec]
// MultiDiscreteRolv's construction with the bins as a parameter: head h owns logits [s_h, s_h + b_h), s_h = b_0 + .. + b_(h-1).  The
// two kernels above stay as they are (their loops unroll completely, so their per-row arrays live in registers); with run-time bins
// the same arrays would be run-time indexed and land in scratch, so these two keep NO per-row array: one thread per row walks the
// heads, and whatever a later step needs again (a head's maximum, its sum, its entropy) is recomputed from the logits, which the
// first walk has left in the cache.  The spec travels by value in the kernel arguments (a uniform index: scalar loads).
int md_spec_make(const int32_t *nvec, int n_heads, const char *who, MdSpec *spec) {
    RLPPO_CHECK_ARG(nvec != nullptr, "%s: nvec is NULL", who);
    RLPPO_CHECK_ARG(n_heads >= 1 && n_heads <= RLPPO_MD_MAX_HEADS, "%s: %d heads, RLPPO_MD_MAX_HEADS allows 1 .. %d", who, n_heads,
                    RLPPO_MD_MAX_HEADS);
    MdSpec s = {};
    s.H = n_heads;
    for (int h = 0; h < n_heads; ++h) {
        RLPPO_CHECK_ARG(nvec[h] >= 1 && nvec[h] <= RLPPO_MD_MAX_BINS, "%s: nvec[%d]=%d, RLPPO_MD_MAX_BINS allows 1 .. %d", who, h, nvec[h],
                        RLPPO_MD_MAX_BINS);
        s.b[h] = (unsigned char)nvec[h];
        s.S += nvec[h];
        s.B = nvec[h] > s.B ? nvec[h] : s.B;
    }
    RLPPO_CHECK_ARG(s.S <= RLPPO_MD_MAX_LOGITS, "%s: sum of nvec = %d logits, RLPPO_MD_MAX_LOGITS allows %d", who, s.S, RLPPO_MD_MAX_LOGITS);
    *spec = s;
    return 0;
}

// [nvec, masked] Invalid-action masking of the general kernels (template <bool MASKED>; the unmasked instantiations keep the
// arithmetic and its order as they were -- the generated code of the sampling kernel differs by one instruction: DESIGN.md, 8b).  A mask row has W = ceil(S / 32) words, one bit per logit (bit c % 32 of word c / 32 set = logit c valid, bits at and
// beyond S ignored); head h owns bits [s_h, s_h + b_h).  A head has at most 64 bins, so its valid set V_h is ONE 64-bit value
// assembled from the two or three words it touches (md_head_valid) -- no per-row array.  Invalid bins are -inf: no candidate of the
// maximum, the sums or the arg-max, gradient exactly 0, noise never read; the maximum and the sums run over the valid bins in c
// order, so an all-valid mask gives the unmasked results bit for bit.  A head without a valid bin counts as all-valid.
__device__ __forceinline__ unsigned long long md_head_valid(const unsigned *__restrict__ words, int s, int b) {
    const int w0 = s >> 5, sh = s & 31, wl = (s + b - 1) >> 5;  // (wl <= (S - 1) / 32 < W: every word read lies inside the row)
    unsigned long long lo = words[w0];
    if (wl > w0) lo |= (unsigned long long)words[w0 + 1] << 32;
    unsigned long long v = lo >> sh;
    if (wl > w0 + 1) v |= (unsigned long long)words[w0 + 2] << (64 - sh);  // (three words: sh + b > 64 with b <= 64, so sh >= 1)
    const unsigned long long all = b >= 64 ? ~0ull : (1ull << b) - 1ull;
    v &= all;
    return v ? v : all;
}
__device__ __forceinline__ bool md_in(unsigned long long valid, int c) { return ((valid >> c) & 1ull) != 0; }

// maximum of one head's logits (running maximum from z[0]; MASKED: over the valid bins, in c order)
template <bool MASKED>
__device__ __forceinline__ float md_head_max(const float *z, int b, unsigned long long valid) {
    if (!MASKED) {
        float mx = z[0];
        for (int c = 1; c < b; ++c) mx = fmaxf(mx, z[c]);
        return mx;
    }
    float mx = -INFINITY;
    for (int c = 0; c < b; ++c)
        if (md_in(valid, c)) mx = fmaxf(mx, z[c]);
    return mx;
}
// sum over the head's (valid) bins of exp(z - mx), in c order
template <bool MASKED>
__device__ __forceinline__ float md_head_sumexp(const float *z, int b, float mx, unsigned long long valid) {
    float sum = 0.f;
    for (int c = 0; c < b; ++c)
        if (!MASKED || md_in(valid, c)) sum += expf(z[c] - mx);
    return sum;
}

// Categorical(logits=[n, H, B]).sample() == first arg-max over c < b_h of softmax(z_h)_c / q[(row H + h) B + c]: the padded slots
// c >= b_h (p = 0 in the reference) are no candidates and their noise is never read.  The arithmetic of a head is that of
// multidiscrete_sample_kernel (the exponentials are formed twice instead of being kept); the row's log-probability -- up to 64 float
// terms -- is summed in double and rounded once, as the Gaussian head does above FLOAT_SUM_K terms (a serial float sum of 64 terms
// near -44 alone drifts by ~1e-5).  MASKED: mask[n][W], row `row` of the call's mask.
template <bool MASKED>
__global__ __launch_bounds__(256) void multidiscrete_nvec_sample_kernel(const float *__restrict__ logits, int64_t ld, int64_t n,
                                                                         const float *__restrict__ noise, int64_t *__restrict__ actions,
                                                                         float *__restrict__ logp, MdSpec spec, unsigned *done_words,
                                                                         unsigned done_value, const unsigned *__restrict__ mask, int W) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // (one barrier site for the whole block, as in multidiscrete_sample_kernel: a wave whose lanes split at `row < n` must not
    // arrive at the barrier of block_done_words twice)
    if (row < n) {
        const float *z = logits + row * ld;
        const float *q = noise + row * spec.H * spec.B;
        const unsigned *words = MASKED ? mask + row * W : nullptr;
        double lp = 0.0;
        int s = 0;
        for (int h = 0; h < spec.H; ++h) {
            const int b = spec.b[h];
            const unsigned long long valid = MASKED ? md_head_valid(words, s, b) : 0ull;
            const float mx = md_head_max<MASKED>(z + s, b, valid);
            const float sum = md_head_sumexp<MASKED>(z + s, b, mx, valid);
            const float lse = mx + logf(sum);
            float best = -INFINITY;
            int bi = MASKED ? __builtin_ctzll(valid) : 0;  // (never kept: a valid bin's score is > -inf unless it is NaN)
            for (int c = 0; c < b; ++c) {
                if (MASKED && !md_in(valid, c)) continue;
                const float v = (expf(z[s + c] - mx) / sum) / q[c];
                if (v > best) {
                    best = v;
                    bi = c;
                }
            }
            actions[row * spec.H + h] = bi;
            lp += (double)(z[s + bi] - lse);
            s += b;
            q += spec.B;
        }
        logp[row] = (float)lp;
    }
    block_done_words(done_words, done_value, n);
}

int launch_multidiscrete_nvec_sample(hipStream_t st, const float *logits, int64_t ld, int64_t n, const float *noise, int64_t *actions,
                                     float *logp, const MdSpec &spec, unsigned *done_words, unsigned done_value, const unsigned *mask,
                                     int W) {
    if (n <= 0) return 0;
    RLPPO_CHECK_ARG(spec.S <= ld, "multi-discrete head: %d logits in rows of %ld", spec.S, (long)ld);
    RLPPO_CHECK_ARG(!mask || W == (spec.S + 31) / 32, "multi-discrete head: mask_words=%d, %d logits need %d", W, spec.S, (spec.S + 31) / 32);
    if (mask)
        hipLaunchKernelGGL(multidiscrete_nvec_sample_kernel<true>, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, logits, ld, n, noise,
                           actions, logp, spec, done_words, done_value, mask, W);
    else
        hipLaunchKernelGGL(multidiscrete_nvec_sample_kernel<false>, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, logits, ld, n, noise,
                           actions, logp, spec, done_words, done_value, nullptr, 0);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

// log-sum-exp of one head's logits (the chain of multidiscrete_loss_kernel: running maximum from z[0], sum in c order)
template <bool MASKED>
__device__ __forceinline__ float md_head_lse(const float *z, int b, unsigned long long valid) {
    const float mx = md_head_max<MASKED>(z, b, valid);
    return mx + logf(md_head_sumexp<MASKED>(z, b, mx, valid));
}
// entropy of one head given its log-sum-exp
template <bool MASKED>
__device__ __forceinline__ float md_head_entropy(const float *z, int b, float lse, unsigned long long valid) {
    float e = 0.f;
    for (int c = 0; c < b; ++c) {
        if (MASKED && !md_in(valid, c)) continue;
        const float ls = z[c] - lse;
        e -= expf(ls) * ls;
    }
    return e;
}
// the stored action of head h, float-encoded; clamped into [0, b) BEFORE it indexes anything (a value outside its head's range is a
// caller error: the row then trains on the nearest valid action, and no address outside the row is ever formed)
__device__ __forceinline__ int md_action(float a, int b) {
    const int i = (int)a;
    return i < 0 ? 0 : (i >= b ? b - 1 : i);
}

// The gradient multidiscrete_loss_kernel writes, per head segment; columns >= S of the padded row are zeroed.  First walk: log p
// and the entropy of the row (float terms summed in double, rounded once: see the sampling kernel); second walk: each head's log-sum-exp and entropy again, then its gradient in place (a head's logits
// are overwritten only after the head's own reads).  MASKED: the row's words are those of the buffer's physical row of idx[row]
// (MaskRows); a stored action its own mask marks invalid (a caller error) takes the literal z[a] - lse_V, its one-hot falls on an
// invalid column and is dropped.
template <bool MASKED>
__global__ __launch_bounds__(256) void multidiscrete_nvec_loss_kernel(float *__restrict__ logits, int64_t ld, const float *__restrict__ actions,
                                                                       const float *__restrict__ old_logp,
                                                                       const float *__restrict__ advantages, int64_t mb, LossCfg cfg,
                                                                       double *__restrict__ stats, MdSpec spec, MaskRows mr) {
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = row < mb;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (active) {
        float *z = logits + row * ld;
        const float *ar = actions + row * spec.H;
        const unsigned *words = MASKED ? mr.mask + ring_row(mr.idx[row], mr.ring_base, mr.ring_cap) * mr.W : nullptr;
        double lpd = 0.0, entd = 0.0;
        int s = 0;
        for (int h = 0; h < spec.H; ++h) {
            const int b = spec.b[h];
            const unsigned long long valid = MASKED ? md_head_valid(words, s, b) : 0ull;
            const float lse = md_head_lse<MASKED>(z + s, b, valid);
            entd += (double)md_head_entropy<MASKED>(z + s, b, lse, valid);
            lpd += (double)(z[s + md_action(ar[h], b)] - lse);
            s += b;
        }
        const float lp = (float)lpd, ent = (float)entd;
        const Surrogate t = surrogate_row(lp, old_logp[row], advantages[row], cfg);
        const float g_ent = -cfg.mb_ratio * cfg.ent_coef * cfg.inv_mb;  // coefficient of d(entropy_row)/dz
        s = 0;
        for (int h = 0; h < spec.H; ++h) {
            const int b = spec.b[h];
            const unsigned long long valid = MASKED ? md_head_valid(words, s, b) : 0ull;
            const float lse = md_head_lse<MASKED>(z + s, b, valid);
            const float eh = md_head_entropy<MASKED>(z + s, b, lse, valid);
            const int a = md_action(ar[h], b);
            for (int c = 0; c < b; ++c) {
                if (MASKED && !md_in(valid, c)) {
                    z[s + c] = 0.f;
                    continue;
                }
                const float ls = z[s + c] - lse, ph = expf(ls);
                const float onehot = (c == a) ? 1.f : 0.f;
                z[s + c] = t.g_logp * (onehot - ph) + g_ent * (-ph * (ls + eh));
            }
            s += b;
        }
        for (int c = spec.S; c < ld; ++c) z[c] = 0.f;
        surrogate_stats_add(st, ent * cfg.inv_mb, t, cfg);
    }
    block_stats_add(stats, st, active, cfg, cfg.kl_slots);
}

int launch_multidiscrete_nvec_loss(hipStream_t st, float *logits, int64_t ld, const float *actions, const float *old_logp, const float *adv,
                                   int64_t mb, const LossCfg &cfg, double *stats, const MdSpec &spec, const MaskRows *mr) {
    if (mb <= 0) return 0;
    RLPPO_CHECK_ARG(spec.S <= ld, "multi-discrete head: %d logits in rows of %ld", spec.S, (long)ld);
    const bool masked = mr && mr->mask;
    RLPPO_CHECK_ARG(!masked || (mr->W == (spec.S + 31) / 32 && mr->idx), "multi-discrete head: mask_words=%d, %d logits need %d", mr->W, spec.S,
                    (spec.S + 31) / 32);
    if (masked)
        hipLaunchKernelGGL(multidiscrete_nvec_loss_kernel<true>, dim3(thread_per_row_grid(mb)), dim3(256), 0, st, logits, ld, actions, old_logp,
                           adv, mb, cfg, stats, spec, *mr);
    else
        hipLaunchKernelGGL(multidiscrete_nvec_loss_kernel<false>, dim3(thread_per_row_grid(mb)), dim3(256), 0, st, logits, ld, actions, old_logp,
                           adv, mb, cfg, stats, spec, MaskRows{});
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo
