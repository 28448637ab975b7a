// hybrid.hip -- the hybrid action head (RLPPO_HEAD_HYBRID, include/rlppo.h "[hybrid]"): k diagonal-Gaussian dimensions with a learnable
// log_std and H independent categoricals of nvec bins in ONE row of k + S network outputs (S = sum nvec): the sampling kernel of the
// rollout and the loss kernel of the update.  The arithmetic of a Gaussian dimension is the diag head's (diag_logp_term) and that of a
// categorical head the [nvec] kernels' (running maximum from the first bin, sum of exponentials in bin order, lse = mx + logf(sum)),
// so a sample decomposes into the two heads' samples bit for bit.
//
// Work split.  A row is up to 256 + 512 columns: one thread per row (the diag and [nvec] kernels) would read and write the whole
// matrix with a stride of ld floats between lanes.  Here a workgroup owns 256 consecutive rows (so the grid, the completion words,
// the KL slots and the log_std partial sums are those of the thread-per-row heads: rlppo_diag_scratch_bytes sizes the scratch) and
// walks them as 16 tiles of R = 16 rows; a 16-lane group works on one row of the tile, split BY HEAD, not by column: lane j takes the
// Gaussian dimensions j, j + 16, ... and the categorical heads j, j + 16, ... (at most 4: 64 heads), each head serially over its
// bins.  Ragged heads therefore need no segmented reduction; the one cross-lane step of a row is the 16-lane butterfly of
// (log p, entropy), taken in double over DPP moves (row16_sum_f64: xor 1, xor 2, half-row mirror, row mirror -- a fixed order).
//
// Data movement.  A tile enters LDS with coalesced 16-byte loads (thread t takes chunk t, t + 256, ... of the tile's rows x ceil(W / 4)
// chunks), lanes read and overwrite their heads there, and dL/dy leaves in place through the same 16-byte path, zeros in the
// padded columns [W, ld).  How R and the padding were chosen:
//   R = 16     one row per 16-lane group of the 256 threads.  The widest row (768 columns) takes 868 words with the padding below, a
//              tile 16 x 868 x 4 = 55,552 bytes: under 64 KiB together with the 2.3 KiB of static LDS, so no launch attribute is needed
//              and two workgroups fit a CU's 160 KiB.  R = 32 would double the tile for no extra lanes at work.
//   columns    column c lives at word c + 4 (c / 32): four pad words behind every 32 columns.  The 16 lanes of a group start at their
//              heads' offsets s_h; with equal power-of-two bins those are multiples of 32 or 64 words apart and would all fall on ONE of
//              the 64 banks.  With the skew, heads 32 apart sit 36 words apart (16 distinct banks), heads 64 apart 72 words (8 banks, two
//              lanes each).  The skew is a multiple of 4, so a 16-byte chunk stays whole and aligned.
//   row stride the padded row rounded to an ODD number of 16-byte chunks: the four rows of a wave start 4 x odd words apart, never on the
//              same bank group.
// nvec's offsets and bins, log_std and exp(log_std) sit in LDS once per workgroup.
#include "head_steps.hpp"
#include "row_layout.hpp"

namespace rlppo {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int HY_ROWS = 16;          // rows of a tile = 16-lane groups of a workgroup
constexpr int HY_BLOCK_ROWS = 256;   // rows of a workgroup: 16 tiles
constexpr int HY_LANE_HEADS = RLPPO_MD_MAX_HEADS / 16, HY_LANE_DIMS = RLPPO_DIAG_MAX_K / 16;

__host__ __device__ __forceinline__ int hy_word(int c) { return c + 4 * (c >> 5); }
static int hy_stride(int W) { return (hy_word((W + 3) / 4 * 4) / 4 | 1) * 4; }  // words per tile row: an odd number of chunks

// the 16-lane all-reduce of row16_sum on a double: each DPP step moves the two halves
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
    struct Halves {
        int lo, hi;
    } h = __builtin_bit_cast(Halves, v);
    h.lo = __builtin_amdgcn_update_dpp(0, h.lo, CTRL, 0xF, 0xF, true);
    h.hi = __builtin_amdgcn_update_dpp(0, h.hi, CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, h);
}
__device__ __forceinline__ double row16_sum_f64(double v) {
    v += dpp_mov_f64<0xB1>(v);
    v += dpp_mov_f64<0x4E>(v);
    v += dpp_mov_f64<0x141>(v);
    v += dpp_mov_f64<0x140>(v);
    return v;
}

// What a workgroup keeps in LDS beside the tile: the heads' first logits (as columns of the row) and bins, log_std and sigma
struct HyShared {
    float ls[RLPPO_DIAG_MAX_K], sd[RLPPO_DIAG_MAX_K];
    short off[RLPPO_MD_MAX_HEADS];
    unsigned char b[RLPPO_MD_MAX_HEADS];
};
// (every thread of the block, before anything diverges: the fill ends in a barrier.  h is uniform: the spec is read with scalar loads)
__device__ __forceinline__ void hy_fill(HyShared &sh, const MdSpec &spec, int k, const float *__restrict__ log_std) {
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const float ls = log_std[j];
        sh.ls[j] = ls;
        sh.sd[j] = expf(ls);
    }
    int s = k;
    for (int h = 0; h < spec.H; ++h) {
        if (threadIdx.x == 0) {
            sh.off[h] = (short)s;
            sh.b[h] = spec.b[h];
        }
        s += spec.b[h];
    }
    __syncthreads();
}

// rows [row0, row0 + rows) of y, W4 chunks each, into the tile; the barrier in front keeps the previous tile's readers apart
__device__ __forceinline__ void hy_stage_in(float *tile, int stride, const float *__restrict__ y, int64_t ld, int64_t row0, int rows, int W4) {
    __syncthreads();
    for (int i = threadIdx.x; i < rows * W4; i += blockDim.x) {
        const int r = i / W4, c = 4 * (i - r * W4);
        *reinterpret_cast<f32x4 *>(tile + r * stride + hy_word(c)) = *reinterpret_cast<const f32x4 *>(y + (row0 + r) * ld + c);
    }
    __syncthreads();
}

// one categorical head in the tile: logit c of the head is z(c)
struct HyHead {
    const float *row;
    int s, b;
    __device__ __forceinline__ float z(int c) const { return row[hy_word(s + c)]; }
    // (the chain of md_head_max / md_head_sumexp of heads.hip: running maximum from z[0], the sum in c order)
    __device__ __forceinline__ float max() const {
        float mx = z(0);
        for (int c = 1; c < b; ++c) mx = fmaxf(mx, z(c));
        return mx;
    }
    __device__ __forceinline__ float sumexp(float mx) const {
        float sum = 0.f;
        for (int c = 0; c < b; ++c) sum += expf(z(c) - mx);
        return sum;
    }
    __device__ __forceinline__ float entropy(float lse) const {
        float e = 0.f;
        for (int c = 0; c < b; ++c) {
            const float ls = z(c) - lse;
            e -= expf(ls) * ls;
        }
        return e;
    }
};

// ------------------------------------------------------------------------------------------------- sampling
// a_j = mu_j + sigma_j eps_j (not clamped); head h: the first arg-max over c < b_h of softmax(z_h)_c / q[(row H + h) B + c]; the
// action row is the k samples, then the H indices as floats; log p of the sample as stored, the float terms summed in double.
__global__ __launch_bounds__(256) void hybrid_sample_kernel(const float *__restrict__ y, int64_t ld, int64_t n, int k, MdSpec spec,
                                                             const float *__restrict__ eps, const float *__restrict__ noise_q,
                                                             const float *__restrict__ log_std, float *__restrict__ actions,
                                                             float *__restrict__ logp, int stride, unsigned *done_words, unsigned done_value) {
    extern __shared__ f32x4 hy_tile_raw[];
    float *tile = reinterpret_cast<float *>(hy_tile_raw);
    __shared__ HyShared sh;
    hy_fill(sh, spec, k, log_std);
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int W4 = (k + spec.S + 3) / 4, adim = k + spec.H;
    for (int t = 0; t < HY_BLOCK_ROWS / HY_ROWS; ++t) {
        const int64_t row0 = (int64_t)blockIdx.x * HY_BLOCK_ROWS + t * HY_ROWS;
        if (row0 >= n) break;  // (uniform)
        const int rows = n - row0 < HY_ROWS ? (int)(n - row0) : HY_ROWS;
        hy_stage_in(tile, stride, y, ld, row0, rows, W4);
        if (g >= rows) continue;  // (a whole 16-lane group; the barriers are in hy_stage_in, which every thread reaches)
        const int64_t row = row0 + g;
        const float *zr = tile + g * stride;
        double lp = 0.0;
        for (int j = l; j < k; j += 16) {
            const float mean = zr[hy_word(j)], sd = sh.sd[j];
            const float a = eps[row * k + j] * sd + mean;  // at::normal: output.mul_(std).add_(mean)
            actions[row * adim + j] = a;
            lp += (double)diag_logp_term(a - mean, sd, sh.ls[j]);
        }
        for (int h = l; h < spec.H; h += 16) {
            const HyHead hd{zr, sh.off[h], sh.b[h]};
            const float *q = noise_q + (row * spec.H + h) * spec.B;
            const float mx = hd.max(), sum = hd.sumexp(mx);
            const float lse = mx + logf(sum);
            float best = -INFINITY;
            int bi = 0;
            for (int c = 0; c < hd.b; ++c) {
                const float v = (expf(hd.z(c) - mx) / sum) / q[c];
                if (v > best) {
                    best = v;
                    bi = c;
                }
            }
            actions[row * adim + k + h] = (float)bi;
            lp += (double)(hd.z(bi) - lse);
        }
        lp = row16_sum_f64(lp);
        if (l == 0) logp[row] = (float)lp;
    }
    block_done_words(done_words, done_value, n);
}

// ----------------------------------------------------------------------------------------------------- loss
// y[row][0 : k + S) is overwritten with dL/dy: the diag head's dL/dmu in the first k columns, the [nvec] head's dL/dz per head segment
// behind them, exact zeros in [k + S, ld).  The row's log p and entropy are the double sums of the float terms of both halves, rounded
// once.  dL/dlog_std_j: a lane adds its rows' float terms in double over the 16 tiles, the four groups of a wave meet by two shuffles,
// the four waves in LDS, and the workgroup's k sums land in its row of `partials` [grid][k] for diag_logstd_finish_kernel.
__global__ __launch_bounds__(256) void hybrid_loss_kernel(float *__restrict__ y, int64_t ld, int k, MdSpec spec,
                                                           const float *__restrict__ actions, const float *__restrict__ old_logp,
                                                           const float *__restrict__ advantages, int64_t mb, LossCfg cfg,
                                                           double *__restrict__ stats, const float *__restrict__ log_std,
                                                           double *__restrict__ partials, int stride) {
    extern __shared__ f32x4 hy_tile_raw[];
    float *tile = reinterpret_cast<float *>(hy_tile_raw);
    __shared__ HyShared sh;
    hy_fill(sh, spec, k, log_std);
    const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
    const int W = k + spec.S, W4 = (W + 3) / 4, adim = k + spec.H, ld4 = (int)(ld / 4);
    const float g_ent = -cfg.mb_ratio * cfg.ent_coef * cfg.inv_mb;  // coefficient of d(entropy_row)/d(output), of d/dlog_std_j too
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    double acc[HY_LANE_DIMS];  // this lane's dimensions l, l + 16, ...: sums over its rows of the log_std terms
#pragma unroll
    for (int i = 0; i < HY_LANE_DIMS; ++i) acc[i] = 0.0;
    for (int t = 0; t < HY_BLOCK_ROWS / HY_ROWS; ++t) {
        const int64_t row0 = (int64_t)blockIdx.x * HY_BLOCK_ROWS + t * HY_ROWS;
        if (row0 >= mb) break;  // (uniform)
        const int rows = mb - row0 < HY_ROWS ? (int)(mb - row0) : HY_ROWS;
        hy_stage_in(tile, stride, y, ld, row0, rows, W4);
        if (g < rows) {
            const int64_t row = row0 + g;
            float *zr = tile + g * stride;
            const float *ar = actions + row * adim;
            double lpd = 0.0, entd = 0.0;
            for (int j = l; j < k; j += 16) {
                lpd += (double)diag_logp_term(ar[j] - zr[hy_word(j)], sh.sd[j], sh.ls[j]);
                entd += (double)(1.4189385332046727f + sh.ls[j]);  // Normal.entropy(): 0.5 + 0.5*log(2*pi) + log(sd)
            }
            float lse[HY_LANE_HEADS], eh[HY_LANE_HEADS];
#pragma unroll
            for (int i = 0; i < HY_LANE_HEADS; ++i) {
                const int h = l + 16 * i;
                lse[i] = eh[i] = 0.f;
                if (h < spec.H) {
                    const HyHead hd{zr, sh.off[h], sh.b[h]};
                    const float mx = hd.max();
                    lse[i] = mx + logf(hd.sumexp(mx));
                    eh[i] = hd.entropy(lse[i]);
                    entd += (double)eh[i];
                    lpd += (double)(hd.z(md_action(ar[k + h], hd.b)) - lse[i]);
                }
            }
            const float lp = (float)row16_sum_f64(lpd), ent = (float)row16_sum_f64(entd);
            const Surrogate s = surrogate_row(lp, old_logp[row], advantages[row], cfg);  // (the same bits in all 16 lanes)
#pragma unroll
            for (int i = 0; i < HY_LANE_DIMS; ++i) {
                const int j = l + 16 * i;
                if (j < k) {
                    const float sd = sh.sd[j], d = ar[j] - zr[hy_word(j)];
                    const float s2 = sd * sd;
                    zr[hy_word(j)] = s.g_logp * d / s2;
                    acc[i] += (double)(s.g_logp * (d * d / s2 - 1.f) + g_ent);
                }
            }
#pragma unroll
            for (int i = 0; i < HY_LANE_HEADS; ++i) {
                const int h = l + 16 * i;
                if (h < spec.H) {
                    const int s0 = sh.off[h], b = sh.b[h], a = md_action(ar[k + h], b);
                    for (int c = 0; c < b; ++c) {
                        const float ls = zr[hy_word(s0 + c)] - lse[i], ph = expf(ls);
                        const float onehot = (c == a) ? 1.f : 0.f;
                        zr[hy_word(s0 + c)] = s.g_logp * (onehot - ph) + g_ent * (-ph * (ls + eh[i]));
                    }
                }
            }
            if (l == 0) surrogate_stats_add(st, ent * cfg.inv_mb, s, cfg);
        }
        __syncthreads();
        // dL/dy out, whole padded rows: the tile's chunks, the last one cut at W, zeros behind
        for (int i = threadIdx.x; i < rows * ld4; i += blockDim.x) {
            const int r = i / ld4, c = 4 * (i - r * ld4);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (c < 4 * W4) {
                v = *reinterpret_cast<const f32x4 *>(tile + r * stride + hy_word(c));
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (c + e >= W) v[e] = 0.f;
            }
            *reinterpret_cast<f32x4 *>(y + (row0 + r) * ld + c) = v;
        }
    }
    // the log_std partial sums: groups of a wave (lanes l, l + 16, l + 32, l + 48), then the waves through the tile's memory
    __syncthreads();
    double *red = reinterpret_cast<double *>(tile);  // [4][k]: 32 k bytes <= the tile's 64 x stride, stride > k
#pragma unroll
    for (int i = 0; i < HY_LANE_DIMS; ++i) {
        double s = acc[i];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        const int j = l + 16 * i;
        if ((threadIdx.x & 63) < 16 && j < k) red[(threadIdx.x >> 6) * k + j] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x)
        partials[(int64_t)blockIdx.x * k + j] = (red[j] + red[k + j]) + (red[2 * k + j] + red[3 * k + j]);
    block_stats_add(stats, st, true, cfg, cfg.kl_slots);
}

int hybrid_check(const char *who, const void *y, int64_t ld, int k, const MdSpec &spec) {
    RLPPO_CHECK_ARG(k >= 1 && k <= RLPPO_DIAG_MAX_K, "%s: k=%d Gaussian dimensions, RLPPO_DIAG_MAX_K allows 1 .. %d", who, k, RLPPO_DIAG_MAX_K);
    RLPPO_CHECK_ARG(ld >= k + spec.S && ld <= (1 << 20) && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0,
                    "%s: rows of ld=%ld floats for k + sum(nvec) = %d outputs (ld a multiple of 4, the rows 16-byte aligned)", who, (long)ld, k + spec.S);
    return 0;
}

}  // namespace

int launch_hybrid_sample(hipStream_t st, const float *y, int64_t ld, int64_t n, int k, const MdSpec &spec, const float *eps, const float *noise_q,
                         const float *log_std, float *actions, float *logp, unsigned *done_words, unsigned done_value) {
    if (n <= 0) return 0;
    if (int rc = hybrid_check("hybrid head", y, ld, k, spec)) return rc;
    const int stride = hy_stride(k + spec.S);
    hipLaunchKernelGGL(hybrid_sample_kernel, dim3((unsigned)cdiv(n, HY_BLOCK_ROWS)), dim3(256), (size_t)HY_ROWS * stride * sizeof(float), st, y, ld, n, k,
                       spec, eps, noise_q, log_std, actions, logp, stride, done_words, done_value);
    RLPPO_LAUNCH_CHECK();
    return 0;
}

int launch_hybrid_loss(hipStream_t st, float *y, int64_t ld, int k, const MdSpec &spec, const float *actions, const float *old_logp,
                       const float *adv, int64_t mb, const LossCfg &cfg, double *stats, const DiagHead &dg, int part) {
    if (mb <= 0) return 0;
    if (int rc = hybrid_check("hybrid head", y, ld, k, spec)) return rc;
    RLPPO_CHECK_ARG(dg.log_std && dg.log_std_grad && dg.scratch && dg.scratch_bytes >= diag_scratch_bytes(mb, k),
                    "hybrid head: log_std / log_std_grad / scratch (%zu bytes, %zu needed)", dg.scratch_bytes, diag_scratch_bytes(mb, k));
    const unsigned grid = (unsigned)cdiv(mb, HY_BLOCK_ROWS);  // = the diag head's: one row of k partial sums per 256 rows
    const int stride = hy_stride(k + spec.S);
    if (part != 2) {  // (part: rlppo_dbg_hybrid_loss times the two launches apart; a pass runs both)
        hipLaunchKernelGGL(hybrid_loss_kernel, dim3(grid), dim3(256), (size_t)HY_ROWS * stride * sizeof(float), st, y, ld, k, spec, actions, old_logp,
                           adv, mb, cfg, stats, dg.log_std, dg.scratch, stride);
        RLPPO_LAUNCH_CHECK();
    }
    return part != 1 ? launch_diag_logstd_finish(st, dg.scratch, (int)grid, k, dg.log_std_grad) : 0;
}

}  // namespace rlppo
