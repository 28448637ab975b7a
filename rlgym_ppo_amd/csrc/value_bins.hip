// value_bins.hip -- the categorical critic: a critic with n output logits over n equal bins of a fixed value range, trained by
// cross-entropy against a target histogram (HL-Gauss: a Gaussian around the value target integrated over each bin; two-hot: the
// mass split between the two neighbouring bin centres), its value the expectation over the bin centres.  Two row kernels:
// value_bins_loss_kernel turns the critic's [mb][pout] logits into dL/dlogits in place (where launch_value_loss stands for the
// one-output critic), value_bins_readout_kernel turns rows of logits into values (the value pass, the bootstrap rows,
// ValueEstimator.forward).  No GEMM and no epilogue knows about either: the critic's last layer is an ordinary layer of width n.
//
// Design.  A row lives in registers in the layouts of the discrete policy loss (row_layout.hpp): 16 lanes per row and four rows per
// wave up to a padded width of 128 (Lanes16: 8 consecutive columns per lane, two 16-byte loads / stores, DPP reductions), a whole
// wave per row for the padded width 256 (WaveRow<4>: 4 strided columns per lane, shuffle reductions).  Max, sum-exp, the
// histogram's normaliser, the cross-entropy and the expectation are the layouts' fixed-order reductions: no LDS for the rows and no
// atomics -- only block_stats_add's 20 floats of LDS, one barrier and one add per statistic and block -- bit-reproducible.  Columns n .. pout of a row are -inf logits on load and
// exact zeros on store, as the discrete loss treats its padding.  Nothing is kept between forward and backward but the logits.
//
// The bins.  With hw = (vmax - vmin) / (2 n) and mid = (vmin + vmax) / 2, edge i is fma(2 i - n, hw, mid) (edge 0 = vmin and edge
// n = vmax exactly) and centre i is fma(2 i + 1 - n, hw, mid): functions of the integer i alone, computed in the kernel.  Taken
// from the middle of the range, edges and centres are antisymmetric about it to the bit and carry half the rounding of
// vmin + i w.
//
// HL-Gauss.  p_i = (Phi((e_{i+1} - t) / s) - Phi((e_i - t) / s)) / Z for the clamped target t, s = sigma_ratio * w.  Every edge is
// evaluated ONCE as a tail: T_i = erfc(|e_i - t| / (s sqrt 2)) / 2, the mass beyond the edge on the side away from t, plus the sign
// of e_i - t.  The two lanes that share an edge evaluate this one expression of (i, t), so they agree bit for bit.  A bin's mass is
// T_i - T_{i+1} above t, T_{i+1} - T_i below it and 1 - T_i - T_{i+1} for the bin that holds t.  erfc of the distance rather than
// differences of erf: far from t an erf difference is 1 - 1 and leaves the rounding noise of 1 (6e-8) where the mass is 1e-12,
// erfc keeps the tail's relative precision -- so the masses telescope to Z = 1 - T_0 - T_n and no bin goes negative (a clamp at 0
// covers erfc's last-place wobble).  Z is the row sum of the masses as computed, so the histogram sums to 1 to rounding.
// The bound relied on: for t in [vmin, vmax], n >= 2 and sigma_ratio in (0, 2] (anything else is refused),
// Z >= Phi(n / sigma_ratio) - 1/2 >= Phi(1) - 1/2 > 0.34 (> 0.49 for sigma_ratio <= 0.75): the division by Z is safe by construction.
//
// Two-hot.  u = clamp((t - c_0) / w, 0, n - 1), k = min(floor(u), n - 2), f = u - k: p_k = 1 - f, p_{k+1} = f; f is evaluated as
// clamp((t - c_k) / w, 0, 1), the same number without the rounding of u.
//
// Loss of a row: -sum_i p_i log q_i with log q the stable log-softmax; gradient (q_i - p_i) * mb_ratio * inv_mb, the factor
// value_row puts on the scalar head's gradient.  With a value scale {mu, 1/sigma, ...} the target is first taken to normalised
// units as fl(fl(target - mu) * (1/sigma)), the expression value_row uses.
#include <math.h>

#include "row_layout.hpp"

namespace rlppo {

namespace {

template <class T>
struct LayoutTag {
    typedef T type;
};
// padded widths up to 128: 16 lanes per row; 256 (n up to RLPPO_VALUE_MAX_BINS): a wave per row
template <class F>
void dispatch_bins_layout(int64_t ld, F f) {
    if (ld <= 128)
        f(LayoutTag<Lanes16>{});
    else
        f(LayoutTag<WaveRow<4>>{});
}
constexpr int64_t BINS_MAX_LD = 256;
constexpr int64_t BINS_LOSS_MAX_BLOCKS = 2048;  // the loss strides its grid over the rows, like the discrete loss

__device__ __forceinline__ float bin_edge(const BinSpec &b, int i) {
    return i <= 0 ? b.vmin : i >= b.n ? b.vmax : __fmaf_rn((float)(2 * i - b.n), b.hw, b.mid);
}
__device__ __forceinline__ float bin_centre(const BinSpec &b, int i) { return __fmaf_rn((float)(2 * i + 1 - b.n), b.hw, b.mid); }

// the Gaussian's mass beyond edge i on the side away from t, and that side
struct EdgeTail {
    float mass;
    bool below;  // the edge lies below t
};
__device__ __forceinline__ EdgeTail edge_tail(const BinSpec &b, int i, float t) {
    const float x = bin_edge(b, i) - t;
    return EdgeTail{0.5f * erfcf(fabsf(x) * b.inv_s_sqrt2), x < 0.f};
}
// the mass between edges lo < hi
__device__ __forceinline__ float bin_mass(const EdgeTail lo, const EdgeTail hi) {
    const float m = hi.below ? hi.mass - lo.mass : lo.below ? (1.f - lo.mass) - hi.mass : lo.mass - hi.mass;
    return fmaxf(m, 0.f);
}

// stable softmax of one row: z holds the lane's logits (-inf where !in(e)) and leaves as log q (where in(e)), q as the probabilities
template <class L, class In>
__device__ __forceinline__ void row_log_softmax(float (&z)[L::EPL], float (&q)[L::EPL], In in) {
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) mx = fmaxf(mx, z[e]);
    mx = L::max(mx);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) {
        z[e] = z[e] - mx;
        q[e] = in(e) ? expf(z[e]) : 0.f;
        s += q[e];
    }
    s = L::sum(s);
    const float log_s = logf(s);
#pragma unroll
    for (int e = 0; e < L::EPL; ++e) {
        z[e] = z[e] - log_s;
        q[e] = q[e] / s;
    }
}

// logits[row][0:pout) -> dL/dlogits in place; targets[mb] the gathered real-unit value targets.  KIND: RLPPO_VALUE_BINS_*.
template <class L, int KIND>
__global__ __launch_bounds__(256) void value_bins_loss_kernel(float *__restrict__ logits, int64_t ld, BinSpec b, const float *__restrict__ targets,
                                                               int64_t mb, LossCfg cfg, double *__restrict__ stats) {
    constexpr int EPL = L::EPL;
    const L lay;
    float st[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const auto in = [&](int e) { return lay.col(e) < b.n; };
    for (int64_t base = (int64_t)blockIdx.x * L::ROWS; base < mb; base += (int64_t)gridDim.x * L::ROWS) {
        const bool live = base + lay.group < mb;
        if (!L::SHADOW && !live) break;
        const int64_t row = live ? base + lay.group : mb - 1;
        float *z = logits + row * ld;
        float lq[EPL], q[EPL], p[EPL];
        lay.load(z, ld, lq, in);
        row_log_softmax<L>(lq, q, in);
        float t = targets[row];
        if (cfg.vnorm) t = __fmul_rn(__fsub_rn(t, cfg.vnorm[0]), cfg.vnorm[1]);
        t = fminf(fmaxf(t, b.vmin), b.vmax);
        if (KIND == RLPPO_VALUE_BINS_HL_GAUSS) {
            float zsum = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
                const int c = lay.col(e);
                p[e] = in(e) ? bin_mass(edge_tail(b, c, t), edge_tail(b, c + 1, t)) : 0.f;
                zsum += p[e];
            }
            zsum = L::sum(zsum);
#pragma unroll
            for (int e = 0; e < EPL; ++e) p[e] = p[e] / zsum;
        } else {
            // k from u; f = u - k then from t's distance to centre k itself (a difference of neighbours: exact), not from u, whose
            // last place is worth n times more -- the histogram's expectation stays within the rounding of one centre of t
            const float w = 2.f * b.hw;
            const float u = fminf(fmaxf((t - bin_centre(b, 0)) / w, 0.f), (float)(b.n - 1));
            const int k = min((int)floorf(u), b.n - 2);
            const float f = fminf(fmaxf((t - bin_centre(b, k)) / w, 0.f), 1.f);
#pragma unroll
            for (int e = 0; e < EPL; ++e) p[e] = lay.col(e) == k ? 1.f - f : lay.col(e) == k + 1 ? f : 0.f;
        }
        float ce = 0.f;
        float g[EPL];
        const float scale = cfg.mb_ratio;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
            if (in(e) && p[e] > 0.f) ce -= p[e] * lq[e];
            g[e] = in(e) ? scale * ((q[e] - p[e]) * cfg.inv_mb) : 0.f;
        }
        ce = L::sum(ce);
        if (live) lay.store(z, ld, g);
        if (live && lay.writer()) st[RLPPO_STAT_VLOSS] += ce * cfg.inv_mb;
    }
    block_stats_add(stats, st, true, cfg);
}

// values[row] = sum_i softmax(logits[row])_i c_i = mid + sum_i q_i (c_i - mid): one store per row
template <class L>
__global__ __launch_bounds__(256) void value_bins_readout_kernel(const float *__restrict__ logits, int64_t ld, BinSpec b, float *__restrict__ values,
                                                                  int64_t n_rows) {
    constexpr int EPL = L::EPL;
    const L lay;
    const int64_t row = (int64_t)blockIdx.x * L::ROWS + lay.group;
    if (row >= n_rows) return;  // (whole groups leave: every lane of a live row takes part in its reductions)
    const auto in = [&](int e) { return lay.col(e) < b.n; };
    float lq[EPL], q[EPL];
    lay.load(logits + row * ld, ld, lq, in);
    row_log_softmax<L>(lq, q, in);
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e)
        if (in(e)) acc += q[e] * ((float)(2 * lay.col(e) + 1 - b.n) * b.hw);
    acc = L::sum(acc);
    if (lay.writer()) values[row] = b.mid + acc;
}

int bins_rows_check(const char *who, const void *logits, int64_t ld, const BinSpec &b) {
    RLPPO_CHECK_ARG(ld >= b.n && ld % 8 == 0 && ld <= BINS_MAX_LD, "%s: rows of %ld floats for n=%d bins (a multiple of 8, n .. %ld)", who, (long)ld, b.n,
                    (long)BINS_MAX_LD);
    RLPPO_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 15) == 0, "%s: logits must be 16-byte aligned", who);
    return 0;
}

}  // namespace

int value_bins_make(const rlppo_value_bins *v, const char *who, BinSpec *spec) {
    RLPPO_CHECK_ARG(v != nullptr, "%s: null bins", who);
    RLPPO_CHECK_ARG(v->kind == RLPPO_VALUE_BINS_HL_GAUSS || v->kind == RLPPO_VALUE_BINS_TWO_HOT, "%s: bins kind=%d (1 = HL-Gauss, 2 = two-hot)", who,
                    v->kind);
    RLPPO_CHECK_ARG(v->n >= 2 && v->n <= RLPPO_VALUE_MAX_BINS, "%s: bins n=%d not in 2 .. RLPPO_VALUE_MAX_BINS = %d", who, v->n, RLPPO_VALUE_MAX_BINS);
    RLPPO_CHECK_ARG(isfinite(v->vmin) && isfinite(v->vmax) && v->vmin < v->vmax, "%s: bins vmin=%g vmax=%g (finite, vmin < vmax)", who, (double)v->vmin,
                    (double)v->vmax);
    const double w = ((double)v->vmax - (double)v->vmin) / v->n;
    RLPPO_CHECK_ARG((float)(0.5 * w) > 0.f && isfinite((float)w), "%s: bins vmin=%g vmax=%g: the bin width is not a float32 number", who, (double)v->vmin,
                    (double)v->vmax);
    spec->kind = v->kind;
    spec->n = v->n;
    spec->vmin = v->vmin;
    spec->vmax = v->vmax;
    spec->mid = (float)(0.5 * (double)v->vmin + 0.5 * (double)v->vmax);
    spec->hw = (float)(0.5 * w);
    spec->inv_s_sqrt2 = 0.f;
    if (v->kind == RLPPO_VALUE_BINS_HL_GAUSS) {
        RLPPO_CHECK_ARG(v->sigma_ratio > 0.f && v->sigma_ratio <= 2.f, "%s: bins sigma_ratio=%g not in (0, 2]", who, (double)v->sigma_ratio);
        spec->inv_s_sqrt2 = (float)(1.0 / ((double)v->sigma_ratio * w * 1.4142135623730951));
        // (a ratio so small that 1 / (s sqrt 2) leaves float32: a target on an edge would be 0 * inf inside erfc)
        RLPPO_CHECK_ARG(isfinite(spec->inv_s_sqrt2), "%s: bins sigma_ratio=%g of a bin width %g: 1 / sigma is not a float32 number", who,
                        (double)v->sigma_ratio, w);
    }
    return 0;
}

int launch_value_bins_loss(hipStream_t st, float *logits, int64_t ld, const BinSpec &b, const float *targets, int64_t mb, const LossCfg &cfg,
                           double *stats) {
    if (mb <= 0) return 0;
    if (int rc = bins_rows_check("value bins loss", logits, ld, b)) return rc;
    dispatch_bins_layout(ld, [&](auto tag) {
        typedef typename decltype(tag)::type L;
        const int64_t blocks = cdiv(mb, L::ROWS);
        const dim3 grid((unsigned)(blocks < BINS_LOSS_MAX_BLOCKS ? blocks : BINS_LOSS_MAX_BLOCKS));
        if (b.kind == RLPPO_VALUE_BINS_HL_GAUSS)
            hipLaunchKernelGGL((value_bins_loss_kernel<L, RLPPO_VALUE_BINS_HL_GAUSS>), grid, dim3(256), 0, st, logits, ld, b, targets, mb, cfg, stats);
        else
            hipLaunchKernelGGL((value_bins_loss_kernel<L, RLPPO_VALUE_BINS_TWO_HOT>), grid, dim3(256), 0, st, logits, ld, b, targets, mb, cfg, stats);
    });
    RLPPO_LAUNCH_CHECK();
    return 0;
}

int launch_value_bins_readout(hipStream_t st, const float *logits, int64_t ld, const BinSpec &b, float *values, int64_t n_rows) {
    if (n_rows <= 0) return 0;
    if (int rc = bins_rows_check("value_bins_readout", logits, ld, b)) return rc;
    dispatch_bins_layout(ld, [&](auto tag) {
        typedef typename decltype(tag)::type L;
        hipLaunchKernelGGL((value_bins_readout_kernel<L>), dim3((unsigned)cdiv(n_rows, L::ROWS)), dim3(256), 0, st, logits, ld, b, values, n_rows);
    });
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo

using namespace rlppo;

extern "C" {

int rlppo_value_bins_readout(void *stream, const float *logits, int64_t ld, const rlppo_value_bins *bins, float *values, int64_t n_rows) {
    BinSpec b;
    if (int rc = value_bins_make(bins, "value_bins_readout", &b)) return rc;
    RLPPO_CHECK_ARG(n_rows >= 0 && (n_rows == 0 || (logits && values)), "value_bins_readout: n_rows=%ld, or a null pointer", (long)n_rows);
    return launch_value_bins_readout((hipStream_t)stream, logits, ld, b, values, n_rows);
}

// the loss launch on its own, on caller-supplied logits and contiguous targets (tests, tools/value_head_cost.py)
int rlppo_dbg_value_bins_loss(void *stream, float *logits, int64_t ld, const rlppo_value_bins *bins, const float *targets, int64_t mb, float mb_ratio,
                              const float *value_scale, double *stats) {
    BinSpec b;
    if (int rc = value_bins_make(bins, "dbg_value_bins_loss", &b)) return rc;
    RLPPO_CHECK_ARG(mb > 0 && logits && targets && stats, "dbg_value_bins_loss: mb=%ld, or a null pointer", (long)mb);
    LossCfg cfg = {};
    cfg.mb_ratio = mb_ratio;
    cfg.inv_mb = 1.0f / (float)mb;
    cfg.vnorm = value_scale;
    return launch_value_bins_loss((hipStream_t)stream, logits, ld, b, targets, mb, cfg, stats);
}

}  // extern "C"
