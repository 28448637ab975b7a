// mirror.hip -- mirror-symmetry augmentation of a minibatch (rsl_rl's symmetry_cfg / use_data_augmentation): ONE launch gathers the mb
// rows of a pass through idx and the ring map and writes 2 mb plain rows into a staging region -- rows [0, mb) the originals, bit
// for bit, rows [mb, 2 mb) their mirror images:
//     state   y[j] = sign[j] * x[perm[j]] for j < d, exact +0 in the padded columns (the critic's matrix likewise, under its own table)
//     action  discrete amap[a]; multi-discrete binmap_h[a[hperm[h]]]; both Gaussian heads asign[j] * a[aperm[j]] (float-encoded)
//     mask    bit c of the mirror = bit mask_tab[c] of the source row (the composed logit permutation)
//     old log-probability, value target and advantage: copied twice
// Permutations, sign flips (an xor of bit 31) and bit moves are exact: no arithmetic, no atomics, the same bits on every run.
//
// Design.  The grid's y index is the part: one per row matrix (policy rows, then the critic's) and a last one for the per-row
// scalars, actions and masks.  Every part walks the rows of the pass with a grid stride, so a lane OWNS FIXED COLUMNS for the whole
// launch and keeps their packed table entries (source column, sign in bit 31, RLPPO_MIRROR_ZERO for a padded column) in registers:
// the tables are read once per workgroup, not once per row.
//   rows    LPR lanes per row: 16 for leading dimensions up to 128 floats (four rows per wave, the shape norm.hip uses), the whole
//           wave above (up to 2048).  Lane `sub` owns the 16-byte chunks sub, sub + LPR, ...: a source row is fetched ONCE through
//           the ring map with 16-byte loads, the original half is stored from those registers with 16-byte stores, the row is staged
//           in LDS, and the mirror is read back through the table element by element and leaves with 16-byte stores.
//   LDS     The permuted read is a 4-byte read per lane at column 4 chunk + e + (whatever the table says).  A typical table is a
//           few block swaps plus scattered sign flips, i.e. locally a SHIFT: 16 lanes of a row then read with stride 4 and hit 16 of
//           the 64 banks, and laid out plainly the four row groups of a wave (or the four 16-lane quarters of a wave-wide row) fall on
//           the SAME 16 banks -- a 4-way serialisation.  Chosen instead: column j of a row lives at word j + (j >> 6) (one pad word
//           per 64 columns), and with several rows per wave the row pitch is 133 words (= 1 mod 4).  Each run of 64 columns and each
//           row slot then starts in another residue class mod 4 of the bank index, so the 64 lanes of any shifted read touch 64
//           different banks, whatever the shift; sign flips do not move an address.  The price is that the staging write is four
//           4-byte writes per chunk (same banks argument: conflict-free) instead of one 16-byte write, since the skew breaks its
//           alignment; the kernel is bound by HBM, not by LDS issue.
//   masks   a wave per row: lanes < W hold the row's words, lane l looks up bits l, l + 64, ... (table entries in registers, the
//           source word arrives by a shuffle), __ballot assembles 64 bits and lanes 0 and 32 each store their 32 with a plain vector
//           store.  Up to 16 words (512 logits) per row.
//   scalars a lane per row; actions a lane per element, the action tables read through the cache.
// The kernel TRUSTS the tables (the host range-checks every entry before the first launch: rlgym_ppo_amd/ppo/symmetry.py); stored
// action indices are data, not tables, and are clamped into their table before they index it.
#include "common.hpp"

namespace rlppo {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));

constexpr int MR_THREADS = 256;
constexpr unsigned MR_ZERO = RLPPO_MIRROR_ZERO;
constexpr int MR_MAX_LD = 2048;        // floats per row of a matrix (eight 16-byte chunks per lane of a wave)
constexpr int MR_MAX_MASK_WORDS = 16;  // eight ballots of 64 bits
constexpr int MR_PITCH16 = 133;        // LDS words per row slot with four rows per wave: >= 128 + 2, = 1 (mod 4)
constexpr int MR_META_ROWS = MR_THREADS;

struct MirrorMat {
    const float *src;     // [N][ld] through the ring map
    const unsigned *tab;  // [ld]
    float *dst;           // [2 mb][ld]
    int64_t ld;
    int shape, pitch;     // 0: <16, 2>; 1 .. 4: <64, 1 / 2 / 4 / 8>; LDS words per row slot
};
struct MirrorMeta {
    const float *actions, *old_logp, *targets, *adv;
    const unsigned *mask, *act_tab, *mask_tab;
    float *o_act, *o_old, *o_tgt, *o_adv;
    unsigned *o_mask;
    int head, act_dim, n_actions, W;
};
struct MirrorArgs {
    MirrorMat mat[2];
    MirrorMeta meta;
    const int64_t *idx;
    int64_t mb, ring_base, ring_cap;
    int n_mat;
};

__device__ __forceinline__ int skew(int j) { return j + (j >> 6); }
__device__ __forceinline__ float flip(float x, unsigned t) { return __uint_as_float(__float_as_uint(x) ^ (t & 0x80000000u)); }

template <int LPR, int VPL>
__device__ __forceinline__ void mirror_rows(const MirrorMat &m, const MirrorArgs &a, float *lds) {
    constexpr int RPB = MR_THREADS / LPR;  // rows per workgroup and step
    const int sub = threadIdx.x % LPR, slot = threadIdx.x / LPR;
    const int cpr = (int)(m.ld / 4);
    float *row = lds + slot * m.pitch;
    u4 t[VPL];  // this lane's columns, for the whole launch
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int c = sub + j * LPR;
        t[j] = u4{MR_ZERO, MR_ZERO, MR_ZERO, MR_ZERO};
        if (c < cpr) t[j] = *reinterpret_cast<const u4 *>(m.tab + 4 * c);
    }
    for (int64_t r0 = (int64_t)blockIdx.x * RPB; r0 < a.mb; r0 += (int64_t)gridDim.x * RPB) {  // (uniform over the workgroup)
        const int64_t r = r0 + slot;
        const bool live = r < a.mb;
        f4 v[VPL];
        if (live) {
            const float *s = m.src + ring_row(a.idx[r], a.ring_base, a.ring_cap) * m.ld;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int c = sub + j * LPR;
                if (c < cpr) v[j] = *reinterpret_cast<const f4 *>(s + 4 * c);
            }
            float *o = m.dst + r * m.ld;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int c = sub + j * LPR;
                if (c < cpr) {
                    *reinterpret_cast<f4 *>(o + 4 * c) = v[j];
#pragma unroll
                    for (int e = 0; e < 4; ++e) row[skew(4 * c + e)] = v[j][e];
                }
            }
        }
        __syncthreads();
        if (live) {
            float *o = m.dst + (a.mb + r) * m.ld;
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int c = sub + j * LPR;
                if (c < cpr) {
                    f4 q;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned te = t[j][e];
                        const bool zero = te == MR_ZERO;
                        const float x = row[skew(zero ? 0 : (int)(te & 0x7fffffffu))];
                        q[e] = zero ? 0.f : flip(x, te);
                    }
                    *reinterpret_cast<f4 *>(o + 4 * c) = q;
                }
            }
        }
        __syncthreads();  // the slot is rewritten by the next step
    }
}

__device__ __forceinline__ int clamp_index(float a, int n) {
    const int i = (int)a;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__device__ __forceinline__ void mirror_meta(const MirrorArgs &a, int64_t *srow) {
    const MirrorMeta &q = a.meta;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int W = q.mask ? q.W : 0;
    unsigned mt[MR_MAX_MASK_WORDS / 2];  // the source bit of this lane's bits lane, lane + 64, ...
#pragma unroll
    for (int i = 0; i < MR_MAX_MASK_WORDS / 2; ++i) {
        const int c = lane + 64 * i;
        mt[i] = c < 32 * W ? q.mask_tab[c] : MR_ZERO;
    }
    for (int64_t r0 = (int64_t)blockIdx.x * MR_META_ROWS; r0 < a.mb; r0 += (int64_t)gridDim.x * MR_META_ROWS) {
        const int64_t r = r0 + threadIdx.x;
        __syncthreads();  // (the previous step's readers of srow are done)
        if (r < a.mb) {
            const int64_t p = ring_row(a.idx[r], a.ring_base, a.ring_cap);
            srow[threadIdx.x] = p;
            const float lo = q.old_logp[p], tg = q.targets[p], ad = q.adv[p];
            q.o_old[r] = lo;
            q.o_old[a.mb + r] = lo;
            q.o_tgt[r] = tg;
            q.o_tgt[a.mb + r] = tg;
            q.o_adv[r] = ad;
            q.o_adv[a.mb + r] = ad;
        }
        __syncthreads();
        const int nrows = (int)(a.mb - r0 < MR_META_ROWS ? a.mb - r0 : MR_META_ROWS);
        const int k = q.act_dim;
        for (int e = threadIdx.x; e < nrows * k; e += MR_THREADS) {
            const int rr = e / k, j = e - rr * k;
            const float *src = q.actions + srow[rr] * k;
            const float orig = src[j];
            float mir;
            if (q.head == RLPPO_HEAD_DISCRETE) {
                mir = (float)q.act_tab[clamp_index(orig, q.n_actions)];
            } else if (q.head == RLPPO_HEAD_MULTIDISCRETE) {  // [hperm | first entry of the bin map | bins | the bin maps]
                const unsigned h_src = q.act_tab[j], first = q.act_tab[k + j], bins = q.act_tab[2 * k + j];
                mir = (float)q.act_tab[first + clamp_index(src[h_src], (int)bins)];
            } else {
                const unsigned te = q.act_tab[j];
                mir = flip(src[te & 0x7fffffffu], te);
            }
            q.o_act[(r0 + rr) * k + j] = orig;
            q.o_act[(a.mb + r0 + rr) * k + j] = mir;
        }
        if (W) {
            for (int rr = wave; rr < nrows; rr += MR_THREADS / 64) {  // a wave per row
                const unsigned w = lane < W ? q.mask[srow[rr] * W + lane] : 0u;
                if (lane < W) q.o_mask[(r0 + rr) * W + lane] = w;
                unsigned *o = q.o_mask + (a.mb + r0 + rr) * W;
#pragma unroll
                for (int i = 0; i < MR_MAX_MASK_WORDS / 2; ++i) {
                    if (2 * i < W) {  // (uniform)
                        const unsigned s = mt[i];
                        const unsigned word = __shfl(w, s == MR_ZERO ? 0 : (int)(s >> 5));
                        const unsigned long long b = __ballot(s != MR_ZERO && ((word >> (s & 31u)) & 1u));
                        const int wi = 2 * i + (lane >> 5);
                        if ((lane & 31) == 0 && wi < W) o[wi] = lane ? (unsigned)(b >> 32) : (unsigned)b;
                    }
                }
            }
        }
    }
}

// MAXS: the widest row shape among the launch's matrices -- an instantiation carries only the shapes up to it, so the common launches
// (rows up to 128 or 256 floats) are not held to the register count, and the occupancy, of the eight-chunks-per-lane shape
template <int MAXS>
__global__ __launch_bounds__(MR_THREADS) void mirror_batch_kernel(const MirrorArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mr_lds[];
    const int part = blockIdx.y;
    if (part >= a.n_mat) {
        mirror_meta(a, reinterpret_cast<int64_t *>(mr_lds));
        return;
    }
    const MirrorMat &m = a.mat[part];
    float *lds = reinterpret_cast<float *>(mr_lds);
    const int s = m.shape;  // (uniform)
    if (s == 0) mirror_rows<16, 2>(m, a, lds);
    if constexpr (MAXS >= 1)
        if (s == 1) mirror_rows<64, 1>(m, a, lds);
    if constexpr (MAXS >= 2)
        if (s == 2) mirror_rows<64, 2>(m, a, lds);
    if constexpr (MAXS >= 3)
        if (s == 3) mirror_rows<64, 4>(m, a, lds);
    if constexpr (MAXS >= 4)
        if (s == 4) mirror_rows<64, 8>(m, a, lds);
}

// the staged arrays, in the order of rlppo_mirror_staging_bytes' offsets
enum { MR_STATES = 0, MR_CRITIC, MR_ACTIONS, MR_OLD, MR_TGT, MR_ADV, MR_MASK, MR_ARRAYS };

size_t staging_plan(int64_t mb, int64_t ld_states, int64_t ld_critic, int act_dim, int mask_words, int64_t *offsets) {
    if (mb <= 0 || ld_states <= 0 || ld_critic < 0 || act_dim <= 0 || mask_words < 0) return 0;
    const int64_t bytes[MR_ARRAYS] = {2 * mb * ld_states * 4, 2 * mb * ld_critic * 4, 2 * mb * act_dim * 4, 2 * mb * 4, 2 * mb * 4, 2 * mb * 4,
                                      2 * mb * mask_words * 4};
    int64_t off = 0;
    for (int i = 0; i < MR_ARRAYS; ++i) {
        if (offsets) offsets[i] = off;
        off += round_up(bytes[i], 256);
    }
    return (size_t)off;
}

int mat_shape(const char *name, const float *src, int64_t ld, const unsigned *tab, int64_t tab_ld, MirrorMat *m) {
    RLPPO_CHECK_ARG(tab != nullptr, "mirror_batch: %s_tab is NULL", name);
    RLPPO_CHECK_ARG(src != nullptr, "mirror_batch: %s rows are NULL", name);
    RLPPO_CHECK_ARG((uintptr_t)src % 16 == 0, "mirror_batch: %s rows must be 16-byte aligned", name);
    RLPPO_CHECK_ARG((uintptr_t)tab % 16 == 0, "mirror_batch: %s_tab must be 16-byte aligned", name);
    RLPPO_CHECK_ARG(ld >= 4 && ld % 4 == 0 && ld <= MR_MAX_LD, "mirror_batch: %s leading dimension %ld must be a multiple of 4 in [4, %d]", name,
                    (long)ld, MR_MAX_LD);
    RLPPO_CHECK_ARG(tab_ld == ld, "mirror_batch: %s_tab has %ld entries, the rows a leading dimension of %ld", name, (long)tab_ld, (long)ld);
    m->src = src;
    m->tab = tab;
    m->ld = ld;
    m->shape = ld <= 128 ? 0 : ld <= 256 ? 1 : ld <= 512 ? 2 : ld <= 1024 ? 3 : 4;
    m->pitch = m->shape == 0 ? MR_PITCH16 : (int)(ld + (ld >> 6));
    return 0;
}

}  // namespace
}  // namespace rlppo

using namespace rlppo;

extern "C" {

size_t rlppo_mirror_staging_bytes(int64_t mb, int64_t ld_states, int64_t ld_critic, int32_t act_dim, int32_t mask_words, int64_t *offsets) {
    return staging_plan(mb, ld_states, ld_critic, act_dim, mask_words, offsets);
}

// every argument is checked here, by name, before any HIP call
int rlppo_mirror_batch(void *stream, const rlppo_minibatch_args *args, const rlppo_critic_rows *critic, const rlppo_symmetry *sym, void *staging,
                       size_t staging_bytes) {
    RLPPO_CHECK_ARG(args != nullptr, "mirror_batch: args is NULL");
    RLPPO_CHECK_ARG(sym != nullptr, "mirror_batch: sym is NULL");
    RLPPO_CHECK_ARG(args->mb > 0 && args->mb <= (int64_t)1 << 30, "mirror_batch: mb=%ld must be in [1, 2^30]", (long)args->mb);
    RLPPO_CHECK_ARG(staging != nullptr, "mirror_batch: staging is NULL");
    RLPPO_CHECK_ARG((uintptr_t)staging % 256 == 0, "mirror_batch: staging must be 256-byte aligned");
    const struct {
        const void *p;
        const char *name;
    } need[] = {{args->idx, "idx"}, {args->actions, "actions"}, {args->old_logp, "old_logp"}, {args->targets, "targets"},
                {args->advantages, "advantages"}, {sym->act_tab, "act_tab"}};
    for (const auto &n : need) RLPPO_CHECK_ARG(n.p != nullptr, "mirror_batch: %s is NULL", n.name);
    MirrorArgs a{};
    const bool with_critic = critic != nullptr && critic->states != nullptr;
    if (const int rc = mat_shape("obs", args->states, args->ld_states, sym->obs_tab, sym->obs_ld, &a.mat[0])) return rc;
    if (with_critic)
        if (const int rc = mat_shape("critic", critic->states, critic->ld_states, sym->critic_tab, sym->critic_ld, &a.mat[1])) return rc;
    a.n_mat = with_critic ? 2 : 1;
    // the head the description was built for
    const int head = args->head, k = args->act_dim;
    RLPPO_CHECK_ARG(head >= RLPPO_HEAD_DISCRETE && head <= RLPPO_HEAD_DIAG_GAUSSIAN, "mirror_batch: head %d", head);
    RLPPO_CHECK_ARG(sym->head == head, "mirror_batch: the symmetry describes head %d, the pass has head %d", sym->head, head);
    RLPPO_CHECK_ARG(k >= 1 && sym->act_dim == k, "mirror_batch: the symmetry's actions have act_dim %d, the pass has act_dim %d", sym->act_dim, k);
    if (head == RLPPO_HEAD_DISCRETE)
        RLPPO_CHECK_ARG(k == 1 && sym->n_actions >= 1, "mirror_batch: the discrete head has act_dim 1 and n_actions >= 1 (act_dim %d, n_actions %d)",
                        k, sym->n_actions);
    if (head == RLPPO_HEAD_MULTIDISCRETE)
        RLPPO_CHECK_ARG(k <= RLPPO_MD_MAX_HEADS && sym->n_actions >= k && sym->n_actions <= RLPPO_MD_MAX_LOGITS,
                        "mirror_batch: the multi-discrete head has at most %d components and %d logits (act_dim %d, n_actions %d)",
                        RLPPO_MD_MAX_HEADS, RLPPO_MD_MAX_LOGITS, k, sym->n_actions);
    const bool masked = args->action_mask != nullptr;
    if (masked) {
        RLPPO_CHECK_ARG(head == RLPPO_HEAD_DISCRETE || head == RLPPO_HEAD_MULTIDISCRETE, "mirror_batch: action_mask with head %d (a Gaussian head has none)", head);
        RLPPO_CHECK_ARG(sym->mask_tab != nullptr, "mirror_batch: mask_tab is NULL and the pass has an action_mask");
        RLPPO_CHECK_ARG(args->mask_words >= 1 && args->mask_words <= MR_MAX_MASK_WORDS, "mirror_batch: mask_words=%d must be in [1, %d]", args->mask_words,
                        MR_MAX_MASK_WORDS);
        RLPPO_CHECK_ARG(sym->mask_words == args->mask_words && args->mask_words == (sym->n_actions + 31) / 32,
                        "mirror_batch: mask_words=%d, the symmetry's mask_tab was built for %d words and %d logits", args->mask_words, sym->mask_words,
                        sym->n_actions);
    }
    if (const int rc = ring_window("mirror_batch", args->ring_base, args->ring_cap, &a.ring_base, &a.ring_cap)) return rc;
    int64_t off[MR_ARRAYS];
    const size_t need_bytes = staging_plan(args->mb, args->ld_states, with_critic ? critic->ld_states : 0, k, masked ? args->mask_words : 0, off);
    if (staging_bytes < need_bytes) {
        set_error("mirror_batch: staging %zu < %zu bytes", staging_bytes, need_bytes);
        return RLPPO_ERR_WORKSPACE;
    }
    char *base = static_cast<char *>(staging);
    a.mat[0].dst = reinterpret_cast<float *>(base + off[MR_STATES]);
    a.mat[1].dst = reinterpret_cast<float *>(base + off[MR_CRITIC]);
    MirrorMeta &q = a.meta;
    q.actions = args->actions;
    q.old_logp = args->old_logp;
    q.targets = args->targets;
    q.adv = args->advantages;
    q.mask = args->action_mask;
    q.act_tab = sym->act_tab;
    q.mask_tab = sym->mask_tab;
    q.o_act = reinterpret_cast<float *>(base + off[MR_ACTIONS]);
    q.o_old = reinterpret_cast<float *>(base + off[MR_OLD]);
    q.o_tgt = reinterpret_cast<float *>(base + off[MR_TGT]);
    q.o_adv = reinterpret_cast<float *>(base + off[MR_ADV]);
    q.o_mask = reinterpret_cast<unsigned *>(base + off[MR_MASK]);
    q.head = head;
    q.act_dim = k;
    q.n_actions = sym->n_actions;
    q.W = masked ? args->mask_words : 0;
    a.idx = args->idx;
    a.mb = args->mb;

    int64_t blocks = cdiv(a.mb, MR_META_ROWS);
    size_t lds = MR_META_ROWS * sizeof(int64_t);
    for (int i = 0; i < a.n_mat; ++i) {
        const int rpb = a.mat[i].shape == 0 ? MR_THREADS / 16 : MR_THREADS / 64;
        blocks = blocks > cdiv(a.mb, rpb) ? blocks : cdiv(a.mb, rpb);
        const size_t b = (size_t)rpb * a.mat[i].pitch * sizeof(float);
        lds = lds > b ? lds : b;
    }
    int cus = 0;
    if (const int rc = device_cu_count(&cus)) return rc;
    const int64_t cap = (int64_t)cus * 8;  // enough workgroups to fill the device; beyond that a workgroup walks on with its tables
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap), a.n_mat + 1);
    const int maxs = a.n_mat == 2 && a.mat[1].shape > a.mat[0].shape ? a.mat[1].shape : a.mat[0].shape;
    switch (maxs) {
        case 0: hipLaunchKernelGGL(mirror_batch_kernel<0>, grid, dim3(MR_THREADS), lds, (hipStream_t)stream, a); break;
        case 1: hipLaunchKernelGGL(mirror_batch_kernel<1>, grid, dim3(MR_THREADS), lds, (hipStream_t)stream, a); break;
        case 2: hipLaunchKernelGGL(mirror_batch_kernel<2>, grid, dim3(MR_THREADS), lds, (hipStream_t)stream, a); break;
        case 3: hipLaunchKernelGGL(mirror_batch_kernel<3>, grid, dim3(MR_THREADS), lds, (hipStream_t)stream, a); break;
        default: hipLaunchKernelGGL(mirror_batch_kernel<4>, grid, dim3(MR_THREADS), lds, (hipStream_t)stream, a); break;
    }
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
