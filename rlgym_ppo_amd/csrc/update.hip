// update.hip -- one PPO minibatch pass (rlppo_ppo_minibatch and its forms): validation, the workspace plan, the gather, the two
// networks' chains (chain.hip) as a paired or a two-chain pass on the slot's streams, the grouped weight gradients.  No device
// allocation, no synchronisation: everything is enqueued on the caller's stream or on library-owned streams joined to it.
#include <math.h>

#include "chain.hpp"

using namespace rlppo;

// ------------------------------------------------------------------------------------------- PPO minibatch
static int g_two_streams = 1;  // tuning: rlppo_dbg_set(4, 0/1)
static int g_fused_gather = 1;  // rlppo_dbg_set(26, 0/1): first-layer launches fetch their rows through the row table
static int g_update_bf16 = 0;   // rlppo_set_update_precision
static int g_group_dw = 1;  // rlppo_dbg_set(37, 0/1): [r5] grouped weight gradients (below)
static int g_head_order = 1;  // rlppo_dbg_set(31, 0/1): the critic's output-layer backward waits for the policy's loss kernel (both HBM-bound)
static int g_paired = 1;  // rlppo_dbg_set(29, 0 / 1 / 2): never / from PAIRED_MIN_ROWS rows / always (tests)
static int g_relu_bits = 1;  // rlppo_dbg_set(19, 0/1): 0 = every fp32 pass takes the plain form (measurements: what the form costs a ReLU pass)
namespace rlppo {
void set_two_streams(int v) { g_two_streams = v; }
void set_fused_gather(int v) { g_fused_gather = v; }
void set_update_precision(int v) { g_update_bf16 = v; }
int get_update_precision() { return g_update_bf16; }
void set_group_dw(int v) { g_group_dw = v; }
void set_head_order(int v) { g_head_order = v; }
void set_paired(int v) { g_paired = v; }
void set_relu_bits(int v) { g_relu_bits = v; }
}  // namespace rlppo

// Library-owned streams: slot s > 0 runs its policy chain on main[s]; every slot runs its critic chain on side[s].  One bank per
// device id (streams and events belong to the device that was current when they were made; a process may drive several).
struct SlotBank {
    hipStream_t main[RLPPO_MAX_SLOTS] = {}, side[RLPPO_MAX_SLOTS] = {};
    hipEvent_t ev_fork[RLPPO_MAX_SLOTS] = {}, ev_join[RLPPO_MAX_SLOTS] = {}, ev_slot[RLPPO_MAX_SLOTS] = {}, ev_mid[RLPPO_MAX_SLOTS] = {};
    bool pending[RLPPO_MAX_SLOTS] = {};
};
static SlotBank g_banks[64];
static int slot_bank(SlotBank **bank) {
    int dev = 0;
    RLPPO_HIP(hipGetDevice(&dev));
    RLPPO_CHECK_ARG(dev >= 0 && dev < 64, "device id %d", dev);
    *bank = &g_banks[dev];
    return 0;
}
static int ensure_slot(SlotBank &b, int s) {
    if (!b.side[s]) {
        RLPPO_HIP(hipStreamCreateWithFlags(&b.side[s], hipStreamNonBlocking));
        RLPPO_HIP(hipStreamCreateWithFlags(&b.main[s], hipStreamNonBlocking));
        RLPPO_HIP(hipEventCreateWithFlags(&b.ev_fork[s], hipEventDisableTiming));
        RLPPO_HIP(hipEventCreateWithFlags(&b.ev_join[s], hipEventDisableTiming));
        RLPPO_HIP(hipEventCreateWithFlags(&b.ev_slot[s], hipEventDisableTiming));
        RLPPO_HIP(hipEventCreateWithFlags(&b.ev_mid[s], hipEventDisableTiming));
    }
    return 0;
}
// `to` waits for everything enqueued on `from` so far
static int order_after(hipStream_t to, hipStream_t from, hipEvent_t ev) {
    RLPPO_HIP(hipEventRecord(ev, from));
    RLPPO_HIP(hipStreamWaitEvent(to, ev, 0));
    return 0;
}

// [r5] grouped weight gradients (gemm.hip: launch_gemm_tn_group): every dW / db product of a pass that is a GEMM (all layers of both
// networks but a one-output head, which is a matrix-vector kernel) is collected while the chains run their forward / dX launches and
// launched ONCE, after the chains have joined.  The group's partial tiles live in the two chains' partial buffers taken as one region.
static bool dw_is_gemv(const NetLayout &net, int l) { return l == net.n_layers - 1 && l > 0 && gemv_head_ok(net.L[l].out, net.L[l].pin); }
static size_t tn_region_floats(const NetLayout &pol, const NetLayout &val, int64_t mb, int prec) {
    const size_t chains = tn_ws_floats(pol, mb, prec) + tn_ws_floats(val, mb, prec);
    int outs[2 * RLPPO_MAX_LAYERS], ins[2 * RLPPO_MAX_LAYERS], n = 0;
    for (const NetLayout *net : {&pol, &val})
        for (int l = 0; l < net->n_layers; ++l)
            if (!dw_is_gemv(*net, l)) {
                outs[n] = net->L[l].out;
                ins[n++] = net->L[l].in;
            }
    const size_t group = tn_group_floats(outs, ins, n, mb);
    return chains > group ? chains : group;
}

// The workspace of one pass, region by region (plan_workspace): per network a NetWs (chain.hpp), and
struct WsPlan {
    NetWs pol, val;
    size_t tn_floats = 0;  // the region from pol.tn on: both chains' partial buffers, one region for the grouped dW launch
    float *states = nullptr;  // the gathered minibatch rows, [mb][policy pin]
    float *cstates = nullptr;  // [critic rows] the critic's gathered rows, [mb][critic pin], when it reads a matrix of its own
    float *g_old = nullptr, *g_adv = nullptr, *g_tgt = nullptr, *g_act = nullptr;  // the gathered per-row scalars (act_dim per row)
    unsigned *rowtab = nullptr;  // the physical buffer row of every row of the pass (gather_meta_kernel)
    unsigned short *states_b = nullptr;  // bf16 update precision: the gathered rows as bf16
};
// Pads in front of the two aligned regions: the bitmasks (8-byte words) and the bf16 region (16-byte loads).  The layout aligns
// them from the address (the base is 256-byte aligned by contract); the size reserves the largest pad.
constexpr size_t BITS_PAD_RESERVE = 2, B16_PAD_RESERVE = 4;
// Lays out the workspace of a pass from `base` into *w and returns its size in floats: the size the host is told and the layout
// the pass uses come from this one walk.  critic_rows: the plan of a pass with separate critic rows (rlppo_ppo_minibatch_critic) -- the
// critic's gathered rows follow the policy's, so they start on the boundary those do and every other plan is what it was.
static size_t plan_workspace(const NetLayout &pol, const NetLayout &val, int64_t mb, int prec, void *base, WsPlan *w, bool critic_rows) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(base);
    const size_t rows = (size_t)mb;
    size_t off = 0, slack = 0;  // floats from the base; the unused part of the pad reserves
    auto take = [&](size_t floats) {
        off += floats;
        return reinterpret_cast<float *>(addr + (off - floats) * sizeof(float));
    };
    auto align = [&](size_t floats, size_t reserve) {  // the next region starts on a boundary of `floats` floats
        const size_t pad = (floats - (addr / sizeof(float) + off) % floats) % floats;
        off += pad;
        slack += reserve - pad;
    };
    const NetLayout *nets[2] = {&pol, &val};
    NetWs *ws[2] = {&w->pol, &w->val};
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l < nets[i]->n_layers; ++l) ws[i]->act[l] = take(rows * nets[i]->L[l].pout);
    const size_t m = max_pout(pol) > max_pout(val) ? max_pout(pol) : max_pout(val);
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l + 1 < nets[i]->n_layers; ++l) ws[i]->dx[l] = take(rows * m);
    w->tn_floats = tn_region_floats(pol, val, mb, prec);
    w->pol.tn = take(w->tn_floats);
    w->val.tn = w->pol.tn + tn_ws_floats(pol, mb, prec);
    align(2, BITS_PAD_RESERVE);
    for (int i = 0; i < 2; ++i)
        for (int l = 0; l + 1 < nets[i]->n_layers; ++l) {
            const size_t f = nt_bits_floats(mb, nets[i]->L[l].pout);
            ws[i]->bits[l] = f ? reinterpret_cast<unsigned long long *>(take(f)) : nullptr;
        }
    w->states = take(rows * pol.L[0].pin);
    w->cstates = critic_rows ? take(rows * val.L[0].pin) : nullptr;
    w->g_old = take(rows);
    w->g_adv = take(rows);
    w->g_tgt = take(rows);
    w->g_act = take(rows * pol.L[pol.n_layers - 1].pout);  // (every head's act_dim is at most the policy's output width)
    w->rowtab = reinterpret_cast<unsigned *>(take(rows));
    if (prec == 1) {
        align(4, B16_PAD_RESERVE);
        size_t el = pol.L[0].pin;  // bf16 elements per row: the gathered row, and per hidden layer the activation and its gradient
        for (int i = 0; i < 2; ++i)
            for (int l = 0; l + 1 < nets[i]->n_layers; ++l) el += 2 * (size_t)nets[i]->L[l].pout;
        unsigned short *hb = reinterpret_cast<unsigned short *>(take((el * rows + 1) / 2));
        auto take16 = [&](size_t n) {
            hb += n;
            return hb - n;
        };
        w->states_b = take16(rows * pol.L[0].pin);
        for (int i = 0; i < 2; ++i)
            for (int l = 0; l + 1 < nets[i]->n_layers; ++l) ws[i]->actb[l] = take16(rows * nets[i]->L[l].pout);
        for (int i = 0; i < 2; ++i)
            for (int l = 0; l + 1 < nets[i]->n_layers; ++l) ws[i]->dxb[l] = take16(rows * nets[i]->L[l].pout);
    }
    return off + slack;
}

// update precision of a call: RLPPO_PRECISION_DEFAULT = what rlppo_set_update_precision chose for the process, else 1 + mode
static int resolve_precision(int32_t precision, int *mode) {
    RLPPO_CHECK_ARG(precision >= 0 && precision <= 3, "update precision %d (0 = process default, 1 = fp32, 2 = bf16 mixed precision, 3 = split-bf16 products)", precision);
    *mode = precision == RLPPO_PRECISION_DEFAULT ? g_update_bf16 : precision - 1;
    return 0;
}

// ---- [r3] paired launches: policy and critic bodies of the same widths (the reference's default: policy_layer_sizes ==
// critic_layer_sizes, learner.py:54-55) run every hidden layer's forward, dX and dW product as ONE launch carrying both networks
// (gemm.hip: NtAlt / TnPair), on one stream; only the two heads (a 90-wide GEMM + loss against a matrix-vector product + loss)
// still fork onto the side stream, where the critic's HBM-bound kernels run beside the policy's MFMA-bound ones.  Same products,
// same summation orders: bit-identical to the two-chain form.  Why: at the 65,536 rows of one rank of an 8-rank job a hidden-layer
// launch is 1024 workgroups = exactly one round of the chip; two such launches on two streams cost two launch boundaries and run
// at the efficiency of the small grid (0.77 of peak isolated against 0.83 at 524,288 rows), 34 launches per optimiser step;
// paired they are 22 launches of two rounds each.  (That reasoning did not survive the measurement at the 8-rank size: see below.)
// Measured (tools/ab_update.py, profiles/r03_ab_update.txt): at one rank (524,288 rows per pass) paired launches take 0.7 % off a
// learn(); at the 65,536 rows of an 8-rank share they ADD 3 % -- with one chain every launch boundary drains the chip, with two
// chains one network's boundary hides under the other's kernel -- so the pairing applies from PAIRED_MIN_ROWS rows per pass up.
constexpr int64_t PAIRED_MIN_ROWS = 262144;
static bool twin_ok(const NetLayout &p, const NetLayout &v, int64_t mb) {
    if (p.n_layers != v.n_layers || p.n_layers < 2) return false;
    for (int l = 0; l + 1 < p.n_layers; ++l) {
        const LayerLayout &a = p.L[l], &b = v.L[l];
        if (a.in != b.in || a.out != b.out || a.pin != b.pin || a.pout != b.pout) return false;
        if (a.pout % 128 != 0 || a.pin % 16 != 0 || nt_bits_floats(mb, a.pout) == 0) return false;
    }
    return true;
}

// [r3] fp32 precision: the four first-layer launches (two forwards, two dW) fetch their rows straight from the experience
// buffer through the row table (the gather fused into the load stage) when their shapes have that form; the
// separate gather pass into the workspace remains for the others.
// [r5] ... from FUSED_GATHER_MIN_ROWS rows per pass: with the weight gradients grouped (section 4.6) a 65,536-row pass is 1 % FASTER
// with the 10 us gather pass and contiguous first-layer operands than with rows fetched through the table inside four of its
// launches (11.59 against 11.71 ms per 10-epoch learn() at the 8-rank share, tools/ab_update.py, profiles/r05_ab_update_final.txt);
// at 524,288 rows per pass the two are equal and the fused form saves the 268 MB copy.  rlppo_dbg_set(26, 2): at every size (tests).
constexpr int64_t FUSED_GATHER_MIN_ROWS = 262144;
// [critic rows] One RowSource per network (rows[0] the policy's, rows[1] the critic's): the same decision for both, as before -- both
// first layers through the one row table, each from its own matrix, or both on gathered rows.  `critic` null: one matrix for both.
static void first_layer_rows(const rlppo_minibatch_args &a, const rlppo_critic_rows *critic, const NetLayout &pol, const NetLayout &val, int prec,
                             const WsPlan &w, bool plain, RowSource rows[2]) {
    const float *vx = critic ? critic->states : a.states;
    const int64_t vld = critic ? critic->ld_states : a.ld_states;
    rows[0] = RowSource{w.states, pol.L[0].pin};
    rows[1] = critic ? RowSource{w.cstates, val.L[0].pin} : rows[0];
    if (plain) return;  // [act] the gathered first layer is a ReLU-bitmask launch: the gather pass
    const int64_t src_rows = a.ring_cap > 0 ? a.ring_cap : a.n_rows;
    auto gather_form = [&](const NetLayout &n, int64_t ld) {
        return n.n_layers > 1 && nt_gather_ok(ld, src_rows, n.L[0].pout, n.L[0].pin) && tn_gather_ok(ld, src_rows) &&
               !(n.L[0].out > 64 && n.L[0].out <= 96 && !(n.L[0].in > 96 && n.L[0].in <= 112));
    };
    if (prec != 1 && (g_fused_gather == 2 || (g_fused_gather == 1 && a.mb >= FUSED_GATHER_MIN_ROWS)) && src_rows > 0 &&
        gather_form(pol, a.ld_states) && gather_form(val, vld)) {
        rows[0] = RowSource{a.states, a.ld_states, w.rowtab, src_rows};
        rows[1] = RowSource{vx, vld, w.rowtab, src_rows};
    }
}

// One validated call of rlppo_ppo_minibatch, as its forms see it
struct Pass {
    const rlppo_minibatch_args *a;
    NetLayout pol, val;
    int64_t mb;
    int prec;  // update precision: 0 fp32, 1 bf16, 2 split-bf16
    int64_t ring_base, ring_cap;
    WsPlan w;
    const rlppo_critic_rows *critic = nullptr;  // [critic rows] the critic's own row matrix (rlppo_ppo_minibatch_critic), or null
    RowSource rows[2];  // the first layers' operand: [0] the policy's, [1] the critic's (the same unless `critic`)
    LossCfg cfg;
    MdSpec md;                   // [nvec] the multi-discrete head's bins when rlppo_ppo_minibatch_nvec gives them
    bool md_general = false;
    const DiagHead *diag = nullptr;  // [diag] the diagonal-Gaussian head's parameter, gradient and scratch (rlppo_ppo_minibatch_diag)
    const float *pol_w, *val_w;  // the packed weights the products read (bf16 precision: their rounded images)
    hipStream_t st, side;        // the policy's and the critic's chain (one stream: rlppo_dbg_set(4, 0))
    DwList *defer;               // [r5] the grouped weight gradients, or null
    // [act] the hidden activation of each network (HiddenAct), and whether the pass is the PLAIN form: two chains on gathered rows,
    // dX by the saved activation -- no bitmasks, no folded value head, no paired launches, no gather-fused first layer.  A pass with
    // a tanh / ELU network is plain (that machinery is ReLU by construction); rlppo_dbg_set(19, 0) makes a ReLU pass plain too.
    int pol_act = ACT_RELU, val_act = ACT_RELU;
    bool plain = false;
};

// One network's chain of a pass: the policy's on p.st, the critic's on p.side.  Only the critic's one-output head may be folded
// into its last hidden layer (its compact outputs were zeroed by the gather launch).
static Chain pass_chain(const Pass &p, bool critic) {
    const rlppo_minibatch_args &a = *p.a;
    const unsigned short *image = reinterpret_cast<const unsigned short *>(critic ? a.val_wb16 : a.pol_wb16);
    Chain c;
    c.st = critic ? p.side : p.st;
    c.net = critic ? &p.val : &p.pol;
    c.w = critic ? p.val_w : p.pol_w;
    c.in = p.rows[critic ? 1 : 0];
    c.in_b = p.w.states_b;
    c.n = p.mb;
    c.out_tanh = !critic && a.head == RLPPO_HEAD_GAUSSIAN;
    c.hidden_act = critic ? p.val_act : p.pol_act;
    c.b = critic ? p.w.val : p.w.pol;
    if (p.plain)  // [act] the plain form: no bitmasks
        for (auto &bits : c.b.bits) bits = nullptr;
    c.grad = critic ? a.val_grad : a.pol_grad;
    c.defer = p.defer;
    c.wb16 = p.prec == 1 ? image : nullptr;
    c.x3 = p.prec == 2 ? image : nullptr;  // [r4] split-bf16
    c.may_fold = c.head_prezeroed = critic && !p.plain;
    return c;
}

static LossCfg loss_cfg(const rlppo_minibatch_args &a) {
    LossCfg c;
    c.clip = a.clip_range;
    c.clip_lo = (float)(1.0 - (double)a.clip_range);
    c.clip_hi = (float)(1.0 + (double)a.clip_range);
    c.ent_coef = a.ent_coef;
    c.mb_ratio = a.mb_ratio;
    c.inv_mb = 1.0f / (float)a.mb;
    c.var_m = a.var_m;
    c.var_b = a.var_b;
    c.adv_norm = a.adv_norm;
    c.vclip = a.value_clip;
    c.kl_slots = a.kl_slots;
    c.stop_word = a.stop_word;
    return c;
}

// the head's loss kernel on the policy's outputs, in place (the head was validated before the first launch)
static int policy_loss(hipStream_t st, const Pass &p) {
    const rlppo_minibatch_args &a = *p.a;
    const int last = p.pol.n_layers - 1;
    const LayerLayout &L = p.pol.L[last];
    const WsPlan &w = p.w;
    // [ABI 8] the masked loss reads the buffer's mask rows through idx and the ring map itself
    const MaskRows mr{a.action_mask, a.mask_words, a.idx, p.ring_base, p.ring_cap};
    if (a.head == RLPPO_HEAD_DISCRETE)
        return launch_discrete_loss(st, w.pol.act[last], L.pout, L.out, w.g_act, w.g_old, w.g_adv, p.mb, p.cfg, a.stats, a.action_mask ? &mr : nullptr);
    if (a.head == RLPPO_HEAD_GAUSSIAN)
        return launch_gaussian_loss(st, w.pol.act[last], L.pout, L.out / 2, w.g_act, w.g_old, w.g_adv, p.mb, p.cfg, a.stats);
    if (a.head == RLPPO_HEAD_DIAG_GAUSSIAN)  // [diag] + the fixed-order finish of the log_std gradient, behind it on the same stream
        return launch_diag_gaussian_loss(st, w.pol.act[last], L.pout, L.out, w.g_act, w.g_old, w.g_adv, p.mb, p.cfg, a.stats, *p.diag);
    if (p.md_general) {  // [nvec] any nvec: the general kernel, also on the reference's bins
        ++g_call_counts[CNT_MD_NVEC];
        return launch_multidiscrete_nvec_loss(st, w.pol.act[last], L.pout, w.g_act, w.g_old, w.g_adv, p.mb, p.cfg, a.stats, p.md,
                                              a.action_mask ? &mr : nullptr);
    }
    return launch_multidiscrete_loss(st, w.pol.act[last], L.pout, w.g_act, w.g_old, w.g_adv, p.mb, p.cfg, a.stats);
}

// The minibatch gather (experience_buffer.py:82-87), once for both nets: the per-row scalars, and the rows unless the first
// layers fetch them through the row table
static int gather(const Pass &p) {
    const rlppo_minibatch_args &a = *p.a;
    const WsPlan &w = p.w;
    const int width = p.pol.L[0].pin;
    float *const vout = w.val.act[p.val.n_layers - 1];
    if (p.prec == 1) {  // the rows as bf16 too
        // the fp32 form of the gathered rows only if a first layer takes the fp32 kernels (the predicates of forward_b16 / backward_b16)
        auto lean0 = [](const NetLayout &n) {
            return n.n_layers > 1 && nt_b16_ok(n.L[0].pout, n.L[0].pin, true) && tn_b16_ok(n.L[0].pout, n.L[0].pin);
        };
        const int rc = launch_gather_rows_round(p.st, a.states, a.ld_states, a.idx, lean0(p.pol) && lean0(p.val) ? nullptr : w.states,
                                                w.states_b, width, p.mb, p.ring_base, p.ring_cap);
        if (rc) return rc;
    } else if (!p.rows[0].rowtab) {  // (the per-row scalars ride in the same launch)
        GatherMeta gm;
        gm.actions = a.actions; gm.old_logp = a.old_logp; gm.adv = a.advantages; gm.targets = a.targets;
        gm.g_old = w.g_old; gm.g_adv = w.g_adv; gm.g_tgt = w.g_tgt; gm.g_act = w.g_act;
        gm.zero_n = vout;
        gm.act_dim = a.act_dim;
        if (p.critic)  // [critic rows] both matrices' rows, still one launch
            return launch_gather_rows2(p.st, a.states, a.ld_states, w.states, width, p.critic->states, p.critic->ld_states, w.cstates,
                                       p.val.L[0].pin, a.idx, p.mb, p.ring_base, p.ring_cap, &gm);
        return launch_gather_rows(p.st, a.states, a.ld_states, a.idx, w.states, width, p.mb, p.ring_base, p.ring_cap, &gm);
    }
    // ... and writes the row table the fused first layers read.  ([r5] It also zeroes the first mb floats of the critic's output
    // buffer: a folded value head accumulates into them; when the rows were gathered by a pass of their own, that launch has done
    // all of this already.)
    return launch_gather_meta(p.st, a.idx, a.actions, a.act_dim, a.old_logp, a.advantages, a.targets, w.g_act, w.g_old, w.g_adv, w.g_tgt,
                              p.mb, p.ring_base, p.ring_cap, p.rows[0].rowtab ? w.rowtab : nullptr, vout);
}

// The paired pass ([r3] paired launches, above).  It joins the critic's stream itself, before the hidden layers' backward.
static int paired_pass(const Pass &p, SlotBank &bk, int slot) {
    const rlppo_minibatch_args &a = *p.a;
    const NetLayout &pol = p.pol, &val = p.val;
    const WsPlan &w = p.w;
    const int64_t mb = p.mb;
    const hipStream_t st = p.st, hs = p.side;
    const int H = pol.n_layers - 1;  // hidden layers (the same number in both networks)
    Chain cp = pass_chain(p, false), cv = pass_chain(p, true);  // the two heads' steps (the hidden layers are launched here, two by two)
    int rc;
    // [r3] The critic's output layer is a dot product per row of activations this launch has in registers: folded into the last
    // hidden layer's forward epilogue (NtDot) it costs no pass over the 4 x 256 B per row the matrix-vector kernel re-read
    // (537 MB per 524,288-row pass, in the stretch of the pass that is HBM-bound).  Values land compact ([mb], stride 1).
    const LayerLayout &Lvh = val.L[H];
    const bool fold_v = cv.head_folded = get_fold_vhead() && gemv_head_ok(Lvh.out, Lvh.pin) && val.L[H - 1].pout / 128 <= 2;
    float *vout = w.val.act[H];
    const int64_t ldv = fold_v ? 1 : Lvh.pout;
    const RowSource &rows = p.rows[0];  // (a paired layer 0 shares one A operand: never a pass with separate critic rows)
    const float *xp = rows.x, *xv = xp;
    int64_t ldx = rows.ld;
    for (int l = 0; l < H; ++l) {
        const LayerLayout &Lp = pol.L[l], &Lv = val.L[l];
        NtAlt alt;
        alt.A = xv;
        alt.B = p.val_w + Lv.off_w;
        alt.bias = p.val_w + Lv.off_b;
        alt.C = w.val.act[l];
        alt.bits = w.val.bits[l];
        NtDot dots[2];
        const bool fold_here = fold_v && l == H - 1;
        if (fold_here) {  // (vout was zeroed by gather_meta_kernel)
            dots[1].w = p.val_w + Lvh.off_w;
            dots[1].out = vout;
            dots[1].b = p.val_w + Lvh.off_b;
        }
        rc = launch_gemm_nt_bits(st, xp, ldx, p.pol_w + Lp.off_w, Lp.pin, p.pol_w + Lp.off_b, w.pol.act[l], Lp.pout, mb, Lp.pout, Lp.pin,
                                 EPI_BIAS_RELU, w.pol.bits[l], l == 0 ? rows.rowtab : nullptr, rows.src_rows, &alt,
                                 fold_here ? dots : nullptr);
        if (rc) {
            if (rc == -1) set_error("paired pass: a hidden layer does not have the bitmask form");
            return rc == -1 ? RLPPO_ERR_ARG : rc;
        }
        cp.have_bits[l] = cv.have_bits[l] = true;
        xp = w.pol.act[l];
        xv = w.val.act[l];
        ldx = Lp.pout;
    }
    // the two heads: forward, loss, output-layer backward -- critic on the side stream
    if (hs != st) {
        rc = order_after(hs, st, bk.ev_fork[slot]);
        if (rc) return rc;
    }
    if (!fold_v) {
        rc = output_forward(cv, xv, ldx);
        if (rc) return rc;
    }
    rc = launch_value_loss(hs, vout, ldv, w.g_tgt, w.g_adv, mb, p.cfg, a.stats);
    if (rc) return rc;
    // The critic's head kernels are matrix-vector products: HBM-bound, like the policy's loss kernel, unlike the policy head's
    // GEMMs.  Ordered so that the two HBM-bound stretches do not meet: critic forward + loss beside the policy head's forward
    // GEMM, the critic's output-layer backward only after the policy's loss, beside the policy head's dW / dX GEMMs.
    const bool ordered = g_head_order && hs != st;
    if (!ordered) {
        rc = layer_backward(cv, H, true);
        if (rc) return rc;
    }
    rc = output_forward(cp, xp, ldx);
    if (rc) return rc;
    rc = policy_loss(st, p);
    if (rc) return rc;
    if (ordered) {
        rc = order_after(hs, st, bk.ev_mid[slot]);
        if (rc) return rc;
        rc = layer_backward(cv, H, true);
        if (rc) return rc;
    }
    rc = layer_backward(cp, H, true);
    if (rc) return rc;
    if (hs != st) {
        rc = order_after(st, hs, bk.ev_join[slot]);
        if (rc) return rc;
    }
    // hidden layers, backward: dW (+ reduction) of both networks, then dX of both
    for (int l = H - 1; l >= 0; --l) {
        const LayerLayout &Lp = pol.L[l], &Lv = val.L[l];
        const RowSource Xp = l > 0 ? RowSource{w.pol.act[l - 1], pol.L[l - 1].pout} : rows;
        const RowSource Xv = l > 0 ? RowSource{w.val.act[l - 1], val.L[l - 1].pout} : rows;
        if (p.defer) {
            p.defer->add(Lp, w.pol.dx[l], Xp, a.pol_grad);
            p.defer->add(Lv, w.val.dx[l], Xv, a.val_grad);
        } else {
            TnPair pr;
            pr.dY = w.val.dx[l];
            pr.X = Xv.x;
            pr.dW = a.val_grad + Lv.off_flat_w;
            pr.db = a.val_grad + Lv.off_flat_b;
            pr.ws = w.val.tn;
            rc = launch_gemm_tn(st, w.pol.dx[l], Lp.pout, Lp.pout, Xp.x, Xp.ld, Lp.pin, a.pol_grad + Lp.off_flat_w, a.pol_grad + Lp.off_flat_b,
                                Lp.out, Lp.in, mb, w.pol.tn, tn_layer_floats(pol, l, mb, 0), Xp.rowtab, Xp.src_rows, &pr);
            if (rc) return rc;
        }
        if (l == 0) break;
        NtAlt alt;
        alt.A = w.val.dx[l];
        alt.B = p.val_w + Lv.off_wt;
        alt.C = w.val.dx[l - 1];
        alt.bits = w.val.bits[l - 1];
        rc = launch_gemm_nt_bits(st, w.pol.dx[l], Lp.pout, p.pol_w + Lp.off_wt, Lp.pout, nullptr, w.pol.dx[l - 1], Lp.pin, mb, Lp.pin,
                                 Lp.pout, EPI_MASK, w.pol.bits[l - 1], nullptr, 0, &alt);
        if (rc) return rc == -1 ? RLPPO_ERR_ARG : rc;
    }
    return 0;
}

// One launch chain per network: the critic's on p.side, then the policy's on p.st
static int two_chain_pass(const Pass &p) {
    Chain val = pass_chain(p, true), pol = pass_chain(p, false);
    const bool b16 = p.prec == 1;
    for (Chain *c : {&val, &pol})
        if (int rc = b16 ? forward_b16(*c) : forward(*c)) return rc;
    // loss epilogue: outputs -> output gradients in place, report statistics accumulated on device.  The value loss only
    // needs the critic's output and the policy loss only the policy's, so each chain runs its own loss kernel and the chains
    // do not meet until the end of the minibatch.
    const int vlast = p.val.n_layers - 1;
    const int64_t ldv = val.head_folded ? 1 : p.val.L[vlast].pout;  // (a folded head's outputs are compact)
    int rc = launch_value_loss(p.side, p.w.val.act[vlast], ldv, p.w.g_tgt, p.w.g_adv, p.mb, p.cfg, p.a->stats);
    if (rc) return rc;
    rc = policy_loss(p.st, p);
    if (rc) return rc;
    for (Chain *c : {&val, &pol})
        if ((rc = b16 ? backward_b16(*c) : backward(*c))) return rc;
    return 0;
}

// What a pass may bring beyond rlppo_minibatch_args: every optional part once, whichever exported form brought it
struct PassOpts {
    const int32_t *md_nvec = nullptr;  // [nvec] the multi-discrete head's md_heads bins (host); null = the reference's head, the fixed kernel
    int32_t md_heads = 0;
    DiagHead diag;  // [diag] the diagonal-Gaussian head's parameter, gradient and scratch, when has_diag
    bool has_diag = false;
    int pol_act = ACT_RELU, val_act = ACT_RELU;  // [act] the hidden activations
    const rlppo_critic_rows *critic = nullptr;   // [critic rows] the critic's own row matrix: non-null only with critic->states set
    const float *vnorm = nullptr;                // [vnorm] the value statistic's scale
};

static int ppo_minibatch(void *stream, const rlppo_minibatch_args *a, const PassOpts &o) {
    // ---- validation: every argument error is reported here, before the first HIP call
    RLPPO_CHECK_ARG(a != nullptr, "ppo_minibatch: null args");
    Pass p;
    p.a = a;
    const DiagHead *const diag = p.diag = o.has_diag ? &o.diag : nullptr;
    const rlppo_critic_rows *const critic = p.critic = o.critic;
    int rc = make_layout(a->pol_dims, a->pol_layers, &p.pol);
    if (rc) return rc;
    rc = make_layout(a->val_dims, a->val_layers, &p.val);
    if (rc) return rc;
    const NetLayout &pol = p.pol, &val = p.val;
    const int64_t mb = p.mb = a->mb;
    if (mb == 0) return 0;
    // [r5] the precision is an argument of the call (two learners of one process may differ); the process-wide switch is its default
    rc = resolve_precision(a->precision, &p.prec);
    if (rc) return rc;
    // [act] the hidden activations: tanh / ELU passes are fp32 (the bf16 and split-bf16 kernels carry the ReLU bitmask by construction)
    RLPPO_CHECK_ARG(hidden_act_ok(o.pol_act) && hidden_act_ok(o.val_act), "ppo_minibatch: pol_hidden_act=%d val_hidden_act=%d (0 = ReLU, 1 = tanh, 2 = ELU)",
                    o.pol_act, o.val_act);
    p.pol_act = o.pol_act;
    p.val_act = o.val_act;
    const bool non_relu = o.pol_act != ACT_RELU || o.val_act != ACT_RELU;
    RLPPO_CHECK_ARG(!(non_relu && p.prec != 0), "ppo_minibatch: hidden activation %s with update precision %s: the %s kernels are ReLU only (use fp32)",
                    hidden_act_name(o.pol_act != ACT_RELU ? o.pol_act : o.val_act), p.prec == 1 ? "bf16" : "x3", p.prec == 1 ? "bf16" : "split-bf16");
    p.plain = non_relu || (p.prec == 0 && !g_relu_bits);
    RLPPO_CHECK_ARG(mb > 0 && a->pol_packed && a->val_packed && a->pol_grad && a->val_grad && a->states && a->actions &&
                        a->old_logp && a->targets && a->advantages && a->idx && a->stats && a->workspace,
                    "ppo_minibatch: null pointer");
    RLPPO_CHECK_ARG(val.L[val.n_layers - 1].out == 1, "ppo_minibatch: critic must have one output");
    RLPPO_CHECK_ARG(a->value_clip >= 0.f && a->value_clip < INFINITY, "ppo_minibatch: value_clip=%g", (double)a->value_clip);
    RLPPO_CHECK_ARG((reinterpret_cast<uintptr_t>(o.vnorm) & 15) == 0, "ppo_minibatch_vnorm: vnorm scale must be 16-byte aligned");
    RLPPO_CHECK_ARG(critic || pol.L[0].in == val.L[0].in, "ppo_minibatch: policy and critic observe different sizes");
    if (critic) {  // [critic rows] val_dims[0] is the width of the critic's own matrix
        RLPPO_CHECK_ARG(critic->ld_states >= val.L[0].pin && critic->ld_states % 4 == 0,
                        "ppo_minibatch_critic: critic ld_states=%ld < %d (the padded width of val_dims[0]=%d), or not a multiple of 4",
                        (long)critic->ld_states, val.L[0].pin, val.L[0].in);
        RLPPO_CHECK_ARG((reinterpret_cast<uintptr_t>(critic->states) & 15) == 0, "ppo_minibatch_critic: critic states must be 16-byte aligned");
        RLPPO_CHECK_ARG(p.prec != 1, "ppo_minibatch_critic: update precision bf16 with separate critic rows: its gather writes one bf16 image, "
                                     "of the policy's rows (use fp32 or x3)");
    }
    RLPPO_CHECK_ARG(a->ld_states >= pol.L[0].pin && a->ld_states % 4 == 0, "ppo_minibatch: ld_states=%ld < %d",
                    (long)a->ld_states, pol.L[0].pin);
    const size_t ws_bytes = plan_workspace(pol, val, mb, p.prec, a->workspace, &p.w, critic != nullptr) * sizeof(float);
    if (a->ws_bytes < ws_bytes) {
        set_error("ppo_minibatch: workspace %zu < %zu bytes%s", a->ws_bytes, ws_bytes,
                  critic ? " (separate critic rows: rlppo_minibatch_workspace_bytes_critic)" : "");
        return RLPPO_ERR_WORKSPACE;
    }
    // every head pins act_dim to at most the policy's output width (the gathered actions' slots); the loss kernel's width too
    const int n_out = pol.L[pol.n_layers - 1].out;
    RLPPO_CHECK_ARG(a->head == RLPPO_HEAD_DISCRETE || a->head == RLPPO_HEAD_GAUSSIAN || a->head == RLPPO_HEAD_MULTIDISCRETE ||
                        a->head == RLPPO_HEAD_DIAG_GAUSSIAN, "ppo_minibatch: unknown head %d", a->head);
    // [diag] the diagonal-Gaussian head has a parameter of its own: only rlppo_ppo_minibatch_diag brings it (and nothing else does)
    RLPPO_CHECK_ARG(a->head != RLPPO_HEAD_DIAG_GAUSSIAN || diag,
                    "ppo_minibatch: head %d (RLPPO_HEAD_DIAG_GAUSSIAN) needs log_std, its gradient and scratch: rlppo_ppo_minibatch_diag", a->head);
    RLPPO_CHECK_ARG(!diag || a->head == RLPPO_HEAD_DIAG_GAUSSIAN, "ppo_minibatch_diag: head %d, but the entry point runs RLPPO_HEAD_DIAG_GAUSSIAN (%d) only",
                    a->head, RLPPO_HEAD_DIAG_GAUSSIAN);
    // [ABI 8] action masks: the discrete head, and [nvec, masked] the multi-discrete head's general kernels (md_nvec given, also for
    // the reference's bins): one bit per output, ceil(n_out / 32) words per buffer row
    RLPPO_CHECK_ARG(!a->action_mask || a->head == RLPPO_HEAD_DISCRETE || (a->head == RLPPO_HEAD_MULTIDISCRETE && o.md_nvec),
                    "ppo_minibatch: action_mask is an option of the discrete head, not of the %s head",
                    a->head == RLPPO_HEAD_GAUSSIAN ? "Gaussian"
                    : a->head == RLPPO_HEAD_DIAG_GAUSSIAN ? "diagonal-Gaussian"
                                                          : "multi-discrete (without md_nvec: the fixed-bin kernels take no mask)");
    if (int rc_mask = mask_words_check(a->action_mask, a->mask_words, n_out, "ppo_minibatch", false)) return rc_mask;
    if (a->head == RLPPO_HEAD_DISCRETE) {
        RLPPO_CHECK_ARG(a->act_dim == 1, "discrete head: act_dim must be 1");
        RLPPO_CHECK_ARG(pol.L[pol.n_layers - 1].pout <= DISCRETE_LOSS_MAX_LD, "discrete head: padded width %ld too large",
                        (long)pol.L[pol.n_layers - 1].pout);
    }
    if (a->head == RLPPO_HEAD_GAUSSIAN)
        RLPPO_CHECK_ARG(n_out % 2 == 0 && a->act_dim == n_out / 2, "gaussian head: act_dim=%d, outputs=%d", a->act_dim, n_out);
    if (a->head == RLPPO_HEAD_DIAG_GAUSSIAN) {
        RLPPO_CHECK_ARG(a->act_dim == n_out, "diagonal-Gaussian head: act_dim=%d, but the policy has %d outputs (pol_dims[pol_layers])", a->act_dim, n_out);
        RLPPO_CHECK_ARG(n_out <= RLPPO_DIAG_MAX_K, "diagonal-Gaussian head: %d action dimensions, RLPPO_DIAG_MAX_K allows 1 .. %d", n_out, RLPPO_DIAG_MAX_K);
        RLPPO_CHECK_ARG(diag->log_std && diag->log_std_grad, "ppo_minibatch_diag: log_std / log_std_grad is NULL");
        RLPPO_CHECK_ARG(diag->scratch && diag->scratch_bytes >= diag_scratch_bytes(mb, n_out),
                        "ppo_minibatch_diag: scratch of %zu bytes, rlppo_diag_scratch_bytes(%ld, %d) = %zu needed", diag->scratch_bytes, (long)mb, n_out,
                        diag_scratch_bytes(mb, n_out));
    }
    // [nvec] md_nvec: the multi-discrete head alone; NULL = the reference's 21 outputs / 8 heads and the fixed kernel
    RLPPO_CHECK_ARG(!o.md_nvec || a->head == RLPPO_HEAD_MULTIDISCRETE, "ppo_minibatch: md_nvec is an option of the multi-discrete head, not of the %s head",
                    a->head == RLPPO_HEAD_GAUSSIAN ? "Gaussian" : a->head == RLPPO_HEAD_DIAG_GAUSSIAN ? "diagonal-Gaussian" : "discrete");
    if (a->head == RLPPO_HEAD_MULTIDISCRETE && o.md_nvec) {
        rc = md_spec_make(o.md_nvec, o.md_heads, "multi-discrete head: md_nvec / md_heads", &p.md);
        if (rc) return rc;
        p.md_general = true;
        RLPPO_CHECK_ARG(p.md.S == n_out, "multi-discrete head: md_nvec sums to %d, but the policy has %d outputs", p.md.S, n_out);
        RLPPO_CHECK_ARG(a->act_dim == p.md.H, "multi-discrete head: act_dim=%d, but md_heads=%d", a->act_dim, p.md.H);
    } else if (a->head == RLPPO_HEAD_MULTIDISCRETE)
        RLPPO_CHECK_ARG(n_out == 21 && a->act_dim == 8, "multi-discrete head: needs 21 outputs and act_dim 8");
    RLPPO_CHECK_ARG(p.prec != 1 || (a->pol_packed_r && a->val_packed_r && a->pol_wb16 && a->val_wb16),
                    "ppo_minibatch: the bf16 update precision needs the rlppo_net_pack_bf16 images of both networks (pol_packed_r / val_packed_r / pol_wb16 / val_wb16)");
    RLPPO_CHECK_ARG(p.prec != 2 || (a->pol_wb16 && a->val_wb16),
                    "ppo_minibatch: the split-bf16 update precision needs the rlppo_net_pack_x3 images of both networks (pol_wb16 / val_wb16)");
    rc = ring_window("ppo_minibatch", a->ring_base, a->ring_cap, &p.ring_base, &p.ring_cap);
    if (rc) return rc;
    const int slot = a->slot;
    RLPPO_CHECK_ARG(slot >= 0 && slot < RLPPO_MAX_SLOTS, "ppo_minibatch: slot %d not in [0, %d)", slot, RLPPO_MAX_SLOTS);

    // ---- plan: the first layers' rows, the form, the loss settings
    first_layer_rows(*a, critic, pol, val, p.prec, p.w, p.plain, p.rows);
    const bool twin = p.prec == 0 && !p.plain && !critic && (g_paired == 2 || (g_paired == 1 && mb >= PAIRED_MIN_ROWS)) && twin_ok(pol, val, mb);
    p.cfg = loss_cfg(*a);
    p.cfg.vnorm = o.vnorm;  // [vnorm] the value loss alone reads it: same plan, same launches
    p.pol_w = p.prec == 1 ? a->pol_packed_r : a->pol_packed;
    p.val_w = p.prec == 1 ? a->val_packed_r : a->val_packed;
    DwList dws;
    p.defer = (g_group_dw && p.prec != 1) ? &dws : nullptr;

    SlotBank *bank = nullptr;
    rc = slot_bank(&bank);
    if (rc) return rc;
    SlotBank &bk = *bank;
    rc = ensure_slot(bk, slot);
    if (rc) return rc;
    const hipStream_t caller = (hipStream_t)stream;
    p.st = caller;
    if (slot > 0) {  // this minibatch's chains run beside the caller's stream; rlppo_ppo_join() brings them back
        p.st = bk.main[slot];
        rc = order_after(p.st, caller, bk.ev_slot[slot]);
        if (rc) return rc;
        bk.pending[slot] = true;
    }
    rc = gather(p);
    if (rc) return rc;
    // The two networks are independent until the loss epilogue and again after it, so their launch chains run on
    // two streams (the caller's + one library-owned side stream, forked/joined with events: capturable).  Each
    // launch is only 50-100 us long at K <= 256, so letting one chain's kernels fill the CUs that the other chain's
    // ramp-up / tail leaves idle is worth more than any single-kernel tweak.
    p.side = p.st;
    if (g_two_streams) {
        p.side = bk.side[slot];
        rc = order_after(p.side, p.st, bk.ev_fork[slot]);
        if (rc) return rc;
    }
    ++g_call_counts[CNT_PASS];
    if (twin) ++g_call_counts[CNT_PAIRED_PASS];
    if (p.rows[0].rowtab) ++g_call_counts[CNT_GATHER_FUSED_PASS];
    if (critic) ++g_call_counts[CNT_CRITIC_ROWS_PASS];
    rc = twin ? paired_pass(p, bk, slot) : two_chain_pass(p);
    if (rc) return rc;
    if (!twin && p.side != p.st) {  // (the paired pass has joined already)
        rc = order_after(p.st, p.side, bk.ev_join[slot]);
        if (rc) return rc;
    }
    if (p.defer && dws.n) {  // [r5] every GEMM-shaped weight gradient of the pass: one launch + one reduction, after the chains have joined
        ++g_call_counts[CNT_GROUP_DW];
        rc = launch_gemm_tn_group(p.st, dws.p, dws.n, mb, p.w.pol.tn, p.w.tn_floats);
    }
    return rc;
}

static DiagHead diag_head(const float *log_std, float *log_std_grad, void *scratch, size_t scratch_bytes) {
    return DiagHead{log_std, log_std_grad, reinterpret_cast<double *>(scratch), scratch_bytes};
}
static bool scratch_aligned(const void *scratch) { return (reinterpret_cast<uintptr_t>(scratch) & 7) == 0; }
// The optional parts of rlppo_ppo_minibatch_ex / _critic / _vnorm, decoded once: a NULL ext is the zeroed one, a critic struct without states
// and a value norm without a scale are absent.  The call is named after the last part it brings, whichever of the three forms it came through.
static int ppo_minibatch_opts(void *stream, const rlppo_minibatch_args *a, const rlppo_minibatch_ext *ext, const rlppo_critic_rows *critic,
                              const rlppo_value_norm *vnorm) {
    const rlppo_minibatch_ext none = {};
    if (!ext) ext = &none;
    const bool has_diag = ext->log_std || ext->log_std_grad || ext->scratch || ext->scratch_bytes;
    const PassOpts o{ext->md_nvec, ext->md_heads, diag_head(ext->log_std, ext->log_std_grad, ext->scratch, ext->scratch_bytes), has_diag,
                     ext->pol_hidden_act, ext->val_hidden_act, critic && critic->states ? critic : nullptr, vnorm ? vnorm->scale : nullptr};
    RLPPO_CHECK_ARG(scratch_aligned(ext->scratch), "%s: scratch must be 8-byte aligned",
                    o.vnorm ? "ppo_minibatch_vnorm" : o.critic ? "ppo_minibatch_critic" : "ppo_minibatch_ex");
    return ppo_minibatch(stream, a, o);
}

static size_t workspace_bytes(const int32_t *pol_dims, int32_t pol_layers, const int32_t *val_dims, int32_t val_layers, int64_t mb,
                              int32_t precision, bool critic_rows) {
    NetLayout pol, val;
    int prec = 0;
    if (make_layout(pol_dims, pol_layers, &pol) || make_layout(val_dims, val_layers, &val) || resolve_precision(precision, &prec)) return 0;
    WsPlan unused;
    return plan_workspace(pol, val, mb > 0 ? mb : 0, prec, nullptr, &unused, critic_rows) * sizeof(float) + 256;
}

extern "C" {

size_t rlppo_minibatch_workspace_bytes_for(const int32_t *pol_dims, int32_t pol_layers, const int32_t *val_dims, int32_t val_layers,
                                           int64_t mb, int32_t precision) {
    return workspace_bytes(pol_dims, pol_layers, val_dims, val_layers, mb, precision, false);
}
size_t rlppo_minibatch_workspace_bytes_critic(const int32_t *pol_dims, int32_t pol_layers, const int32_t *val_dims, int32_t val_layers,
                                              int64_t mb, int32_t precision) {
    return workspace_bytes(pol_dims, pol_layers, val_dims, val_layers, mb, precision, true);
}
size_t rlppo_minibatch_workspace_bytes(const int32_t *pol_dims, int32_t pol_layers, const int32_t *val_dims,
                                       int32_t val_layers, int64_t mb) {
    return workspace_bytes(pol_dims, pol_layers, val_dims, val_layers, mb, RLPPO_PRECISION_DEFAULT, false);
}

// one call with optional parts: each form fills a PassOpts with what it brings
int rlppo_ppo_minibatch(void *stream, const rlppo_minibatch_args *a) { return ppo_minibatch(stream, a, PassOpts{}); }
int rlppo_ppo_minibatch_nvec(void *stream, const rlppo_minibatch_args *a, const int32_t *md_nvec, int32_t md_heads) {
    return ppo_minibatch(stream, a, PassOpts{md_nvec, md_heads});
}
int rlppo_ppo_minibatch_diag(void *stream, const rlppo_minibatch_args *a, const float *log_std, float *log_std_grad, void *scratch,
                             size_t scratch_bytes) {
    RLPPO_CHECK_ARG(scratch_aligned(scratch), "ppo_minibatch_diag: scratch must be 8-byte aligned");
    return ppo_minibatch(stream, a, PassOpts{nullptr, 0, diag_head(log_std, log_std_grad, scratch, scratch_bytes), true});
}
// [act] every head through one call: the hidden activations + what the _nvec / _diag entry points bring.  NULL / zeroed ext: rlppo_ppo_minibatch
int rlppo_ppo_minibatch_ex(void *stream, const rlppo_minibatch_args *a, const rlppo_minibatch_ext *ext) {
    return ppo_minibatch_opts(stream, a, ext, nullptr, nullptr);
}
// [critic rows] the same call with the critic's own row matrix; no matrix: rlppo_ppo_minibatch_ex
int rlppo_ppo_minibatch_critic(void *stream, const rlppo_minibatch_args *a, const rlppo_minibatch_ext *ext, const rlppo_critic_rows *critic) {
    return ppo_minibatch_opts(stream, a, ext, critic, nullptr);
}
// [vnorm] the same call with the critic trained on normalised value targets; no scale: rlppo_ppo_minibatch_critic
int rlppo_ppo_minibatch_vnorm(void *stream, const rlppo_minibatch_args *a, const rlppo_minibatch_ext *ext, const rlppo_critic_rows *critic,
                              const rlppo_value_norm *vnorm) {
    return ppo_minibatch_opts(stream, a, ext, critic, vnorm);
}

size_t rlppo_diag_scratch_bytes(int64_t mb, int32_t k) { return diag_scratch_bytes(mb, k); }
// [diag] the diagonal-Gaussian head's loss launch and the finish of its log_std reduction on their own (tools/diag_gaussian_cost.py)
int rlppo_dbg_diag_loss(void *stream, float *y, int64_t ld, int32_t k, const float *actions, const float *old_logp, const float *advantages,
                        int64_t mb, float clip_range, float ent_coef, float mb_ratio, const float *log_std, float *log_std_grad, void *scratch,
                        size_t scratch_bytes, double *stats, int32_t part) {
    RLPPO_CHECK_ARG(mb > 0 && y && actions && old_logp && advantages && stats && part >= 0 && part <= 2, "dbg_diag_loss: bad argument");
    rlppo_minibatch_args a = {};
    a.clip_range = clip_range;
    a.ent_coef = ent_coef;
    a.mb_ratio = mb_ratio;
    a.mb = mb;
    return launch_diag_gaussian_loss((hipStream_t)stream, y, ld, k, actions, old_logp, advantages, mb, loss_cfg(a), stats,
                                     diag_head(log_std, log_std_grad, scratch, scratch_bytes), part);
}

int rlppo_ppo_join(void *stream) {
    SlotBank *bank = nullptr;
    int rc = slot_bank(&bank);
    if (rc) return rc;
    SlotBank &bk = *bank;
    for (int s = 1; s < RLPPO_MAX_SLOTS; ++s)
        if (bk.pending[s]) {
            rc = order_after((hipStream_t)stream, bk.main[s], bk.ev_slot[s]);
            if (rc) return rc;
            bk.pending[s] = false;
        }
    return 0;
}

}  // extern "C"
