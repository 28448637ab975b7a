// api.hip -- the extern "C" surface declared in include/rlppo.h, but for the PPO pass (update.hip) and the single-kernel
// rlppo_dbg_* entry points (dbg_api.hip): argument checking, packed-layout bookkeeping and the launch sequences (forward,
// sampling, GAE, clip+Adam), the switches and counters.  No device allocation, no synchronisation: everything is enqueued on
// the caller's stream.
#include "build_id.h"
#include <math.h>
#include <stdarg.h>
#include <string.h>

#include "chain.hpp"

namespace rlppo {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// Width the first layer's contraction is padded to (zero columns in the packed weights, zero-padded observation rows).  The
// fp32 kernels step K in tiles of 16 and the bf16 kernels in tiles of 64: pad to 16 when that saves at least a tenth of the
// contraction over padding to 64 (107 -> 112 instead of 128: an eighth of the first layer's products, forward and dW, multiplied
// zeros [r3]), else to 64 (231 -> 256: the bf16 update precision keeps its kernels on BASELINE configs[4]).
static int64_t padded_width(int64_t d) {
    const int64_t p16 = round_up(d, 16), p64 = round_up(d, 64);
    return (p64 - p16) * 10 >= p64 ? p16 : p64;
}
static int64_t padded_out(int64_t d) {
    if (d <= 32) return 32;
    if (d <= 64) return 64;
    if (d <= 96) return 96;
    return round_up(d, 128);
}

int make_layout(const int32_t *dims, int32_t n_layers, NetLayout *out) {
    RLPPO_CHECK_ARG(dims != nullptr && n_layers >= 1 && n_layers <= RLPPO_MAX_LAYERS, "network: n_layers=%d not in [1,%d]",
                    n_layers, RLPPO_MAX_LAYERS);
    for (int i = 0; i <= n_layers; ++i) RLPPO_CHECK_ARG(dims[i] >= 1, "network: dims[%d]=%d", i, dims[i]);
    out->n_layers = n_layers;
    int64_t off = 0, flat = 0;
    int pin = (int)padded_width(dims[0]);
    for (int l = 0; l < n_layers; ++l) {
        LayerLayout &L = out->L[l];
        L.in = dims[l];
        L.out = dims[l + 1];
        L.pin = pin;
        L.pout = (int)padded_out(dims[l + 1]);
        L.off_w = off;
        off += (int64_t)L.pout * L.pin;
        L.off_wt = off;
        off += (int64_t)L.pin * L.pout;
        L.off_b = off;
        off += L.pout;
        L.off_flat_w = flat;
        flat += (int64_t)L.out * L.in;
        L.off_flat_b = flat;
        flat += L.out;
        pin = L.pout;
    }
    out->packed_floats = off;
    out->flat_floats = flat;
    return 0;
}

// [ABI 8] a mask has the words per row its entries need.  who: the caller's name; logits: it calls an entry a logit, not an action
// (every caller's message reads as it always did)
int mask_words_check(const void *mask, int mask_words, int bits, const char *who, bool logits) {
    RLPPO_CHECK_ARG(!mask || mask_words == (bits + 31) / 32,
                    logits ? "%s: mask_words=%d, but %d logits need %d words per row" : "%s: mask_words=%d, but n_actions=%d needs %d words per row",
                    who, mask_words, bits, (bits + 31) / 32);
    return 0;
}

std::atomic<long long> g_call_counts[CNT_COUNT];

}  // namespace rlppo

using namespace rlppo;

static int g_fused_act = 1;  // rlppo_dbg_set(27, 0/1): rlppo_discrete_act as one fused launch (fused_act.hip)
// One workgroup per 16 rows and one workgroup per CU (102 KiB of LDS): a launch is rounds of 4096 rows at ~25 us each, whatever
// the round's fill.  Measured (tools/act_kernel_time.py): 64 rows 26 us (chain 70), 4096 rows 29 us (chain 75), 16,384 rows 100 us
// (chain 86): beyond two rounds the layer-by-layer GEMMs, which fill the chip, win.
constexpr int64_t FUSED_ACT_MAX_ROWS = 8192;

// [r5] per-call options of the rollout entry points (rlppo_act_opts): the inference precision of THIS call, and the words the call
// stores into host-visible memory once every output is visible (the host polls them instead of synchronising the stream)
struct ActCtx {
    int bf16 = 0;
    unsigned *done = nullptr;
    unsigned done_value = 0;
    unsigned *noise_ctl = nullptr;
    const unsigned *mask = nullptr;  // [ABI 8] rlppo_act_opts.action_mask / mask_words
    int mask_words = 0;
    int hidden_act = ACT_RELU;       // [act] rlppo_act_opts.hidden_act
};
// One call of a rollout entry point: the network, the call's options and, once act_chain has run, the last layer's output
struct ActCall {
    NetLayout net;
    ActCtx cx;
    const float *o = nullptr;
    int64_t ldo = 0;
};
// late_noise: the entry point can take its noise while it runs (rlppo_act_opts.noise_ctl; rlppo_discrete_step alone)
// mask_for: nullptr = the entry point samples the discrete head and takes an action mask; else the name of what it runs instead
static int act_open(ActCall *call, const int32_t *dims, int32_t n_layers, const rlppo_act_opts *o, bool late_noise, const char *mask_for) {
    if (int rc = make_layout(dims, n_layers, &call->net)) return rc;
    ActCtx *c = &call->cx;
    c->bf16 = get_infer_bf16();
    if (!o) return 0;
    RLPPO_CHECK_ARG(o->precision == RLPPO_PRECISION_DEFAULT || o->precision == RLPPO_PRECISION_FP32 || o->precision == RLPPO_PRECISION_BF16,
                    "act options: inference precision %d (0 = process default, 1 = fp32, 2 = bf16 operands)", o->precision);
    if (o->precision != RLPPO_PRECISION_DEFAULT) c->bf16 = o->precision == RLPPO_PRECISION_BF16;
    RLPPO_CHECK_ARG(hidden_act_ok(o->hidden_act), "act options: hidden_act %d (0 = ReLU, 1 = tanh, 2 = ELU)", o->hidden_act);
    c->hidden_act = o->hidden_act;
    RLPPO_CHECK_ARG(!(c->bf16 && c->hidden_act != ACT_RELU),
                    "act options: hidden activation %s with the bf16 inference precision: the bf16-operand kernels are ReLU only",
                    hidden_act_name(c->hidden_act));
    c->done = o->done_words;
    c->done_value = o->done_value;
    c->noise_ctl = o->noise_ctl;
    c->mask = o->action_mask;
    c->mask_words = o->mask_words;
    RLPPO_CHECK_ARG(!o->action_mask || !mask_for, "act options: action_mask is an option of the discrete head, not of %s", mask_for ? mask_for : "");
    RLPPO_CHECK_ARG(!o->noise_ctl || late_noise, "act options: noise_ctl is an option of rlppo_discrete_step");
    RLPPO_CHECK_ARG(!o->noise_ctl || (o->done_words && !(o->done_value & 0x80000000u)),
                    "act options: noise_ctl needs done_words (a kernel that gives up on the noise reports it there) and done_value < 2^31");
    return 0;
}
static size_t forward_ws_floats(const NetLayout &net, int64_t n) { return (size_t)2 * (size_t)n * (size_t)max_pout(net); }
// runs the call's layer chain (inference: no bitmasks, nothing saved) with ping-pong buffers from the workspace; the last layer's
// output goes to final_out when that is given; call->o / ldo find it
static int act_chain(hipStream_t st, ActCall *call, const float *packed, const float *obs, int64_t ld_obs, int64_t n, int out_tanh, void *ws,
                     size_t ws_bytes, float *final_out) {
    const NetLayout &net = call->net;
    if (ws_bytes < forward_ws_floats(net, n) * sizeof(float)) {
        set_error("forward: workspace %zu < %zu bytes", ws_bytes, forward_ws_floats(net, n) * sizeof(float));
        return RLPPO_ERR_WORKSPACE;
    }
    RLPPO_CHECK_ARG(ld_obs >= net.L[0].pin && ld_obs % 4 == 0, "forward: ld_obs=%ld must be >= %d (zero padded rows)",
                    (long)ld_obs, net.L[0].pin);
    float *b0 = reinterpret_cast<float *>(ws);
    float *b1 = b0 + (size_t)n * max_pout(net);
    Chain c;
    c.st = st;
    c.net = &net;
    c.w = packed;
    c.in = RowSource{obs, ld_obs};
    c.n = n;
    c.out_tanh = out_tanh;
    c.hidden_act = call->cx.hidden_act;
    c.bf16_operands = call->cx.bf16;
    for (int l = 0; l < net.n_layers; ++l) c.b.act[l] = (l & 1) ? b1 : b0;
    if (final_out) c.b.act[net.n_layers - 1] = final_out;
    call->o = c.b.act[net.n_layers - 1];
    call->ldo = net.L[net.n_layers - 1].pout;
    return forward(c);
}
static int act_mask_check(const ActCtx &c, int n_actions) { return mask_words_check(c.mask, c.mask_words, n_actions, "act options", false); }
// the completion words of a call whose last launch does not write them itself: one more (tiny) launch behind it
static int act_done(hipStream_t st, const ActCtx &c, int64_t n) {
    return c.done ? launch_signal_words(st, c.done, (int)rlppo_act_done_words(n), c.done_value) : 0;
}
// what the one-launch step (fused_act.hip) takes from every caller
static FusedActIO fused_act_io(const ActCtx &cx, const float *noise_q, int64_t *actions, float *logp) {
    FusedActIO io;
    io.noise = noise_q;
    io.actions = actions;
    io.logp = logp;
    io.done_words = cx.done;
    io.done_value = cx.done_value;
    io.noise_ctl = cx.noise_ctl;
    io.mask = cx.mask;
    io.mask_words = cx.mask_words;
    return io;
}

extern "C" {

int rlppo_abi_version(void) { return RLPPO_ABI_VERSION; }
const char *rlppo_build_id(void) { return RLPPO_BUILD_ID; }
const char *rlppo_last_error(void) { return g_err; }

int64_t rlppo_padded_width(int64_t d) { return padded_width(d); }
int64_t rlppo_padded_out(int64_t d) { return padded_out(d); }

int64_t rlppo_packed_floats(const int32_t *dims, int32_t n_layers) {
    NetLayout net;
    if (make_layout(dims, n_layers, &net)) return -1;
    return net.packed_floats;
}
int64_t rlppo_flat_floats(const int32_t *dims, int32_t n_layers) {
    NetLayout net;
    if (make_layout(dims, n_layers, &net)) return -1;
    return net.flat_floats;
}

int rlppo_net_pack(void *stream, const int32_t *dims, int32_t n_layers, const float *flat, float *packed) {
    NetLayout net;
    int rc = make_layout(dims, n_layers, &net);
    if (rc) return rc;
    RLPPO_CHECK_ARG(flat && packed, "net_pack: null pointer");
    return launch_pack((hipStream_t)stream, net, flat, packed);
}

int rlppo_pad_rows(void *stream, const void *src, int32_t src_is_f64, int64_t n, int64_t d, int64_t ld_src, float *dst,
                   int64_t ld_dst, int32_t standardize, float mean0, float std0) {
    RLPPO_CHECK_ARG(n >= 0 && d >= 1 && ld_src >= d && ld_dst >= d, "pad_rows: n=%ld d=%ld ld_src=%ld ld_dst=%ld", (long)n,
                    (long)d, (long)ld_src, (long)ld_dst);
    RLPPO_CHECK_ARG(n == 0 || (src && dst), "pad_rows: null pointer");
    return launch_pad_rows((hipStream_t)stream, src, src_is_f64, n, d, ld_src, dst, ld_dst, standardize, mean0, std0);
}

int rlppo_pad_rows_per_feature(void *stream, const void *src, int32_t src_is_f64, int64_t n, int64_t d, int64_t ld_src,
                               float *dst, int64_t ld_dst, const float *mean, const float *stdv) {
    RLPPO_CHECK_ARG(n >= 0 && d >= 1 && ld_src >= d && ld_dst >= d, "pad_rows_per_feature: n=%ld d=%ld ld_src=%ld ld_dst=%ld",
                    (long)n, (long)d, (long)ld_src, (long)ld_dst);
    RLPPO_CHECK_ARG(n == 0 || (src && dst && mean && stdv), "pad_rows_per_feature: null pointer");
    return launch_pad_rows_vec((hipStream_t)stream, src, src_is_f64, n, d, ld_src, dst, ld_dst, mean, stdv);
}

size_t rlppo_forward_workspace_bytes(const int32_t *dims, int32_t n_layers, int64_t n) {
    NetLayout net;
    if (make_layout(dims, n_layers, &net)) return 0;
    return forward_ws_floats(net, n > 0 ? n : 0) * sizeof(float) + 256;
}

int rlppo_mlp_forward(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                      int64_t ld_obs, int64_t n, int32_t out_tanh, float *out, int64_t ld_out, void *workspace,
                      size_t ws_bytes, const rlppo_act_opts *opts) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, false, "rlppo_mlp_forward");
    if (rc) return rc;
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && out && workspace, "mlp_forward: bad argument");
    RLPPO_CHECK_ARG(ld_out == c.net.L[n_layers - 1].pout, "mlp_forward: ld_out=%ld must equal the padded output width %d",
                    (long)ld_out, c.net.L[n_layers - 1].pout);
    rc = act_chain((hipStream_t)stream, &c, packed, obs, ld_obs, n, out_tanh, workspace, ws_bytes, out);
    return rc ? rc : act_done((hipStream_t)stream, c.cx, n);
}

int rlppo_discrete_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                       int64_t ld_obs, int64_t n, const float *noise_q, int64_t *actions, float *logp, float *probs_out,
                       void *workspace, size_t ws_bytes, const rlppo_act_opts *opts) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, false, nullptr);
    if (rc) return rc;
    const NetLayout &net = c.net;
    const ActCtx &cx = c.cx;
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && noise_q && actions && logp && workspace, "discrete_act: bad argument");
    rc = act_mask_check(cx, dims[n_layers]);
    if (rc) return rc;
    // [r3] one launch for the whole step when the network has the form fused_act.hip covers (fp32 inference precision); the
    // layer-by-layer chain below otherwise -- bit-identical results either way
    if (g_fused_act && !cx.bf16 && !cx.hidden_act && fused_act_ok(net) && n <= FUSED_ACT_MAX_ROWS && ld_obs >= net.L[0].pin && ld_obs % 4 == 0 &&
        (reinterpret_cast<uintptr_t>(obs) & 15) == 0) {  // (the kernel stages the padded rows with 16-byte loads)
        FusedActIO io = fused_act_io(cx, noise_q, actions, logp);
        io.rows = obs;
        io.ld_rows = ld_obs;
        io.probs_out = probs_out;
        ++g_call_counts[CNT_FUSED_ACT];
        return launch_discrete_act_fused((hipStream_t)stream, net, packed, io, n);
    }
    ++g_call_counts[CNT_ACT_CHAIN];
    rc = act_chain((hipStream_t)stream, &c, packed, obs, ld_obs, n, 0, workspace, ws_bytes, nullptr);
    if (rc) return rc;
    rc = launch_discrete_sample_logits((hipStream_t)stream, c.o, c.ldo, n, dims[n_layers], noise_q, actions, logp, probs_out, cx.mask, cx.mask_words);
    return rc ? rc : act_done((hipStream_t)stream, cx, n);
}

size_t rlppo_discrete_step_workspace_bytes(const int32_t *dims, int32_t n_layers, int64_t n) {
    NetLayout net;
    if (make_layout(dims, n_layers, &net)) return 0;
    n = n > 0 ? n : 0;
    return forward_ws_floats(net, n) * sizeof(float) + ((size_t)n * net.L[0].pin * sizeof(float) + 255) / 256 * 256 + 512;
}

static int g_window_mode = 0;  // rlppo_dbg_set(41, v), test hook: 1 = answer as a device without a large BAR, 2 = windows without a flush register
int rlppo_host_window_alloc(size_t bytes, void **ptr) {
    RLPPO_CHECK_ARG(ptr && bytes > 0, "host_window_alloc: bad argument");
    *ptr = nullptr;
    int dev = 0, large_bar = 0;
    RLPPO_HIP(hipGetDevice(&dev));
    RLPPO_HIP(hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev));
    if (g_window_mode == 1) large_bar = 0;
    RLPPO_CHECK_ARG(large_bar, "host_window_alloc: device %d does not expose its memory to the host (no large BAR)", dev);
    RLPPO_HIP(hipExtMallocWithFlags(ptr, bytes, hipDeviceMallocFinegrained));
    RLPPO_HIP(hipMemset(*ptr, 0, bytes));
    RLPPO_HIP(hipDeviceSynchronize());
    // the register whose store flushes the device's host data path: rlppo_host_push / _stage_* store to it behind their bytes
    hipDeviceProp_t prop;
    RLPPO_HIP(hipGetDeviceProperties(&prop, dev));
    host_window_register(*ptr, bytes, g_window_mode == 2 ? nullptr : prop.hdpMemFlushCntl);
    return 0;
}
int rlppo_host_window_free(void *ptr) {
    if (ptr) {
        host_window_unregister(ptr);
        RLPPO_HIP(hipFree(ptr));
    }
    return 0;
}

int rlppo_discrete_step_one_launch(const int32_t *dims, int32_t n_layers, int64_t n, const rlppo_act_opts *opts) {
    ActCall c;
    if (act_open(&c, dims, n_layers, opts, true, nullptr)) return -1;
    return g_fused_act && !c.cx.bf16 && !c.cx.hidden_act && fused_act_ok(c.net) && n <= FUSED_ACT_MAX_ROWS ? 1 : 0;
}

int rlppo_discrete_step(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const void *obs, int32_t obs_is_f64,
                        int64_t ld_obs, int64_t n, int32_t standardize, float mean0, float std0, const float *mean_v,
                        const float *std_v, const float *noise_q, int64_t *actions, float *actions_f32, float *logp, float *rows_out,
                        int64_t ld_rows_out, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, true, nullptr);
    if (rc) return rc;
    const NetLayout &net = c.net;
    const ActCtx &cx = c.cx;
    if (n == 0) return 0;
    const int d = net.L[0].in, pin = net.L[0].pin;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && noise_q && actions && logp && workspace, "discrete_step: bad argument");
    RLPPO_CHECK_ARG(ld_obs >= d && standardize >= 0 && standardize <= 2 && (standardize != 2 || (mean_v && std_v)),
                    "discrete_step: ld_obs=%ld standardize=%d", (long)ld_obs, standardize);
    RLPPO_CHECK_ARG(!rows_out || ld_rows_out >= pin, "discrete_step: ld_rows_out=%ld < padded width %d", (long)ld_rows_out, pin);
    rc = act_mask_check(cx, dims[n_layers]);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (g_fused_act && !cx.bf16 && !cx.hidden_act && fused_act_ok(net) && n <= FUSED_ACT_MAX_ROWS) {
        FusedActIO io = fused_act_io(cx, noise_q, actions, logp);
        io.raw = obs;
        io.raw_is_f64 = obs_is_f64;
        io.ld_raw = ld_obs;
        io.standardize = standardize;
        io.mean0 = mean0;
        io.std0 = std0;
        io.mean_v = mean_v;
        io.std_v = std_v;
        io.rows_out = rows_out;
        io.ld_rows_out = ld_rows_out;
        io.actions_f32 = actions_f32;
        ++g_call_counts[CNT_FUSED_ACT];
        return launch_discrete_act_fused(st, net, packed, io, n);
    }
    RLPPO_CHECK_ARG(!cx.noise_ctl, "discrete_step: noise_ctl needs the one-launch kernel (rlppo_discrete_step_one_launch tells)");
    ++g_call_counts[CNT_ACT_CHAIN];
    // the same step launch by launch: pad (+ standardise) into rows_out (or the head of the workspace), forward chain, sample
    float *rows = rows_out;
    int64_t ld_rows = ld_rows_out;
    char *ws = reinterpret_cast<char *>(workspace);
    if (!rows) {
        const size_t need = (size_t)n * pin * sizeof(float);
        RLPPO_CHECK_ARG(ws_bytes >= need + 256, "discrete_step: workspace %zu too small", ws_bytes);
        rows = reinterpret_cast<float *>(ws);
        ld_rows = pin;
        ws += (need + 255) / 256 * 256;
        ws_bytes -= (need + 255) / 256 * 256;
    }
    if (standardize == 2)
        rc = launch_pad_rows_vec(st, obs, obs_is_f64, n, d, ld_obs, rows, ld_rows, mean_v, std_v);
    else
        rc = launch_pad_rows(st, obs, obs_is_f64, n, d, ld_obs, rows, ld_rows, standardize, mean0, std0);
    if (rc) return rc;
    rc = act_chain(st, &c, packed, rows, ld_rows, n, 0, ws, ws_bytes, nullptr);
    if (rc) return rc;
    rc = launch_discrete_sample_logits(st, c.o, c.ldo, n, dims[n_layers], noise_q, actions, logp, nullptr, cx.mask, cx.mask_words);
    if (rc == 0 && actions_f32) rc = launch_i64_to_f32(st, actions, actions_f32, n);
    return rc ? rc : act_done(st, cx, n);
}

int rlppo_discrete_probs(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                         int64_t ld_obs, int64_t n, int32_t clamp_probs, float *probs_out, int64_t ld_probs,
                         int64_t *flat_argmax, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, false, nullptr);
    if (rc) return rc;
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && workspace && (probs_out || flat_argmax), "discrete_probs: bad argument");
    RLPPO_CHECK_ARG(!probs_out || ld_probs >= dims[n_layers], "discrete_probs: ld_probs %lld < n_actions %d", (long long)ld_probs,
                    dims[n_layers]);
    rc = act_mask_check(c.cx, dims[n_layers]);
    if (rc) return rc;
    rc = act_chain((hipStream_t)stream, &c, packed, obs, ld_obs, n, 0, workspace, ws_bytes, nullptr);
    if (rc) return rc;
    rc = launch_discrete_probs((hipStream_t)stream, c.o, c.ldo, n, dims[n_layers], clamp_probs != 0, probs_out, ld_probs, flat_argmax, c.cx.mask,
                               c.cx.mask_words);
    return rc ? rc : act_done((hipStream_t)stream, c.cx, n);
}

int rlppo_categorical_select(void *stream, const float *probs, int64_t ld_p, int64_t n, int32_t n_cat,
                             const float *noise_q, int64_t *actions, float *logp) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && probs && noise_q && actions && logp && n_cat >= 1 && ld_p >= n_cat, "categorical_select: bad argument");
    return launch_categorical_select((hipStream_t)stream, probs, ld_p, n, n_cat, noise_q, actions, logp);
}

int rlppo_gaussian_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                       int64_t ld_obs, int64_t n, const float *noise_eps, float var_m, float var_b, float *actions,
                       float *logp, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, false, "the Gaussian head (rlppo_gaussian_act)");
    if (rc) return rc;
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && noise_eps && actions && logp && workspace, "gaussian_act: bad argument");
    RLPPO_CHECK_ARG(dims[n_layers] % 2 == 0, "gaussian_act: output width %d must be 2k", dims[n_layers]);
    rc = act_chain((hipStream_t)stream, &c, packed, obs, ld_obs, n, 1, workspace, ws_bytes, nullptr);
    if (rc) return rc;
    // (the completion words ride in the sampling kernel: a block of it holds 256 whole rows)
    return launch_gaussian_sample((hipStream_t)stream, c.o, c.ldo, n, dims[n_layers] / 2, noise_eps, var_m, var_b, actions, logp, c.cx.done,
                                  c.cx.done_value);
}

// [diag] the diagonal-Gaussian head: the layer chain WITHOUT tanh, then the sampling kernel, which reads log_std from device memory
// when it runs (a captured call sees the parameter as it is at every replay)
int rlppo_diag_gaussian_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs, int64_t ld_obs,
                            int64_t n, const float *noise_eps, const float *log_std, float *actions, float *logp, void *workspace,
                            size_t ws_bytes, const rlppo_act_opts *opts) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, false, "the diagonal-Gaussian head (rlppo_diag_gaussian_act)");
    if (rc) return rc;
    RLPPO_CHECK_ARG(dims[n_layers] <= RLPPO_DIAG_MAX_K, "diag_gaussian_act: %d action dimensions, RLPPO_DIAG_MAX_K allows 1 .. %d", dims[n_layers],
                    RLPPO_DIAG_MAX_K);
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && noise_eps && log_std && actions && logp && workspace, "diag_gaussian_act: bad argument");
    rc = act_chain((hipStream_t)stream, &c, packed, obs, ld_obs, n, 0, workspace, ws_bytes, nullptr);
    if (rc) return rc;
    // (the completion words ride in the sampling kernel: a block of it holds 256 whole rows)
    return launch_diag_gaussian_sample((hipStream_t)stream, c.o, c.ldo, n, dims[n_layers], noise_eps, log_std, actions, logp, c.cx.done,
                                       c.cx.done_value);
}

int rlppo_multidiscrete_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                            int64_t ld_obs, int64_t n, const float *noise_q, int64_t *actions, float *logp,
                            void *workspace, size_t ws_bytes, const rlppo_act_opts *opts) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, false, "the multi-discrete head (rlppo_multidiscrete_act)");
    if (rc) return rc;
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && noise_q && actions && logp && workspace, "multidiscrete_act: bad argument");
    RLPPO_CHECK_ARG(dims[n_layers] == 21, "multidiscrete_act: output width %d must be 21", dims[n_layers]);
    rc = act_chain((hipStream_t)stream, &c, packed, obs, ld_obs, n, 0, workspace, ws_bytes, nullptr);
    if (rc) return rc;
    return launch_multidiscrete_sample((hipStream_t)stream, c.o, c.ldo, n, noise_q, actions, logp, c.cx.done, c.cx.done_value);
}

// [nvec] the same step for any nvec: the general sampling kernel, always (the fixed one stays behind rlppo_multidiscrete_act).
// [nvec, masked] `mask` (one bit per logit, ceil(sum(nvec) / 32) words per row) is rlppo_multidiscrete_act_nvec_masked's argument:
// a mask in rlppo_act_opts stays refused by both entry points, with the text it always had.
static int multidiscrete_act_nvec(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                                  int64_t ld_obs, int64_t n, const float *noise_q, int64_t *actions, float *logp, void *workspace,
                                  size_t ws_bytes, const rlppo_act_opts *opts, const int32_t *nvec, int32_t n_heads, const char *who,
                                  const char *opts_for, const unsigned *mask, int mask_words) {
    ActCall c;
    int rc = act_open(&c, dims, n_layers, opts, false, opts_for);
    if (rc) return rc;
    MdSpec spec;
    rc = md_spec_make(nvec, n_heads, who, &spec);
    if (rc) return rc;
    RLPPO_CHECK_ARG(dims[n_layers] == spec.S, "%s: output width %d, but nvec sums to %d", who, dims[n_layers], spec.S);
    rc = mask_words_check(mask, mask_words, spec.S, who, true);
    if (rc) return rc;
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && packed && obs && noise_q && actions && logp && workspace, "%s: bad argument", who);
    rc = act_chain((hipStream_t)stream, &c, packed, obs, ld_obs, n, 0, workspace, ws_bytes, nullptr);
    if (rc) return rc;
    ++g_call_counts[CNT_MD_NVEC];
    return launch_multidiscrete_nvec_sample((hipStream_t)stream, c.o, c.ldo, n, noise_q, actions, logp, spec, c.cx.done, c.cx.done_value, mask,
                                            mask_words);
}

int rlppo_multidiscrete_act_nvec(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                                 int64_t ld_obs, int64_t n, const float *noise_q, int64_t *actions, float *logp, void *workspace,
                                 size_t ws_bytes, const rlppo_act_opts *opts, const int32_t *nvec, int32_t n_heads) {
    return multidiscrete_act_nvec(stream, dims, n_layers, packed, obs, ld_obs, n, noise_q, actions, logp, workspace, ws_bytes, opts, nvec, n_heads,
                                  "multidiscrete_act_nvec", "the multi-discrete head (rlppo_multidiscrete_act_nvec)", nullptr, 0);
}

int rlppo_multidiscrete_act_nvec_masked(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs,
                                        int64_t ld_obs, int64_t n, const float *noise_q, int64_t *actions, float *logp, void *workspace,
                                        size_t ws_bytes, const rlppo_act_opts *opts, const int32_t *nvec, int32_t n_heads,
                                        const uint32_t *action_mask, int32_t mask_words) {
    RLPPO_CHECK_ARG(action_mask != nullptr, "multidiscrete_act_nvec_masked: action_mask is NULL (the unmasked step is rlppo_multidiscrete_act_nvec)");
    return multidiscrete_act_nvec(stream, dims, n_layers, packed, obs, ld_obs, n, noise_q, actions, logp, workspace, ws_bytes, opts, nvec, n_heads,
                                  "multidiscrete_act_nvec_masked",
                                  "the multi-discrete head (rlppo_multidiscrete_act_nvec_masked takes its mask as an argument)", action_mask,
                                  mask_words);
}

int64_t rlppo_act_done_words(int64_t n) { return n > 0 ? cdiv(n, 16) : 0; }

size_t rlppo_gae_workspace_bytes(int64_t n) { return gae_workspace_bytes(n) + 256; }

// the three forms of the scan: one check, one launch.  who: the form's name in the error text
static int gae(const char *who, void *stream, const float *rews, const float *dones, const float *truncated, const float *values,
               const float *boot_values, const float *value_scale, int64_t n, double gamma, double lmbda, float return_std,
               float *value_targets, float *advantages, float *returns, void *workspace, size_t ws_bytes) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && rews && dones && truncated && values && value_targets && advantages && returns && workspace,
                    "%s: bad argument", who);
    return launch_gae((hipStream_t)stream, rews, dones, truncated, values, boot_values, n, gamma, lmbda, return_std, value_targets,
                      advantages, returns, workspace, ws_bytes, value_scale);
}
int rlppo_gae(void *stream, const float *rews, const float *dones, const float *truncated, const float *values, int64_t n,
              double gamma, double lmbda, float return_std, float *value_targets, float *advantages, float *returns,
              void *workspace, size_t ws_bytes) {
    return gae("gae", stream, rews, dones, truncated, values, nullptr, nullptr, n, gamma, lmbda, return_std, value_targets, advantages,
               returns, workspace, ws_bytes);
}
int rlppo_gae_boot(void *stream, const float *rews, const float *dones, const float *truncated, const float *values,
                   const float *boot_values, int64_t n, double gamma, double lmbda, float return_std, float *value_targets,
                   float *advantages, float *returns, void *workspace, size_t ws_bytes) {
    return gae("gae_boot", stream, rews, dones, truncated, values, boot_values, nullptr, n, gamma, lmbda, return_std, value_targets,
               advantages, returns, workspace, ws_bytes);
}
// [vnorm] the scan on normalised values; no scale: rlppo_gae_boot (no boot values either: rlppo_gae)
int rlppo_gae_norm(void *stream, const float *rews, const float *dones, const float *truncated, const float *values,
                   const float *boot_values, const float *value_scale, int64_t n, double gamma, double lmbda, float return_std,
                   float *value_targets, float *advantages, float *returns, void *workspace, size_t ws_bytes) {
    return gae(value_scale ? "gae_norm" : "gae_boot", stream, rews, dones, truncated, values, boot_values, value_scale, n, gamma, lmbda,
               return_std, value_targets, advantages, returns, workspace, ws_bytes);
}

// the two forms of the statistic's update: one check.  who: the form's name in the error text
static int value_norm_check(const char *who, const float *targets, int64_t n, double *state, float *scale, void *ws) {
    RLPPO_CHECK_ARG(n >= 1, "%s: n=%ld < 1", who, (long)n);
    RLPPO_CHECK_ARG(targets != nullptr, "%s: targets is NULL", who);
    RLPPO_CHECK_ARG(state != nullptr, "%s: state is NULL", who);
    RLPPO_CHECK_ARG(scale != nullptr, "%s: scale is NULL", who);
    RLPPO_CHECK_ARG(ws != nullptr, "%s: ws is NULL", who);
    RLPPO_CHECK_ARG((uintptr_t)targets % 4 == 0, "%s: targets must be 4-byte aligned", who);
    RLPPO_CHECK_ARG((uintptr_t)state % 8 == 0, "%s: state must be 8-byte aligned", who);
    RLPPO_CHECK_ARG((uintptr_t)scale % 16 == 0, "%s: scale must be 16-byte aligned", who);
    RLPPO_CHECK_ARG((uintptr_t)ws % 8 == 0, "%s: ws must be 8-byte aligned", who);
    return 0;
}
int rlppo_value_norm_update(void *stream, const float *targets, int64_t n, double *state, float *scale, void *ws) {
    if (const int rc = value_norm_check("value_norm_update", targets, n, state, scale, ws)) return rc;
    return launch_value_norm_update((hipStream_t)stream, targets, n, state, scale, ws);
}
// [vnorm] ... with PopArt's weight-preserving step on the critic's last layer; no layer: rlppo_value_norm_update
int rlppo_value_norm_update_popart(void *stream, const float *targets, int64_t n, double *state, float *scale, void *ws, float *w_last,
                                   int64_t n_w, float *b_last) {
    if (!w_last && !b_last) return rlppo_value_norm_update(stream, targets, n, state, scale, ws);
    const char *who = "value_norm_update_popart";
    if (const int rc = value_norm_check(who, targets, n, state, scale, ws)) return rc;
    RLPPO_CHECK_ARG(w_last != nullptr, "%s: w_last is NULL but b_last is not (give both or neither)", who);
    RLPPO_CHECK_ARG(b_last != nullptr, "%s: b_last is NULL but w_last is not (give both or neither)", who);
    RLPPO_CHECK_ARG(n_w >= 1, "%s: n_w=%ld < 1", who, (long)n_w);
    RLPPO_CHECK_ARG((uintptr_t)w_last % 4 == 0, "%s: w_last must be 4-byte aligned", who);
    RLPPO_CHECK_ARG((uintptr_t)b_last % 4 == 0, "%s: b_last must be 4-byte aligned", who);
    return launch_value_norm_update_popart((hipStream_t)stream, targets, n, state, scale, ws, w_last, n_w, b_last);
}

int rlppo_clip_adam(void *stream, float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                    double max_norm, double lr, double beta1, double beta2, double eps, int64_t step, double *gnorm2) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && params && grads && exp_avg && exp_avg_sq && gnorm2 && step >= 1, "clip_adam: bad argument");
    // torch/optim/adam.py (_single_tensor_adam): python-double scalars, cast to fp32 where they meet a tensor
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const float step_size = (float)(lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    return launch_clip_adam((hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, n, (float)max_norm, step_size, bc2_sqrt,
                            (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, gnorm2);
}

// tail[k]: parameters of network k behind its layers' rlppo_flat_floats (rlppo_clip_adam_pack2_tail), 0 = the plain call; lr: the two
// rates in device memory (rlppo_clip_adam_pack2_lr), null = the descriptors' own
static int clip_adam_pack2(void *stream, const rlppo_opt_net *a, const rlppo_opt_net *b, void *sync_ws, const int64_t *tail,
                           const double *const *lr) {
    RLPPO_CHECK_ARG(a && b, "clip_adam_pack2: null descriptor");
    RLPPO_CHECK_ARG(tail[0] >= 0 && tail[1] >= 0, "clip_adam_pack2_tail: tail_floats %ld / %ld < 0", (long)tail[0], (long)tail[1]);
    const rlppo_opt_net *d[2] = {a, b};
    NetLayout nets[2];
    float *p[2], *g[2], *m[2], *v[2], *packed[2];
    double *gn[2];
    int64_t n[2];
    float max_norm[2], step_size[2], bc2_sqrt[2], omb1[2], beta2[2], omb2[2], eps[2];
    const unsigned *skip[2];
    double bc1s[2];
    for (int k = 0; k < 2; ++k) {
        skip[k] = d[k]->skip_word;
        int rc = make_layout(d[k]->dims, d[k]->n_layers, &nets[k]);
        if (rc) return rc;
        RLPPO_CHECK_ARG(d[k]->params && d[k]->grads && d[k]->exp_avg && d[k]->exp_avg_sq && d[k]->packed && d[k]->gnorm2 &&
                            d[k]->step >= 1, "clip_adam_pack2: bad argument (net %d)", k);
        // torch/optim/adam.py (_single_tensor_adam): python-double scalars, cast to fp32 where they meet a tensor
        const double bc1 = 1.0 - pow(d[k]->beta1, (double)d[k]->step);
        const double bc2 = 1.0 - pow(d[k]->beta2, (double)d[k]->step);
        p[k] = d[k]->params; g[k] = d[k]->grads; m[k] = d[k]->exp_avg; v[k] = d[k]->exp_avg_sq; packed[k] = d[k]->packed;
        gn[k] = d[k]->gnorm2;
        bc1s[k] = bc1;  // [lr] a rate in device memory is divided by the same double on the device
        const LayerLayout &last = nets[k].L[nets[k].n_layers - 1];
        n[k] = last.off_flat_b + last.out + tail[k];  // = rlppo_flat_floats (+ the parameter tail)
        max_norm[k] = (float)d[k]->max_norm; step_size[k] = (float)(d[k]->lr / bc1); bc2_sqrt[k] = (float)sqrt(bc2);
        omb1[k] = (float)(1.0 - d[k]->beta1); beta2[k] = (float)d[k]->beta2; omb2[k] = (float)(1.0 - d[k]->beta2);
        eps[k] = (float)d[k]->eps;
    }
    return launch_clip_adam_pack2((hipStream_t)stream, nets, p, g, m, v, packed, gn, n, max_norm, step_size, bc2_sqrt, omb1, beta2,
                                  omb2, eps, sync_ws, skip, tail, lr, bc1s);
}
int rlppo_clip_adam_pack2(void *stream, const rlppo_opt_net *a, const rlppo_opt_net *b, void *sync_ws) {
    const int64_t tail[2] = {0, 0};
    return clip_adam_pack2(stream, a, b, sync_ws, tail, nullptr);
}
int rlppo_clip_adam_pack2_tail(void *stream, const rlppo_opt_net *a, const rlppo_opt_net *b, void *sync_ws, int64_t tail_a, int64_t tail_b) {
    const int64_t tail[2] = {tail_a, tail_b};
    return clip_adam_pack2(stream, a, b, sync_ws, tail, nullptr);
}

int rlppo_clip_adam_pack2_lr(void *stream, const rlppo_opt_net *a, const rlppo_opt_net *b, void *sync_ws, int64_t tail_a, int64_t tail_b,
                             const double *lr_a, const double *lr_b) {
    const int64_t tail[2] = {tail_a, tail_b};
    const double *lr[2] = {lr_a, lr_b};
    RLPPO_CHECK_ARG((((uintptr_t)lr_a | (uintptr_t)lr_b) & 7) == 0, "clip_adam_pack2_lr: a rate must be 8-byte aligned");
    return clip_adam_pack2(stream, a, b, sync_ws, tail, lr);
}

int64_t rlppo_kl_slots_doubles(int64_t mb) { return kl_slots_doubles(mb); }

int rlppo_adv_stats(void *stream, const int64_t *idx, int64_t n, const float *advantages, int64_t ring_base, int64_t ring_cap,
                    float *out, void *ws) {
    RLPPO_CHECK_ARG(n >= 1 && idx && advantages && out && ws, "adv_stats: bad argument");
    int64_t base, cap;
    if (int rc = ring_window("adv_stats", ring_base, ring_cap, &base, &cap)) return rc;
    return launch_adv_stats((hipStream_t)stream, idx, n, advantages, base, cap, out, ws);
}

// what both gates check first.  who: the entry point's name in the texts; need_stop: it writes the stop word
static int kl_gate_check(const rlppo_kl_gate_args *a, const char *who, bool need_stop) {
    RLPPO_CHECK_ARG(a && a->kl_slots && a->n_passes >= 0 && a->slot_stride >= 3 && a->phase >= 0 && a->phase <= 2 && (!need_stop || a->stop_word),
                    "%s: bad argument", who);
    RLPPO_CHECK_ARG(a->phase == 0 || a->exchange, "%s: phases 1 and 2 need the exchange words", who);
    return 0;
}
int rlppo_kl_gate(void *stream, const rlppo_kl_gate_args *a) {
    if (int rc = kl_gate_check(a, "kl_gate", true)) return rc;
    RLPPO_CHECK_ARG(a->phase == 1 || a->host_words, "kl_gate: host_words missing");
    return launch_kl_gate((hipStream_t)stream, *a);
}

int rlppo_kl_gate_lr(void *stream, const rlppo_kl_gate_args *a, const rlppo_lr_adapt_args *l) {
    if (int rc = kl_gate_check(a, "kl_gate_lr", false)) return rc;
    RLPPO_CHECK_ARG(l && l->lr && ((uintptr_t)l->lr & 7) == 0 && l->n_lr >= 1 && l->n_lr <= RLPPO_LR_MAX_RATES, "kl_gate_lr: 1 to %d adjacent rates",
                    RLPPO_LR_MAX_RATES);
    RLPPO_CHECK_ARG(std::isfinite(l->desired_kl) && l->desired_kl > 0 && std::isfinite(l->factor) && l->factor > 1 && std::isfinite(l->lr_min) &&
                        std::isfinite(l->lr_max) && l->lr_min > 0 && l->lr_min <= l->lr_max,
                    "kl_gate_lr: desired_kl=%g factor=%g bounds=[%g, %g]", l->desired_kl, l->factor, l->lr_min, l->lr_max);
    return launch_kl_gate_lr((hipStream_t)stream, *a, *l);
}

int rlppo_learn_report(void *stream, const rlppo_report_args *a) {
    RLPPO_CHECK_ARG(a != nullptr, "learn_report: null args");
    RLPPO_CHECK_ARG(a->n_pol >= 0 && a->n_val >= 0 && (a->n_pol == 0 || (a->pol_before && a->pol_now)) && (a->n_val == 0 || (a->val_before && a->val_now)),
                    "learn_report: parameter vectors missing");
    RLPPO_CHECK_ARG(a->stats && a->out && a->done_word && a->ws, "learn_report: null pointer (stats / out / done_word / ws)");
    RLPPO_CHECK_ARG((reinterpret_cast<uintptr_t>(a->ws) & 15) == 0, "learn_report: ws must be 16-byte aligned");
    return launch_learn_report((hipStream_t)stream, *a);
}

// ------------------------------------------------------------------------------------------ diagnostics
int rlppo_gather_rows(void *stream, const float *src, int64_t ld_src, const int64_t *idx, float *dst, int32_t width, int64_t n) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && src && idx && dst, "gather_rows: null pointer");
    return launch_gather_rows((hipStream_t)stream, src, ld_src, idx, dst, width, n);
}
int rlppo_gather_rows2(void *stream, const rlppo_gather2_args *a) {
    RLPPO_CHECK_ARG(a != nullptr, "gather_rows2: null args");
    if (a->n == 0) return 0;
    RLPPO_CHECK_ARG(a->n > 0 && a->src && a->critic_src && a->idx && a->dst && a->critic_dst, "gather_rows2: null pointer");
    RLPPO_CHECK_ARG((a->old_logp && a->advantages && a->targets && a->actions && a->g_old && a->g_adv && a->g_tgt && a->g_act && a->act_dim > 0) ||
                        !(a->old_logp || a->advantages || a->targets || a->actions || a->g_old || a->g_adv || a->g_tgt || a->g_act || a->zero_n),
                    "gather_rows2: the per-row scalars come together (actions / old_logp / advantages / targets and their four destinations, act_dim > 0) or not at all");
    RLPPO_CHECK_ARG(((reinterpret_cast<uintptr_t>(a->src) | reinterpret_cast<uintptr_t>(a->critic_src) | reinterpret_cast<uintptr_t>(a->dst) |
                      reinterpret_cast<uintptr_t>(a->critic_dst)) & 15) == 0, "gather_rows2: the four matrices must be 16-byte aligned");
    int64_t base, cap;
    if (int rc = ring_window("gather_rows2", a->ring_base, a->ring_cap, &base, &cap)) return rc;
    GatherMeta gm;
    gm.actions = a->actions; gm.old_logp = a->old_logp; gm.adv = a->advantages; gm.targets = a->targets;
    gm.g_old = a->g_old; gm.g_adv = a->g_adv; gm.g_tgt = a->g_tgt; gm.g_act = a->g_act;
    gm.zero_n = a->zero_n;
    gm.act_dim = a->act_dim;
    return launch_gather_rows2((hipStream_t)stream, a->src, a->ld_src, a->dst, a->width, a->critic_src, a->critic_ld_src, a->critic_dst, a->critic_width,
                               a->idx, a->n, base, cap, a->g_old ? &gm : nullptr);
}
int rlppo_welford_increment(void *stream, const float *samples, int64_t ld, int64_t n, int32_t d, void *mean, void *m2,
                            int64_t count, int32_t state_is_f64) {
    if (n == 0) return 0;
    RLPPO_CHECK_ARG(n > 0 && d > 0 && ld >= d && count >= 0 && samples && mean && m2, "welford_increment: bad argument");
    return launch_welford((hipStream_t)stream, samples, ld, n, d, mean, m2, (long long)count, state_is_f64 != 0);
}
int rlppo_welford_merge(void *stream, int32_t d, void *mean, void *m2, int64_t count, const float *other_mean,
                        const float *other_m2, int64_t other_count, int32_t state_is_f64) {
    if (other_count == 0) return 0;
    RLPPO_CHECK_ARG(d > 0 && count >= 0 && other_count > 0 && mean && m2 && other_mean && other_m2, "welford_merge: bad argument");
    return launch_welford_merge((hipStream_t)stream, d, mean, m2, (long long)count, other_mean, other_m2, (long long)other_count,
                                state_is_f64 != 0);
}
// the device-resident vector environment's bookkeeping (csrc/rollout.hip): launches only
static bool dt_ok(int32_t dt) { return dt == RLPPO_DT_F32 || dt == RLPPO_DT_F64 || dt == RLPPO_DT_U8; }
int rlppo_rollout_record(void *stream, const void *rewards, int32_t rewards_dt, const void *dones, int32_t dones_dt, const void *truncated,
                         int32_t truncated_dt, int64_t n_agents, int64_t t, int64_t T, float *rdt, double *ep_sums, void *state,
                         float *patch) {
    RLPPO_CHECK_ARG(rewards && dones && rdt && ep_sums && state, "rollout_record: null pointer (rewards / dones / rdt / ep_sums / state)");
    RLPPO_CHECK_ARG(n_agents > 0 && T > 0 && t >= 0 && t < T, "rollout_record: n_agents=%ld, step %ld of %ld", (long)n_agents, (long)t, (long)T);
    RLPPO_CHECK_ARG(dt_ok(rewards_dt) && rewards_dt != RLPPO_DT_U8 && dt_ok(dones_dt) && (!truncated || dt_ok(truncated_dt)),
                    "rollout_record: dtype codes %d / %d / %d (rewards float32 or float64; flags float32, float64 or one byte)", rewards_dt,
                    dones_dt, truncated_dt);
    RLPPO_CHECK_ARG((reinterpret_cast<uintptr_t>(state) & 7) == 0 && (reinterpret_cast<uintptr_t>(ep_sums) & 7) == 0,
                    "rollout_record: state and ep_sums must be 8-byte aligned");
    return launch_rollout_record((hipStream_t)stream, rewards, rewards_dt, dones, dones_dt, truncated, truncated_dt, n_agents, t, T, rdt, ep_sums,
                                 state, patch);
}
int rlppo_obs_scalars(void *stream, const void *mean, const void *m2, int32_t state_is_f64, int64_t count, int32_t d, int32_t per_feature,
                      float *mean_v, float *std_v) {
    RLPPO_CHECK_ARG(mean && m2 && mean_v && std_v && d > 0 && count >= 0, "obs_scalars: bad argument");
    return launch_obs_scalars((hipStream_t)stream, mean, m2, state_is_f64 != 0, (long long)count, d, per_feature != 0, mean_v, std_v);
}
int rlppo_rollout_to_trajectory_major(void *stream, const float *S, const float *acts, const float *logp, const float *rdt, int64_t n_agents,
                                      int64_t T, int32_t ld, int32_t k, const float *patch, const float *final_rows, float *flat, float *nxt,
                                      float *actions, float *log_probs, float *rewards, float *dones, float *truncated) {
    RLPPO_CHECK_ARG(S && acts && logp && rdt && flat && nxt && actions && log_probs && rewards && dones && truncated,
                    "rollout_to_trajectory_major: null pointer");
    RLPPO_CHECK_ARG(n_agents > 0 && T > 0 && ld > 0 && ld % 4 == 0 && k > 0, "rollout_to_trajectory_major: n_agents=%ld T=%ld ld=%d k=%d",
                    (long)n_agents, (long)T, ld, k);
    RLPPO_CHECK_ARG((patch == nullptr) == (final_rows == nullptr), "rollout_to_trajectory_major: patch and final_rows come together");
    RLPPO_CHECK_ARG(((reinterpret_cast<uintptr_t>(S) | reinterpret_cast<uintptr_t>(flat) | reinterpret_cast<uintptr_t>(nxt) |
                      reinterpret_cast<uintptr_t>(final_rows)) & 15) == 0, "rollout_to_trajectory_major: rows must be 16-byte aligned");
    RLPPO_CHECK_ARG((T + 1) * n_agents * (int64_t)(ld / 4) < (int64_t)256 * 0x7fffffff, "rollout_to_trajectory_major: too many rows for one launch");
    return launch_to_trajectory_major((hipStream_t)stream, S, acts, logp, rdt, n_agents, T, ld, k, patch, final_rows, flat, nxt, actions, log_probs,
                                      rewards, dones, truncated);
}
int64_t rlppo_wb16_elems(const int32_t *dims, int32_t n_layers) {
    NetLayout net;
    if (make_layout(dims, n_layers, &net)) return -1;
    B16Layout bl;
    b16_layout(net, &bl);
    return bl.total;
}
int rlppo_net_pack_bf16(void *stream, const int32_t *dims, int32_t n_layers, const float *flat, float *packed_r, void *wb16) {
    NetLayout net;
    int rc = make_layout(dims, n_layers, &net);
    if (rc) return rc;
    RLPPO_CHECK_ARG(flat && packed_r && wb16, "net_pack_bf16: null pointer");
    return launch_pack_bf16((hipStream_t)stream, net, flat, packed_r, reinterpret_cast<unsigned short *>(wb16));
}
int64_t rlppo_x3_elems(const int32_t *dims, int32_t n_layers) {
    NetLayout net;
    if (make_layout(dims, n_layers, &net)) return -1;
    X3Layout xl;
    x3_layout(net, &xl);
    return xl.total;
}
int rlppo_net_pack_x3(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, void *planes) {
    NetLayout net;
    int rc = make_layout(dims, n_layers, &net);
    if (rc) return rc;
    X3Layout xl;
    x3_layout(net, &xl);
    if (xl.total == 0) return 0;
    RLPPO_CHECK_ARG(packed && planes, "net_pack_x3: null pointer");
    unsigned short *pl = reinterpret_cast<unsigned short *>(planes);
    for (int l = 0; l < net.n_layers; ++l) {
        const LayerLayout &L = net.L[l];
        if (xl.fwd[l] >= 0) {  // W [pout][pin]: the forward's B operand
            rc = launch_pack_split((hipStream_t)stream, packed + L.off_w, L.pin, L.pout, L.pin, pl + xl.fwd[l]);
            if (rc) return rc;
        }
        if (xl.dx[l] >= 0) {  // W^T [pin][pout]: dX's B operand
            rc = launch_pack_split((hipStream_t)stream, packed + L.off_wt, L.pout, L.pin, L.pout, pl + xl.dx[l]);
            if (rc) return rc;
        }
    }
    return 0;
}
static int64_t g_selection_epoch = 0;  // bumped by every call that changes which kernels later launches select
int rlppo_set_update_precision(int32_t mode) {
    RLPPO_CHECK_ARG(mode >= 0 && mode <= 2, "set_update_precision: mode %d (0 = fp32, 1 = bf16 mixed precision, 2 = split-bf16 products)", mode);
    set_update_precision(mode);
    ++g_selection_epoch;
    return 0;
}
int rlppo_get_update_precision(void) { return get_update_precision(); }
int rlppo_set_inference_precision(int32_t mode) {
    RLPPO_CHECK_ARG(mode == 0 || mode == 1, "set_inference_precision: mode %d (0 = fp32, 1 = bf16 operands)", mode);
    set_infer_bf16(mode);
    ++g_selection_epoch;
    return 0;
}
int rlppo_dbg_set(int32_t key, int32_t value) {
    ++g_selection_epoch;
    switch (key) {
        case 1: set_gae_algo(value); return 0;
        case 4: set_two_streams(value); return 0;
        case 19: set_relu_bits(value); return 0;
        case 21: set_gae_spin_limit(value); return 0;
        case 22: set_gae_oversubscribe(value); return 0;
        case 34: set_fused_spin_limit(value); return 0;
        case 35: set_fused_test_hold(value); return 0;
        case 36: set_split_persistent(value); return 0;
        case 23: set_b16_wide_tiles(value); return 0;
        case 24: set_exp_fast_transform(value); return 0;
        case 26: set_fused_gather(value); return 0;
        case 27: g_fused_act = value; return 0;
        case 29: set_paired(value); return 0;
        case 31: set_head_order(value); return 0;
        case 32: set_fold_vhead(value); return 0;
        case 33: set_pair_interleave(value); return 0;
        case 37: set_group_dw(value); return 0;
        case 38: set_tn_group_budget(value); return 0;
        case 40: set_nt_skinny(value); return 0;
        case 41: g_window_mode = value; return 0;
        default: break;
    }
    set_error("dbg_set: unknown key %d", key);
    return RLPPO_ERR_ARG;
}
int64_t rlppo_selection_epoch(void) { return g_selection_epoch; }
const int64_t *rlppo_selection_epoch_ptr(void) { return &g_selection_epoch; }
// a host that REPLAYS a captured call accounts for the runs itself (the launchers count when they are called, not when a graph
// that holds their launches is replayed): ppo/_mlp.py::ActGraph, the masked multi-discrete call
int rlppo_dbg_count(int32_t key, int64_t delta) {
    RLPPO_CHECK_ARG(key == 6, "dbg_count: key %d (only counter 6 is kept by hosts that replay)", key);
    g_call_counts[CNT_MD_NVEC] += delta;
    return 0;
}
int64_t rlppo_dbg_counter(int32_t key) {
    switch (key) {
        case 0: case 1: case 2: case 3: case 4: case 5: case 6: return g_call_counts[key];
        case 7: return rollout_record_count();
        case 8: case 9: case 10: case 11: case 12: case 13: return g_form_launches[key - 8];
        case 15: return g_call_counts[CNT_CRITIC_ROWS_PASS];
        default: return -1;
    }
}
}
