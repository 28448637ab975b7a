// chain.hip -- the layer chain of one network (chain.hpp: Chain): forward and backward launch sequences of the fp32, split-bf16
// and bf16 precisions, the weight-image layouts they read and their weight-gradient workspace.  Launches only.
#include "chain.hpp"

namespace rlppo {

int max_pout(const NetLayout &net) {
    int m = 0;
    for (int l = 0; l < net.n_layers; ++l) m = net.L[l].pout > m ? net.L[l].pout : m;
    return m;
}

void x3_layout(const NetLayout &net, X3Layout *o) {
    int64_t off = 0;
    const int last = net.n_layers - 1;
    for (int l = 0; l < net.n_layers; ++l) {
        const LayerLayout &L = net.L[l];
        o->fwd[l] = o->dx[l] = -1;
        if (l >= 1 && l < last && nt_split_ok(L.pout, L.pin)) {
            o->fwd[l] = off;
            off += (int64_t)3 * L.pout * L.pin;
        }
        if (l >= 1 && !(l == last && gemv_head_ok(L.out, L.pin)) && nt_split_ok(L.pin, L.pout)) {
            o->dx[l] = off;
            off += (int64_t)3 * L.pin * L.pout;
        }
    }
    o->total = off;
}

void b16_layout(const NetLayout &net, B16Layout *o) {
    int64_t half = 0;
    for (int l = 0; l < net.n_layers; ++l) {
        o->w[l] = half;
        half += (int64_t)net.L[l].pout * net.L[l].pin;
    }
    for (int l = 0; l < net.n_layers; ++l) o->wt[l] = half + o->w[l];
    o->total = 2 * half;
}

static int g_fold_vhead = 1;  // rlppo_dbg_set(32, 0/1): a one-output head inside the last hidden layer's forward epilogue (update passes)
void set_fold_vhead(int v) { g_fold_vhead = v; }
int get_fold_vhead() { return g_fold_vhead; }

size_t tn_layer_floats(const NetLayout &net, int l, int64_t mb, int prec) {
    size_t f = tn_partial_floats(net.L[l].out, net.L[l].in, mb);
    if (net.L[l].out == 1) {  // one-output head: block partials of gemv_dw_kernel (64 rows per block)
        const size_t g = (size_t)cdiv(mb, 64) * (size_t)(net.L[l].pin + 4);  // upper bound: at least 64 rows per block
        if (g > f) f = g;
    }
    if (prec == 1 && l == net.n_layers - 1) {  // narrow head of the bf16 precision: per-lane partials of thin_dw_b16
        const size_t g = thin_dw_ws_floats(net.L[l].out, net.L[l].pin, mb);
        if (g > f) f = g;
    }
    return (f + 3) / 4 * 4;
}
// The launches run one after the other on the net's stream, each followed by its reduction, so one buffer
// of the largest size serves them all.  ([r3] measured: the reductions on streams of their own, one partial buffer per layer --
// a reduction depends on its dW launch only and nothing waits for it before the optimiser step.  The GPU is throughput-bound
// with two chains in flight, so taking them out of the chain saved nothing and their HBM / atomic traffic beside the same
// chain's GEMMs cost 0.6 ms per 10-epoch learn() at one rank and 0.5 ms at the 8-rank share: profiles/r03_ab_update_side_streams.txt.)
size_t tn_ws_floats(const NetLayout &net, int64_t mb, int prec) {
    size_t m = 0;
    for (int l = 0; l < net.n_layers; ++l) {
        const size_t f = tn_layer_floats(net, l, mb, prec);
        m = f > m ? f : m;
    }
    return m;
}

int output_forward(Chain &c, const float *x, int64_t ldx) {
    const LayerLayout &L = c.net->L[c.net->n_layers - 1];
    float *out = c.b.act[c.net->n_layers - 1];
    if (!c.out_tanh && gemv_head_ok(L.out, L.pin))  // one-output head: matrix-vector kernel (gemv.hip)
        return launch_gemv_fwd(c.st, x, ldx, c.w + L.off_w, c.w + L.off_b, out, L.pout, c.n, L.pin, L.pout);
    return launch_gemm_nt(c.st, x, ldx, c.w + L.off_w, L.pin, c.w + L.off_b, nullptr, 0, out, L.pout, c.n, L.pout, L.pin,
                          c.out_tanh ? EPI_BIAS_TANH : EPI_BIAS, c.bf16_operands);
}

int forward(Chain &c) {
    const NetLayout &net = *c.net;
    const int hl = net.n_layers - 1;
    bool any_bits = false;
    for (int l = 0; l < hl; ++l) any_bits |= c.b.bits[l] != nullptr;
    if (c.hidden_act != ACT_RELU && (c.bf16_operands || any_bits || c.may_fold || c.x3 || c.in.rowtab)) {
        set_error("forward: hidden activation %s runs the plain fp32 layer chain only", hidden_act_name(c.hidden_act));
        return RLPPO_ERR_ARG;
    }
    X3Layout xl;
    if (c.x3) x3_layout(net, &xl);
    for (int l = 0; l < net.n_layers; ++l) c.have_bits[l] = false;
    const float *x = c.in.x;
    int64_t ldx = c.in.ld;
    bool fold = c.may_fold && g_fold_vhead && hl >= 1 && !c.out_tanh && !c.bf16_operands && c.b.bits[hl - 1] &&
                gemv_head_ok(net.L[hl].out, net.L[hl].pin) && net.L[hl - 1].pout / 128 <= 2;
    if (c.x3 && hl >= 1 && xl.fwd[hl - 1] >= 0) fold = false;  // (the split forward has no dot-product epilogue: the head keeps its own launch)
    c.head_folded = false;
    for (int l = 0; l < hl; ++l) {
        const LayerLayout &L = net.L[l];
        unsigned long long *bits = c.b.bits[l];
        int rc = -1;
        if (bits && c.x3 && xl.fwd[l] >= 0) {  // [r4] fp32 data, bf16 MFMA pipe, fp32-grade result
            rc = launch_gemm_nt_split(c.st, x, ldx, c.x3 + xl.fwd[l], c.w + L.off_b, c.b.act[l], L.pout, c.n, L.pout, L.pin, 0, bits);
            if (rc == 0) c.have_bits[l] = true;
        } else if (bits && !c.bf16_operands) {
            NtDot dots[2];
            const bool fold_here = fold && l == hl - 1;
            if (fold_here) {
                if (!c.head_prezeroed) RLPPO_HIP(hipMemsetAsync(c.b.act[hl], 0, (size_t)c.n * sizeof(float), c.st));
                dots[0].w = c.w + net.L[hl].off_w;
                dots[0].b = c.w + net.L[hl].off_b;
                dots[0].out = c.b.act[hl];
            }
            rc = launch_gemm_nt_bits(c.st, x, ldx, c.w + L.off_w, L.pin, c.w + L.off_b, c.b.act[l], L.pout, c.n, L.pout, L.pin, EPI_BIAS_RELU,
                                     bits, l == 0 ? c.in.rowtab : nullptr, c.in.src_rows, nullptr, fold_here ? dots : nullptr);
            if (rc == 0) c.have_bits[l] = true;
            if (fold_here) c.head_folded = rc == 0;  // (rc == -1: the layer has no bitmask form; the values stay zero-filled but unused)
        }
        if (l == 0 && c.in.rowtab && rc != 0) {
            if (rc == -1) set_error("forward: the gathered first layer needs the bitmask form");
            return rc == -1 ? RLPPO_ERR_ARG : rc;
        }
        if (rc == -1)
            rc = launch_gemm_nt(c.st, x, ldx, c.w + L.off_w, L.pin, c.w + L.off_b, nullptr, 0, c.b.act[l], L.pout, c.n, L.pout, L.pin,
                                hidden_act_fwd_epi(c.hidden_act), c.bf16_operands);
        if (rc) return rc;
        x = c.b.act[l];
        ldx = L.pout;
    }
    RLPPO_CHECK_ARG(hl > 0 || !c.in.rowtab, "forward: the gathered first layer needs the bitmask form");
    return c.head_folded ? 0 : output_forward(c, x, ldx);
}

// Forward pass of the bf16 UPDATE precision (rlppo_set_update_precision(1)): every product multiplies bf16-rounded operands
// and accumulates in fp32.  in.x / in_b: the layer input as rounded fp32 and as bf16 (same values); b.actb[l] receives the hidden
// output rounded to bf16, b.bits[l] its ReLU bitmask; b.act[l] receives the same values as fp32 only where somebody will read them
// (want: the next layer or its weight gradient takes an fp32 kernel) -- f32_valid[l] reports it; the output layer is
// stored unrounded in fp32.  Layers whose shape gemm_nt_b16_kernel does not cover run the fp32 kernels on the fp32 copies
// (identical products) and are rounded by a separate pass.
static bool b16_next_wants_f32(const NetLayout &net, int l) {  // does the consumer of hidden activation l read it as fp32?
    const int nx = l + 1, last = net.n_layers - 1;
    const LayerLayout &N = net.L[nx];
    if (nx == last) {
        const bool fwd_b16 = gemv_head_ok(N.out, N.pin) || nt_b16_ok(N.pout, N.pin, false);
        return !(fwd_b16 && thin_head_ok(N.out, N.pin));
    }
    return !(nt_b16_ok(N.pout, N.pin, true) && tn_b16_ok(N.pout, N.pin));
}
int forward_b16(Chain &c) {
    const NetLayout &net = *c.net;
    const hipStream_t st = c.st;
    const int64_t n = c.n;
    float *const *acts = c.b.act;
    unsigned short *const *actsb = c.b.actb;
    unsigned long long *const *bits = c.b.bits;
    for (int l = 0; l < net.n_layers; ++l) c.have_bits[l] = c.f32_valid[l] = false;
    B16Layout bl;
    b16_layout(net, &bl);
    const float *x = c.in.x;
    const unsigned short *xb = c.in_b;
    int64_t ldx = c.in.ld;
    bool x_f32 = true;  // the gathered states exist in both forms
    for (int l = 0; l < net.n_layers; ++l) {
        const LayerLayout &L = net.L[l];
        const bool last = l == net.n_layers - 1;
        int rc = 0;
        auto need_x_f32 = [&]() -> int {  // an fp32 kernel is about to read this layer's input
            if (x_f32) return 0;
            x_f32 = c.f32_valid[l - 1] = true;
            return launch_expand_rows(st, actsb[l - 1], acts[l - 1], n * (int64_t)net.L[l - 1].pout);
        };
        if (last) {
            const int epi = c.out_tanh ? EPI_BIAS_TANH : EPI_BIAS;
            if (!c.out_tanh && gemv_head_ok(L.out, L.pin))
                rc = launch_gemv_fwd_b16(st, xb, ldx, c.w + L.off_w, c.w + L.off_b, acts[l], L.pout, n, L.pin, L.pout);
            else if (nt_b16_ok(L.pout, L.pin, false))
                rc = launch_gemm_nt_b16(st, xb, ldx, c.wb16 + bl.w[l], L.pin, c.w + L.off_b, acts[l], L.pout, nullptr, 0, n, L.pout,
                                        L.pin, epi, 0, nullptr);
            else {
                rc = need_x_f32();
                if (rc == 0)
                    rc = launch_gemm_nt(st, x, ldx, c.w + L.off_w, L.pin, c.w + L.off_b, nullptr, 0, acts[l], L.pout, n,
                                        L.pout, L.pin, epi);
            }
            c.f32_valid[l] = true;
        } else if (nt_b16_ok(L.pout, L.pin, true) && bits[l]) {
            const bool want = b16_next_wants_f32(net, l);
            rc = launch_gemm_nt_b16(st, xb, ldx, c.wb16 + bl.w[l], L.pin, c.w + L.off_b, want ? acts[l] : nullptr, L.pout, actsb[l],
                                    L.pout, n, L.pout, L.pin, EPI_BIAS_RELU, 1, bits[l]);
            c.have_bits[l] = rc == 0;
            c.f32_valid[l] = want;
        } else {
            rc = need_x_f32();
            if (rc) return rc;
            rc = -1;
            if (bits[l]) {
                rc = launch_gemm_nt_bits(st, x, ldx, c.w + L.off_w, L.pin, c.w + L.off_b, acts[l], L.pout, n, L.pout, L.pin,
                                         EPI_BIAS_RELU, bits[l]);
                c.have_bits[l] = rc == 0;
            }
            if (rc == -1)
                rc = launch_gemm_nt(st, x, ldx, c.w + L.off_w, L.pin, c.w + L.off_b, nullptr, 0, acts[l], L.pout, n, L.pout,
                                    L.pin, EPI_BIAS_RELU);
            if (rc == 0) rc = launch_round_rows(st, acts[l], actsb[l], n * (int64_t)L.pout);
            c.f32_valid[l] = true;
        }
        if (rc) return rc;
        x = acts[l];
        xb = actsb[l];
        x_f32 = c.f32_valid[l];
        ldx = L.pout;
    }
    return 0;
}

// Layer l's share of a backward pass: b.act[l] = saved output of layer l, b.act[last] holds dL/d(out) on entry; b.dx[l-1] receives
// dL/d(b.act[l-1]) = dY of layer l-1 (one buffer per layer: the dW launches read them later)
int layer_backward(Chain &c, int l, bool need_bits) {
    const NetLayout &net = *c.net;
    const int last = net.n_layers - 1;
    const LayerLayout &L = net.L[l];
    const hipStream_t st = c.st;
    const int64_t mb = c.n;
    float *const *acts = c.b.act, *const *dx = c.b.dx;
    const float *dY = l == last ? acts[last] : dx[l];
    const int64_t ld_hy = c.head_folded ? 1 : L.pout;  // stride of a one-output head's dY (compact when it was folded, forward())
    const RowSource X = l > 0 ? RowSource{acts[l - 1], net.L[l - 1].pout} : c.in;
    const bool gemv = l == last && l > 0 && gemv_head_ok(L.out, L.pin);  // one-output head (gemv.hip)
    const size_t floats = tn_layer_floats(net, l, mb, 0);  // (fp32 / split-bf16 precisions: the bf16 one has backward_b16)
    int rc = 0;
    if (gemv)
        rc = launch_gemv_dw(st, dY, ld_hy, X.x, X.ld, c.grad + L.off_flat_w, c.grad + L.off_flat_b, L.in, L.pin, mb, c.b.tn, floats);
    else if (c.defer)  // [r5] collected: launched with every other product of the pass once the chains have joined
        c.defer->add(L, dY, X, c.grad);
    else
        rc = launch_gemm_tn(st, dY, L.pout, L.pout, X.x, X.ld, L.pin, c.grad + L.off_flat_w, c.grad + L.off_flat_b, L.out, L.in, mb,
                            c.b.tn, floats, X.rowtab, X.src_rows);
    if (rc || l == 0) return rc;
    // dX[mb][pin] = (dY[mb][pout] . W[pout][pin]) masked by relu'(acts[l-1]); B operand = W^T [pin][pout].  The mask is the
    // bitmask the forward left when there is one (no re-read of the activation), else the saved activation itself.
    // [act] tanh / ELU: times f'(acts[l-1]), a function of the saved OUTPUT alone (1 - h^2; h > 0 ? 1 : h + 1) -- the same
    // "by the saved activation" launches with the derivative epilogue; there are no bitmasks (have_bits is all false)
    unsigned long long *bits = c.have_bits[l - 1] ? c.b.bits[l - 1] : nullptr;
    rc = -1;
    if (bits && gemv)
        rc = launch_gemv_dx_bits(st, dY, ld_hy, c.w + L.off_w, bits, dx[l - 1], L.pin, L.pin, mb);
    else if (bits) {
        X3Layout xl;
        if (c.x3) x3_layout(net, &xl);
        if (c.x3 && xl.dx[l] >= 0)  // [r4] split-bf16 dX
            rc = launch_gemm_nt_split(st, dY, L.pout, c.x3 + xl.dx[l], nullptr, dx[l - 1], L.pin, mb, L.pin, L.pout, 1, bits);
        else
            rc = launch_gemm_nt_bits(st, dY, L.pout, c.w + L.off_wt, L.pout, nullptr, dx[l - 1], L.pin, mb, L.pin, L.pout, EPI_MASK, bits);
    }
    if (rc == -1 && need_bits) {
        set_error("paired pass: the output layer's dX needs the bitmask form");
        return RLPPO_ERR_ARG;
    }
    if (rc == -1 && gemv) rc = launch_gemv_dx(st, dY, ld_hy, c.w + L.off_w, acts[l - 1], L.pin, dx[l - 1], L.pin, L.pin, mb, c.hidden_act);
    else if (rc == -1)
        rc = launch_gemm_nt(st, dY, L.pout, c.w + L.off_wt, L.pout, nullptr, acts[l - 1], L.pin, dx[l - 1], L.pin, mb, L.pin, L.pout,
                            hidden_act_dx_epi(c.hidden_act));
    return rc;
}

int backward(Chain &c) {
    for (int l = c.net->n_layers - 1; l >= 0; --l)
        if (int rc = layer_backward(c, l, false)) return rc;
    return 0;
}

// Backward of one net in the bf16 update precision: the hidden activations are bf16 tensors,
// so the gradient with respect to each of them is rounded to bf16 (dxb[l], already masked by relu'), and every product
// multiplies bf16 values with fp32 accumulation: dW_l = dxb[l]^T . actsb[l-1] (gemm_tn_b16_kernel), dX = dxb[l] . r(W_l)
// (gemm_nt_b16_kernel, B16_DX).  dW / db accumulate unrounded into the fp32 gradient arena.  The output layer's gradient comes
// from the loss kernel in fp32: narrow heads stream it through thin_dw_b16 / thin_dx_b16 (gemv.hip).  Shapes those kernels do
// not cover take the fp32 kernels on fp32 copies of the same bf16 values (expanded on demand), followed by the same rounding:
// identical mathematics.
int backward_b16(Chain &c) {
    const NetLayout &net = *c.net;
    const hipStream_t st = c.st;
    const int64_t mb = c.n;
    float *const *acts = c.b.act, *const *dx = c.b.dx, *grad = c.grad, *tn_ws = c.b.tn;
    unsigned short *const *actsb = c.b.actb, *const *dxb = c.b.dxb;
    unsigned long long *const *bits = c.b.bits;
    const size_t tn_floats = tn_ws_floats(net, mb, 1);
    const int last = net.n_layers - 1;
    B16Layout bl;
    b16_layout(net, &bl);
    bool dx_f32[RLPPO_MAX_LAYERS] = {};  // dx[l] holds the fp32 copy of dxb[l]
    int rc = 0;
    auto act_f32 = [&](int l) -> int {  // an fp32 kernel is about to read hidden activation l
        if (l < 0 || c.f32_valid[l]) return 0;
        c.f32_valid[l] = true;
        return launch_expand_rows(st, actsb[l], acts[l], mb * (int64_t)net.L[l].pout);
    };
    auto grad_f32 = [&](int l) -> int {  // ... or the gradient of hidden activation l
        if (dx_f32[l]) return 0;
        dx_f32[l] = true;
        return launch_expand_rows(st, dxb[l], dx[l], mb * (int64_t)net.L[l].pout);
    };
    for (int l = last; l >= 0; --l) {
        const LayerLayout &L = net.L[l];
        const float *X = l > 0 ? acts[l - 1] : c.in.x;
        const unsigned short *Xb = l > 0 ? actsb[l - 1] : c.in_b;
        const int64_t ldx = l > 0 ? net.L[l - 1].pout : c.in.ld;
        const bool gemv = l == last && l > 0 && gemv_head_ok(L.out, L.pin);
        // ---- dW, db
        if (l == last) {
            rc = l > 0 ? launch_thin_dw_b16(st, acts[last], L.pout, Xb, ldx, grad + L.off_flat_w, grad + L.off_flat_b, L.out, L.in,
                                            L.pin, mb, tn_ws, tn_floats)
                       : -1;
            if (rc == -1) {
                rc = act_f32(l - 1);
                if (rc) return rc;
                if (gemv)
                    rc = launch_gemv_dw(st, acts[last], L.pout, X, ldx, grad + L.off_flat_w, grad + L.off_flat_b, L.in, L.pin, mb,
                                        tn_ws, tn_floats);
                else
                    rc = launch_gemm_tn(st, acts[last], L.pout, L.pout, X, ldx, L.pin, grad + L.off_flat_w, grad + L.off_flat_b,
                                        L.out, L.in, mb, tn_ws, tn_floats);
            }
        } else if (tn_b16_ok(L.pout, L.pin) && ldx % 8 == 0) {
            rc = launch_gemm_tn_b16(st, dxb[l], L.pout, Xb, ldx, grad + L.off_flat_w, grad + L.off_flat_b, L.pout, L.pin, L.out, L.in,
                                    mb, tn_ws, tn_floats);
        } else {
            rc = grad_f32(l);
            if (rc == 0) rc = act_f32(l - 1);
            if (rc) return rc;
            rc = launch_gemm_tn(st, dx[l], L.pout, L.pout, X, ldx, L.pin, grad + L.off_flat_w, grad + L.off_flat_b, L.out, L.in, mb,
                                tn_ws, tn_floats);
        }
        if (rc) return rc;
        if (l == 0) break;
        // ---- dX of layer l = the (rounded, masked) gradient of hidden activation l - 1
        if (l < last && c.have_bits[l - 1] && nt_b16_ok(L.pin, L.pout, true)) {
            rc = launch_gemm_nt_b16(st, dxb[l], L.pout, c.wb16 + bl.wt[l], L.pout, nullptr, nullptr, 0, dxb[l - 1], L.pin, mb,
                                    L.pin, L.pout, EPI_MASK, 2, bits[l - 1]);
            if (rc) return rc;
            continue;
        }
        if (l == last && c.have_bits[l - 1]) {
            rc = launch_thin_dx_b16(st, acts[last], L.pout, L.out, c.w + L.off_w, L.pin, bits[l - 1], dxb[l - 1], L.pin, L.pin, mb);
            if (rc == 0) continue;
            if (rc != -1) return rc;
        }
        const float *dY = acts[last];
        if (l < last) {
            rc = grad_f32(l);
            if (rc) return rc;
            dY = dx[l];
        }
        rc = -1;
        if (gemv) {
            if (c.have_bits[l - 1]) rc = launch_gemv_dx_bits(st, dY, L.pout, c.w + L.off_w, bits[l - 1], dx[l - 1], L.pin, L.pin, mb);
            if (rc == -1) {
                rc = act_f32(l - 1);
                if (rc) return rc;
                rc = launch_gemv_dx(st, dY, L.pout, c.w + L.off_w, acts[l - 1], L.pin, dx[l - 1], L.pin, L.pin, mb);
            }
        } else {
            if (c.have_bits[l - 1])
                rc = launch_gemm_nt_bits(st, dY, L.pout, c.w + L.off_wt, L.pout, nullptr, dx[l - 1], L.pin, mb, L.pin, L.pout,
                                         EPI_MASK, bits[l - 1]);
            if (rc == -1) {
                rc = act_f32(l - 1);
                if (rc) return rc;
                rc = launch_gemm_nt(st, dY, L.pout, c.w + L.off_wt, L.pout, nullptr, acts[l - 1], L.pin, dx[l - 1], L.pin, mb,
                                    L.pin, L.pout, EPI_MASK);
            }
        }
        if (rc) return rc;
        rc = launch_round_rows(st, dx[l - 1], dxb[l - 1], mb * (int64_t)L.pin);  // the gradient of a bf16 activation is bf16
        if (rc) return rc;
        dx_f32[l - 1] = true;
    }
    return rc;
}

}  // namespace rlppo
