// chain.hpp -- one network's layer chain (chain.hip) as the rollout entry points (api.hip) and the PPO pass (update.hip) see it.
#pragma once
#include "common.hpp"

namespace rlppo {

int max_pout(const NetLayout &net);

// [r4] The weight image of the split-bf16 update precision (rlppo_set_update_precision(2), csrc/gemm_split.hip): for every hidden
// layer l >= 1 whose shape the split kernels cover, the three bf16 planes of W_l in stage-major order (forward), and for every
// layer l >= 1 whose dX they cover (the output layer included, unless it is a one-output head) the planes of W_l^T.  Offsets in
// bf16 elements; -1 = that product keeps its fp32 kernel.
struct X3Layout {
    int64_t fwd[RLPPO_MAX_LAYERS], dx[RLPPO_MAX_LAYERS], total;
};
void x3_layout(const NetLayout &net, X3Layout *o);
// The weight image of the bf16 update precision (rlppo_net_pack_bf16): every layer's W block, then every layer's W^T block.
// Offsets in bf16 elements.
struct B16Layout {
    int64_t w[RLPPO_MAX_LAYERS], wt[RLPPO_MAX_LAYERS], total;
};
void b16_layout(const NetLayout &net, B16Layout *o);

// Where a first layer finds its rows: a row-major matrix x [n][ld], or -- rowtab != nullptr, the fused gather [r3] -- the
// experience buffer's state matrix x (src_rows rows), row r of the pass being x[rowtab[r]].
struct RowSource {
    const float *x;
    int64_t ld;
    const unsigned *rowtab = nullptr;
    int64_t src_rows = 0;
};

struct DwList {
    TnProduct p[2 * RLPPO_MAX_LAYERS];
    int n = 0;
    void add(const LayerLayout &L, const float *dY, const RowSource &X, float *grad) {  // dW / db of layer L = dY^T . X into grad
        TnProduct &q = p[n++];
        q.dY = dY; q.ldy = L.pout; q.ny_valid = L.pout; q.X = X.x; q.ldx = X.ld; q.kx_valid = L.pin;
        q.dW = grad + L.off_flat_w; q.db = grad + L.off_flat_b; q.out = L.out; q.in = L.in;
        q.rowtab = X.rowtab; q.src_rows = X.src_rows;
    }
};

// The per-layer buffers of one network (update passes: a region each of the pass's workspace, update.hip: plan_workspace):
struct NetWs {
    float *act[RLPPO_MAX_LAYERS] = {};                // the saved output of every layer, [mb][pout]
    float *dx[RLPPO_MAX_LAYERS] = {};                 // dL/d(act[l]) of every hidden layer, [mb][widest pout of both nets]
    unsigned long long *bits[RLPPO_MAX_LAYERS] = {};  // the ReLU bitmask of every hidden layer that has that form (1/32 of act[l])
    unsigned short *actb[RLPPO_MAX_LAYERS] = {};      // bf16 update precision: the hidden activations ...
    unsigned short *dxb[RLPPO_MAX_LAYERS] = {};       // ... and their gradients as bf16
    float *tn = nullptr;                              // the partial dW tiles of the net's chain
};

// What one network contributes to one pass or one inference call.  b.act[l] receives the output of layer l ([n][pout_l]): for
// inference two ping-pong buffers, for training one buffer per layer (they are the saved activations of the backward pass).
// Training only: b.bits[l] (may be null) receives the ReLU bitmask of hidden layer l and have_bits[l] says whether it was written
// (csrc/gemm.hip, launch_gemm_nt_bits); backward() then masks dX with it instead of re-reading b.act[l].
// in.rowtab != nullptr: the first layer fetches its rows through the table (nt_gather_ok must hold for it).
// [act] hidden_act (HiddenAct): the activation of every hidden layer.  tanh / ELU have the plain form only -- the callers give them no
// bitmasks, no folded head, no row table, no bf16 operands and no split planes (all of those carry ReLU by construction).
struct Chain {
    hipStream_t st = nullptr;
    const NetLayout *net = nullptr;
    const float *w = nullptr;  // the packed weights the products read (bf16 update precision: their rounded image)
    RowSource in = {nullptr, 0};
    const unsigned short *in_b = nullptr;  // bf16 update precision: the rows of `in` as bf16
    int64_t n = 0;
    int out_tanh = 0, hidden_act = ACT_RELU;
    int bf16_operands = 0;  // inference precision: fp32 data, bf16-rounded operands
    NetWs b;
    float *grad = nullptr;     // the gradient arena, and ...
    DwList *defer = nullptr;   // ... [r5] where its GEMM-shaped weight gradients are collected (null: launched in the chain)
    const unsigned short *wb16 = nullptr, *x3 = nullptr;  // the bf16 / [r4] split-bf16 weight image
    // update passes: a one-output head may be computed in the epilogue of the hidden layer that feeds it (NtDot, csrc/gemm.hip) --
    // b.act[last] then holds the outputs COMPACT ([n], stride 1) and head_folded says so; head_prezeroed: somebody zeroed them already
    bool may_fold = false, head_prezeroed = false;
    // what a forward leaves for its backward (f32_valid: bf16 precision, which activations also exist as fp32)
    bool have_bits[RLPPO_MAX_LAYERS] = {}, f32_valid[RLPPO_MAX_LAYERS] = {}, head_folded = false;
};

int forward(Chain &c), backward(Chain &c), forward_b16(Chain &c), backward_b16(Chain &c);
// the output layer's forward on x [n][ldx] / layer l's dW, db and dX (need_bits: no bitmask form for the dX is an error, not a
// fallback to the saved activation -- the paired pass)
int output_forward(Chain &c, const float *x, int64_t ldx);
int layer_backward(Chain &c, int l, bool need_bits);

size_t tn_layer_floats(const NetLayout &net, int l, int64_t mb, int prec);  // partial-tile workspace of one weight-gradient launch of a net
size_t tn_ws_floats(const NetLayout &net, int64_t mb, int prec);            // ... of a net's chain
void set_fold_vhead(int v);
int get_fold_vhead();

}  // namespace rlppo
