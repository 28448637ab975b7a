// dbg_api.hip -- the single-kernel rlppo_dbg_* entry points (include/rlppo.h, diagnostics): one launcher each, for tests, tools and
// bench.py.  Nothing of the product calls them.
#include "common.hpp"

using namespace rlppo;

extern "C" {
// single-kernel entry points of the split-bf16 products (tests, bench.py)
int rlppo_dbg_pack_x3(void *stream, const float *S, int64_t ld, int32_t R, int32_t C, void *planes) {
    return launch_pack_split((hipStream_t)stream, S, ld, R, C, reinterpret_cast<unsigned short *>(planes));
}
int rlppo_dbg_gemm_nt_x3(void *stream, const float *A, int64_t lda, const void *planes, const float *bias, float *C, int64_t ldc, int64_t M,
                         int32_t N, int32_t K, int32_t mode, void *bits) {
    return launch_gemm_nt_split((hipStream_t)stream, A, lda, reinterpret_cast<const unsigned short *>(planes), bias, C, ldc, M, N, K, mode,
                                reinterpret_cast<unsigned long long *>(bits));
}
size_t rlppo_dbg_gemm_nt_bits_bytes(int64_t M, int32_t N) { return nt_bits_floats(M, N) * sizeof(float); }
int rlppo_dbg_gemm_nt_bits(void *stream, const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C,
                           int64_t ldc, int64_t M, int32_t N, int32_t K, int32_t epilogue, void *bits) {
    const int rc = launch_gemm_nt_bits((hipStream_t)stream, A, lda, B, ldb, bias, C, ldc, M, N, K, epilogue,
                                       reinterpret_cast<unsigned long long *>(bits));
    if (rc == -1) {
        set_error("dbg_gemm_nt_bits: the bitmask form does not apply to this call");
        return RLPPO_ERR_ARG;
    }
    return rc;
}
int rlppo_dbg_gemm_nt(void *stream, const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias,
                      const float *mask_src, int64_t ld_mask, float *C, int64_t ldc, int64_t M, int32_t N, int32_t K,
                      int32_t epilogue) {
    return launch_gemm_nt((hipStream_t)stream, A, lda, B, ldb, bias, mask_src, ld_mask, C, ldc, M, N, K, epilogue);
}
int rlppo_dbg_gemm_nt_b16(void *stream, const void *A, int64_t lda, const void *W, int64_t ldw, const float *bias, float *C,
                          int64_t ldc, void *Cb, int64_t ldcb, int64_t M, int32_t N, int32_t K, int32_t epilogue, int32_t hidden,
                          void *bits) {
    return launch_gemm_nt_b16((hipStream_t)stream, reinterpret_cast<const unsigned short *>(A), lda,
                              reinterpret_cast<const unsigned short *>(W), ldw, bias, C, ldc, reinterpret_cast<unsigned short *>(Cb),
                              ldcb, M, N, K, epilogue, hidden, reinterpret_cast<unsigned long long *>(bits));
}
int rlppo_dbg_gemm_tn_b16(void *stream, const void *dY, int64_t ldy, const void *X, int64_t ldx, float *dW, float *db, int32_t pout,
                          int32_t pin, int32_t out, int32_t in, int64_t M, void *ws, size_t ws_bytes) {
    return launch_gemm_tn_b16((hipStream_t)stream, reinterpret_cast<const unsigned short *>(dY), ldy,
                              reinterpret_cast<const unsigned short *>(X), ldx, dW, db, pout, pin, out, in, M, (float *)ws,
                              ws_bytes / sizeof(float));
}
size_t rlppo_dbg_thin_head_workspace_bytes(int32_t out, int32_t kp, int64_t M) { return thin_dw_ws_floats(out, kp, M) * sizeof(float); }
int rlppo_dbg_thin_head_b16(void *stream, const float *dY, int64_t ldy, int32_t out, const float *W, int64_t ldw, const void *bits,
                            const void *hb, int64_t ldh, void *dxb, float *dW, float *db, int32_t in, int32_t kp, int64_t M, void *ws,
                            size_t ws_bytes) {
    int rc = launch_thin_dx_b16((hipStream_t)stream, dY, ldy, out, W, ldw, reinterpret_cast<const unsigned long long *>(bits),
                                reinterpret_cast<unsigned short *>(dxb), kp, kp, M);
    if (rc) return rc == -1 ? RLPPO_ERR_ARG : rc;
    rc = launch_thin_dw_b16((hipStream_t)stream, dY, ldy, reinterpret_cast<const unsigned short *>(hb), ldh, dW, db, out, in, kp, M,
                            (float *)ws, ws_bytes / sizeof(float));
    return rc == -1 ? RLPPO_ERR_ARG : rc;
}
// the fp32 one-output head's matrix-vector kernels, one at a time (tests)
static bool gemv_dbg_ok(int32_t kp, int64_t M) { return gemv_head_ok(1, kp) && M >= 0; }
int rlppo_dbg_gemv_fwd(void *stream, const float *x, int64_t ldx, const float *w, const float *b, float *y, int64_t ldy, int64_t M,
                       int32_t kp, int32_t pout) {
    RLPPO_CHECK_ARG(gemv_dbg_ok(kp, M) && x && w && b && y && ldx >= kp && ldx % 4 == 0 && pout >= 4 && pout <= 64 && pout % 4 == 0 &&
                        ldy >= pout && ldy % 4 == 0,
                    "dbg_gemv_fwd: kp=%d pout=%d ldx=%ld ldy=%ld", kp, pout, (long)ldx, (long)ldy);
    return launch_gemv_fwd((hipStream_t)stream, x, ldx, w, b, y, ldy, M, kp, pout);
}
int rlppo_dbg_gemv_dx(void *stream, const float *dy, int64_t ldy, const float *w, const float *mask, int64_t ldm, const void *bits,
                      float *dx, int64_t ldc, int32_t kp, int64_t M) {
    RLPPO_CHECK_ARG(gemv_dbg_ok(kp, M) && dy && w && dx && ldy >= 1 && ldc >= kp && ldc % 4 == 0 &&
                        (bits ? kp % 128 == 0 : (mask && ldm >= kp && ldm % 4 == 0)),
                    "dbg_gemv_dx: kp=%d ldy=%ld ldm=%ld ldc=%ld", kp, (long)ldy, (long)ldm, (long)ldc);
    if (bits) return launch_gemv_dx_bits((hipStream_t)stream, dy, ldy, w, reinterpret_cast<const unsigned long long *>(bits), dx, ldc, kp, M);
    return launch_gemv_dx((hipStream_t)stream, dy, ldy, w, mask, ldm, dx, ldc, kp, M, ACT_RELU);
}
size_t rlppo_dbg_gemv_dw_workspace_bytes(int32_t kp, int64_t M) { return gemv_dw_ws_floats(kp, M) * sizeof(float); }
int rlppo_dbg_gemv_dw(void *stream, const float *dy, int64_t ldy, const float *x, int64_t ldx, float *dw, float *db, int32_t in,
                      int32_t kp, int64_t M, void *ws, size_t ws_bytes) {
    RLPPO_CHECK_ARG(gemv_dbg_ok(kp, M) && dy && x && dw && ldy >= 1 && ldx >= kp && ldx % 4 == 0 && in >= 1 && in <= kp,
                    "dbg_gemv_dw: kp=%d in=%d ldy=%ld ldx=%ld", kp, in, (long)ldy, (long)ldx);
    return launch_gemv_dw((hipStream_t)stream, dy, ldy, x, ldx, dw, db, in, kp, M, (float *)ws, ws_bytes / sizeof(float));
}
static int tn_products(const rlppo_tn_product *p, int32_t n, TnProduct *q) {
    RLPPO_CHECK_ARG(p && n > 0 && n <= 2 * RLPPO_MAX_LAYERS, "gemm_tn_group: %d products (1..%d)", n, 2 * RLPPO_MAX_LAYERS);
    for (int i = 0; i < n; ++i) {
        q[i].dY = p[i].dY; q[i].ldy = p[i].ldy; q[i].ny_valid = p[i].ny_valid; q[i].X = p[i].X; q[i].ldx = p[i].ldx;
        q[i].kx_valid = p[i].kx_valid; q[i].dW = p[i].dW; q[i].db = p[i].db; q[i].out = p[i].out; q[i].in = p[i].in;
        q[i].rowtab = p[i].rowtab; q[i].src_rows = p[i].src_rows;
    }
    return 0;
}
size_t rlppo_dbg_gemm_tn_group_workspace_bytes(const rlppo_tn_product *p, int32_t n, int64_t M) {
    if (!p || n <= 0 || n > 2 * RLPPO_MAX_LAYERS) return 0;
    int outs[2 * RLPPO_MAX_LAYERS], ins[2 * RLPPO_MAX_LAYERS];
    for (int i = 0; i < n; ++i) {
        outs[i] = p[i].out;
        ins[i] = p[i].in;
    }
    return tn_group_floats(outs, ins, n, M) * sizeof(float);
}
int rlppo_dbg_gemm_tn_group(void *stream, const rlppo_tn_product *p, int32_t n, int64_t M, void *ws, size_t ws_bytes) {
    TnProduct q[2 * RLPPO_MAX_LAYERS];
    const int rc = tn_products(p, n, q);
    if (rc) return rc;
    return launch_gemm_tn_group((hipStream_t)stream, q, n, M, (float *)ws, ws_bytes / sizeof(float));
}
size_t rlppo_dbg_gemm_tn_workspace_bytes(int32_t out, int32_t in, int64_t M) { return tn_partial_floats(out, in, M) * sizeof(float); }
int rlppo_dbg_gemm_tn(void *stream, const float *dY, int64_t ldy, int32_t ny_valid, const float *X, int64_t ldx,
                      int32_t kx_valid, float *dW, float *db, int32_t out, int32_t in, int64_t M, void *ws, size_t ws_bytes) {
    return launch_gemm_tn((hipStream_t)stream, dY, ldy, ny_valid, X, ldx, kx_valid, dW, db, out, in, M, (float *)ws,
                          ws_bytes / sizeof(float));
}
}
