// fused_act.hip -- the rollout step of the discrete policy in ONE launch (reference:
// rlgym_ppo/ppo/discrete_policy.py:35-62: MLP -> softmax -> clamp -> multinomial (= argmax(p / q)) -> log p).
//
// At rollout sizes (8 ... 4096 observations per call) the layer-by-layer chain of rlppo_discrete_act is latency, not work:
// 4 GEMM launches of 64 workgroups each + the sampling kernel take 76 us for 1.5 GFLOP at 4096 rows
// (tools/rollout_breakdown.py).  Here a workgroup of 4 or 8 waves owns 16 observation rows and carries them through every layer:
//   * activations never leave the CU: a layer's output is written into LDS in exactly the K-step-major, swizzled image the
//     next layer's MFMA fragments are read from (the A-tile image of gemm_nt_dma_kernel);
//   * a wave computes its own share (1/4 or 1/8) of a layer's outputs, so the weights it needs are its own: every wave streams ITS rows of
//     W (packed copy, 0.73 MB for the 256x3 policy: L2-resident) through a private ring of 4 LDS tiles by LDS-DMA, three K-steps
//     ahead, ACROSS layer boundaries (weights do not depend on activations) and waits with counted vmcnt -- no workgroup barrier
//     in the K loop, one per layer for the activations;
//   * the head's logits go to LDS and the waves sample 16 / NW rows each with the code of discrete_sample_kernel.
// [ABI 8] MASKED instantiations: the sampling stage reads the (<= 4) mask words of its rows -- requested with the noise, before the
// layers -- and treats invalid actions as the padded columns c >= A (heads.hip).  With a.noise_ctl only the noise is late: the host
// knows the mask before it launches and stages the words with the observations; both late-noise fetch sites are those of the
// unmasked form, and rows at and beyond the live-row word (stale mask words of a replayed graph) store nothing.
// Arithmetic is that of the chain, operation for operation (accumulators start from the bias, k in tiles of 16 through the same
// v_mfma_f32_16x16x4_f32 sequence, relu as v_med3, the same softmax / division / arg-max order): logits, actions and
// log-probabilities are BIT-identical to the layer-by-layer path (tests/test_gpu_kernels.py).
#include "gemm_detail.hpp"

namespace rlppo {

namespace {
constexpr int FA_ROWS = 16;      // observation rows per workgroup (the MFMA's 16 columns)
constexpr int FA_STAGES = 4;     // weight tiles per wave in flight / being read
constexpr int FA_MAX_LAYERS = 6;
constexpr float FA_PROB_MIN = 1e-11f;
constexpr unsigned FA_OOR = 0x80000000u;  // a scalar offset no descriptor's range check passes
constexpr int FA_QLD = 128;               // floats per row of the late-noise buffer (the kernel's limit of 128 actions)
constexpr int FA_QFLOATS = FA_ROWS * FA_QLD + FA_ROWS;
}  // namespace

struct FusedActArgs {
    const float *rows;       // [n][ld_rows] zero-padded observation rows, or nullptr: `raw` below
    unsigned ld_rows;        // floats
    // raw observations (what the environment hands over: rlppo_pad_rows fused in): [n][ld_raw] fp32 or fp64, d features,
    // optionally standardised like batched_agent_manager.py:313-315 -- clip((x - mean) / std, -5, 5) with the reference's scalars
    // of feature 0 (mode 1) or per-feature vectors (mode 2); the padded rows can be written out for the rollout storage
    const void *raw;
    int raw_is_f64, d, standardize;
    int64_t ld_raw;
    float mean0, std0;
    const float *mean_v, *std_v;
    float *rows_out;         // optional [n][ld_rows_out]
    int64_t ld_rows_out;
    float *actions_f32;      // optional [n]: the action index as float (the experience buffer's encoding, experience_buffer.py:72)
    int64_t n;
    const float *packed;     // rlppo_net_pack image
    int n_layers;
    int k[FA_MAX_LAYERS];          // padded contraction width of layer l
    int nblk[FA_MAX_LAYERS];       // 16-wide output blocks of layer l (H / 16 for hidden layers, padded head width / 16 for the last)
    int64_t off_w[FA_MAX_LAYERS], off_b[FA_MAX_LAYERS];  // float offsets into packed
    int A;                   // actions
    const float *noise;      // [n][A] Exp(1)
    int64_t *actions;
    float *logp;
    float *probs_out;        // optional [n][A]
    unsigned *done_words;    // optional (host-visible): done_words[blockIdx.x] <- done_value when this workgroup's outputs are visible
    unsigned done_value;
    // [r5] noise that arrives WHILE the kernel runs (rlppo_act_opts.noise_ctl): {sequence of this call, rows that are sampled,
    // sequence of the noise that is complete in `noise`, 2 statistics words} in memory the host writes directly
    unsigned *noise_ctl;
    const unsigned *mask;    // [ABI 8] MASKED instantiations: [n][mask_words] action-mask words (bit c % 32 of word c / 32 = action c valid)
    int mask_words;
};

// 20 ms of the 100 MHz wall clock (100-1000 x what the host needs for the draw): a host that is held up between launch and publish --
// worst of all by something that itself waits for the GPU -- gets the kernel out of its way soon and launches again (ActGraph.run)
constexpr long long FA_NOISE_WAIT_TICKS = 2000000LL;
constexpr unsigned FA_DONE_FAILED = 0x80000000u;         // or-ed into the completion word by a workgroup that gave up

// [r5] Lane exchange of the sampling stage's butterflies (offsets 32, 16, 8, 4, 2, 1 in that order).  Offsets 32 and 16 cross the
// 16-lane rows: ds_bpermute (a ~100-cycle trip through the LDS crossbar).  From offset 8 down the partner sits in the lane's own row
// and a DPP move delivers it: row_ror:8 IS lane ^ 8; row_ror:4 delivers lane ^ 4 or (lane ^ 4) ^ 8 -- the same value, because the
// offset-8 step has just made lanes l and l ^ 8 equal (sum, max and the arg-max triple are all computed identically by both
// partners of a step); quad_perm delivers lane ^ 2 and lane ^ 1 exactly.  Same values as __shfl_xor, so the same bits out.
template <int O>
__device__ __forceinline__ int fa_xor_i(int v) {
    if (O >= 16) return __shfl_xor(v, O);
    if (O == 8) return __builtin_amdgcn_update_dpp(v, v, 0x128, 0xF, 0xF, false);  // row_ror:8
    if (O == 4) return __builtin_amdgcn_update_dpp(v, v, 0x124, 0xF, 0xF, false);  // row_ror:4
    if (O == 2) return __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false);   // quad_perm:[2,3,0,1]
    return __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false);               // quad_perm:[1,0,3,2]
}
template <int O>
__device__ __forceinline__ float fa_xor_f(float v) { return __int_as_float(fa_xor_i<O>(__float_as_int(v))); }

// NW waves; JH: output blocks a wave owns in a hidden layer (H = 16 JH NW); the head's blocks are dealt ceil(nblk / NW) per wave.
// H = 256 runs 8 waves x 2 blocks: with one wave per SIMD (4 x 4) a K-step was LDS-DMA issue (4 pieces, ~100 cycles each) + fragment
// reads + 16 MFMAs one after the other, ~1350 cycles for 512 cycles of MFMA (36 us per 4096-row step); two waves per SIMD take
// turns on the MFMA pipe.
template <int JH, int NW, bool MASKED = false>
__global__ __launch_bounds__(64 * NW, 1) void discrete_act_fused_kernel(FusedActArgs a) {
    constexpr int H = 16 * JH * NW, NT = 64 * NW, RPWV = FA_ROWS / NW;  // rows each wave samples
    constexpr int TILE = JH * 16 * 16;  // floats of one wave's weight tile (JH*16 rows x 16 k)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *act0 = lds;                        // [H/16 k-steps][16 rows][16] swizzled (also holds the staged input rows)
    float *act1 = lds + H * FA_ROWS;
    float *wring = lds + 2 * H * FA_ROWS;     // [NW waves][FA_STAGES][TILE]
    float *biasl = wring + NW * FA_STAGES * TILE;  // [FA_MAX_LAYERS][H]: the biases, so that no register-destination load sits in the weight stream's vmcnt window
    float *qbuf = biasl + FA_MAX_LAYERS * H;       // [r5] [FA_ROWS][FA_QLD] late noise fetched by the waves that have no block of the head layer
    int *qok = reinterpret_cast<int *>(qbuf + FA_ROWS * FA_QLD);  // [FA_ROWS] 1: the row's noise is in qbuf
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = (int)blockIdx.x;
    const int64_t row0 = (int64_t)tile * FA_ROWS;
    // (time stamps of the call's last workgroup in the statistics words of late noise: tools/get_action_modes.py)
#define FA_TS(k) do { if (a.noise_ctl && tid == 0 && tile == (int)gridDim.x - 1) a.noise_ctl[8 + (k)] = (unsigned)wall_clock64(); } while (0)
    FA_TS(0);
    const int last = a.n_layers - 1;
    float *const wr = wring + wave_u * FA_STAGES * TILE;

    // ---- weight stream of this wave: step t of the whole network = (layer pl, k-tile pkt); every step that exists issues exactly
    // JH pieces (pieces whose rows this wave does not own in that layer -- the head's surplus -- fall outside the descriptor: they
    // move no data but keep the vmcnt arithmetic uniform)
    const int lr = lane >> 2, pch = lane & 3;
    const int lch = pch ^ ((0 - (lr >> 2)) & 3);
    // [r3] every layer's step count is padded to a multiple of FA_STAGES (the padding steps move no data: an offset that fails the
    // descriptor's range check; the consumer skips their products), so that a step's ring slot is its position in a group of four --
    // a compile-time constant in the unrolled K loop below
    int pl = 0, pkt = 0, issued = 0, prk = a.k[0] / 16, pnk = (prk + FA_STAGES - 1) & ~(FA_STAGES - 1);
    auto layer_rsrc = [&](int l) {
        const int own = l == last ? (a.nblk[l] + NW - 1) / NW : JH;      // blocks per wave in this layer
        int rows = a.nblk[l] * 16 - wave_u * own * 16;                     // rows of W this wave streams
        rows = rows < 0 ? 0 : (rows > own * 16 ? own * 16 : rows);
        return make_rsrc(a.packed + a.off_w[l] + (int64_t)wave_u * own * 16 * a.k[l], (unsigned)rows * (unsigned)a.k[l] * 4u);
    };
    __amdgpu_buffer_rsrc_t w_rs = layer_rsrc(0);
    unsigned w_off = (unsigned)lr * (unsigned)a.k[0] * 4u + lch * 16;
    unsigned w_row16 = 16u * (unsigned)a.k[0] * 4u;
    auto issue_next = [&]() {
        if (pl > last) return;  // past the network's end (the waits below count what is really in flight)
        float *dst = wr + (issued % FA_STAGES) * TILE;
        const unsigned kb = pkt < prk ? (unsigned)pkt * 64u : FA_OOR;
#pragma unroll
        for (int i = 0; i < JH; ++i) __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, dst + i * 256, 16, w_off, kb + i * w_row16, 0, 0);
        ++issued;
        if (++pkt == pnk) {
            pkt = 0;
            ++pl;
            if (pl <= last) {
                prk = a.k[pl] / 16;
                pnk = (prk + FA_STAGES - 1) & ~(FA_STAGES - 1);
                w_rs = layer_rsrc(pl);
                w_off = (unsigned)lr * (unsigned)a.k[pl] * 4u + lch * 16;
                w_row16 = 16u * (unsigned)a.k[pl] * 4u;
            }
        }
    };
#pragma unroll
    for (int s = 0; s < FA_STAGES - 1; ++s) issue_next();

    // the biases: one element per thread and layer (16 nblk <= H <= NT), all layers' requests in flight together -- and together
    // with the observation requests below ([r5]: a request + LDS store per layer was four round trips one after the other)
    float bias_v[FA_MAX_LAYERS];
#pragma unroll
    for (int l = 0; l < FA_MAX_LAYERS; ++l) bias_v[l] = l <= last && tid < a.nblk[l] * 16 ? a.packed[a.off_b[l] + tid] : 0.f;
    // ---- the Exp(1) noise of this wave's rows: requested now, used after the last layer
    // [r5] with noise_ctl the host writes the noise AFTER it has launched (the draw hides behind the launch latency and the layers)
    // and then control word 2.  The waves that have no block of the head layer look at that word when the head layer starts and
    // bring the noise of all 16 rows into LDS while the others multiply; if the host was not done by then, every wave waits for the
    // word after the last layer and reads its own rows
    float qn[RPWV][2];
    unsigned want = 0, live_raw = 0;
    if (a.noise_ctl) {  // (used from the head layer on: nobody waits for these two loads here)
        want = __hip_atomic_load(a.noise_ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        live_raw = __hip_atomic_load(a.noise_ctl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int rr = 0; rr < RPWV; ++rr)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t row = row0 + wave * RPWV + rr;
            const int c = lane + 64 * e;
            qn[rr][e] = (!a.noise_ctl && row < a.n && c < a.A) ? a.noise[row * a.A + c] : 1.f;
        }
    // [ABI 8] the mask word of each of this lane's two elements (c = lane + 64 e sits in word (lane >> 5) + 2 e, bit lane & 31)
    unsigned mw[RPWV][2];
    if (MASKED) {
#pragma unroll
        for (int rr = 0; rr < RPWV; ++rr)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int64_t row = row0 + wave * RPWV + rr;
                mw[rr][e] = (row < a.n && lane + 64 * e < a.A) ? a.mask[row * a.mask_words + (lane >> 5) + 2 * e] : 0u;
            }
    }
    // ---- stage the 16 observation rows into act0 (K-step-major image), zero rows past n
    if (a.rows) {
        const int cpr = a.k[0] / 4;  // 16-byte chunks per row
        for (int c = tid; c < FA_ROWS * cpr; c += NT) {
            const int r = c / cpr, ch = c - r * cpr;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (row0 + r < a.n) v = *reinterpret_cast<const f32x4 *>(a.rows + (row0 + r) * (int64_t)a.ld_rows + ch * 4);
            *reinterpret_cast<f32x4 *>(&act0[(ch >> 2) * 256 + dswz<16>(r, ch & 3)]) = v;
        }
    } else {  // pad_rows_kernel / pad_rows_vec_kernel, element for element
        // [r5] every request of a thread is in flight before the first is used: the observations of a small call sit in memory the
        // HOST writes (pinned, or device memory it writes through the PCIe aperture), where a round trip is microseconds -- one per
        // loop iteration was 11 us of a 35 us kernel at 8 rows
        const int k0 = a.k[0];
        constexpr int SE = FA_ROWS * H / NT;  // elements per thread at the widest input (k0 <= H)
        float v[SE];
        if (a.raw_is_f64) {
            double vd[SE];
#pragma unroll
            for (int i = 0; i < SE; ++i) {
                const int e = tid + i * NT, r = e / k0, c = e - r * k0;
                vd[i] = 0.0;
                if (e < FA_ROWS * k0 && row0 + r < a.n && c < a.d) vd[i] = reinterpret_cast<const double *>(a.raw)[(row0 + r) * a.ld_raw + c];
            }
#pragma unroll
            for (int i = 0; i < SE; ++i) v[i] = (float)vd[i];
        } else {
#pragma unroll
            for (int i = 0; i < SE; ++i) {
                const int e = tid + i * NT, r = e / k0, c = e - r * k0;
                v[i] = 0.f;
                if (e < FA_ROWS * k0 && row0 + r < a.n && c < a.d) v[i] = reinterpret_cast<const float *>(a.raw)[(row0 + r) * a.ld_raw + c];
            }
        }
#pragma unroll
        for (int i = 0; i < SE; ++i) {
            const int e = tid + i * NT;
            if (e >= FA_ROWS * k0) break;
            const int r = e / k0, c = e - r * k0;
            const int64_t row = row0 + r;
            float x = v[i];
            if (row < a.n && c < a.d) {
                if (a.standardize == 1) x = fminf(fmaxf((x - a.mean0) / a.std0, -5.f), 5.f);
                else if (a.standardize == 2) x = fminf(fmaxf((x - a.mean_v[c]) / a.std_v[c], -5.f), 5.f);
            }
            act0[(c >> 4) * 256 + dswz<16>(r, (c >> 2) & 3) + (c & 3)] = x;
            if (a.rows_out && row < a.n) a.rows_out[row * a.ld_rows_out + c] = x;
        }
    }
#pragma unroll
    for (int l = 0; l < FA_MAX_LAYERS; ++l)
        if (l <= last && tid < a.nblk[l] * 16) biasl[l * H + tid] = bias_v[l];
    __syncthreads();  // (drains the stream's first tiles too: once per launch)
    FA_TS(1);

    float *cur = act0, *nxt = act1;
    int consumed = 0;
    for (int l = 0; l <= last; ++l) {
        const bool head = l == last;
        const int own = head ? (a.nblk[l] + NW - 1) / NW : JH;
        const int jb0 = wave_u * own;                    // first output block of this wave
        const int nj = head ? (a.nblk[l] - jb0 < own ? (a.nblk[l] - jb0 < 0 ? 0 : a.nblk[l] - jb0) : own) : JH;
        f32x4 acc[JH];
#pragma unroll
        for (int j = 0; j < JH; ++j) {
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (j < nj) acc[j] = *reinterpret_cast<const f32x4 *>(&biasl[l * H + (jb0 + j) * 16 + q * 4]);
        }
        if (head && a.noise_ctl && nj == 0) {
            // this wave has nothing to multiply in the head layer: it fetches late noise.  Idle waves are [first_idle, NW); wave i of
            // them takes rows i, i + n_idle, ...; all its requests are in flight together, one wait
            const int first_idle = (a.nblk[l] + own - 1) / own, n_idle = NW - first_idle, iw = wave_u - first_idle;
            const int64_t n_live = (int64_t)live_raw < a.n ? (int64_t)live_raw : a.n;
            const bool there = __hip_atomic_load(a.noise_ctl + 2, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) == want;  // (wave-uniform)
            const unsigned *src = reinterpret_cast<const unsigned *>(a.noise);
            unsigned pp[FA_ROWS][2];
#pragma unroll
            for (int i = 0; i < FA_ROWS; ++i) {
                const int r = iw + i * n_idle;
                const int64_t row = row0 + r;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    pp[i][e] = 0x3f800000u;
                    if (there && r < FA_ROWS && row < n_live && lane + 64 * e < a.A)
                        pp[i][e] = __hip_atomic_load(src + row * a.A + lane + 64 * e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
#pragma unroll
            for (int i = 0; i < FA_ROWS; ++i) {
                const int r = iw + i * n_idle;
                if (r >= FA_ROWS) break;
                if (there) {
                    qbuf[r * FA_QLD + lane] = __uint_as_float(pp[i][0]);
                    qbuf[r * FA_QLD + 64 + lane] = __uint_as_float(pp[i][1]);
                }
                if (lane == 0) qok[r] = there && row0 + r < n_live;
            }
        } else if (head && a.noise_ctl && wave_u == 0 && (a.nblk[l] + own - 1) / own >= NW) {
            if (lane < FA_ROWS) qok[lane] = 0;  // no idle wave in this network: every row is fetched after the layer
        }
        // K loop in groups of FA_STAGES steps, unrolled: ring slot and activation K-step are immediates of the ds_reads, so a step is
        // DMA issue (scalar), a counted wait, three ds_read_b128 and 4 JH MFMAs with NO vector ALU instruction (while the other wave
        // of the SIMD streams MFMAs a VALU instruction of any kind takes ~400 cycles to issue, DESIGN section 5: the two address
        // updates per step of the rolled loop were ~800 of its ~955 cycles); one pointer bump per group
        const int nk = a.k[l] / 16;
        const float *ag = cur + dswz<16>(r16, q);
        const float *wg = wr + dswz<16>(r16, q);
        for (int kt0 = 0; kt0 < nk; kt0 += FA_STAGES) {
#pragma unroll
            for (int d = 0; d < FA_STAGES; ++d) {
                issue_next();  // keeps FA_STAGES - 1 tiles in flight behind the one about to be read
                // all but the pieces of the `ahead` tiles issued behind this step's have landed: the tile of this step is in LDS
                // (vmcnt immediates: ahead * JH; ahead < FA_STAGES - 1 only in the network's last steps)
                const int ahead = issued - consumed - 1;
                if (ahead >= 3) {
                    if (JH == 4) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
                    else if (JH == 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                } else if (ahead == 2) {
                    if (JH == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                    else if (JH == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                } else if (ahead == 1) {
                    if (JH == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else if (JH == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                ++consumed;  // (consumed % FA_STAGES == d: every layer starts a group)
                if (kt0 + d < nk) {  // not a padding step
                    const f32x4 fa = *reinterpret_cast<const f32x4 *>(&ag[d * 256]);
                    f32x4 fb[JH];
#pragma unroll
                    for (int j = 0; j < JH; ++j) fb[j] = *reinterpret_cast<const f32x4 *>(&wg[d * TILE + j * 256]);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int j = 0; j < JH; ++j) acc[j] = MFMA16(fb[j][s], fa[s], acc[j]);
                }
            }
            ag += FA_STAGES * 256;
        }
        if (!head) {
            // relu, then straight into the next layer's fragment image: block jb = k-step jb, row r16, chunk q
#pragma unroll
            for (int j = 0; j < JH; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] = relu1(acc[j][e]);
                *reinterpret_cast<f32x4 *>(&nxt[(jb0 + j) * 256 + dswz<16>(r16, q)]) = acc[j];
            }
        } else {
            // logits, row-major [16][nblk*16] in the free activation buffer
            const int ldz = a.nblk[l] * 16;
#pragma unroll
            for (int j = 0; j < JH; ++j)
                if (j < nj) *reinterpret_cast<f32x4 *>(&nxt[r16 * ldz + (jb0 + j) * 16 + q * 4]) = acc[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // raw: the weight tiles in flight stay in flight
        float *t = cur;
        cur = nxt;
        nxt = t;
    }

    FA_TS(2);
    // ---- sampling: wave w takes RPWV rows; element c = lane + 64 e (discrete_sample_kernel<2, false>, op for op)
    const int A = a.A, ldz = a.nblk[last] * 16;
    bool gave_up = false;
    const int64_t n_live = a.noise_ctl && (int64_t)live_raw < a.n ? (int64_t)live_raw : a.n;
    if (a.noise_ctl) {
        const unsigned *src = reinterpret_cast<const unsigned *>(a.noise);
        bool need[RPWV];
        bool any = false;
#pragma unroll
        for (int rr = 0; rr < RPWV; ++rr) {
            const int r = wave * RPWV + rr;
            need[rr] = row0 + r < n_live && !qok[r];
            any |= need[rr];
            if (row0 + r < n_live && !need[rr]) {
                qn[rr][0] = qbuf[r * FA_QLD + lane];
                qn[rr][1] = qbuf[r * FA_QLD + 64 + lane];
            }
        }
        const long long t0 = wall_clock64();
        unsigned rounds = 0;
        if (any) {  // (wave-uniform) the host was not done when the head layer started: wait for its word, then read
            while (__hip_atomic_load(a.noise_ctl + 2, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != want) {
                ++rounds;
                if (wall_clock64() - t0 > FA_NOISE_WAIT_TICKS) {
                    gave_up = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(8);
            }
            if (!gave_up) {
#pragma unroll
                for (int rr = 0; rr < RPWV; ++rr)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int64_t row = row0 + wave * RPWV + rr;
                        const int c = lane + 64 * e;
                        if (need[rr] && c < A)
                            qn[rr][e] = __uint_as_float(__hip_atomic_load(src + row * A + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
                    }
            }
        }
        // statistics of the call's first wave (for tools): polls it made itself, 10 ns ticks from the last layer to its noise
        if (tile == 0 && tid == 0) {
            a.noise_ctl[3] = rounds + (any ? 1u : 0u);
            a.noise_ctl[4] = (unsigned)(wall_clock64() - t0);
        }
    }
    // [r5] the wave's RPWV rows go through the stages TOGETHER (each cross-lane step is a ~100-cycle round trip through the LDS
    // crossbar: the rows' chains are independent and overlap) -- same operations per row as before, bit for bit; rows past n_live
    // run on whatever their logits hold and store nothing
    {
        float p[RPWV][2], pc[RPWV][2], mx[RPWV], sm[RPWV], best[RPWV], bestp[RPWV];
        int besti[RPWV];
        bool live[RPWV];
        // (MASKED) element c takes part: c < A and its action is valid -- a row without a valid action is all-valid; the unmasked
        // instantiations test c < A where they always did
        bool ok[RPWV][2];
        if (MASKED) {
#pragma unroll
            for (int rr = 0; rr < RPWV; ++rr) {
                const bool i0 = lane < A, i1 = lane + 64 < A;
                const bool v0 = i0 && ((mw[rr][0] >> (lane & 31)) & 1u), v1 = i1 && ((mw[rr][1] >> (lane & 31)) & 1u);
                const bool any = __ballot(v0 || v1) != 0;  // (wave-uniform)
                ok[rr][0] = any ? v0 : i0;
                ok[rr][1] = any ? v1 : i1;
            }
        }
#define FA_IN(rr, e, c) (MASKED ? ok[rr][e] : (c) < A)
#pragma unroll
        for (int rr = 0; rr < RPWV; ++rr) {
            const int r = wave * RPWV + rr;
            live[rr] = row0 + r < n_live;
            const float *z = cur + r * ldz;
            mx[rr] = -INFINITY;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = lane + 64 * e;
                p[rr][e] = FA_IN(rr, e, c) ? z[c] : -INFINITY;
                mx[rr] = fmaxf(mx[rr], p[rr][e]);
            }
        }
#define FA_BFLY(STEP) STEP(32) STEP(16) STEP(8) STEP(4) STEP(2) STEP(1)
#define FA_MAX_STEP(O)                                                                  \
    _Pragma("unroll") for (int rr = 0; rr < RPWV; ++rr) mx[rr] = fmaxf(mx[rr], fa_xor_f<O>(mx[rr]));
        FA_BFLY(FA_MAX_STEP)
#pragma unroll
        for (int rr = 0; rr < RPWV; ++rr) {
            sm[rr] = 0.f;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = lane + 64 * e;
                p[rr][e] = FA_IN(rr, e, c) ? expf(p[rr][e] - mx[rr]) : 0.f;
                sm[rr] += p[rr][e];
            }
        }
#define FA_SUM_STEP(O)                                                                  \
    _Pragma("unroll") for (int rr = 0; rr < RPWV; ++rr) sm[rr] += fa_xor_f<O>(sm[rr]);
        FA_BFLY(FA_SUM_STEP)
#pragma unroll
        for (int rr = 0; rr < RPWV; ++rr) {
            const int64_t row = row0 + wave * RPWV + rr;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                p[rr][e] = p[rr][e] / sm[rr];
                pc[rr][e] = fminf(fmaxf(p[rr][e], FA_PROB_MIN), 1.0f);
            }
            best[rr] = -INFINITY;
            bestp[rr] = 1.f;
            besti[rr] = 0x7fffffff;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int c = lane + 64 * e;
                if (FA_IN(rr, e, c)) {
                    const float v = pc[rr][e] / qn[rr][e];  // IEEE fp32 division, as at::div
                    if (v > best[rr]) {
                        best[rr] = v;
                        besti[rr] = c;
                        bestp[rr] = pc[rr][e];
                    }
                    if (a.probs_out && live[rr]) a.probs_out[row * A + c] = pc[rr][e];
                } else if (MASKED && c < A) {
                    if (a.probs_out && live[rr]) a.probs_out[row * A + c] = 0.f;
                }
            }
        }
#define FA_ARG_STEP(O)                                                                  \
    _Pragma("unroll") for (int rr = 0; rr < RPWV; ++rr) {                               \
        const float ov = fa_xor_f<O>(best[rr]);                                         \
        const int oi = fa_xor_i<O>(besti[rr]);                                          \
        const float op = fa_xor_f<O>(bestp[rr]);                                        \
        if (ov > best[rr] || (ov == best[rr] && oi < besti[rr])) {                      \
            best[rr] = ov;                                                              \
            besti[rr] = oi;                                                             \
            bestp[rr] = op;                                                             \
        }                                                                               \
    }
        FA_BFLY(FA_ARG_STEP)
#undef FA_ARG_STEP
#undef FA_IN
#undef FA_SUM_STEP
#undef FA_MAX_STEP
#undef FA_BFLY
#pragma unroll
        for (int rr = 0; rr < RPWV; ++rr) {
            const int64_t row = row0 + wave * RPWV + rr;
            if (lane == 0 && live[rr]) {
                a.actions[row] = besti[rr];
                a.logp[row] = logf(bestp[rr]);
                if (a.actions_f32) a.actions_f32[row] = (float)besti[rr];
            }
        }
    }
    // [r5] completion word of this workgroup's 16 rows: every wave releases its stores at system scope, then ONE word follows them
    // (a host that polls the word -- pinned memory -- reads the results without synchronising the stream: rlppo_act_opts)
    FA_TS(3);
    if (a.done_words) {
        __shared__ int fa_gave_up;
        if (a.noise_ctl) {  // (the layers' last barrier is behind every wave)
            if (tid == 0) fa_gave_up = 0;
            __syncthreads();
            if (gave_up && lane == 0) fa_gave_up = 1;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __syncthreads();
        if (tid == 0) {
            const unsigned v = a.noise_ctl && fa_gave_up ? a.done_value | FA_DONE_FAILED : a.done_value;
            __hip_atomic_store(a.done_words + tile, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

#undef FA_TS

// Does the network have the form the fused kernel covers?  n_layers in [2, 6]; all hidden widths equal, 64 / 128 / 256; the first
// layer's padded input at most the hidden width; at most 128 actions.
bool fused_act_ok(const NetLayout &net) {
    if (net.n_layers < 2 || net.n_layers > FA_MAX_LAYERS) return false;
    const int H = net.L[0].pout;
    if (H != 64 && H != 128 && H != 256) return false;
    for (int l = 0; l + 1 < net.n_layers; ++l)
        if (net.L[l].pout != H || net.L[l].out != H) return false;
    const LayerLayout &o = net.L[net.n_layers - 1];
    if (o.out > 128 || o.pout > 128 || o.pout > H) return false;
    if (net.L[0].pin > H || net.L[0].pin % 16 != 0) return false;
    // the kernel's dynamic LDS (up to 102 KiB at H = 256) against what THIS device grants a workgroup: a device with a 64 KiB
    // limit takes the bit-identical layer chain instead of failing the launch (advisor finding, round 3)
    const int J = H == 256 ? 2 : 1, W = H == 64 ? 4 : 8;
    const size_t need = (size_t)(2 * 16 * J * W * FA_ROWS + W * FA_STAGES * J * 256 + FA_MAX_LAYERS * 16 * J * W + FA_QFLOATS) * 4;
    static std::atomic<long> lds_limit[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    long lim = lds_limit[dev].load(std::memory_order_acquire);
    if (lim == 0) {
        int v = 0;
        // (the opt-in maximum: hipFuncSetAttribute raises a kernel's limit up to it)
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) v = 65536;
        int vo = 0;
        if (hipDeviceGetAttribute(&vo, hipDeviceAttributeSharedMemPerBlockOptin, dev) == hipSuccess && vo > v) v = vo;
        lim = v;
        lds_limit[dev].store(lim, std::memory_order_release);
    }
    return need <= (size_t)lim;
}

int launch_discrete_act_fused(hipStream_t st, const NetLayout &net, const float *packed, const FusedActIO &io, int64_t n) {
    if (n <= 0) return 0;
    FusedActArgs a;
    a.rows = io.rows;
    a.ld_rows = (unsigned)io.ld_rows;
    a.raw = io.raw;
    a.raw_is_f64 = io.raw_is_f64;
    a.d = net.L[0].in;
    a.standardize = io.standardize;
    a.ld_raw = io.ld_raw;
    a.mean0 = io.mean0;
    a.std0 = io.std0;
    a.mean_v = io.mean_v;
    a.std_v = io.std_v;
    a.rows_out = io.rows_out;
    a.ld_rows_out = io.ld_rows_out;
    a.actions_f32 = io.actions_f32;
    a.n = n;
    a.packed = packed;
    a.n_layers = net.n_layers;
    for (int l = 0; l < net.n_layers; ++l) {
        a.k[l] = net.L[l].pin;
        a.nblk[l] = net.L[l].pout / 16;
        a.off_w[l] = net.L[l].off_w;
        a.off_b[l] = net.L[l].off_b;
    }
    a.A = net.L[net.n_layers - 1].out;
    a.noise = io.noise;
    a.actions = io.actions;
    a.logp = io.logp;
    a.probs_out = io.probs_out;
    a.done_words = io.done_words;
    a.done_value = io.done_value;
    a.noise_ctl = io.noise_ctl;
    a.mask = io.mask;
    a.mask_words = io.mask_words;
    RLPPO_CHECK_ARG(!io.mask || io.mask_words == (a.A + 31) / 32,
                    "discrete act: action_mask needs mask_words=%d == ceil(n_actions=%d / 32)", io.mask_words, a.A);
    const int H = net.L[0].pout;
    dim3 grid((unsigned)cdiv(n, FA_ROWS));
    static PerDeviceOnce attr_set[6];
#define FA_LAUNCH(J, W, SLOT)                                                                                                    \
    do {                                                                                                                         \
        constexpr int LDS_BYTES = (2 * 16 * J * W * FA_ROWS + W * FA_STAGES * J * 256 + FA_MAX_LAYERS * 16 * J * W + FA_QFLOATS) * 4; \
        /* up to 110 KiB of dynamic LDS (H = 256): above the default 64 KiB limit */                                             \
        if (a.mask) { /* [ABI 8] */                                                                                             \
            if (int rc_ = set_dynamic_lds_once((const void *)discrete_act_fused_kernel<J, W, true>, LDS_BYTES, attr_set[3 + SLOT])) return rc_; \
            hipLaunchKernelGGL((discrete_act_fused_kernel<J, W, true>), grid, dim3(64 * W), LDS_BYTES, st, a);                   \
            break;                                                                                                               \
        }                                                                                                                        \
        if (int rc_ = set_dynamic_lds_once((const void *)discrete_act_fused_kernel<J, W>, LDS_BYTES, attr_set[SLOT])) return rc_; \
        hipLaunchKernelGGL((discrete_act_fused_kernel<J, W>), grid, dim3(64 * W), LDS_BYTES, st, a);                              \
    } while (0)
    switch (H) {
        case 256: FA_LAUNCH(2, 8, 0); break;
        case 128: FA_LAUNCH(1, 8, 1); break;
        default: FA_LAUNCH(1, 4, 2); break;
    }
#undef FA_LAUNCH
    RLPPO_LAUNCH_CHECK();
    return 0;
}

}  // namespace rlppo
