/*
 * rlppo.h -- C ABI of librlppo.so, the MI355X (gfx950) hot path of rlgym-ppo.
 *
 * The reference (AechPro/rlgym-ppo v1.3.13) is pure Python and has no FFI; its boundary for this path is
 * the Python class API.  The host-side mirror of that API lives in
 * rlgym_ppo_amd/ and calls the entry points below through ctypes.  Every entry point names the reference
 * code it replaces (paths relative to the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  All `const float*` / `float*` / `int64_t*` data arguments
 *     are DEVICE pointers borrowed from the caller (torch tensors' data_ptr()), except where a parameter is
 *     explicitly marked HOST.  The library never allocates or frees device memory: scratch space is a
 *     caller-provided workspace sized by the matching *_workspace_bytes() query.
 *   - `stream` is a hipStream_t passed as void*.  All device work is enqueued asynchronously on it; no entry
 *     point synchronises the device, so every call is legal inside a hipGraph capture.
 *   - Return value: 0 = OK; non-zero = error (RLPPO_ERR_* or a hipError_t).  rlppo_last_error() returns a
 *     thread-local description of the most recent failure.  No C++ exception crosses the ABI.
 *   - A network is described by `dims[0..n_layers]` = {d_in, h_1, ..., h_L, d_out} (logical sizes, exactly the
 *     nn.Linear sizes the reference builds: discrete_policy.py:22-31, value_estimator.py:19-28) and by its
 *     parameters in `torch.nn.utils.parameters_to_vector` order: W_0[out][in], b_0, W_1, b_1, ...
 *     ("flat arena").  Kernels consume a PACKED copy (tile-padded W, W^T and b) built by rlppo_net_pack().
 *   - Row-major everywhere.  Observation matrices have a leading dimension `ld` (floats) >= d_in; rows that the
 *     kernels read directly must have ld a multiple of 32 with zero fill beyond d_in (rlppo_padded_width()).
 */
#ifndef RLPPO_H
#define RLPPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The export table: the library is built with -fvisibility=hidden, and exactly the functions declared between this push and
 * the matching pop have default visibility (`nm -D` shows them and nothing else of the library's own; tests/test_abi_and_layout.py). */
#pragma GCC visibility push(default)

#define RLPPO_ABI_VERSION 8
#define RLPPO_MAX_LAYERS 16
/* [nvec] limits of a multi-discrete action space MultiDiscrete(nvec) (rlppo_multidiscrete_act_nvec, rlppo_ppo_minibatch_nvec):
 * 1 <= heads <= RLPPO_MD_MAX_HEADS, 1 <= nvec[h] <= RLPPO_MD_MAX_BINS, sum of nvec <= RLPPO_MD_MAX_LOGITS.  Anything beyond is
 * RLPPO_ERR_ARG with a message naming the limit, before any launch.
 *
 * [nvec, masked] Invalid-action masking of the multi-discrete head: rlppo_multidiscrete_act_nvec_masked (an added entry point, as
 * the _nvec ones were) and rlppo_ppo_minibatch_nvec with md_nvec given; no new struct field, the ABI version stays 8.  A mask row has S = sum(nvec) bits, ONE PER LOGIT, in the encoding of rlppo_act_opts.action_mask: W = ceil(S / 32)
 * words per row, bit c % 32 of word c / 32 set = logit c valid, bits at and beyond S ignored.  Head h owns bits [s_h, s_h + b_h);
 * with V_h its valid set:
 *   distribution  head h is Categorical(logits = z_h with -inf outside V_h): MultiDiscreteRolv's construction with more -inf than the
 *                 padding alone;
 *   sampling      the first arg-max over c in V_h of softmax_V(z_h)_c / noise_q[(row * H + h) * B + c]; the noise keeps its
 *                 [n * H][B] shape and the noise of invalid bins is never read;
 *   loss terms    log p = sum_h (z[a_h] - lse_V(z_h)), entropy = sum_h -sum_{c in V_h} p_c log p_c; the row sums are taken in double
 *                 and rounded once, as without a mask;
 *   gradient      dL/dz is exactly 0 on every invalid logit and on the padded columns >= S; on valid logits the unmasked
 *                 expression with p, lse and the head's entropy taken over V_h;
 *   one valid bin such a head contributes log-probability 0, entropy 0 and a zero gradient, as a head of one bin does;
 *   no valid bin  a caller error: hosts reject such a row before launch; inside the kernels that head counts as all-valid;
 *   a stored action its own mask marks invalid (a caller error): its term is the literal z[a] - lse_V, its one-hot falls on an
 *                 invalid column and is dropped; everything stays finite;
 *   no mask       the library as it is, launch for launch; an all-valid mask gives the unmasked general kernels' results bit for
 *                 bit (the maximum and the sums run over the valid bins in c order);
 *   fixed bins    rlppo_multidiscrete_act, and rlppo_ppo_minibatch / _nvec with md_nvec == NULL, refuse a mask (RLPPO_ERR_ARG): a
 *                 masked call on the reference's bins gives md_nvec = {3, 3, 3, 3, 3, 2, 2, 2} and runs the general kernels;
 *   act options   a mask in rlppo_act_opts stays refused by every multi-discrete rollout entry point, rlppo_multidiscrete_act_nvec
 *                 included (the text callers know): the masked step takes its mask as an argument of its own entry point.
 *   captured     rlppo_multidiscrete_act_nvec_masked may be captured into a graph with completion words (rlppo_act_opts.done_words)
 *                 and a mask in host-visible memory (a host window, or pinned memory) that the host rewrites before every
 *                 replay: the kernel reads only words inside a row's W words and writes row r's results to row r, so rows
 *                 whose words are stale are harmless and a stale head without a valid bin is all-valid (rule above);
 *   collection    process-mode collection carries the S entries of a row behind its observation (the opt-in trailer of
 *                 rlgym_ppo_amd/batched_agents/comm_consts.py) and rlppo_collector_set_mask_heads gives the C++ loop the layout.
 * A wrong mask_words is RLPPO_ERR_ARG naming the field and the needed count, before any HIP call.  A head has at most 64 bins, so
 * the kernels assemble V_h as one 64-bit value from the two or three words it touches (no per-row array, no scratch). */
#define RLPPO_MD_MAX_HEADS 64
#define RLPPO_MD_MAX_BINS 64
#define RLPPO_MD_MAX_LOGITS 512

#define RLPPO_OK 0
#define RLPPO_ERR_ARG 1001        /* bad argument / unsupported shape */
#define RLPPO_ERR_WORKSPACE 1002  /* workspace too small */
#define RLPPO_ERR_COLLECT_TIMEOUT 1003  /* rlppo_collector_collect: no worker message for a minute */
#define RLPPO_ERR_INTERRUPTED 1004     /* rlppo_collector_collect: a signal arrived; n_collected holds the progress, call again with resume = 1 */
#define RLPPO_ERR_MASK_ROW 1005        /* rlppo_collector_ready_masks: a worker reported an action-mask row (a head of one) without a valid action */

/* policy head codes == the reference's `policy_type` (ppo_learner.py:34-50) */
#define RLPPO_HEAD_DISCRETE 0
#define RLPPO_HEAD_MULTIDISCRETE 1
#define RLPPO_HEAD_GAUSSIAN 2
/* [diag] The diagonal-Gaussian head with a learnable, state-independent log-std (Stable-Baselines3, CleanRL, rl_games; not in the
 * reference): opt-in, a fourth head beside the reference's three (added entry points: rlppo_diag_gaussian_act,
 * rlppo_ppo_minibatch_diag, rlppo_diag_scratch_bytes, rlppo_clip_adam_pack2_tail; no struct changes, the ABI version stays 8).  The
 * policy network has dims {obs, hidden.., k}, its last layer is plain bias (NO tanh); log_std is k floats of DEVICE memory that are
 * not a layer of the network: the first parameter that lives in a TAIL behind a network's rlppo_flat_floats.
 *   sigma_j = exp(log_std_j), mu = net(obs), 1 <= k <= RLPPO_DIAG_MAX_K
 *   sample         a_j = mu_j + sigma_j eps_j with the caller's eps[n][k] ~ N(0, 1); the sample is NOT clamped
 *   deterministic  a = mu, row by row (rlppo_mlp_forward with out_tanh = 0; not the discrete head's one-index-per-batch quirk)
 *   log p          sum_j [ -(a_j - mu_j)^2 / (2 sigma_j^2) - log_std_j - 1/2 log 2 pi ]: torch.distributions.Normal.log_prob's terms in
 *                  its order, of the sample as drawn / as stored; up to 32 dimensions the float terms are summed in float in j order,
 *                  above that in double and rounded once (the rule of RLPPO_HEAD_GAUSSIAN's kernels)
 *   entropy        of one row: sum_j (1.4189385332046727 + log_std_j), summed over the dimensions with NO division by k; the report's
 *                  entropy is its mean over the rows.  This deliberately DIFFERS from RLPPO_HEAD_GAUSSIAN, which averages over the
 *                  action dimensions too (the reference's quirk Q8): here the entropy bonus is Normal.entropy().sum(-1), as in SB3
 *   gradients      through the surrogate every head shares (clip range, torch.min's tie rule, adv_norm, stop_word, kl_slots as for
 *                  the other heads): dL/dmu_j = g_logp (a_j - mu_j) / sigma_j^2, in place over the head output;
 *                  dL/dlog_std_j = sum over the rows of [ g_logp ((a_j - mu_j)^2 / sigma_j^2 - 1) - mb_ratio ent_coef / mb ]
 *   reduction      the log_std gradient is bit-reproducible: every workgroup of the loss launch (256 rows) writes its k partial sums
 *                  (double, fixed tree) into its row of the caller's scratch (rlppo_diag_scratch_bytes(mb, k) bytes, no zeroing
 *                  needed), a second small launch adds the rows in a fixed order (double) and adds the rounded sum ONCE per element
 *                  and launch into log_std_grad -- the rule the weight gradients follow; no floating-point atomics inside the sum
 *   masks          refused (RLPPO_ERR_ARG, the text the Gaussian head's refusal has)
 *   optimiser      rlppo_clip_adam is n-based (n = rlppo_flat_floats + k); rlppo_clip_adam_pack2_tail is rlppo_clip_adam_pack2 with
 *                  tail_floats more elements behind each network's layers: same norm, same Adam, zeroed gradient, skip_word, and
 *                  never written into `packed`. */
#define RLPPO_HEAD_DIAG_GAUSSIAN 3
#define RLPPO_DIAG_MAX_K 256

/* precision of a call (rlppo_act_opts.precision, rlppo_minibatch_args.precision): 0 = the process default set with
 * rlppo_set_inference_precision / rlppo_set_update_precision, else 1 + that setter's mode */
#define RLPPO_PRECISION_DEFAULT 0
#define RLPPO_PRECISION_FP32 1
#define RLPPO_PRECISION_BF16 2
#define RLPPO_PRECISION_X3 3   /* update only: fp32 with split-bf16 hidden products */

int rlppo_abi_version(void);
const char *rlppo_last_error(void);
/* [r6] 16 hex digits: SHA-256 over the sources this library was built from (csrc/Makefile).  Evidence replayed from profiles/
 * (bench.py's `roofline.traffic`: PMC bytes per launch, measured by a builder-run rocprofv3 pass) is stamped with the id of the
 * library it was measured on and reported only while that is the library in use. */
const char *rlppo_build_id(void);

/* ---------------------------------------------------------------------------------------------- layout */

/* Width (floats) to which an input feature dimension is padded for the kernels (multiple of 32). */
int64_t rlppo_padded_width(int64_t d);
/* Width to which a layer OUTPUT dimension is padded (32, 64, 96, 128 or a multiple of 128). */
int64_t rlppo_padded_out(int64_t d);
/* Number of floats in the packed copy of a network. */
int64_t rlppo_packed_floats(const int32_t *dims, int32_t n_layers);
/* Number of floats in the flat arena of a network (sum of out*in + out). */
int64_t rlppo_flat_floats(const int32_t *dims, int32_t n_layers);

/* Build the packed copy (padded W, W^T, b per layer) from the flat arena.  Called after every optimiser step.
 * Replaces nothing in the reference (it is the price of tile-aligned kernels).  The image, layer after layer with
 * Pin_0 = rlppo_padded_width(dims[0]), Pin_l = Pout_(l-1), Pout_l = rlppo_padded_out(dims[l+1]):
 *     W[Pout][Pin] | W^T[Pin][Pout] | b[Pout],   zero wherever no parameter lands.
 * The call writes EVERY one of the rlppo_packed_floats entries, the zero padding included: `packed` needs no
 * initialisation (rlppo_clip_adam_pack2, which rewrites the parameters' slots only, relies on an image built here). */
int rlppo_net_pack(void *stream, const int32_t *dims, int32_t n_layers, const float *flat, float *packed);

/* Copy/convert observation rows into the padded device layout: dst[r][0:d] = (float)src[r][0:d], zero fill to
 * ld_dst.  `src_is_f64` selects a float64 source (learner.py:347 builds a float64 value-net input).
 * Optional standardisation with the reference's SCALAR statistics (quirk Q5, batched_agent_manager.py:313-315):
 * if standardize != 0, dst = clip((src - mean0) / std0, -5, 5). */
int rlppo_pad_rows(void *stream, const void *src, int32_t src_is_f64, int64_t n, int64_t d, int64_t ld_src,
                   float *dst, int64_t ld_dst, int32_t standardize, float mean0, float std0);
/* The same copy with per-feature statistics (device vectors of d floats): dst = clip((src - mean[c]) / std[c], -5, 5).
 * Not the reference's behaviour (it applies the scalars of feature 0 to every feature, batched_agent_manager.py:230-235,
 * 313-315): the corrected form SURVEY.md section 8(f) row 4 asks for, selected by per_feature_obs_standardization=True. */
int rlppo_pad_rows_per_feature(void *stream, const void *src, int32_t src_is_f64, int64_t n, int64_t d, int64_t ld_src,
                               float *dst, int64_t ld_dst, const float *mean, const float *stdv);

/* ------------------------------------------------------------------------------------ rollout inference */

/* [r5] Per-call options of the rollout entry points below (their last parameter; NULL = all defaults).
 *   precision: the inference precision of THIS call -- RLPPO_PRECISION_DEFAULT (what rlppo_set_inference_precision chose for the
 *     process), RLPPO_PRECISION_FP32 or RLPPO_PRECISION_BF16 (operands rounded to bf16, fp32 accumulate): two policies of one
 *     process may act in different precisions.
 *   done_words / done_value: completion without a stream synchronisation.  done_words (optional) points at rlppo_act_done_words(n)
 *     uint32 in HOST-VISIBLE memory (pinned / page-locked, coherent); word b receives done_value -- stored with release semantics
 *     at system scope -- once every output of rows 16 b .. 16 b + 15 is visible to the host (the one-launch kernel of
 *     rlppo_discrete_act / _step stores it itself, workgroup by workgroup; the layer chains append one tiny launch that stores them
 *     all).  A host whose outputs live in pinned memory clears the words, makes the call and polls them (rlppo_host_wait_words)
 *     instead of hipStreamSynchronize: batched_agent_manager.py:202-204 calls get_action on 8-80 observations per environment
 *     step, where the synchronisation was a third of the call.
 *   noise_ctl (rlppo_discrete_step's one-launch kernel only; needs done_words, done_value < 2^31): the noise arrives WHILE the
 *     kernel runs -- the bit-exact Exp(1) draw of the reference's CPU stream (5-11 us at 8-80 rows) hides behind the launch
 *     latency and the layers.  noise_ctl points at 32 uint32 the host can write and the kernel reads past its caches (pinned
 *     memory, or better a host window, below): [0] the call's sequence (never the previous call's), [1] live rows -- both written
 *     BEFORE the call -- [2] the sequence of the noise that is complete in noise_q, [3..] statistics the kernel writes
 *     ([3] polls / [4] 10 ns ticks the first wave spent on its noise after the last layer; [8..11] 100 MHz time stamps of the last
 *     workgroup: start, observations staged, layers done, sampled).  noise_q
 *     is [n][n_actions] floats in such memory too; the host fills it AFTER the launch and then stores the call's sequence into
 *     word 2 (rlppo_host_push does both in order).  The waves that have nothing to multiply in the head layer look at word 2 when
 *     that layer starts and bring the numbers in; if the host was not done by then every wave waits for the word after the last
 *     layer.  Rows >= live rows are not sampled (their outputs are untouched).  Between the launch and word 2 the host must not
 *     wait for the GPU (the kernel waits for the host).  A workgroup that has waited 20 ms gives up: it stores
 *     done_value | 0x80000000 (rlppo_host_wait_words returns 2), its outputs are void; the caller completes word 2 and makes the
 *     call again. */
typedef struct rlppo_act_opts {
    int32_t precision;
    uint32_t done_value;
    uint32_t *done_words;
    uint32_t *noise_ctl;
    /* [ABI 8] invalid-action masking (discrete head: rlppo_discrete_act / _step / _probs; any other entry point answers
     * RLPPO_ERR_ARG -- the multi-discrete head's masked step is rlppo_multidiscrete_act_nvec_masked, "[nvec, masked]" above).  action_mask: DEVICE [n][mask_words] words, mask_words == ceil(n_actions / 32), bit c % 32 of word c / 32 set =
     * action c is valid in that row; bits at and beyond n_actions are ignored; NULL = no mask (the call is the unmasked one, launch
     * for launch).  Semantics: an invalid action's logit is -inf (what the padded columns c >= n_actions always were), so
     * p = softmax(z') is exactly 0 on it; pc = clamp(p, 1e-11, 1) on valid actions; action = first arg-max over VALID c of
     * pc_c / q_c (the clamp's floor never makes an invalid action selectable), logp = log(pc_action).  noise_q stays
     * [n][n_actions]: the entries of invalid actions are ignored.  probs_out / rlppo_discrete_probs (with and without clamp_probs)
     * hold 0 on invalid actions and flat_argmax runs over valid entries only.  A row without a valid action is treated as all-valid
     * (hosts reject such rows before they get here).  An all-valid mask gives the unmasked results bit for bit.  Together with
     * noise_ctl (rlppo_discrete_step's one-launch kernel) only the noise is late: the words are in place BEFORE the launch, in
     * memory the kernel reads like its observations (a host window, or pinned memory), and rows at and beyond the live-row word
     * -- whose mask words may be stale -- store nothing. */
    const uint32_t *action_mask;
    int32_t mask_words;
    /* [act] the activation of every hidden layer: RLPPO_ACT_RELU (0: today's call, launch for launch), RLPPO_ACT_TANH, RLPPO_ACT_ELU
     * (alpha = 1).  The member occupies what were the struct's 4 bytes of tail padding (size and every other offset unchanged: ABI 8
     * stays), so a zeroed struct and a NULL pointer are the ReLU call.  Every rollout entry point honours it through its layer
     * chain; with tanh / ELU rlppo_discrete_act / _step skip the one-launch kernel (rlppo_discrete_step_one_launch answers 0, so
     * noise_ctl is refused), and the bf16 inference precision is RLPPO_ERR_ARG (its kernels are ReLU only).  Any other value:
     * RLPPO_ERR_ARG before the first HIP call. */
    int32_t hidden_act;
} rlppo_act_opts;
#define RLPPO_ACT_RELU 0
#define RLPPO_ACT_TANH 1
#define RLPPO_ACT_ELU 2
#ifdef __cplusplus
static_assert(sizeof(rlppo_act_opts) == 40 && offsetof(rlppo_act_opts, hidden_act) == 36, "rlppo_act_opts: hidden_act lives in the former tail padding");
#else
_Static_assert(sizeof(rlppo_act_opts) == 40 && offsetof(rlppo_act_opts, hidden_act) == 36, "rlppo_act_opts: hidden_act lives in the former tail padding");
#endif
int64_t rlppo_act_done_words(int64_t n);
/* HOST: spins until words[0..count) all hold `value` (acquire loads) or timeout_us has passed; 0 = all there, 1 = timed out,
 * 2 = a word holds value | 0x80000000 (the kernel gave up: noise_ctl above). */
int rlppo_host_wait_words(const uint32_t *words, int64_t count, uint32_t value, int64_t timeout_us);
/* [r5] Host window: DEVICE memory (fine-grained, zeroed) that the host writes directly through the PCIe aperture -- a posted write
 * of a small call's observations costs the host 1.5-2.5 us, where the kernel's own reads of pinned host memory cost it 11-20 us
 * (a GPU-initiated PCIe read is a round trip of microseconds and ~30 ns per 64 bytes behind it).  Write-only for the host
 * (its reads are uncached: 65 us per 3 KB).  Fails (RLPPO_ERR_ARG) on a device that does not expose its memory (no large BAR).
 * rlppo_host_push: HOST: memcpy(dst, src, bytes), a store fence, then -- if flag is not NULL -- *flag = value and another fence:
 * nothing that follows (the doorbell of a launch, the flag) can overtake the bytes. */
int rlppo_host_window_alloc(size_t bytes, void **ptr);
int rlppo_host_window_free(void *ptr);
/* HOST: flushes the host data path of the window's device (a store to the HDP flush register HIP maps into the process): every
 * host write that has left the CPU is in device memory on return.  ~1-2.5 us.  Ordering without it: host writes reach the device in
 * program order (posted PCIe writes behind a store fence), so a flag word written after the bytes it announces arrives after them
 * (the late noise), and a launch's doorbell arrives after the bytes staged before it, with the packet fetch and the dispatch (>= 3 us)
 * between the doorbell and the kernel's first read.  ActGraph issues the flush between staging and launch (by the book: 0.9 us of a
 * 39 us call); behind the launch it is free. */
int rlppo_host_window_flush(const void *window);
int rlppo_host_push(void *dst, const void *src, size_t bytes, uint32_t *flag, uint32_t value);
/* HOST: what precedes the launch of a small rollout call, in one call: ctl[0] = sequence, ctl[1] = live_rows (ctl may be NULL),
 * memcpy(obs_dst, obs_src, obs_bytes), one store fence. */
int rlppo_host_stage_call(uint32_t *ctl, uint32_t sequence, uint32_t live_rows, void *obs_dst, const void *obs_src, size_t obs_bytes);
/* ... with the observations as ROWS of a padded image: row r (row_bytes, src_stride apart) goes to dst + r * dst_stride.  A host window
 * that only ever receives the first row_bytes of its rows stays zero beyond them: it IS the zero-padded input the forward entry points
 * read (ld = dst_stride / 4), and the layer chain of a small call needs no rlppo_pad_rows launch. */
int rlppo_host_stage_rows(uint32_t *ctl, uint32_t sequence, uint32_t live_rows, void *dst, size_t dst_stride, const void *src,
                          size_t src_stride, size_t row_bytes, int64_t rows);

/* Bytes of workspace needed by the forward entry points for `n` rows. */
size_t rlppo_forward_workspace_bytes(const int32_t *dims, int32_t n_layers, int64_t n);

/* MLP forward: out[n][ld_out] = Linear_L(relu(...relu(Linear_0(obs)))) (+ tanh if out_tanh).
 * Replaces nn.Sequential.forward of value_estimator.py:30-36 / the body of *_policy.get_output. */
int rlppo_mlp_forward(void *stream, const int32_t *dims, int32_t n_layers, const float *packed,
                      const float *obs, int64_t ld_obs, int64_t n, int32_t out_tanh,
                      float *out, int64_t ld_out, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts);

/* DiscreteFF.get_action (discrete_policy.py:44-62): forward, softmax, clamp(1e-11,1), action =
 * argmax_a(p_a / q_a) with the caller's Exp(1) noise q[n][n_actions] (== torch.multinomial(p,1,True), SURVEY
 * 8(a1); first index wins ties), logp = log(p_action).  actions: int64[n]; logp: float[n];
 * probs_out (optional, may be NULL): float[n][n_actions]. */
int rlppo_discrete_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed,
                       const float *obs, int64_t ld_obs, int64_t n, const float *noise_q,
                       int64_t *actions, float *logp, float *probs_out, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts);

/* The whole rollout step of the discrete policy [r3] (discrete_policy.py:35-62 behind batched_agent_manager.py:202-204,303-315):
 * raw observations as the environment hands them over ([n][ld_obs] fp32 or fp64, d = dims[0] features) -> standardise
 * (0: no; 1: the reference's scalars of feature 0, clip((x - mean0) / std0, -5, 5); 2: per-feature vectors mean_v / std_v) and
 * zero-pad -> MLP -> softmax -> clamp -> argmax(p / q) -> log p.  One launch when the network has the form csrc/fused_act.hip
 * covers (equal hidden widths of 64 / 128 / 256, <= 128 actions, fp32 inference precision), else rlppo_pad_rows + the chain of
 * rlppo_discrete_act: the same numbers, bit for bit.  Outputs: actions (int64; may be pinned host memory, like logp: the kernel
 * stores straight into it), actions_f32 (optional: the index as float, the experience buffer's encoding), logp, rows_out
 * (optional: the padded, standardised rows [n][ld_rows_out] -- the policy-input rows a device-resident rollout stores).
 * workspace: rlppo_discrete_step_workspace_bytes(dims, n_layers, n). */
size_t rlppo_discrete_step_workspace_bytes(const int32_t *dims, int32_t n_layers, int64_t n);
/* 1: rlppo_discrete_step(dims, n rows, opts) runs as the one-launch kernel under the current switches; 0: as the chain; -1: bad argument */
int rlppo_discrete_step_one_launch(const int32_t *dims, int32_t n_layers, int64_t n, const rlppo_act_opts *opts);
int rlppo_discrete_step(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const void *obs, int32_t obs_is_f64,
                        int64_t ld_obs, int64_t n, int32_t standardize, float mean0, float std0, const float *mean_v,
                        const float *std_v, const float *noise_q, int64_t *actions, float *actions_f32, float *logp, float *rows_out,
                        int64_t ld_rows_out, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts);

/* DiscreteFF.get_output (discrete_policy.py:34-42) and the deterministic branch of get_action (:52-57).
 * probs_out (optional): float[n][ld_probs] = softmax of the head (clamp_probs = 0, get_output) or clamp(softmax, 1e-11, 1)
 * (clamp_probs = 1, what get_action works on).  flat_argmax (optional): int64[1] = numpy's argmax over the FLATTENED clamped
 * [n, n_actions] array -- the reference's deterministic action (one index for the whole batch, first occurrence of the maximum;
 * n * n_actions < 2^32).  At least one of the two outputs must be given.  Workspace: rlppo_forward_workspace_bytes. */
int rlppo_discrete_probs(void *stream, const int32_t *dims, int32_t n_layers, const float *packed,
                         const float *obs, int64_t ld_obs, int64_t n, int32_t clamp_probs, float *probs_out,
                         int64_t ld_probs, int64_t *flat_argmax, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts);

/* The selection step alone on caller-supplied probabilities p[n][ld_p] (used by tests to show index equality
 * is exact given identical probs, and by the multi-discrete head with n*8 rows of 3). */
int rlppo_categorical_select(void *stream, const float *probs, int64_t ld_p, int64_t n, int32_t n_cat,
                             const float *noise_q, int64_t *actions, float *logp);

/* ContinuousPolicy.get_action (continuous_policy.py:75-98): tanh head, std = y*var_m + var_b
 * (torch_functions.py:30-33), action = clamp(mean + std*eps, -1, 1) with the caller's N(0,1) noise
 * eps[n][k], logp = sum_k logpdf(action) with the reference's 4-term formula (continuous_policy.py:54-63).
 * dims[n_layers] == 2k, any k >= 1 (above 32 action dimensions the float terms of logp are summed in double, here and in the
 * update's loss kernel).  actions: float[n][k]; logp: float[n]. */
int rlppo_gaussian_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed,
                       const float *obs, int64_t ld_obs, int64_t n, const float *noise_eps, float var_m, float var_b,
                       float *actions, float *logp, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts);

/* [diag] The rollout step of the diagonal-Gaussian head ("[diag]" above): the layer chain with out_tanh = 0, then the sampling kernel.
 * dims[n_layers] == k; noise_eps[n][k] ~ N(0, 1) (the stream ContinuousPolicy draws); log_std: DEVICE, k floats, read when the
 * kernel RUNS -- a changed parameter is seen by the next call, a replay of a captured call included.  actions: float[n][k], not
 * clamped; logp: float[n].  opts as rlppo_gaussian_act: bf16 inference precision and completion words (they ride in the sampling
 * kernel) work, an action mask is refused. */
int rlppo_diag_gaussian_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, const float *obs, int64_t ld_obs,
                            int64_t n, const float *noise_eps, const float *log_std, float *actions, float *logp, void *workspace,
                            size_t ws_bytes, const rlppo_act_opts *opts);

/* MultiDiscreteFF.get_action (multi_discrete_policy.py:46-74, torch_functions.py:93-122): 21 logits -> 8
 * categoricals (5x3 + 3x2); noise_q[n*8][3] as Categorical.sample draws it; actions int64[n][8]; logp[n]. */
int rlppo_multidiscrete_act(void *stream, const int32_t *dims, int32_t n_layers, const float *packed,
                            const float *obs, int64_t ld_obs, int64_t n, const float *noise_q,
                            int64_t *actions, float *logp, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts);
/* [nvec] The same step for MultiDiscrete(nvec) of any nvec -- MultiDiscreteRolv's construction (torch_functions.py:81-122) with the
 * bins as a parameter.  nvec: HOST, n_heads = H entries b_0 .. b_(H-1), read during the call (limits: RLPPO_MD_MAX_*);
 * dims[n_layers] == S = sum b_h.  Head h owns logits [s_h, s_h + b_h), s_h = b_0 + .. + b_(h-1); with B = max b_h the distribution
 * is Categorical(logits = [n, H, B]), every head padded with -inf to B.  noise_q[n * H][B] as Categorical.sample draws it
 * (torch.empty(n * H, B).exponential_(1)); the action of head h is the first arg-max over c < b_h of
 * softmax(z_h)_c / noise_q[(row * H + h) * B + c] -- padded slots are no candidates, their noise is not read; actions int64[n][H];
 * logp[n] = sum_h log_softmax(z_h)[a_h].  A head of one bin: action 0, log-probability 0.  opts as rlppo_multidiscrete_act (bf16
 * inference and completion words work; an action mask is refused).  It always runs the general sampling kernel, also for the
 * reference's nvec {3, 3, 3, 3, 3, 2, 2, 2}, where rlppo_multidiscrete_act keeps its fixed kernel. */
int rlppo_multidiscrete_act_nvec(void *stream, const int32_t *dims, int32_t n_layers, const float *packed,
                                 const float *obs, int64_t ld_obs, int64_t n, const float *noise_q,
                                 int64_t *actions, float *logp, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts,
                                 const int32_t *nvec, int32_t n_heads);
/* [nvec, masked] The same step under an action mask ("[nvec, masked]" above): action_mask DEVICE [n][mask_words] words, one bit per
 * logit, mask_words == ceil(sum(nvec) / 32) (otherwise RLPPO_ERR_ARG naming mask_words and the needed count, before any HIP call);
 * row `row` of the mask belongs to row `row` of obs.  action_mask == NULL is RLPPO_ERR_ARG.  Everything else, opts included, as
 * rlppo_multidiscrete_act_nvec; an all-valid mask gives that entry point's results bit for bit. */
int rlppo_multidiscrete_act_nvec_masked(void *stream, const int32_t *dims, int32_t n_layers, const float *packed,
                                        const float *obs, int64_t ld_obs, int64_t n, const float *noise_q,
                                        int64_t *actions, float *logp, void *workspace, size_t ws_bytes, const rlppo_act_opts *opts,
                                        const int32_t *nvec, int32_t n_heads, const uint32_t *action_mask, int32_t mask_words);

/* ---------------------------------------------------------------------------------------------- GAE */

size_t rlppo_gae_workspace_bytes(int64_t n);

/* compute_gae (util/torch_functions.py:36-78) as two segmented reverse affine scans.
 * rews, dones, truncated: float[n]; values: float[n+1] (V of every state + V(next_state of the last step),
 * learner.py:347-352).  return_std: the running return std (learner.py:356); pass NaN for `None`
 * (no reward scaling).  Outputs float[n]: value_targets = V + adv, advantages, returns.
 * Arithmetic: reward scaling in float32 (as the reference's float32/float32 division), recurrences in
 * float64, outputs rounded once to float32 -- the reference's behaviour under its pinned NumPy < 2.
 * One launch (chunk scans + decoupled look-back; per-launch record tags, so launches on one workspace never interfere); inside
 * a stream capture the stateless two-launch form is used instead.  A look-back wait is bounded: if it ever times out (not
 * expected: a chunk only waits on workgroups dispatched before it) the affected outputs are NaN and word 1 of the workspace
 * (uint32) counts the event -- never a silent wrong result, never a hang. */
int rlppo_gae(void *stream, const float *rews, const float *dones, const float *truncated, const float *values,
              int64_t n, double gamma, double lmbda, float return_std,
              float *value_targets, float *advantages, float *returns, void *workspace, size_t ws_bytes);

/* rlppo_gae with truncated trajectories bootstrapped from V of their OWN next state (time-limit handling as Stable-Baselines3,
 * CleanRL and Gymnasium do it).  Per step t, with nd = 1 - done[t], nt = 1 - truncated[t] (flags exactly 0.0 or 1.0):
 *     vnext            = boot_values[t]   if truncated[t] != 0 and done[t] == 0      (done wins over truncated)
 *                        values[t + 1]    otherwise
 *     delta            = clip(r/sigma) + gamma * vnext * nd - values[t]
 *     adv[t]           = delta + gamma * lambda * nd * nt * adv[t + 1]
 *     value_targets[t] = values[t] + adv[t]
 *     ret[t]           = r[t] + gamma * nd * nt * ret[t + 1]                           (as rlppo_gae: returns are not bootstrapped)
 * boot_values: float[n], 16-byte aligned, USED only at steps that are truncated and not done -- every other entry may hold
 * anything (NaN, uninitialised memory) and never reaches an output (the kernels read the array as a fifth input stream and select
 * by the flags: measured faster than a sparse read behind the flags).  boot_values == NULL is exactly rlppo_gae, launch for launch.
 * Same arithmetic, same workspace (rlppo_gae_workspace_bytes), same forms (one launch; two under stream capture), same bounded
 * look-back wait and timeout word as rlppo_gae. */
int rlppo_gae_boot(void *stream, const float *rews, const float *dones, const float *truncated, const float *values,
                   const float *boot_values, int64_t n, double gamma, double lmbda, float return_std,
                   float *value_targets, float *advantages, float *returns, void *workspace, size_t ws_bytes);

/* [vnorm] rlppo_gae_boot on NORMALISED values (value normalisation: the critic is trained on standardised value targets, so what it
 * puts out is v^ = (V - mu) / sigma).  value_scale: DEVICE float[4] = {mu, 1/sigma, sigma, 0}, 16-byte aligned, as
 * rlppo_value_norm_update publishes it.  Every value the scan reads -- values[t], values[t + 1] and boot_values[t] -- is first taken
 * to real units as V = fmaf(v^, value_scale[2], value_scale[0]): ONE float32 fused multiply-add, spelled out (it does not depend on
 * the build's contraction setting), with the two floats read once per workgroup.  Everything behind it is rlppo_gae_boot: the
 * outputs (value_targets, advantages, returns) are in REAL units.  boot_values may be NULL (the plain scan on normalised values).
 * value_scale == NULL is exactly rlppo_gae_boot, launch for launch, with the kernels it always ran; value_scale = {0, 1, 1, 0} runs
 * the normalised kernels and gives the same bits.  Same workspace, alignment rules, forms (one launch; two under stream capture --
 * a replay reads value_scale as it stands then), bounded look-back wait and timeout word.  A value_scale that is not 16-byte
 * aligned is RLPPO_ERR_ARG before any HIP call. */
int rlppo_gae_norm(void *stream, const float *rews, const float *dones, const float *truncated, const float *values,
                   const float *boot_values, const float *value_scale, int64_t n, double gamma, double lmbda, float return_std,
                   float *value_targets, float *advantages, float *returns, void *workspace, size_t ws_bytes);

/* [vnorm] The running statistic of the value targets, advanced by one batch on the device (rl_games' normalize_value / RunningMeanStd;
 * PopArt's statistic; its weight-preserving step is rlppo_value_norm_update_popart below).  targets: DEVICE float[n].  state: DEVICE double[4] = {count, mean, M2, rejected},
 * 8-byte aligned, zero for a fresh statistic.  scale: DEVICE float[4], 16-byte aligned, what rlppo_gae_norm and
 * rlppo_ppo_minibatch_vnorm read: {mu, 1/sigma, sigma, 0} with sigma = sqrt(M2 / count + 1e-5) (population variance), each entry
 * computed in double and rounded once; the owner of a fresh statistic fills it with {0, 1, 1, 0}.  ONE launch: every workgroup sums
 * (x - x_0) and its square in double, the workgroup that arrives last (an atomic ticket; nobody waits) adds the slots in slot order,
 * forms n_b = n, mean_b, M2_b and merges with Chan's formula
 *     delta = mean_b - mean;  tot = count + n_b;  mean += delta * n_b / tot;  M2 += M2_b + delta^2 * count * n_b / tot
 * and writes scale.  Bit-reproducible, no floating-point atomics.  A batch whose sums are not finite (a NaN or infinite target)
 * leaves state[0..2] and scale as they are and adds 1 to state[3].  ws: RLPPO_VALUE_NORM_WS_BYTES of device memory zeroed once by
 * its owner (every call leaves it armed).  n <= 0, a NULL pointer or a misaligned one is RLPPO_ERR_ARG before any HIP call. */
#define RLPPO_VALUE_NORM_WS_BYTES 4096
int rlppo_value_norm_update(void *stream, const float *targets, int64_t n, double *state, float *scale, void *ws);

/* [vnorm] rlppo_value_norm_update with PopArt's weight-preserving step (van Hasselt et al. 2016; an added entry point, the ABI version
 * stays as it is): the critic's last layer -- w_last: DEVICE float[n_w], b_last: DEVICE float[1], each 4-byte aligned, anywhere inside
 * the critic's flat arena -- is rescaled in the SAME launch, so that the critic's real-unit output is what it was:
 *     sigma_1 v^' + mu_1 = sigma_0 v^ + mu_0     up to the rounding of w', b' and the forward itself.
 * {mu_0, ., sigma_0, .} is `scale` as PUBLISHED before the update -- the floats the last scan and loss read --, read before they are
 * overwritten and widened to double; a fresh statistic has {0, 1, 1, 0} and the formula applies to it as it stands.
 * {mu_1, ., sigma_1, .} are the floats the same launch has just published, widened to double.  With r = sigma_0 / sigma_1 (ONE double
 * division):
 *     w'_i = (float)((double)w_i * r)                                         for each of the n_w weights
 *     b'   = (float)(fma((double)b, sigma_0, mu_0 - mu_1) / sigma_1)
 * every operation spelled out (a double multiplication, one fma, a double subtraction and two double divisions, each rounded to
 * nearest): the build's contraction setting cannot change a bit.  State and scale after the call are, bit for bit, what
 * rlppo_value_norm_update produces from the same state and batch.  A rejected batch (non-finite targets) moves no statistic, stores
 * NOTHING into w_last or b_last and adds 1 to state[3]; the ticket is re-armed on every path.  The last-arriving workgroup does the
 * merge in one thread and the rescale in all 256: no floating-point atomics, no spin-wait, plain vector stores, the same bits every
 * run.  The caller owns what derives from the weights (packed images: rebuild them) and the optimiser's moments (left alone, as in
 * PopArt).  w_last == NULL && b_last == NULL is exactly rlppo_value_norm_update; exactly one of them NULL, n_w < 1 with weights
 * given, or a misaligned pointer is RLPPO_ERR_ARG, naming the argument, before any HIP call. */
int rlppo_value_norm_update_popart(void *stream, const float *targets, int64_t n, double *state, float *scale, void *ws, float *w_last,
                                   int64_t n_w, float *b_last);

/* -------------------------------------------------------------------------------------- PPO update */

size_t rlppo_minibatch_workspace_bytes(const int32_t *pol_dims, int32_t pol_layers, const int32_t *val_dims,
                                       int32_t val_layers, int64_t mb);
size_t rlppo_minibatch_workspace_bytes_for(const int32_t *pol_dims, int32_t pol_layers, const int32_t *val_dims, int32_t val_layers,
                                           int64_t mb, int32_t precision);

typedef struct rlppo_minibatch_args {
    int32_t head;                 /* RLPPO_HEAD_* */
    int32_t pol_layers;
    int32_t val_layers;
    int32_t act_dim;              /* floats per action row in `actions` (1, 8, k) */
    int32_t slot;                 /* 0..RLPPO_MAX_SLOTS-1: minibatches given different slots (and different workspaces) may run
                                     concurrently on library-owned streams; rlppo_ppo_join() makes `stream` wait for all of them */
    int32_t precision;            /* [r5] update precision of THIS call: RLPPO_PRECISION_DEFAULT (0: what rlppo_set_update_precision
                                     chose for the process) or 1 + mode (RLPPO_PRECISION_FP32 / _BF16 / _X3): two learners of one
                                     process may train in different precisions; size the workspace with
                                     rlppo_minibatch_workspace_bytes_for(..., precision) */
    const int32_t *pol_dims;      /* HOST */
    const int32_t *val_dims;      /* HOST */
    const float *pol_packed;
    const float *val_packed;
    const float *pol_packed_r;    /* bf16 update precision only (else NULL): rlppo_net_pack_bf16's images of both networks; in the
                                   * split-bf16 precision (mode 2) pol_wb16 / val_wb16 hold rlppo_net_pack_x3's planes instead */
    const float *val_packed_r;
    const void *pol_wb16;
    const void *val_wb16;
    float *pol_grad;              /* flat arena, accumulated (+=) */
    float *val_grad;
    /* device-resident experience (ExperienceBuffer, experience_buffer.py:42-50), gathered by `idx` */
    const float *states;          /* [N][ld_states], padded rows */
    int64_t ld_states;
    int64_t n_rows;               /* N, the rows the experience arrays hold (ring_cap when they are a ring).  With it known the
                                     first layer's four launches fetch row idx[r] straight from `states` (the gather of
                                     experience_buffer.py:82-87 fused into their load stage); 0 = unknown: the rows
                                     are gathered into the workspace by a pass of their own first */
    const float *actions;         /* [N][act_dim], float-encoded (experience_buffer.py:72) */
    const float *old_logp;        /* [N] */
    const float *targets;         /* [N]  value targets ("values" in the buffer) */
    const float *advantages;      /* [N] */
    const int64_t *idx;           /* [mb] LOGICAL rows of this minibatch (a slice of the epoch's permutation) */
    int64_t mb;                   /* rows in this minibatch */
    int64_t ring_base, ring_cap;  /* the experience arrays as a ring (the FIFO of experience_buffer.py:18-37 without the
                                     torch.cat re-allocation): logical row i is physical row (i + ring_base) mod ring_cap;
                                     ring_cap == 0: plain arrays */
    float clip_range;
    float ent_coef;
    float mb_ratio;               /* mini_batch_size / batch_size (ppo_learner.py:175) */
    float var_m, var_b;           /* gaussian head only */
    double *stats;                /* [RLPPO_N_STATS] device accumulators, += */
    void *workspace;
    size_t ws_bytes;
    /* [ABI 7] options beyond the reference; zero / NULL = the reference's update ("Options beyond the reference") */
    const float *adv_norm;        /* device {mean, scale} of the current batch (rlppo_adv_stats): the surrogate reads
                                     (A - mean) * scale instead of A; NULL = the stored advantages */
    float value_clip;             /* > 0: Stable-Baselines3's clipped value prediction, v_old = fl32(target - A) (the buffer holds
                                     V + A and A), v_pred = v_old + clamp(v - v_old, -c, c), loss (v_pred - target)^2; 0 = off */
    double *kl_slots;             /* this pass's region of rlppo_kl_slots_doubles(mb) doubles: [0] <- workgroups of the policy loss
                                     launch, [1] <- mb_ratio, [2 + w] <- workgroup w's sum of the RLPPO_STAT_KL term (read by
                                     rlppo_kl_gate); NULL = not armed.  Slot 2 + w holds THE double workgroup w adds to
                                     stats[RLPPO_STAT_KL] (its rows' ((ratio - 1) - log ratio) / mb, NOT weighted by mb_ratio), so
                                     the pass's increment of stats[RLPPO_STAT_KL] equals the sum of slots [2, 2 + [0]) up to the order
                                     of the double additions; nothing behind slot 2 + [0] is written; a set stop_word keeps the
                                     pass out of `stats` but not out of the slots */
    const uint32_t *stop_word;    /* device; once non-zero, the pass adds nothing to `stats`; NULL = never */
    /* [ABI 8] invalid-action masking: the discrete head, and the multi-discrete head through rlppo_ppo_minibatch_nvec with md_nvec
     * given (one bit per logit, mask_words == ceil(sum(md_nvec) / 32), in every pass form and update precision: "[nvec, masked]"
     * above); another head, or the multi-discrete head without md_nvec: RLPPO_ERR_ARG.  action_mask: [N][mask_words] words, a
     * buffer field like `actions` (row idx[r] through the ring map), mask_words == ceil(n_actions / 32), encoding as in
     * rlppo_act_opts; NULL = off (the parent's launches).  The loss kernel reads the words ITSELF through idx / ring_base / ring_cap --
     * they do not travel with the minibatch gather, so the workspace of a pass (rlppo_minibatch_workspace_bytes) and its gather
     * launches are those of the unmasked pass in every form.  Loss: log p_a, ratio, surrogate, KL and clip fraction as without a
     * mask on the masked pc; entropy = -sum over valid c of pc_c log pc_c; dL/dz_c = 0 exactly on invalid actions, on valid ones the
     * unmasked chain (softmax Jacobian, the clamp's zero-gradient region, torch.min's tie rule) restricted to the valid set.  A stored
     * action its own mask marks invalid is a caller error: pc_a = 1e-11, zero gradient, finite.  A row without a valid action
     * counts as all-valid. */
    const uint32_t *action_mask;
    int32_t mask_words;
} rlppo_minibatch_args;

#define RLPPO_STAT_ENTROPY 0     /* += entropy of this minibatch (mean over rows)            ppo_learner.py:184 */
#define RLPPO_STAT_KL 1          /* += mean((ratio-1) - log ratio)                            ppo_learner.py:161-162 */
#define RLPPO_STAT_VLOSS 2       /* += mse(v, target)                                         ppo_learner.py:182 */
#define RLPPO_STAT_CLIPFRAC 3    /* += mean(|ratio-1| > clip)                                 ppo_learner.py:165-169 */
#define RLPPO_STAT_PLOSS 4       /* += -mean(min(ratio*A, clamp(ratio)*A))  (diagnostic)      ppo_learner.py:172-174 */
#define RLPPO_STAT_GNORM2_POL 5  /* written by rlppo_clip_adam: squared grad norm, policy */
#define RLPPO_STAT_GNORM2_VAL 6
#define RLPPO_STAT_PASSES 7      /* host side: number of rlppo_ppo_minibatch passes behind the sums (all-reduced with them) */
#define RLPPO_N_STATS 8

#define RLPPO_MAX_SLOTS 8

/* One minibatch of PPOLearner.learn (ppo_learner.py:134-185): value forward, policy forward,
 * get_backprop_data, clipped surrogate + entropy + value losses, both backward passes; gradients are ADDED into
 * pol_grad / val_grad (the reference accumulates over the minibatches of a batch, ppo_learner.py:179-180). */
int rlppo_ppo_minibatch(void *stream, const rlppo_minibatch_args *args);
/* [nvec] The same pass with the multi-discrete head for MultiDiscrete(nvec) of any nvec (an added entry point: the struct and the ABI
 * version stay as they are).  md_nvec: HOST, md_heads = H entries, read during the call (limits: RLPPO_MD_MAX_*).  md_nvec == NULL is
 * exactly rlppo_ppo_minibatch (the reference's head: 21 outputs, act_dim 8, the fixed kernel; md_heads ignored).  Not NULL with
 * RLPPO_HEAD_MULTIDISCRETE: the policy must have sum(md_nvec) outputs and args->act_dim == md_heads, and the loss runs the general
 * kernel -- also when md_nvec holds the reference's bins.  Not NULL with another head: RLPPO_ERR_ARG.  `actions` holds H float-encoded
 * indices per row; log p = sum_h log_softmax(z_h)[a_h], entropy = sum_h H(z_h) averaged over the rows (no division by H),
 * dL/dz per head segment as the reference's head forms it, exactly 0 in the padded columns >= sum(md_nvec).  A head of one bin
 * contributes log-probability 0, entropy 0 and a zero gradient.  A stored index outside [0, md_nvec[h]) is a caller error: it is
 * clamped into the head's range before it indexes anything (the row trains on the nearest valid action; no address outside the row
 * is formed).  The workspace of a pass does not depend on md_nvec.  With md_nvec the pass takes args->action_mask / mask_words
 * ("[nvec, masked]" above): the loss kernel reads row idx[r]'s words through the ring map itself, as the discrete head's does. */
int rlppo_ppo_minibatch_nvec(void *stream, const rlppo_minibatch_args *args, const int32_t *md_nvec, int32_t md_heads);

/* [diag] The same pass with the diagonal-Gaussian head ("[diag]" above; an added entry point: the struct and the ABI version stay as
 * they are).  args->head must be RLPPO_HEAD_DIAG_GAUSSIAN and args->act_dim == pol_dims[pol_layers] == k; var_m / var_b are ignored;
 * an action mask is RLPPO_ERR_ARG.  log_std: DEVICE k floats; log_std_grad: DEVICE k floats, += (one add per element and launch);
 * scratch: DEVICE, 8-byte aligned, rlppo_diag_scratch_bytes(args->mb, k) bytes owned by the caller for the duration of the pass (one
 * region per slot in flight; it needs no initialisation and the pinned rlppo_minibatch_workspace_bytes_for values do not include
 * it).  Every pass form (two streams, paired launches, fused minibatches, ring-mapped buffers, n_rows == 0) and every update
 * precision works as for the other heads: the head math is fp32 on whatever the forward produced.  rlppo_ppo_minibatch and
 * rlppo_ppo_minibatch_nvec answer head 3 with RLPPO_ERR_ARG; every argument check happens before the first HIP call. */
size_t rlppo_diag_scratch_bytes(int64_t mb, int32_t k);
int rlppo_ppo_minibatch_diag(void *stream, const rlppo_minibatch_args *args, const float *log_std, float *log_std_grad, void *scratch,
                             size_t scratch_bytes);

/* [act] The same pass for every head, with the hidden activation of each network (an added entry point: rlppo_minibatch_args and the
 * ABI version stay as they are).  ext == NULL or all-zero is exactly rlppo_ppo_minibatch.  md_nvec / md_heads: as
 * rlppo_ppo_minibatch_nvec's; log_std / log_std_grad / scratch / scratch_bytes: as rlppo_ppo_minibatch_diag's (any of them set = that
 * entry point's checks).  pol_hidden_act / val_hidden_act: RLPPO_ACT_* of every hidden layer of the policy / the critic.  When either
 * is tanh or ELU the pass takes the PLAIN form -- one launch chain per network on rows gathered into the workspace, dX multiplied by
 * f'(h) of the SAVED OUTPUT h (tanh: 1 - h^2; ELU: h > 0 ? 1 : h + 1 -- no pre-activation is stored) -- without ReLU bitmasks, paired
 * launches, the folded value head or the gather-fused first layer; the grouped weight-gradient launch is used as it is.  The
 * workspace is rlppo_minibatch_workspace_bytes_for, unchanged.  tanh / ELU with update precision bf16 or x3 is RLPPO_ERR_ARG (those
 * kernels carry the ReLU bitmask by construction), as is any other activation code; every check comes before the first HIP call. */
typedef struct rlppo_minibatch_ext {
    int32_t pol_hidden_act, val_hidden_act;
    const int32_t *md_nvec;
    int32_t md_heads;
    const float *log_std;
    float *log_std_grad;
    void *scratch;
    size_t scratch_bytes;
} rlppo_minibatch_ext;
int rlppo_ppo_minibatch_ex(void *stream, const rlppo_minibatch_args *args, const rlppo_minibatch_ext *ext);

/* [critic rows] The same pass with a critic that reads a row matrix of its own (asymmetric actor-critic: "privileged observations";
 * an added entry point: the structs and the ABI version stay as they are).  critic->states: DEVICE, 16-byte aligned, [N][ld_states]
 * padded rows -- a buffer field like args->states over the SAME physical rows: row idx[r] through the same ring map, with args->n_rows,
 * ring_base and ring_cap.  critic == NULL or critic->states == NULL is exactly rlppo_ppo_minibatch_ex(stream, args, ext).  Otherwise
 * val_dims[0] is the width of the critic's matrix and may differ from pol_dims[0]; critic->ld_states >= rlppo_padded_width(val_dims[0]),
 * a multiple of 4; columns val_dims[0] .. padded width of every row must be zero, as for args->states.  The workspace is
 * rlppo_minibatch_workspace_bytes_critic (the plan of rlppo_minibatch_workspace_bytes_for + the critic's gathered rows,
 * [mb][padded width of val_dims[0]]); one sized by the other functions is RLPPO_ERR_WORKSPACE.  Every head, mask, hidden activation,
 * slot, ring and n_rows == 0 works as in rlppo_ppo_minibatch_ex, and so do update precisions fp32 and x3; bf16 is RLPPO_ERR_ARG (its
 * gather writes one bf16 image, of the policy's rows).  The pass starts with ONE gather launch for both matrices, or -- gather-fused
 * form, decided as before on both networks' first layers, the critic's on its own ld -- both first layers read through the one row
 * table, each from its own matrix.  It never takes paired launches (a paired layer 0 shares one A operand).  Every argument error
 * is reported before the first HIP call.  rlppo_dbg_counter(15) counts these passes. */
typedef struct rlppo_critic_rows {
    const float *states;
    int64_t ld_states;
} rlppo_critic_rows;
size_t rlppo_minibatch_workspace_bytes_critic(const int32_t *pol_dims, int32_t pol_layers, const int32_t *val_dims, int32_t val_layers,
                                              int64_t mb, int32_t precision);
int rlppo_ppo_minibatch_critic(void *stream, const rlppo_minibatch_args *args, const rlppo_minibatch_ext *ext, const rlppo_critic_rows *critic);

/* [vnorm] The same pass with the critic trained on normalised value targets (an added entry point: the structs and the ABI version stay
 * as they are).  vnorm->scale: DEVICE float[4] = {mu, 1/sigma, sigma, 0}, 16-byte aligned (rlppo_value_norm_update).  vnorm == NULL or
 * vnorm->scale == NULL is exactly rlppo_ppo_minibatch_critic(stream, args, ext, critic).  Otherwise the critic's output v^ is a
 * normalised value and the value loss reads the buffer's real-unit target as t^ = (target - mu) * (1/sigma) -- a float32 subtraction,
 * then a float32 multiplication -- and is (v^ - t^)^2; with args->value_clip > 0 the clipping happens in normalised units around
 * v^_old = (fl32(target - A) - mu) * (1/sigma), the rest as in rlppo_ppo_minibatch.  RLPPO_STAT_VLOSS is then in normalised units.
 * Nothing else of the pass changes: the same workspace, the same launches, every head, mask, hidden activation, precision (the value
 * loss is fp32 on whatever the forward produced), critic rows, slot and ring as before. */
typedef struct rlppo_value_norm {
    const float *scale;
} rlppo_value_norm;
int rlppo_ppo_minibatch_vnorm(void *stream, const rlppo_minibatch_args *args, const rlppo_minibatch_ext *ext, const rlppo_critic_rows *critic,
                              const rlppo_value_norm *vnorm);

/* Orders `stream` after every minibatch enqueued through non-zero slots since the last join (call it before the
 * gradient all-reduce / rlppo_clip_adam).  Independent minibatches of one batch only meet in the gradient arena
 * (one add per element and launch), so they may overlap; each launch is short (50-100 us at 65,536 rows), and overlapping
 * chains fill the CUs that one chain's ramp-up and tail leave idle. */
int rlppo_ppo_join(void *stream);

/* [ABI 7] rlppo_minibatch_args.kl_slots: doubles one pass of `mb` rows needs (the policy loss launch's widest grid + 2). */
int64_t rlppo_kl_slots_doubles(int64_t mb);

/* [ABI 7] Advantage normalisation of one batch (Stable-Baselines3's normalize_advantage, over the ref's batch = one optimiser step):
 * out[0] <- mean, out[1] <- 1 / (std + 1e-8) of advantages[idx[0 .. n)] (logical rows mapped through the ring as in
 * rlppo_ppo_minibatch), std the unbiased (n - 1) deviation; n == 1: out = {0, 1} (the row is used as it is).  One launch: sums of
 * (A - A_first) and its square in double per workgroup, the last arriving workgroup adds the slots in a fixed order
 * (bit-reproducible; a constant batch gives exactly mean = A, scale * (A - mean) = 0).  ws: RLPPO_ADV_STATS_WS_BYTES of device
 * memory zeroed once by its owner (every call leaves it armed). */
#define RLPPO_ADV_STATS_WS_BYTES 4096
int rlppo_adv_stats(void *stream, const int64_t *idx, int64_t n, const float *advantages, int64_t ring_base, int64_t ring_cap,
                    float *out, void *ws);

/* [ABI 7] The target-KL gate of one optimiser step.  KL_b = sum over the batch's passes of mb_ratio x (sum of the pass's
 * kl_slots), added in a fixed order (bit-reproducible).
 *   phase 0 (one rank): decide from KL_b;
 *   phase 1 (several ranks, before the gradient exchange): write KL_b as two floats hi + lo to exchange[0..1], no decision;
 *   phase 2 (after the exchange): decide from (double)exchange[0] + (double)exchange[1], the sum over the ranks.
 * Deciding: if *stop_word == 0 and KL_b > threshold, *stop_word <- batch + 1 (it is never cleared by the call).  Phases 0 and 2
 * then store *stop_word to host_words[0] and done_value to host_words[1], with release semantics at system scope
 * (rlppo_host_wait_words polls it).  host_words is HOST-VISIBLE (pinned) memory.  The optimiser step of the batch passes the same
 * stop word as rlppo_opt_net.skip_word. */
typedef struct rlppo_kl_gate_args {
    const double *kl_slots;   /* the batch's pass regions, one every slot_stride doubles */
    int64_t slot_stride;
    int32_t n_passes;
    int32_t phase;
    double threshold;         /* 1.5 x target_kl */
    float *exchange;
    uint32_t *stop_word;      /* device */
    uint32_t batch;
    uint32_t *host_words;     /* pinned [2] */
    uint32_t done_value;
} rlppo_kl_gate_args;
int rlppo_kl_gate(void *stream, const rlppo_kl_gate_args *args);

/* clip_grad_norm_(max_norm) + torch.optim.Adam.step() on one flat arena (ppo_learner.py:187-193).
 * Hyper-parameters are doubles (python floats in the reference); `step` is the 1-based Adam step count of
 * THIS update; the bias corrections lr/(1-beta1^t), sqrt(1-beta2^t) are formed in double and cast to fp32 where
 * they meet tensor data, as torch/optim/adam.py does.  gnorm2: device double that receives the squared gradient
 * norm before clipping.  grads are scaled in place by the clip coefficient, as clip_grad_norm_ does. */
int rlppo_clip_adam(void *stream, float *params, float *grads, float *exp_avg, float *exp_avg_sq, int64_t n,
                    double max_norm, double lr, double beta1, double beta2, double eps, int64_t step,
                    double *gnorm2);

/* The optimiser tail of one batch for BOTH networks in ONE launch (ppo_learner.py:187-193: clip_grad_norm_ x2,
 * value_optimizer.step(), policy_optimizer.step()) + the re-packing rlppo_net_pack would do + the zero_grad of the next batch
 * (ppo_learner.py:135-136): squared norms of both gradient arenas, then clip + Adam on both, every updated parameter written
 * straight into its W / W^T / b slots of `packed` (which must already hold a full rlppo_net_pack image: the zero padding is not
 * rewritten), gradients left ZERO.  Element for element the arithmetic of rlppo_clip_adam + rlppo_net_pack.  Used by
 * PPOLearner.learn; FusedAdam.step() (the public optimiser API, gradients scaled in place) stays on rlppo_clip_adam.
 * sync_ws: RLPPO_OPT_SYNC_BYTES of device memory, 16-byte aligned, owned by the caller and ZEROED ONCE when it is allocated
 * (never again: every completed call leaves it armed for the next): the state of
 * the grid barrier between the norm and the update (arrival counter, generation word, one partial-sum slot per workgroup, added
 * in a fixed order: the norm is bit-reproducible), and at byte offset 8 a uint32 that counts barrier waits that gave up.
 * Giving up is all or nothing: NO element of either network is then touched by that call (parameters, moments, gradients and
 * `packed` stay as they were), the block is dead -- every later call on it skips its update at once and counts itself --
 * until the caller has zeroed it again; callers read the word back with their report and can repeat the step with
 * sync_ws == NULL.  The grid is clamped to what the device keeps resident (a device too small for one workgroup per network
 * takes the three-operation form by itself).  Not shareable between concurrent calls.  sync_ws == NULL selects the
 * three-operation form (fill, norms, update). */
#define RLPPO_OPT_SYNC_BYTES 16384
typedef struct rlppo_opt_net {
    const int32_t *dims;  /* layer widths, n_layers + 1 entries */
    int32_t n_layers;
    float *params, *grads, *exp_avg, *exp_avg_sq; /* flat arenas, rlppo_flat_floats entries */
    float *packed;        /* rlppo_packed_floats entries */
    double *gnorm2;       /* receives the squared gradient norm before clipping */
    double max_norm, lr, beta1, beta2, eps;
    int64_t step;         /* 1-based Adam step count of THIS update */
    const uint32_t *skip_word;  /* [ABI 7] device; non-zero when the call runs: it touches no parameter, moment or packed image of
                                   this network (both forms; rlppo_kl_gate's stop word); NULL = never skip */
} rlppo_opt_net;
int rlppo_clip_adam_pack2(void *stream, const rlppo_opt_net *a, const rlppo_opt_net *b, void *sync_ws);
/* [diag] The same call for networks that carry a parameter TAIL: params / grads / exp_avg / exp_avg_sq of network a hold
 * rlppo_flat_floats(dims) + tail_a floats (b: tail_b), the tail behind the last bias (the diagonal-Gaussian head's log_std; any
 * later parameter that is not a layer).  Tail elements are part of that network's squared norm (clipped under the SAME norm, as
 * Stable-Baselines3 and CleanRL clip the whole policy together), updated by Adam, their gradients zeroed, they respect skip_word
 * and the all-or-nothing give-up -- and are never written into `packed`.  Both forms (one launch with the grid barrier; three
 * operations with sync_ws == NULL).  tail_a == tail_b == 0 is rlppo_clip_adam_pack2, launch for launch and bit for bit. */
int rlppo_clip_adam_pack2_tail(void *stream, const rlppo_opt_net *a, const rlppo_opt_net *b, void *sync_ws, int64_t tail_a, int64_t tail_b);

/* [lr] A learning rate that lives on the device: the KL-adaptive schedule of rsl_rl / rl_games ("adaptive"), decided by the gate and
 * read by the optimiser step without the host in between (added entry points: rlppo_kl_gate_lr, rlppo_clip_adam_pack2_lr; no struct
 * of an existing entry point changes, the ABI version stays 8).
 *
 * rlppo_kl_gate_lr is rlppo_kl_gate -- the same three phases, the same fixed-order sum KL_b -- plus the rate rule.  Phase 1 writes
 * the exchange words and nothing else.  Phases 0 and 2, in this order:
 *   1. the stop decision of rlppo_kl_gate, when args->stop_word is not NULL (threshold, batch as there);
 *   2. *kl_out <- KL_b (when kl_out is not NULL);
 *   3. when no stop word is given or it is 0 AFTER step 1 (a gate that stops the run moves no rate), for each of the n_lr adjacent
 *      doubles lr[i], in double:
 *          KL_b > 2 desired_kl         lr[i] <- max(lr_min, lr[i] / factor)
 *          0 < KL_b < desired_kl / 2   lr[i] <- min(lr_max, lr[i] * factor)
 *          otherwise                   unchanged
 *      Both inequalities are strict; KL_b == 0, KL_b exactly on a threshold and a NaN KL_b change nothing.  Every rate is compared,
 *      moved and clamped on its own.  KL_b is the SAMPLE estimate mean((ratio - 1) - log ratio) every head's loss launch writes, not
 *      rsl_rl's analytic Gaussian KL;
 *   4. the host words of rlppo_kl_gate, when args->host_words is not NULL.
 * args->stop_word and args->host_words may both be NULL (the schedule without target_kl): the call then writes device memory only.
 * 1 <= n_lr <= RLPPO_LR_MAX_RATES, desired_kl > 0, factor > 1, 0 < lr_min <= lr_max, all finite.
 *
 * rlppo_clip_adam_pack2_lr is rlppo_clip_adam_pack2_tail whose networks may take their rate from a device double: a non-NULL lr_a
 * replaces a->lr (lr_b: b->lr).  The kernel forms step_size = (float)(*lr / bc1) with bc1 = 1 - beta1^step passed in as the host's
 * double: the value the host forms for the same rate, bit for bit (IEEE double division, one rounding to float).  The rate is read
 * after the grid barrier (one-launch form: once per workgroup; three-operation form: once per thread of the update launch), so the
 * writer is any launch earlier on the stream -- the gate of the same batch.  The call never writes a rate: a step that is skipped
 * (skip_word) or gives up leaves the rates as the gate set them.  Barrier protocol, give-up rule, skip_word, tails and both forms
 * (sync_ws == NULL: three operations) are those of rlppo_clip_adam_pack2_tail; lr_a == lr_b == NULL is that call, launch for
 * launch and bit for bit. */
#define RLPPO_LR_MAX_RATES 8
typedef struct rlppo_lr_adapt_args {
    double *lr;          /* device: n_lr adjacent rates */
    int32_t n_lr;
    double desired_kl;
    double factor;       /* 1.5 in rsl_rl */
    double lr_min, lr_max;
    double *kl_out;      /* device, optional: receives KL_b (phases 0 and 2) */
} rlppo_lr_adapt_args;
int rlppo_kl_gate_lr(void *stream, const rlppo_kl_gate_args *args, const rlppo_lr_adapt_args *lr);
int rlppo_clip_adam_pack2_lr(void *stream, const rlppo_opt_net *a, const rlppo_opt_net *b, void *sync_ws, int64_t tail_a, int64_t tail_b,
                             const double *lr_a, const double *lr_b);

/* [r6] The tail of PPOLearner.learn in ONE launch (ppo_learner.py:213-234: the update magnitudes ||theta_before - theta_after||_2 of
 * both networks, the report means' sums read out, one device -> host synchronisation): round 5 spent ten dependent eager launches
 * and a blocking copy here, 0.1 ms of a 3 ms learn() at the reference's own batch size.  The kernel
 *   - adds add_passes to stats[RLPPO_STAT_PASSES], copies the RLPPO_N_STATS accumulators to out[0 .. RLPPO_N_STATS) and ZEROES them
 *     (the next learn() starts from clean sums without a fill of its own);
 *   - out[RLPPO_N_STATS], out[RLPPO_N_STATS + 1] <- sqrt(sum (before_i - now_i)^2) of the policy / the critic: float32 differences as
 *     the reference forms them, squares and sums in double, partial sums added in a fixed order (bit-reproducible);
 *   - out[RLPPO_N_STATS + 2] <- *timeout_word (the give-up counter of rlppo_clip_adam_pack2's sync block; 0 when NULL),
 *     out[RLPPO_N_STATS + 3] <- *extra (a device double the caller wants back with the report -- the give-up count summed over the
 *     ranks of a data-parallel run; out[RLPPO_N_STATS + 2] again when NULL);
 *   - then stores done_value into *done_word with release semantics at system scope (rlppo_host_wait_words polls it).
 * `out` and `done_word` are HOST-VISIBLE (pinned) memory; ws: RLPPO_REPORT_WS_BYTES of device memory owned by the caller, zeroed
 * once when it is allocated (arrival counter + one partial-sum slot per workgroup; every call leaves it armed for the next). */
#define RLPPO_REPORT_WS_BYTES 4096
#define RLPPO_REPORT_OUT_DOUBLES (RLPPO_N_STATS + 4)
typedef struct rlppo_report_args {
    const float *pol_before, *pol_now;
    int64_t n_pol;
    const float *val_before, *val_now;
    int64_t n_val;
    double *stats;
    double add_passes;
    const uint32_t *timeout_word;
    const double *extra;
    double *out;
    uint32_t *done_word;
    uint32_t done_value;
    void *ws;
} rlppo_report_args;
int rlppo_learn_report(void *stream, const rlppo_report_args *args);

/* ---------------------------------------------------------------------------- process-mode collection (host only) */

/* [r6] The learner-side loop of the reference's process-per-environment collection (rlgym_ppo/batched_agents/
 * batched_agent_manager.py:126-350, batched_trajectory.py:58-105) as host C++ behind the SAME wire format (UDP headers of three magic
 * floats + one slab per worker of a shared float32 array: rlgym_ppo_amd/batched_agents/comm_consts.py): wait for the ready sockets,
 * read the datagram, parse the slab, advance the observation statistics (Welford, in the state's dtype and the reference's operation
 * order), standardise, keep the episode-reward bookkeeping, bank the timestep into the environment's trajectory, and lay the
 * trajectories out agent by agent at the end of a collect_timesteps call (last step force-marked truncated unless done: quirk Q4).
 * The policy call stays with the host; one inference is  _ready -> [policy.get_action] -> _send -> _collect.  All pointers HOST.
 *   create: socket_fds[i] = the learner's UDP socket of worker i (owned by the caller), peer_ports[i] = that worker's port on
 *     127.0.0.1, shm_base + i * shm_floats_per_worker = its slab.
 *   set_obs: current_obs[worker] <- rows x obs_dim floats (a reset state, as received: not standardised), ready != 0: the worker
 *     waits for actions.
 *   ready: the stacked observations of the workers waiting for actions (at most cap_rows rows) -> n_rows.
 *   send: actions[n_rows][act_width] float32 and log_probs[n_rows] for exactly those rows: recorded, and sent to the workers.
 *   collect: blocks until messages worth >= min_obs agent-steps have been banked (a message counts its prev_n_agents) -> n_collected;
 *     a signal makes it return RLPPO_ERR_INTERRUPTED with the progress so far (the host's handlers run; resume = 1 continues the wait);
 *     standardize 0 = off, 1 = (x - mean[0]) / std[0] clipped to +-5 (the reference's scalars, quirk Q5), 2 = per feature;
 *     stats_mean / stats_var / stats_count / steps_since_increment: the WelfordRunningStat's state (float32 arrays; float64 when
 *     stats_f64 -- statistics restored from JSON -- and then mean / std are doubles too and the standardisation is formed in float64
 *     and rounded once, as numpy does) and the manager's cadence counter, advanced in place every steps_per_increment-th message with
 *     the RAW rows.
 *   finish: flushes every trajectory -> the sizes _emit needs; emit: states / next_states [n][obs_dim], actions [n][act_width],
 *     log_probs [n] float32, rewards / dones / truncated [n] float64 (the dtypes the reference's lists become), and every message's
 *     metrics record (values flat; 9 ints per record: rank, dimensions).
 *   average_reward: get (set == 0) / set the manager's running average (is_none: it has not seen an episode end yet).
 * Masked runs (the workers' environments have action_masks(): the opt-in mask trailer of comm_consts.py, n_agents x n_actions
 * floats of 0 / 1 behind every observation).  Masks cross this boundary as BYTES, one per action, 0 = invalid (the host packs them
 * to the kernels' words where it stages them for a launch: util/action_mask.py):
 *   set_masked: once, before the first _collect: every slab carries the trailer for n_actions actions.
 *   set_mask_heads: a multi-discrete run ("[nvec, masked]" above), after set_masked(S): the masks have one byte per LOGIT,
 *     S = sum(nvec), head h owning bytes [s_h, s_h + nvec[h]); RLPPO_ERR_ARG unless nvec sums to the mask width.  Without the call
 *     the S bytes of a row are one head (the discrete head).
 *   set_mask: the mask [rows][n_actions] of the observation last given to set_obs for that worker.
 *   ready_masks: after _ready, the mask rows of exactly that batch, row for row with its observations; RLPPO_ERR_MASK_ROW (the
 *     text names worker and agent) when a row has no valid action -- with set_mask_heads: when a HEAD of a row has no valid bin,
 *     the text naming worker, agent and head -- nothing has been sent for the batch at that point.
 *   emit_masks: between _finish and _emit, the masks the actions were sampled under, [n_steps][n_actions], row for row with
 *     _emit's states. */
int rlppo_collector_create(int32_t n_workers, const int32_t *socket_fds, const int32_t *peer_ports, const float *shm_base,
                           int64_t shm_floats_per_worker, int32_t obs_dim, void **handle);
int rlppo_collector_destroy(void *handle);
int rlppo_collector_set_obs(void *handle, int32_t worker, const float *obs, int32_t rows, int32_t ready);
int rlppo_collector_ready(void *handle, float *obs_out, int64_t cap_rows, int64_t *n_rows);
int rlppo_collector_send(void *handle, const float *actions, int32_t act_width, const float *log_probs);
int rlppo_collector_collect(void *handle, int64_t min_obs, int32_t resume, int32_t standardize, const void *mean, const void *stdv, void *stats_mean,
                            void *stats_var, int64_t *stats_count, int32_t stats_f64, int64_t steps_per_increment, int64_t *steps_since_increment,
                            int64_t *n_collected);
int rlppo_collector_finish(void *handle, int64_t *n_steps, int32_t *act_width, int64_t *n_metrics, int64_t *metrics_floats);
int rlppo_collector_emit(void *handle, float *states, float *actions, float *log_probs, double *rewards, float *next_states, double *dones,
                         double *truncated, float *metrics_values, int32_t *metrics_shapes);
int rlppo_collector_average_reward(void *handle, int32_t set, double *value, int32_t *is_none);
int rlppo_collector_set_masked(void *handle, int32_t n_actions);
int rlppo_collector_set_mask(void *handle, int32_t worker, const uint8_t *mask, int32_t rows);
int rlppo_collector_ready_masks(void *handle, uint8_t *mask_out, int64_t cap_rows);
int rlppo_collector_emit_masks(void *handle, uint8_t *masks);
int rlppo_collector_set_mask_heads(void *handle, const int32_t *nvec, int32_t n_heads);

/* ------------------------------------------------------------------------------------- data-parallel exchange */

/* The one exchange step of the path: an in-place sum over the ranks of the flat
 * [grad_policy | grad_value] arena, after a rank's last backward of a batch and before clip_grad_norm_ / Adam, which then
 * run replicated (ppo_learner.py:187-193 sees the reduced gradients).  The reference is single-device and has no
 * counterpart.  RCCL is loaded at run time (rlppo_comm_set_library(path) to name a particular librccl.so, e.g. PyTorch's
 * own copy; default: the loader's "librccl.so").  One communicator per process (one process per GPU): rank 0 obtains
 * the 128-byte id with rlppo_comm_unique_id and hands it to the other ranks by any host channel; every rank then calls
 * rlppo_comm_init on the thread whose current device is its GPU.  rlppo_allreduce enqueues ncclAllReduce(sum) on the
 * caller's stream (fp32, or fp64 for the report statistics) and returns without synchronising.  Errors: 2000 + ncclResult_t.
 * rlgym_ppo_amd/dp.py uses these when RLPPO_RCCL_DIRECT=1 and torch.distributed's all_reduce otherwise. */
#define RLPPO_COMM_ID_BYTES 128
int rlppo_comm_set_library(const char *path);
int rlppo_comm_unique_id(void *id128);
int rlppo_comm_init(int32_t rank, int32_t world, const void *id128);
int rlppo_allreduce(void *stream, void *buf, int64_t n, int32_t is_f64);
int rlppo_comm_destroy(void);

/* ----------------------------------------------------------------------------------------- host helpers */

/* numpy.random.RandomState legacy stream (MT19937 + masked rejection + reverse Fisher-Yates): the index stream
 * of ExperienceBuffer.get_all_batches_shuffled (experience_buffer.py:52,97-98).  HOST code, HOST pointers.
 * state: 625 uint32 (624 words of key + position), as numpy's get_state() exposes it. */
int rlppo_mt19937_seed(uint32_t *state625, uint32_t seed);
int rlppo_mt19937_permutation(uint32_t *state625, int64_t n, int64_t *out);
/* The same permutation in two phases (same stream consumption, same result).  draw_targets: the serial phase -- advances
 * the generator exactly as rlppo_mt19937_permutation(n) does and records the n-1 swap targets of numpy's reverse
 * Fisher-Yates loop (mtrand.pyx _shuffle_raw) in draw order: targets[t] = j_i for i = n-1-t.  apply_swap_targets: applies
 * those swaps to arange(n); no generator state, so it can run on another thread while the next epoch is being drawn
 * (the shuffle of experience_buffer.py:97-98 is the serial host work of an epoch once 8 ranks share the GPU work). */
int rlppo_mt19937_draw_targets(uint32_t *state625, int64_t n, uint32_t *targets);
int rlppo_apply_swap_targets(int64_t n, const uint32_t *targets, int64_t *out);

/* torch.empty(n).exponential_(lambda) of PyTorch's CPU generator, bit for bit: the Exp(1) noise torch.multinomial(probs, 1,
 * True) / Categorical.sample() consume in the reference's rollout (discrete_policy.py:59), i.e. the stream
 * that makes a seeded run pick the reference's action indices.  HOST code, HOST pointers.  `state`: the generator's serialised
 * state as torch.get_rng_state() returns it (5056 bytes), advanced in place exactly as torch advances it (2 n MT19937 words).
 * The serial MT19937 phase is vectorised and the double-precision log1p transform runs on `threads` threads: 4096 x 90 values
 * in ~0.5 ms instead of the ~4.7 ms of torch's serial kernel. */
int rlppo_torch_cpu_exponential(void *state, int64_t state_bytes, int64_t n, double lambda, float *out, int32_t threads);
/* The same draw in two calls, for callers that pipeline consecutive draws (the stream phase of the next draw needs only the state
 * this one's stream phase leaves behind): _words fills words[2 n + 8] with the tempered MT19937 words and advances `state` exactly as
 * the one-call form does; rlppo_exponential_from_words turns them into the identical n float32 values (no generator involved: any
 * thread). */
int rlppo_torch_cpu_exponential_words(void *state, int64_t state_bytes, int64_t n, uint32_t *words);
int rlppo_exponential_from_words(const uint32_t *words, int64_t n, double lambda, float *out);
/* One draw as one call that chains itself to its predecessor on another thread: link blocks are { int32 ready; padding to 64 bytes;
 * the generator state (state_bytes) }.  The call waits (spinning, in C) until `link_in` -- the block its predecessor publishes as soon
 * as that call's STREAM phase is done -- is ready (link_in == NULL: starts from `state`, which is not modified), runs its stream phase,
 * publishes `link_out` (zero its first word beforehand) and then transforms into `out`; `words` is scratch of 2 n + 8 uint32.  The state
 * after the draw is link_out's.  Values and states are those of rlppo_torch_cpu_exponential. */
#define RLPPO_EXP_LINK_HEADER 64
int rlppo_torch_cpu_exponential_chained(const void *state, int64_t state_bytes, int64_t n, double lambda, float *out, uint32_t *words,
                                        void *link_in, void *link_out);
/* [r4] A run of chained draws on the calling thread: of a burst of `count` consecutive draws of n values each, the draws first,
 * first + step, ... (`step` threads share a burst, one call each, first = 0 .. step - 1).  Draw i writes out + i * out_stride floats
 * and publishes the link block links + i * link_stride bytes, laid out as above with one more word: { int32 ready; int32 done
 * (1: the values are complete; -1: failed or cancelled); padding to 64 bytes; state }; zero the first 8 bytes of every block
 * beforehand.  Draw 0 starts from `state` (not modified), or from `link_in0` -- the block an earlier chained call publishes -- when
 * that is not NULL.  `cancel`: caller-owned int32 read before every draw; non-zero ends the run (remaining draws marked failed).
 * Values and states are those of `count` consecutive rlppo_torch_cpu_exponential calls.  (engine.HostExponential.prefetch: the
 * next rollout's noise, drawn while PPOLearner.learn runs -- learner.py:257-270, discrete_policy.py:59.) */
int rlppo_torch_cpu_exponential_burst(const void *state, void *link_in0, int64_t state_bytes, int64_t n, double lambda, float *out,
                                      int64_t out_stride, void *links, int64_t link_stride, int32_t first, int32_t step, int32_t count,
                                      const int32_t *cancel);

/* dst[r][0..width) = src[idx[r]][0..width), fp32 rows, 16 bytes per thread (width, ld_src multiples of 4; dst rows are
 * `width` floats apart).  The minibatch gather of experience_buffer.py:82-87 (used inside rlppo_ppo_minibatch) and the
 * step-major -> trajectory-major flatten of a device-resident rollout (batched_agent_manager.py:154-172 builds the same
 * order with Python lists). */
int rlppo_gather_rows(void *stream, const float *src, int64_t ld_src, const int64_t *idx, float *dst, int32_t width, int64_t n);
/* [critic rows] The gather launch of a pass with separate critic rows, on its own: for r < n, with s = the physical row of idx[r]
 * (ring_cap == 0: s = idx[r]; else (idx[r] + ring_base) mod ring_cap), dst[r][0..width) = src[s][0..width) and
 * critic_dst[r][0..critic_width) = critic_src[s][0..critic_width) in ONE launch (16 bytes per thread; widths and lds multiples of
 * 4, the four matrices 16-byte aligned, dst rows `width` / `critic_width` floats apart).  The per-row scalars ride along when given
 * (all of them or none): g_old[r] = old_logp[s], g_adv[r] = advantages[s], g_tgt[r] = targets[s], g_act[r][0..act_dim) =
 * actions[s][0..act_dim), and zero_n[r] = 0 when zero_n is given. */
typedef struct rlppo_gather2_args {
    const float *src;
    int64_t ld_src;
    float *dst;
    int32_t width;
    const float *critic_src;
    int64_t critic_ld_src;
    float *critic_dst;
    int32_t critic_width;
    const int64_t *idx;
    int64_t n;
    int64_t ring_base, ring_cap;
    const float *actions, *old_logp, *advantages, *targets;
    int32_t act_dim;
    float *g_act, *g_old, *g_adv, *g_tgt, *zero_n;
} rlppo_gather2_args;
int rlppo_gather_rows2(void *stream, const rlppo_gather2_args *args);

/* WelfordRunningStat.increment(samples, n) (running_stats.py:28-46) on the device, bit-exact with the reference's sample-by-
 * sample update: mean[d], m2[d] (= running_mean, running_variance) are updated in place with the n rows of `samples` (fp32,
 * row stride ld floats); `count` is the number of samples already absorbed (the caller adds n afterwards).  The state is
 * float32 as the class constructs it, or float64 (state_is_f64 != 0) as WelfordRunningStat.from_json leaves it after a
 * checkpoint load (running_stats.py:121-125: np.asarray of Python floats) -- the reference then updates in float64. */
int rlppo_welford_increment(void *stream, const float *samples, int64_t ld, int64_t n, int32_t d, void *mean, void *m2,
                            int64_t count, int32_t state_is_f64);
/* WelfordRunningStat.increment_from_serialized_other (running_stats.py:71-98): combine the running statistics of another
 * instance (other_mean[d], other_m2[d] fp32 -- the reference casts the serialised list to float32 -- and other_count) into
 * mean / m2 in place, in the reference's operation order; the caller sets count += other_count.  SURVEY.md 8(f) row 4. */
int rlppo_welford_merge(void *stream, int32_t d, void *mean, void *m2, int64_t count, const float *other_mean,
                        const float *other_m2, int64_t other_count, int32_t state_is_f64);

/* ------------------------------------------------------------------- device-resident vector environments (csrc/rollout.hip)
 * The bookkeeping between two steps of an environment that lives on the GPU (batched_agents/vector_agent_manager.py,
 * the _DeviceEnv side of the collect loop).  The three entry points below make LAUNCHES ONLY: none of them contains a stream synchronisation, a blocking
 * copy or an allocation, so a host that enqueues a whole collect through them never waits for the device. */
#define RLPPO_DT_F32 0
#define RLPPO_DT_F64 1
#define RLPPO_DT_U8 2   /* one byte per entry: bool / uint8 */
/* One environment step's rewards / dones / truncated (device arrays of n_agents entries; a dtype code each; rewards float32 or
 * float64; the flags are zero / non-zero; truncated may be NULL = all zero) enter
 *   rdt[3][T][n_agents] (float32, time-major planes rewards / dones / truncated) at step t: r rounded ONCE to float32, the flags as
 *     exact 0.0 / 1.0; at t == T - 1 the truncated plane takes the flush rule instead (1 where done == 0, else 0: quirk Q4,
 *     batched_agent_manager.py:154-172) -- the bookkeeping below has used the environment's own flags by then;
 *   ep_sums[n_agents] (double): += (double)(float)r;
 *   state (int64[3]: the bits of the double average, a has-value word, the ended-episode counter): every agent with done or
 *     truncated set BY THE ENVIRONMENT'S FLAGS is folded into the average IN AGENT ORDER with the reference's operations
 *     (batched_agent_manager.py:377-399): the first episode ever sets avg = x, after that avg = avg * 0.9 + x * 0.1 -- two double
 *     multiplications and one addition, never contracted -- where x is the agent's episode sum including this step; its sum is
 *     then zeroed and the counter advanced;
 *   patch (optional, float32[n_agents], this step's row of a patch plane): 1.0 where the environment truncated and did not
 *     terminate the episode (the steps whose next-state row is the final observation), else 0.0.
 * One workgroup; the ended agents of a 1024-agent chunk are compacted in agent order and folded by one thread: the cost of a
 * step on which every agent ends is n_agents dependent double multiply-adds (DESIGN.md section 8b has the measurement). */
int rlppo_rollout_record(void *stream, const void *rewards, int32_t rewards_dt, const void *dones, int32_t dones_dt, const void *truncated,
                         int32_t truncated_dt, int64_t n_agents, int64_t t, int64_t T, float *rdt, double *ep_sums, void *state,
                         float *patch);
/* WelfordRunningStat.mean / .std (running_stats.py:100-117) of a device-resident state (mean[d], m2[d] in the state's dtype, as
 * rlppo_welford_increment keeps them) for the HOST-KNOWN sample count, as the float32 vectors mean_v[d] / std_v[d] that mode 2 of
 * rlppo_discrete_step and rlppo_pad_rows_per_feature read: count < 2 gives 0 / 1; else var = m2 / (count - 1) in the state's dtype,
 * 1 where var == 0, the IEEE square root, one rounding to float32.  per_feature == 0: every entry holds feature 0's pair (the
 * reference's scalar standardisation, quirk Q5); else each its own. */
int rlppo_obs_scalars(void *stream, const void *mean, const void *m2, int32_t state_is_f64, int64_t count, int32_t d, int32_t per_feature,
                      float *mean_v, float *std_v);
/* Time-major rollout storage -> the reference's trajectory-major arrays (row a * T + t of agent a, batched_trajectory.py:58-105), one
 * launch that reads the storage once.  In: S[T + 1][n_agents][ld] policy-input rows (ld a multiple of 4, rows 16-byte aligned),
 * acts[T][n_agents][k], logp[T][n_agents], rdt[3][T][n_agents].  Out (N = n_agents * T): flat[N + 1][ld] -- S[t][a] at a * T + t,
 * flat[N] = S[T][n_agents - 1] --, nxt[N][ld] -- S[t][a] at a * T + t - 1 for t >= 1 --, actions[N][k], log_probs / rewards / dones /
 * truncated[N].  patch[T][n_agents] with final_rows[T][n_agents][ld] (both or neither): where patch[t][a] != 0 the next-state row
 * of step t of agent a is final_rows[t][a] instead. */
int rlppo_rollout_to_trajectory_major(void *stream, const float *S, const float *acts, const float *logp, const float *rdt, int64_t n_agents,
                                      int64_t T, int32_t ld, int32_t k, const float *patch, const float *final_rows, float *flat, float *nxt,
                                      float *actions, float *log_probs, float *rewards, float *dones, float *truncated);

/* Precision of the ROLLOUT forward passes (rlppo_mlp_forward, rlppo_*_act): 0 = fp32 (default; the parity mode),
 * 1 = activations and master weights rounded to bf16 as MFMA operands, fp32 accumulation / bias / activation
 * (BASELINE configs[4] "bf16 fwd / fp32 master weights").  The update has its own switch (rlppo_set_update_precision).  The reference
 * has no such mode (it is fp32 throughout): outputs then agree with an fp32 forward to ~1e-2, not 1e-5. */
int rlppo_set_inference_precision(int32_t mode);

/* Precision of the PPO UPDATE (rlppo_ppo_minibatch): 0 = fp32 (default; the parity mode: fp32 losses/grads within 1e-5 of the
 * reference), 2 = fp32 with split-bf16 hidden products (below), 1 = BASELINE configs[4] "bf16 fwd / fp32 master weights" = mixed-precision training as torch writes it:
 *   - every forward product of both networks multiplies bf16-rounded operands (activations and weights, round-to-nearest-even)
 *     on the bf16 MFMA pipe and accumulates in fp32; bias and activation in fp32; the hidden activations are stored as bf16;
 *   - the gradient with respect to each hidden activation is therefore a bf16 tensor too (rounded once, after the fp32
 *     accumulation), and every backward product -- dX = dY . r(W), dW = dY^T . r(X) -- multiplies bf16 values on the bf16 MFMA
 *     pipe with fp32 accumulation;
 *   - the loss and its gradient with respect to the network outputs, dW / db accumulation, clip and Adam are fp32 and the master
 *     weights are the fp32 arena (the gradient of a weight is never rounded).
 * It is torch.autograd of F.linear(h.bfloat16().float(), r(W), b) per layer, r = rounding of a master weight with an identity
 * backward.  The reference has no such mode; the test suite restates it on the CPU (tests/test_gpu_cfg5.py).  Changing the mode
 * changes rlppo_minibatch_workspace_bytes.
 * rlppo_net_pack_bf16: the rounded images the mode needs, rebuilt after every optimiser step -- packed_r: the packed layout
 * (rlppo_packed_floats) holding the rounded weights as fp32; wb16: rlppo_wb16_elems bf16 values, the W[Pout][Pin] blocks of all
 * layers followed by the W^T[Pin][Pout] blocks. */
int rlppo_set_update_precision(int32_t mode);
int rlppo_get_update_precision(void);
int64_t rlppo_wb16_elems(const int32_t *dims, int32_t n_layers);
int rlppo_net_pack_bf16(void *stream, const int32_t *dims, int32_t n_layers, const float *flat, float *packed_r, void *wb16);
/* [r4] mode 2 (OPT-IN, not the default and not what bench.py's headline runs): the update stays fp32 in memory and in meaning --
 * activations, gradients, losses, dW, clip, Adam exactly as mode 0 -- but the hidden-layer FORWARD and dX products (widths that are
 * multiples of 256, contraction a multiple of 32, layers >= 1) run on the bf16 MFMA pipe from three-piece operands: every fp32
 * value x = x_h + x_m + x_l (bf16 pieces, rounded to nearest), six piece products per element pair, the five small ones summed
 * apart from the accumulator (csrc/gemm_split.hip).  gfx950's fp32-input MFMA has 1/16 of the bf16 rate; this form is 1.35 x
 * faster per launch and, against float64, MORE accurate than the fp32 MFMA's fmaf chain (0.43-0.46 x its error at K = 256).  The
 * gradients then differ from mode 0's by fp32 rounding noise only (tests/test_gpu_kernels.py, tests/test_gpu_learner.py hold
 * mode 2 to the same float64 gates as mode 0) -- for FINITE operands of ordinary magnitude: a +-inf, a NaN or a finite
 * |x| >= 3.396e38 (it rounds to a bf16 infinity) makes x - bf16(x) an inf - inf, so every output of that ROW is NaN where the fp32 MFMA
 * returns +-inf (or a finite product); pieces of |x| below ~1e-33 fall under bf16's normal range and lose low bits (an error relative
 * to 1e-38, not to the data).  Clipped observations and ReLU activations never get there; test_gemm_nt_x3_special_values
 * (tests/test_gpu_kernels.py) pins this behaviour.  Needs, per network, the image rlppo_net_pack_x3 derives from the PACKED copy
 * after every optimiser step: rlppo_x3_elems bf16 values (the stage-major planes [K / 32][3][N / 16][1 KiB block] of W for every
 * covered forward and of W^T for every covered dX; inside a 16-row block the 16-byte chunk (row r, k quarter q) at chunk
 * 4 r + (q ^ (-(r / 4) & 3)): the image the kernels' LDS fragment reads are bank-conflict-free on), handed over in rlppo_minibatch_args.pol_wb16 / val_wb16.  Policy and critic run as two
 * chains in this mode (no paired launches, the critic's head as its own matrix-vector launch). */
int64_t rlppo_x3_elems(const int32_t *dims, int32_t n_layers);
int rlppo_net_pack_x3(void *stream, const int32_t *dims, int32_t n_layers, const float *packed, void *planes);
/* single-kernel entry points of that precision (tests, bench.py): planes[C / 32][3][R / 16][1 KiB block, chunk order as above] <- the pieces of S[R][C] (row stride ld; R % 16 == 0);
 * C[M][N] = relu(A[M][K] . W^T + bias) with bits <- [C > 0] (mode 0) or (A . B^T) masked by bits (mode 1); N % 256 == 0, K % 32 == 0,
 * bits as rlppo_dbg_gemm_nt_bits_bytes(M, N). */
int rlppo_dbg_pack_x3(void *stream, const float *S, int64_t ld, int32_t R, int32_t C, void *planes);
int rlppo_dbg_gemm_nt_x3(void *stream, const float *A, int64_t lda, const void *planes, const float *bias, float *C, int64_t ldc, int64_t M,
                         int32_t N, int32_t K, int32_t mode, void *bits);

/* ------------------------------------------------------------------------------------------ diagnostics */
/* A/B switches for measurements and tests (also RLPPO_TUNE="key=value,..." in the Python host).  Defaults in brackets.
 *   1 GAE algorithm [1 single-pass look-back | 0 two launches]
 *   4 policy / critic chains of rlppo_ppo_minibatch on two streams [1]
 *  19 [act] fp32 update passes [1 = the ReLU bitmask forms where they apply (default) | 0 = every pass takes the plain form of a
 *     tanh / ELU pass: two chains on gathered rows, dX by the saved activation (measurements: what the form costs a ReLU pass)]
 *  21 GAE look-back spin limit [-1 = default 2^20 | 0 = every wait times out at once (tests)]
 *  22 GAE grid [0 = at most the resident capacity, workgroups loop over chunks beyond it | 1 = one workgroup per chunk always]
 *  23 bf16 update precision, form of the hidden-layer forward / dX / dW products [2 = 256 x 256 tiles walked by persistent workgroups
 *     (forward / dX; default) | 1 = 256 x 256, one workgroup per tile | 0 = 128 x 128]
 *  24 rlppo_torch_cpu_exponential transform [1 = AVX2 logarithm certified element by element against float32 rounding, libm for the
 *     rest (default) | 0 = libm for every element]
 *  26 minibatch gather [1 = fused into the first layer's GEMM launches through a row table from 262,144 rows per pass, a gather pass of its
 *     own below (default; [r5]: measured, csrc/update.hip) | 2 = fused at every size | 0 = always a gather pass of its own]
 *  27 rlppo_discrete_act / rlppo_discrete_step [1 = one fused launch where the network has that form (default) | 0 = layer chain]
 *  29 policy + critic layers of equal widths as ONE launch [1 = from 262,144 rows per pass (default) | 0 = never | 2 = always]
 *  31 paired pass: the critic's output-layer backward waits for the policy's loss kernel [1 (default) | 0 = both chains free-running]
 *  32 a one-output critic head is computed in the last hidden layer's forward epilogue [1 (default) | 0 = its own matrix-vector launch]
 *  33 paired launches: the two products' tiles interleave in the grid (a row tile's workgroups of both networks back to back on one
 *     XCD) [1 (default) | 0 = the second product stacked behind the first]
 *  34 rlppo_clip_adam_pack2 grid-barrier spin limit [-1 = default 2^22 | 0 = a waiter gives up at once (tests)]
 *  35 rlppo_clip_adam_pack2 test hook [0 | 1 = workgroup (0, 0) never arrives at the barrier: a grid that is not co-resident]
 *  36 split-bf16 products (update precision 2) [1 = persistent workgroups for large launches (default) | 0 = one workgroup per tile]
 *  37 [r5] the weight-gradient products of a pass [1 = ONE grouped launch + ONE reduction after the chains have joined (default; fp32 and
 *     split-bf16 precisions) | 0 = one launch + reduction per layer inside the chains]
 *  38 [r5] workgroups of a grouped weight-gradient launch [0 = two per CU (default) | n]
 *  40 [r5] forward layers of up to 1024 rows (the layer chain of a small rollout call) [1 = one wave per 16 x 16 output block, operands
 *     straight from L2 (default) | 0 = the 128-row tiles of the large kernel]: bit-identical outputs
 *  41 [r6] test hook of rlppo_host_window_alloc [0 = as the device is (default) | 1 = answer like a device that does not expose its
 *     memory to the host (no large BAR: the call fails, the host falls back to pinned memory) | 2 = windows are registered without a
 *     flush register (rlppo_host_window_flush then does nothing)] */
int rlppo_dbg_set(int32_t key, int32_t value);
/* Counter bumped by every call that changes which kernels later launches select (rlppo_dbg_set, rlppo_set_*_precision): a
 * host that caches captured graphs of library calls keys them on it (rlgym_ppo_amd/ppo/_mlp.py::ActGraph). */
int64_t rlppo_selection_epoch(void);
const int64_t *rlppo_selection_epoch_ptr(void);   /* the counter itself (a host that reads it per call) */
/* Which form calls took so far in this process (tests assert that the kernel they mean to pin is the one that ran): 0 = rollout steps
 * served by the one-launch kernel (rlppo_discrete_act / rlppo_discrete_step), 1 = by the layer chain, 2 = rlppo_ppo_minibatch passes,
 * 3 = of them with paired policy + critic launches, 4 = of them with the gather fused into the first layer, 5 = of them with the
 * grouped weight-gradient launch, 6 = [nvec] launches of the multi-discrete head's general (any nvec) kernels, sampling and loss,
 * 7 = rlppo_rollout_record launches (the device-resident collect form of the vector manager ran); launches by the kernel form the
 * launcher selected: 8 = rlppo_dbg_gemm_nt / layer-chain fp32 NT products by the few-row kernel, 9 = by the 128-row-tile kernel, 10 = bf16 hidden / dX product on
 * 256 x 256 tiles with one workgroup per tile, 11 = with persistent workgroups, 12 = split-bf16 product with persistent workgroups,
 * 13 = the one-output head's dW through fixed-order partials (not atomics); 15 = [critic rows] rlppo_ppo_minibatch passes with separate
 * critic rows (rlppo_ppo_minibatch_critic with a matrix); -1 for an unknown key (14 is none). */
int64_t rlppo_dbg_counter(int32_t key);
/* Debug helper, like rlppo_dbg_counter: adds delta to counter `key` (6 only; anything else RLPPO_ERR_ARG).  The launchers count when
 * they are CALLED; a host that captures a call into a graph and replays it (rlgym_ppo_amd/ppo/_mlp.py::ActGraph, the masked
 * multi-discrete call) takes the capture's launches off again and adds one run per replay, so that counter 6 keeps meaning "runs of
 * the general kernels".  For such a graph counter 6 is HOST-MAINTAINED: it witnesses that the host replayed a graph whose body is
 * the general kernel, not a launcher call. */
int rlppo_dbg_count(int32_t key, int64_t delta);
/* Single-kernel entry points used by tests/ and bench.py to check / time each GEMM flavour in isolation.
 * epilogue: 0 bias, 1 bias+relu, 2 bias+tanh, 3 relu-mask (mask_src > 0).  Shapes as in csrc/gemm.hip.
 * [act] 4 bias+ELU (alpha = 1: x > 0 ? x : expm1(x)); the dX epilogues of a tanh / ELU hidden layer, which read the saved activation
 * h from mask_src exactly as epilogue 3 does: 5 times tanh' (C = (A.B^T) (1 - h^2)), 6 times ELU' (C = (A.B^T) (h > 0 ? 1 : h + 1)). */
int rlppo_dbg_gemm_nt(void *stream, const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias,
                      const float *mask_src, int64_t ld_mask, float *C, int64_t ldc, int64_t M, int32_t N, int32_t K,
                      int32_t epilogue);
/* The bitmask form of the hidden-layer forward (epilogue 1: C = relu(A.B^T + bias), bits <- [C > 0], 8 bytes per lane and
 * 128 x 128 tile) and of the masked dX product (epilogue 3: C = (A.B^T) masked by bits).  N % 128 == 0. */
size_t rlppo_dbg_gemm_nt_bits_bytes(int64_t M, int32_t N);
int rlppo_dbg_gemm_nt_bits(void *stream, const float *A, int64_t lda, const float *B, int64_t ldb, const float *bias, float *C,
                           int64_t ldc, int64_t M, int32_t N, int32_t K, int32_t epilogue, void *bits);
/* The forward product of the bf16 update precision: A[M][K] and W[N][K] bf16 in memory, fp32 accumulate.  hidden != 0:
 * C (fp32, may be NULL) and Cb (bf16, may be NULL) receive relu(A.W^T + bias) rounded to bf16, bits (may be NULL) the ReLU
 * bitmask; N % 128 == 0.  hidden == 0: C = A.W^T + bias (epilogue 0) or tanh of it (epilogue 2), fp32.  K % 64 == 0. */
int rlppo_dbg_gemm_nt_b16(void *stream, const void *A, int64_t lda, const void *W, int64_t ldw, const float *bias, float *C,
                          int64_t ldc, void *Cb, int64_t ldcb, int64_t M, int32_t N, int32_t K, int32_t epilogue, int32_t hidden,
                          void *bits);
/* hidden == 2 is the backward product of that precision: Cb[M][N] (bf16) = round_bf16(A . W^T) masked by the ReLU bitmask `bits`
 * the hidden forward of the same M x N geometry wrote (epilogue 3, bias and C NULL; N % 128 == 0, K % 64 == 0).
 * rlppo_dbg_gemm_tn_b16: the weight-gradient product of that precision, dW[out][in] += dY^T . X, db[out] += colsum(dY), both
 * operands bf16 [M][ld] with pout / pin (multiples of 128) columns of which out / in are meaningful (the others are read and may hold any
 * finite values, as the padded columns of rlppo_dbg_gemm_tn; nothing beyond pout / pin is read); workspace as rlppo_dbg_gemm_tn. */
int rlppo_dbg_gemm_tn_b16(void *stream, const void *dY, int64_t ldy, const void *X, int64_t ldx, float *dW, float *db, int32_t pout,
                          int32_t pin, int32_t out, int32_t in, int64_t M, void *ws, size_t ws_bytes);
/* The output layer's two backward products in the bf16 update precision for a head of out <= 32 outputs (gemv.hip): dY[M][ldy]
 * fp32 (the loss gradient), W[out][ldw] fp32 (bf16-rounded values), hb[M][ldh] the last hidden activation as bf16, bits its ReLU
 * bitmask (rlppo_dbg_gemm_nt_bits_bytes(M, kp)): dxb[M][kp] (bf16) = round_bf16(dY . W) masked; dW[out][in] += dY^T . hb,
 * db[out] += colsum(dY) with a fixed summation order.  kp: padded hidden width, a power of two and a multiple of 128.  dY is read over
 * its first max(4, po) columns, po = out rounded up to 1, 8, 16, 24 or 32 (ldy >= that, a multiple of 4): the columns from `out` on may
 * hold any finite values (a pass leaves zeros), they reach no output; W is read over its first `out` rows and all kp columns, hb over kp
 * columns; nothing outside dxb[M][kp], dW[out][in], db[out] and the stated workspace is written. */
size_t rlppo_dbg_thin_head_workspace_bytes(int32_t out, int32_t kp, int64_t M);
int rlppo_dbg_thin_head_b16(void *stream, const float *dY, int64_t ldy, int32_t out, const float *W, int64_t ldw, const void *bits,
                            const void *hb, int64_t ldh, void *dxb, float *dW, float *db, int32_t in, int32_t kp, int64_t M, void *ws,
                            size_t ws_bytes);
/* The fp32 one-output (critic) head's matrix-vector kernels (csrc/gemv.hip), one at a time (tests): kp, the padded hidden width, a
 * power of two in 32 .. 1024; every row stride but ldy of the backward calls a multiple of 4 floats; x, w, mask, y and dx 16-byte aligned.
 * rlppo_dbg_gemv_fwd: y[m][0] = b[0] + sum_k x[m][k] w[k] over ALL kp columns, y[m][1 .. pout - 1] = 0 (the layout's padded outputs;
 * pout a multiple of 4, at most 64; nothing beyond column pout - 1 is written).
 * rlppo_dbg_gemv_dx: dx[m][k] = dy[m][0] w[k] where the hidden unit was on, 0 where it was off, for all kp columns -- by the ReLU
 * bitmask `bits` of the M x kp geometry (rlppo_dbg_gemm_nt_bits_bytes; kp % 128 == 0) when bits != NULL, else by mask[m][k] > 0 (the
 * saved activation, row stride ldm).
 * rlppo_dbg_gemv_dw: dw[k] += sum_m dy[m][0] x[m][k] for k < in, db[0] += sum_m dy[m][0] (db may be NULL); x is read over all kp
 * columns.  With ws_bytes >= rlppo_dbg_gemv_dw_workspace_bytes the blocks' partial sums meet in a fixed order (what a pass runs:
 * bit-reproducible), with less (or ws == NULL) they are added atomically. */
int rlppo_dbg_gemv_fwd(void *stream, const float *x, int64_t ldx, const float *w, const float *b, float *y, int64_t ldy, int64_t M,
                       int32_t kp, int32_t pout);
int rlppo_dbg_gemv_dx(void *stream, const float *dy, int64_t ldy, const float *w, const float *mask, int64_t ldm, const void *bits,
                      float *dx, int64_t ldc, int32_t kp, int64_t M);
size_t rlppo_dbg_gemv_dw_workspace_bytes(int32_t kp, int64_t M);
int rlppo_dbg_gemv_dw(void *stream, const float *dy, int64_t ldy, const float *x, int64_t ldx, float *dw, float *db, int32_t in,
                      int32_t kp, int64_t M, void *ws, size_t ws_bytes);
/* [diag] The diagonal-Gaussian head's loss step on its own, on caller-supplied head outputs y[mb][ld] (the means; overwritten with
 * dL/dmean), actions[mb][k], old_logp / advantages[mb] -- contiguous rows, as a pass has gathered them: part 0 = the loss launch and
 * the fixed-order finish of the log_std reduction (what a pass runs), 1 = the loss launch alone (partial sums into scratch), 2 = the
 * finish alone (on the partial sums an earlier call left).  tools/diag_gaussian_cost.py times them apart. */
int rlppo_dbg_diag_loss(void *stream, float *y, int64_t ld, int32_t k, const float *actions, const float *old_logp, const float *advantages,
                        int64_t mb, float clip_range, float ent_coef, float mb_ratio, const float *log_std, float *log_std_grad, void *scratch,
                        size_t scratch_bytes, double *stats, int32_t part);
/* dW[out][in] += dY^T . X, db[out] += colsum(dY) through partial tiles in `ws` (rlppo_dbg_gemm_tn_workspace_bytes) and a
 * fixed-order reduction: the form rlppo_ppo_minibatch uses.  dY[M][ldy] is read over its first ny_valid columns and X[M][ldx] over its
 * first kx_valid (multiples of 4, out <= ny_valid <= ldy, in <= kx_valid <= ldx); nothing beyond them is read.  The padded columns
 * out .. ny_valid - 1 of dY and in .. kx_valid - 1 of X may hold ANY FINITE values (a pass leaves zeros there): they are multiplied,
 * but their products land in partial-tile elements the reduction drops and reach no element of dW or db.  dW is the contiguous
 * out x in block of the flat gradient arena (4-byte aligned); nothing outside dW, db and the first
 * rlppo_dbg_gemm_tn_workspace_bytes of ws is written.  The same holds per product of rlppo_dbg_gemm_tn_group, for the rows a row
 * table names. */
size_t rlppo_dbg_gemm_tn_workspace_bytes(int32_t out, int32_t in, int64_t M);
int rlppo_dbg_gemm_tn(void *stream, const float *dY, int64_t ldy, int32_t ny_valid, const float *X, int64_t ldx,
                      int32_t kx_valid, float *dW, float *db, int32_t out, int32_t in, int64_t M, void *ws, size_t ws_bytes);

/* [r5] Every weight-gradient product of a pass as ONE launch + ONE fixed-order reduction (the form rlppo_ppo_minibatch uses from
 * round 5 on, rlppo_dbg_set(37)): product i is dW_i[out][in] += dY_i^T . X_i, db_i[out] += colsum(dY_i) over the same M rows (db may be
 * NULL); rowtab != NULL: sample m of product i is X_i[rowtab[m]] of a src_rows-row matrix (the fused minibatch gather of
 * experience_buffer.py:82-87).  The row splits of each product are sized so that every workgroup of the grid multiplies the same
 * number of MFMA blocks; the result depends on the SET of shapes and M, not on the order of the products. */
typedef struct rlppo_tn_product {
    const float *dY;
    int64_t ldy;
    int32_t ny_valid;
    const float *X;
    int64_t ldx;
    int32_t kx_valid;
    float *dW, *db;
    int32_t out, in;
    const uint32_t *rowtab;
    int64_t src_rows;
} rlppo_tn_product;
size_t rlppo_dbg_gemm_tn_group_workspace_bytes(const rlppo_tn_product *p, int32_t n, int64_t M);
int rlppo_dbg_gemm_tn_group(void *stream, const rlppo_tn_product *p, int32_t n, int64_t M, void *ws, size_t ws_bytes);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* RLPPO_H */
