/* fvhd.h - C ABI of libfvhd.so: the MI355X (gfx950) FastViTHD encode_images() path.
 *
 * The reference (apple/ml-fastvlm) is pure Python and has no FFI for this path; the boundary it
 * exposes is the duck-typed nn.Module `MobileCLIPVisionTower`
 * (llava/model/multimodal_encoder/mobileclip_encoder.py:13-116) created by `build_vision_tower`
 * (llava/model/multimodal_encoder/builder.py:6-19) and called from `encode_images`
 * (llava/model/llava_arch.py:141-144).  This header is what a binding for that boundary binds to;
 * `ml_fastvlm_amd/_lib.py` is the ctypes stub, `INTEGRATION.md` shows the reference-side patch.
 *
 * Conventions: every function returns 0 on success and a non-zero code on failure
 * (`fvhd_last_error()` gives a thread-local message); no C++ exception crosses the boundary; all
 * `void*` data arguments are DEVICE pointers unless the name says `host_`; work is enqueued on the
 * caller's HIP stream and never synchronises the device; the caller owns input/output buffers, the
 * context owns packed weights and workspace.  A context is bound to one device and is not
 * thread-safe (one context per stream/thread; the reference's callers enter `forward` one at a
 * time, llava/serve/model_worker.py:168-187).
 *
 * The multi-GPU boundary (one tower per rank + one all-gather of visual tokens) has NO entry point here on purpose: the
 * collective belongs to the host framework's process group (RCCL through torch.distributed, ml_fastvlm_amd/distributed.py);
 * the library produces the tokens a rank contributes.
 */
#ifndef FVHD_H
#define FVHD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fvhd_ctx fvhd_ctx;
typedef void* fvhd_stream_t; /* hipStream_t */

/* element types of caller-visible tensors */
#define FVHD_F32 0
#define FVHD_F16 1
#define FVHD_BF16 2

/* GEMM epilogues (fvhd_op_gemm) */
#define FVHD_EPI_NONE 0          /* out = A.W^T                                   (MHSA.qkv, mci.py:668) */
#define FVHD_EPI_BIAS 1          /* out = A.W^T + b                               (projector Linear #2)   */
#define FVHD_EPI_BIAS_GELU 2     /* out = gelu(A.W^T + b)                         (fc1, 1x1 convs, projector Linear #1) */
#define FVHD_EPI_BIAS_LS_RESID 3 /* out = resid + ls * (A.W^T + b)                (fc2 / proj + layer scale + skip) */

/* ABI version: major * 100 + minor.  A caller built against this header compares fvhd_version() with FVHD_VERSION before anything else
 * (ml_fastvlm_amd/_lib.py does): the major part changes whenever an exported signature or the meaning of an argument changes.
 * 100 = rounds 1-3; round 4 changed signatures under the same number (fvhd_op_stem_fused + w2 / b2, fvhd_op_ffn_fused / fvhd_ffn_pack +
 * precision, fvhd_op_rope + rope_theta) - a mistake this number corrects; 500 = round 5 (adds the range guard, fvhd_op_dw7_amax,
 * fvhd_op_gemm_qkv_rope / fvhd_gemm_qkv_rope_supported, the fvhd_llm_* stream contract; no signature of round 4 changed); 501 adds the
 * LLM decode (fvhd_llm_cache_reserve / start / decode / cache_state / set_tied_embeddings, the optional model.embed_tokens.weight key,
 * fvhd_op_dec_*); nothing earlier changed.  502 adds LLM sampling (fvhd_llm_set_sampling, fvhd_op_dec_sample): greedy stays the
 * default and computes what 501 did; no earlier signature changed.  503 widens the LLM decode from 16 to 64 sequences per step
 * (fvhd_llm_cache_reserve, fvhd_op_dec_gemm / _qkv / _attention / _lm_argmax: B in [1, 64]; the scratch of the single ops grows with
 * ceil(B / 16)); no signature changed and B <= 16 computes what 502 did, bit for bit.  504 adds 8-bit LLM weights
 * (fvhd_llm_set_weight_format, fvhd_llm_weight_bytes, fvhd_llm_debug_packed_e4m3, fvhd_op_quantize_e4m3, fvhd_op_dec_gemm_w8 / _qkv_w8 /
 * _lm_argmax_w8): bf16 stays the default and computes what 503 did, bit for bit; nothing earlier changed.  505 adds beam search
 * (fvhd_llm_beam_reserve, fvhd_llm_cache_gather, fvhd_llm_beam_topk, fvhd_op_dec_beam_topk, fvhd_op_dec_cache_gather; error word 3):
 * greedy and sampled steps compute what 504 did, bit for bit, and fvhd_llm_cache_reserve allocates what it did; nothing earlier changed.
 * 506 adds logits processors in the decode step (fvhd_llm_set_logits_processors, fvhd_op_dec_logits_process): off by default, and then
 * every launch of fvhd_llm_start / fvhd_llm_decode is what 505 enqueued, bit for bit; fvhd_llm_cache_reserve also allocates the token
 * history (4 * batch * capacity + batch * vocab / 8 + 4 * batch bytes); nothing earlier changed.  508 adds fvhd_gemm_kernel_plan, a read-only query of
 * fvhd_op_gemm's kernel choice (the FVHD_GEMM_PLAN_* codes): the launcher switches on the same function's value, every launch and its
 * bits are what 507 ran; nothing earlier changed.  509 adds the extension of a started KV cache by a chunk of tokens and its rewind
 * (fvhd_llm_extend, fvhd_llm_cache_rewind, fvhd_op_attention_extend / _cache_append / _extend_positions / _cache_rewind; error word 4):
 * fvhd_llm_prefill, fvhd_llm_start, fvhd_llm_decode, fvhd_llm_verify and the lookup step enqueue what 508 did, launch for launch and bit for
 * bit; the prefill workspace grows by 8 bytes per row (the positions of a chunk); nothing earlier changed.  510 changes behaviour without a new
 * symbol: behind fvhd_llm_cache_rewind / fvhd_llm_cache_gather the calls that would feed the ids "the previous step chose"
 * (fvhd_llm_decode(token_ids = NULL), fvhd_llm_verify, fvhd_llm_lookup_begin / _step) are refused until fvhd_llm_start, fvhd_llm_extend or a
 * fvhd_llm_decode on explicit token_ids, and fvhd_llm_decode, fvhd_llm_verify and fvhd_llm_cache_gather end a lookup generation; every call
 * that is accepted enqueues what 509 did, launch for launch and bit for bit.  Added under 510 (new symbols only, the number stays): scoring
 * given tokens - fvhd_lm_score_scratch_bytes, fvhd_lm_score_plan, fvhd_op_lm_score, fvhd_llm_score_reserve, fvhd_llm_score; every existing
 * call enqueues what it did and fvhd_llm_reserve allocates what it did.  Also added under 510 (new symbols only, the number stays): 4-bit
 * LLM weights - FVHD_W_MXFP4 for fvhd_llm_set_weight_format, fvhd_llm_debug_packed_mxfp4, fvhd_op_quantize_mxfp4, fvhd_op_dec_gemm_w4 /
 * _qkv_w4 / _lm_argmax_w4, fvhd_op_w4_unpack; bf16 and e4m3 contexts enqueue what they did, bit for bit (a caller detects the symbols, as
 * ml_fastvlm_amd/_lib.py w4_lib() does).  Also added under 510 (new symbols only, the number stays): log-probabilities of the chosen tokens -
 * fvhd_dec_logprobs_scratch_bytes, fvhd_op_dec_logprobs, fvhd_llm_set_logprobs, fvhd_llm_logprobs; with the setting off (the default) every
 * existing call enqueues what it did and fvhd_llm_cache_reserve allocates what it did (_lib.py logprobs_lib() detects the symbols).  Also added
 * under 510 (new symbols only, the number stays): constrained decoding - fvhd_llm_set_constraint, fvhd_llm_constraint_state,
 * fvhd_op_dec_constrain, fvhd_dec_constrain_slice; with no constraint set (the default) every call enqueues what it did and allocates what it
 * did (_lib.py constraint_lib() detects the symbols).  Also added under 510 (new symbols only, the number stays): prompt-lookup decoding
 * under sampling and with log-probabilities - fvhd_llm_set_verify_sampling, fvhd_llm_lookup_logprobs, fvhd_op_dec_sample_rows; with the
 * setting off (the default) and no arrays registered every call enqueues, refuses and allocates what it did (_lib.py lookup_sample_lib()
 * detects the symbols).  Also added under 510 (new symbols only, the number stays): classifier-free guidance - fvhd_dec_guidance_scratch_bytes,
 * fvhd_op_dec_guidance, fvhd_llm_set_guidance; with the scale at 1 (the default) every call enqueues, refuses and allocates what it did
 * (_lib.py guidance_lib() detects the symbols).  Also added under 510 (new symbols only, the number stays): the sampling warpers behind
 * top-p - fvhd_llm_set_sampling_warpers, fvhd_op_dec_sample_warpers; with the four at their off values (the default) every call enqueues,
 * refuses and allocates what it did (_lib.py sampling_warpers_lib() detects the symbols).  Also added under 510 (new symbols only, the number
 * stays): beam-search sampling - fvhd_llm_beam_sample_reserve, fvhd_llm_beam_sample_topk, fvhd_op_dec_beam_sample; every existing call
 * enqueues, refuses and allocates what it did (_lib.py beam_sample_lib() detects the symbols). */
#define FVHD_VERSION 510
int fvhd_version(void);
const char* fvhd_last_error(void);

/* ---- context ------------------------------------------------------------------------------------
 * Replaces MobileCLIPVisionTower.__init__/load_model (mobileclip_encoder.py:14-58): one context per
 * (device, input resolution).  `image_size` is the R of the tower name `mobileclip_l_<R>`
 * (mobileclip_encoder.py:20), a multiple of 64.  Workspace is sized for `max_batch` images and
 * grows on demand. */
int fvhd_create(fvhd_ctx** out, int device, int image_size, int max_batch);
void fvhd_destroy(fvhd_ctx* ctx);

/* Size the workspace for `max_batch` images NOW.  Growing it (here, or implicitly when a larger batch reaches fvhd_encode*)
 * synchronises the device, frees and re-allocates the arena and drops the cached graphs - the only place where the library
 * synchronises.  Implicit growth inside fvhd_encode* / fvhd_project is refused while the caller's stream is being captured;
 * fvhd_reserve itself takes no stream and must not be called while ANY stream of the device is capturing (it synchronises the
 * device, which invalidates a capture): reserve before capturing.  An arena that a caller's capture has recorded pointers into (an
 * fvhd_encode* / fvhd_project call made while the caller's stream was capturing) is retired instead of freed when a later, larger batch
 * replaces it: the caller's graph keeps replaying on valid memory until fvhd_destroy (round 5).  Every entry point
 * that takes a context runs on the context's device and restores the caller's current device before returning. */
int fvhd_reserve(fvhd_ctx* ctx, int max_batch);

/* Hand one tensor of the reference's inference-mode state dict to the library
 * (key relative to the FastViT module, e.g. "network.7.0.token_mixer.qkv.weight"; the 629 keys of
 * tests/golden/keys.json).  `host_data` is contiguous fp32 HOST memory in the reference's own
 * layout ([out,in,kh,kw] for convs, [out,in] for linears); it is copied before the call returns.
 * Replaces nn.Module.load_state_dict for the tower (model/builder.py:131). */
int fvhd_set_tensor(fvhd_ctx* ctx, const char* key, const float* host_data, const int64_t* shape, int ndim);

/* Fold eval-mode BatchNorm into the dw7x7 taps (mci.py:901-907), transpose depthwise taps to
 * [kh*kw][C], round GEMM weights to bf16, upload.  Fails if any required tensor is missing. */
int fvhd_finalize_weights(fvhd_ctx* ctx);

/* mlp2x_gelu projector weights (multimodal_projector/builder.py:23-30): host fp32,
 * w0 [hidden, mm_hidden], b0 [hidden], w2 [hidden, hidden], b2 [hidden]. */
int fvhd_set_projector(fvhd_ctx* ctx, const float* host_w0, const float* host_b0, const float* host_w2,
                       const float* host_b2, int mm_hidden, int hidden);

/* ---- hot path -----------------------------------------------------------------------------------
 * MobileCLIPVisionTower.forward_images + feature_select (mobileclip_encoder.py:60-88):
 * images [B,3,R,R] NCHW contiguous of `img_dtype` -> tokens_out [B,(R/64)^2,3072] of `out_dtype`. */
int fvhd_encode(fvhd_ctx* ctx, const void* images, int img_dtype, int batch, void* tokens_out, int out_dtype,
                fvhd_stream_t stream);

/* mm_projector forward (llava_arch.py:143): tokens [rows, mm_hidden] -> out [rows, hidden]. */
int fvhd_project(fvhd_ctx* ctx, const void* tokens, int in_dtype, int rows, void* out, int out_dtype,
                 fvhd_stream_t stream);

/* encode_images (llava_arch.py:141-144) = tower then projector, tokens kept in bf16 in workspace. */
int fvhd_encode_images(fvhd_ctx* ctx, const void* images, int img_dtype, int batch, void* out, int out_dtype,
                       fvhd_stream_t stream);

/* ---- precision of the fused ConvFFN's hidden activation ------------------------------------------
 * ConvFFN.fc1 -> GELU -> fc2 (mci.py:922-926) runs for C in {96,192,384} as ONE kernel whose hidden activation never reaches HBM.  By
 * default it is kept as gelu(x)/4 in IEEE half (FVHD_FFN_HALF: 11 mantissa bits, better than the bf16 the reference's bf16 execution
 * carries, but |fc1 output| > 262 016 SATURATES where bf16 / fp32 carry on).  The same kernel exists with an f32 GELU and a bf16 hidden
 * operand (FVHD_FFN_BF16: no range limit, ~3-7 % slower); both are compiled in and both weight images are packed, so the choice is a
 * per-block run-time switch:
 *   fvhd_set_ffn_precision / fvhd_get_ffn_precision  - by step index (fvhd_step_info); get returns -1 for a step without a fused ConvFFN.
 *     A block whose |4 * fc2.weight| would overflow f16, whose largest |fc2.weight| is below 2^-10 (f16(4 W2) would sink into the f16
 *     subnormals) or whose fc1 biases alone exceed 2^17 (range guard, below) starts as FVHD_FFN_BF16.
 *   fvhd_audit_ranges - one eager pass over `images` (a calibration batch of the deployment's real inputs) that also materialises every
 *     ConvFFN's fc1 output and reduces it to max |.|: max_abs_out[fvhd_num_steps] (0 for steps without a ConvFFN; Inf / NaN if the fc1
 *     output itself overflowed) and, when switch_above > 0, switches every fused block whose maximum exceeds it (or is not finite) to
 *     FVHD_FFN_BF16, reporting how many in *n_switched.  A margin below the 262 016 limit (the Python wrapper uses 65 504 = a factor 4)
 *     covers inputs hotter than the calibration batch.  Synchronises `stream`; not during capture.  max_abs_out / n_switched may be NULL. */
#define FVHD_FFN_HALF 0
#define FVHD_FFN_BF16 1
int fvhd_set_ffn_precision(fvhd_ctx* ctx, int step, int precision);
int fvhd_get_ffn_precision(const fvhd_ctx* ctx, int step);
int fvhd_audit_ranges(fvhd_ctx* ctx, const void* images, int img_dtype, int batch, float switch_above, float* max_abs_out,
                      int* n_switched, fvhd_stream_t stream);

/* ---- range guard (round 5): the half-precision form is never run outside its proven range twice ------
 * An audit says nothing about an image hotter than the calibration batch.  The guard is always on and costs nothing measurable: the
 * depthwise 7x7 (+BN) that produces a fused block's input A reduces max |A| on the fly (free issue slots of the matrix-core kernel),
 * and since |fc1 out_j| <= L1(W1 row j) * max|A| + |b1_j|, a block is PROVABLY inside the half-precision range while
 *     max|A| <= limit = (2^17 - max_j |b1_j|) / max_j L1(W1 row j)          (2^17 = half of the 262 016 saturation point)
 * holds (fvhd_range_guard_limit; computed from the packed weights at fvhd_finalize_weights; a block whose biases alone exceed 2^17
 * starts as FVHD_FFN_BF16).  Every fvhd_encode* call zeroes the per-step maxima, its kernels reduce into them, and the array is read
 * back asynchronously (pinned host memory + an event; no synchronisation).  The NEXT fvhd_encode* call - or fvhd_range_guard_poll -
 * compares the finished read-backs with the limits: a block over its limit is switched to FVHD_FFN_BF16 for every later call and reported.
 * The bound is sufficient, not necessary: it can move a block that would not have saturated (costing that block 3-7 %), never the other
 * way round.  What it cannot do is repair the one batch that crossed the limit - that call's output used the half form; callers that need
 * the guarantee per batch poll with wait = 1 after the call and re-encode when a step is reported (the Python tower does exactly that
 * when mm_vision_range_guard = "strict").  Inactive while the caller's stream is being captured (an event inside a graph cannot be
 * polled): graph-capturing callers calibrate with fvhd_audit_ranges first.
 * WHERE the maximum is taken (FVHD_GUARD_SITE in the environment of fvhd_create; default 0): 0 = max |A| inside the dw7x7 (+BN) kernel, limit as
 * above; 1 = one convolution earlier, max |y| of the RepMixer output inside the dw3x3 kernel, with |A_c| <= L1(folded 7x7 taps of c) max|y| +
 * |folded BN bias_c|, i.e. limit_y = (limit - max_c |bias_c|) / max_c L1(taps_c) - a looser bound (by the 7x7 taps' L1 norm, 2-7x: it moves
 * blocks to the slower form sooner than needed).  Measured on one box, whole step at B = 32 (profiles/r05_guard_cost_ab.log): guard on
 * (site 0) 23.76 / 23.77 ms, off 23.71 / 23.69 = 0.27 %; site 1 23.62 (one run).
 *   fvhd_set_range_guard(ctx, 0 / 1)   - default 1 (environment: FVHD_RANGE_GUARD=0).
 *   fvhd_range_guard_limit             - the limit on the tracked maximum (max|A| / max|y|) of a fused step (INFINITY if the weights are all
 *                                        zero, < 0 if the block can never run the half form).
 *   fvhd_range_guard_poll              - consume the finished read-backs (wait != 0: all outstanding ones, synchronising on their events);
 *                                        steps_out / amax_out [max_out] receive the steps switched since the last poll and the max|A| that
 *                                        did it, *n_out how many; with max_out <= 0 nothing is handed out and nothing forgotten: *n_out = the
 *                                        number waiting (a count query).
 * Run-ahead: four read-backs can be in flight; a fifth fvhd_encode* call whose predecessors' read-backs nobody has consumed waits on the host
 * for the oldest one's event (an asynchronous caller runs at most four encodes ahead of the GPU). */
int fvhd_set_range_guard(fvhd_ctx* ctx, int on);
int fvhd_range_guard_limit(const fvhd_ctx* ctx, int step, float* limit_out);
int fvhd_range_guard_poll(fvhd_ctx* ctx, int wait, int* steps_out, float* amax_out, int max_out, int* n_out);

/* geometry helpers (mobileclip_encoder.py:106-116) */
int fvhd_num_tokens(const fvhd_ctx* ctx);   /* (R/64)^2 */
int fvhd_hidden_size(const fvhd_ctx* ctx);  /* 3072     */

/* ---- step-level execution (parity tests / debugging) ---------------------------------------------
 * The tower is a list of "steps", one per forward() of a reference module on the running activation, in
 * the execution order of FastViT.forward (mci.py:1427-1451): step 0 = convolutional_stem, then per stage
 * [RepCPE], every RepMixerBlock / AttentionBlock, [PatchEmbed], and last conv_exp (+SE+GELU).
 * fvhd_step_info: kind 0 stem, 1 RepCPE, 2 RepMixerBlock, 3 AttentionBlock, 4 PatchEmbed, 5 conv_exp;
 * (c_in,h_in) / (c_out,h_out) = channels and side of the NHWC activation entering / leaving the step.
 * fvhd_run_steps runs steps first..last (inclusive) on x_in and writes the result to x_out, both NHWC
 * bf16 device buffers ([batch,h,h,c]; for first == 0 x_in is the NCHW bf16 image batch, for the last
 * step x_out is the [batch,T,3072] bf16 token tensor).  This is how the tests feed every block the
 * oracle's input for that block ("teacher forcing") instead of comparing only after 44 blocks. */
int fvhd_num_steps(const fvhd_ctx* ctx);
int fvhd_step_info(const fvhd_ctx* ctx, int step, int* kind, int* stage, int* block, int* c_in, int* h_in,
                   int* c_out, int* h_out);
int fvhd_run_steps(fvhd_ctx* ctx, int first, int last, const void* x_in, int batch, void* x_out,
                   fvhd_stream_t stream);

/* ---- measurement --------------------------------------------------------------------------------
 * With profiling on, every kernel launch inside fvhd_encode/fvhd_project is bracketed by HIP events
 * on the caller's stream.  fvhd_profile_read synchronises those events and returns, per kernel
 * class, the accumulated milliseconds and launch count since the last reset.  Class names:
 * "stem", "dw3", "dw7", "dw_down", "gemm_fc1", "gemm_fc2", "gemm_1x1", "gemm_qkv", "gemm_proj",
 * "layernorm", "attention", "head", "projector", "ffn_fused". */
int fvhd_profile_enable(fvhd_ctx* ctx, int on);

/* Precision option of the MHSA core (mci.py:670-679) for BASELINE.json configs[4] ("fp8 MFMA attention path"), OPT-IN:
 * on != 0 runs QK^T and PV with OCP e4m3 operands (fvhd_op_attention_fp8) in every AttentionBlock of fvhd_encode /
 * fvhd_run_steps; default 0 = bf16 operands (the parity path).  The reference has no such switch: its attention runs in
 * the tower dtype (mobileclip_encoder.py:85).  Also settable with the environment variable FVHD_ATTN_FP8=1 at fvhd_create.
 * Measured: no faster than bf16 on gfx950 (the non-scaled fp8 MFMA issues at the bf16 rate; DESIGN.md "fp8"). */
int fvhd_set_attention_fp8(fvhd_ctx* ctx, int on);

/* Kernel selection.  Default (0): every launch takes the fastest kernel for its shape INCLUDING the batch - below ~0.75 workgroups
 * per CU the depthwise 7x7 runs on the VALU kernel instead of the matrix-core one and ConvFFN as two tiled GEMMs instead of the
 * fused kernel (B = 1 at 1024^2: 4.3 -> 3.5 ms).  Results are then bit-identical for a given batch size (any order, any
 * neighbours) and equal across batch sizes only to bf16 rounding.  on != 0: the choice depends on the shape of ONE image only, so
 * an image produces the same bits in whatever batch it travels (dynamic batching with reproducible outputs).  The reference
 * makes no such promise either way (cuDNN / MIOpen pick algorithms by shape). */
int fvhd_set_batch_invariant(fvhd_ctx* ctx, int on);

/* hipGraph replay: on != 0 makes fvhd_encode / fvhd_encode_images capture the interior steps of the tower (everything between
 * the stem, which reads the caller's images, and the head, which writes the caller's buffer: ~170 launches)
 * into one hipGraph per (batch, options) on the second call with that batch size and replay it from then on - the launch-bound
 * small-batch case (TTFT, B = 1..8).  The reference's analogue is none (eager PyTorch, mobileclip_encoder.py:70-88).
 * A caller that is itself stream-capturing gets plain launches.  Also FVHD_GRAPH=1 at fvhd_create.  Default off. */
int fvhd_set_graph(fvhd_ctx* ctx, int on);
int fvhd_profile_reset(fvhd_ctx* ctx);
int fvhd_profile_read(fvhd_ctx* ctx, int max_classes, const char** names, double* ms, int64_t* launches,
                      int* n_classes);

/* ---- single ops (unit-test entry points; device pointers, packed layouts as documented) ---------- */
/* depthwise conv, NHWC bf16: x [B,H,W,Cin] -> y [B,OH,OW,Cin*mult]; w fp32 [K*K][Cout]; bias fp32 [Cout] or NULL.
 * (K,stride,mult,gelu) in {(3,1,1,0),(3,2,1,1),(7,1,1,0),(7,2,2,1),(3,1,2,0)}  - mci.py:808-811, 575-586, 921, 992-995, 442-451, 1401-1411.
 * Cin * mult must be a multiple of 32 (every FastViTHD width is: 96 ... 3072); any other combination is an error with a message. */
int fvhd_op_dwconv(fvhd_stream_t stream, const void* x, void* y, const float* w, const float* bias,
                   int B, int H, int W, int Cin, int K, int stride, int mult, int gelu);

/* The 7x7 stride-1 depthwise conv (+ bias) on the matrix cores (csrc/dwconv_mfma.hip: 16-block 4x4x4 bf16 MFMA, taps rounded to
 * bf16, fp32 accumulation) for ANY batch size - fvhd_op_dwconv / the tower take this kernel by themselves once the launch fills
 * the chip (or always, under fvhd_set_batch_invariant).  Same arguments as fvhd_op_dwconv(K = 7, stride 1, mult 1, no GELU);
 * needs C % 64 == 0 or C % 96 == 0 and W >= 16, anything else is an error. */
int fvhd_op_dw7_mfma(fvhd_stream_t stream, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int C);
/* The same convolution with the range guard's reduction (round 5): amax_bits (device, FVHD_AMAX_SLOTS = 64 32-bit words, zeroed by the caller; the
 * workgroups spread their atomics over the words, the result is the maximum of all 64) receives max |y| - over
 * everything the launch stores (VALU kernel, mfma = 0) or over the stored rows and the columns of the kernel's 64-px strips (matrix-core kernel,
 * mfma = 1: for W % 64 != 0 a superset of the image, computed from the zero padding) - as the fp32 bit pattern of a non-negative number
 * (combined with atomicMax: unsigned order = numeric order), taken from the fp32 accumulators before the rounding to bf16.  mfma = 0 is an error
 * for shapes the dispatcher gives to the matrix-core kernel, mfma = 1 for shapes that kernel does not take. */
/* RepMixer dw3x3 (+ bias) followed by the ConvFFN's dw7x7 (+ folded BatchNorm bias) in ONE launch (round 6, csrc/dwconv_fused.hip;
 * mci.py:808-811 -> :920-921): x [B,H,W,C] -> y = dw3x3(x) + b3 [B,H,W,C] (the block's residual stream, written once) and
 * a = dw7x7(y) + b7 [B,H,W,C], all NHWC bf16; w3 fp32 [9][C], w7 fp32 [49][C], b3 / b7 fp32 [C] or NULL.  Both convolutions run on the
 * 16-block 4x4x4 bf16 MFMA: the 3x3 with every tap split into two bf16 halves (16 mantissa bits - the re-parameterised centre tap is
 * 1 + eps), the 7x7 exactly as fvhd_op_dw7_mfma (taps rounded to bf16; the same bits as that entry point given the same y).
 * amax_bits: NULL or FVHD_AMAX_SLOTS words (zeroed by the caller) receiving max |a| as in fvhd_op_dw7_amax(mfma = 1).
 * Needs C % 32 == 0, C >= 64, W % 4 == 0, W >= 16; anything else is an error (C % 64 == 32 - stage 0's C = 96 - runs its last 64-channel
 * block half masked).  The tower takes this kernel for a RepMixerBlock by itself once
 * the launch fills the chip (fvhd_dw3_dw7_supported(..., 0)); never under fvhd_set_batch_invariant. */
int fvhd_op_dw3_dw7(fvhd_stream_t stream, const void* x, void* y, void* a, const float* w3, const float* b3, const float* w7,
                    const float* b7, int B, int H, int W, int C, void* amax_bits);
/* 1 when fvhd_op_dw3_dw7 takes the shape (force != 0) / when the tower picks it by itself (force == 0) */
int fvhd_dw3_dw7_supported(int B, int H, int W, int C, int force);
/* 1 when fvhd_op_dwconv runs PatchEmbed's depthwise conv (K = 7, stride 2, mult 2; mci.py:442-451) on the matrix cores (round 6,
 * csrc/dwconv_down.hip: stride 2 as two Toeplitz products over the even and the odd input pixels, taps rounded to bf16 as in fvhd_op_dw7_mfma,
 * fp32 accumulation, fp32 GELU): C_in % 32 == 0 and, for force == 0, an output map at least 24 pixels wide (narrower maps: the VALU
 * kernel's finer tiles).  A choice by shape only - the same bits whatever the batch.  The TOWER additionally keeps the VALU kernel (fp32
 * taps) for a PatchEmbed whose packed taps are not bf16 numbers (an fp32 / fp16 checkpoint): with a re-parameterised bf16 checkpoint the
 * kernel's bf16 operands are the taps themselves.  FVHD_DWDOWN_MFMA=0 in the environment keeps the VALU kernel everywhere. */
int fvhd_dw7s2_mfma_supported(int B, int H, int W, int Cin, int force);
/* the same conv on that kernel directly: x [B,H,W,Cin] -> y [B,ceil(H/2),ceil(W/2),2 Cin] NHWC bf16, w fp32 [49][2 Cin], bias fp32 [2 Cin] or
 * NULL, GELU applied; any shape with fvhd_dw7s2_mfma_supported(..., 1) */
int fvhd_op_dw7s2_mfma(fvhd_stream_t stream, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int Cin);
#define FVHD_AMAX_SLOTS 64
int fvhd_op_dw7_amax(fvhd_stream_t stream, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int C, int mfma,
                     void* amax_bits);
/* out[M,N] = epi(A[M,K] . Wt[N,K]^T): A, Wt, resid bf16; bias, ls fp32 [N]; K % 32 == 0, N % 16 == 0.  out_dtype other than bf16 only with
 * FVHD_EPI_BIAS (f16 / f32) and FVHD_EPI_NONE (f32: lm_head logits); FVHD_EPI_SWIGLU writes [M, N/2].  A NULL A, Wt or out, and a NULL bias /
 * ls / resid under an epilogue that reads it (bias: BIAS, BIAS_GELU, BIAS_LS_RESID; ls: BIAS_LS_RESID; resid: BIAS_LS_RESID, RESID), is refused
 * with an error and nothing is launched; the vectors an epilogue does not read may be NULL. */
int fvhd_op_gemm(fvhd_stream_t stream, const void* A, const void* Wt, const float* bias, const float* ls,
                 const void* resid, void* out, int M, int N, int K, int epilogue, int out_dtype);
/* the residual GEMM of ConvFFN.fc2 / MHSA.proj (out = resid + ls * (A . Wt^T + bias); mci.py:926 + 1106-1109, :681 + 1185-1187) with K split over
 * `splits` workgroups per output tile - what fvhd_encode launches instead of fvhd_op_gemm(..., EPI_BIAS_LS_RESID) when fvhd_gemm_splitk_plan(M, N, K)
 * > 1 (a handful of tiles with a long K: batches of 1-8 images; never in batch-invariant mode).  partial: fp32 scratch [splits][M][N];
 * N % 128 == 0, K % (64 * splits) == 0; resid may alias out. */
int fvhd_op_gemm_splitk_ls(fvhd_stream_t stream, const void* A, const void* Wt, const float* bias, const float* ls, const void* resid, void* out,
                           float* partial, int M, int N, int K, int splits);
int fvhd_gemm_splitk_plan(int M, int N, int K);
/* Which kernel fvhd_op_gemm launches for this call on the CURRENT device (version 508; pure host code, the device supplies its CU count: the
 * thresholds between the classes are rounds of tiles per CU) - one of the codes below, or a negative value for a call fvhd_op_gemm refuses.
 * The launcher switches on the value of the same function, so the answer cannot drift from the launch.  Every class adds the K tiles of an
 * output element in the same order: the classes give identical bits.  For tests that have to know which kernel they compare. */
#define FVHD_GEMM_PLAN_V1_NF4_BK64 0 /* v1: 128 x 128 tiles (ragged M and N), K tiles of 64 */
#define FVHD_GEMM_PLAN_V1_NF4_BK32 1 /* v1: 128 x 128, K tiles of 32 (K % 64 != 0) */
#define FVHD_GEMM_PLAN_V1_NF3_BK64 2 /* v1: 128 x 96 tiles (N % 96 == 0, N % 128 != 0), K tiles of 64 */
#define FVHD_GEMM_PLAN_V1_NF3_BK32 3 /* v1: 128 x 96, K tiles of 32 */
#define FVHD_GEMM_PLAN_V1S 4         /* v1s: the streaming 128 x 128 kernel, at most one tile per CU */
#define FVHD_GEMM_PLAN_256X128 5     /* streaming 256 x 128 */
#define FVHD_GEMM_PLAN_256X256 6     /* streaming 256 x 256 */
#define FVHD_GEMM_PLAN_PINGPONG 7    /* ping-pong 256 x 256 (K >= 3072) */
#define FVHD_GEMM_PLAN_128X192 8     /* v1 with ONE 128 x 192 tile per row block (N = 192, FVHD_EPI_BIAS_GELU, many rows) */
int fvhd_gemm_kernel_plan(int M, int N, int K, int epilogue, int out_dtype);
/* LayerNormChannel (mci.py:617-623) on NHWC rows: x,y [M,C] bf16; w,b fp32 [C]. */
int fvhd_op_layernorm(fvhd_stream_t stream, const void* x, void* y, const float* w, const float* b, int M, int C, float eps);
/* MHSA core (mci.py:670-679): qkv [B*N,3C] bf16 -> out [B*N,C] bf16, head_dim 32. */
int fvhd_op_attention(fvhd_stream_t stream, const void* qkv, void* out, int B, int N, int C);
/* same, Q/K/V and P = exp(s - max) rounded to OCP e4m3 (RNE) as MFMA operands, fp32 accumulation and running maximum; the softmax
 * denominator sums the same e4m3 P values that multiply V. */
int fvhd_op_attention_fp8(fvhd_stream_t stream, const void* qkv, void* out, int B, int N, int C);
/* stem[0] (mci.py:563-574): img [B,3,R,R] of dtype -> out [B,R/2,R/2,96] bf16; w fp32 [27][96] (k = ci*9+ky*3+kx). */
int fvhd_op_stem_conv(fvhd_stream_t stream, const void* img, int dtype, void* out, const float* w, const float* bias, int B, int R);
/* convolutional_stem in one launch (mci.py:553-603): img [B,3,R,R] of dtype -> out [B,R/4,R/4,96] bf16;
 * w0 fp32 [27][96], b0 [96] as fvhd_op_stem_conv; w1 fp32 [9][96] (tap-major), b1 [96] as fvhd_op_dwconv(K=3, stride 2, gelu);
 * w2 bf16 [96][96] ([out][in], as fvhd_op_gemm takes weights), b2 fp32 [96]: stem[2], the 1x1 conv + GELU (mci.py:587-598) - or both
 * NULL: stem[0] + stem[1] only.  Bit-identical to fvhd_op_stem_conv -> fvhd_op_dwconv [-> fvhd_op_gemm(FVHD_EPI_BIAS_GELU)]. */
int fvhd_op_stem_fused(fvhd_stream_t stream, const void* img, int dtype, void* out, const float* w0, const float* b0,
                       const float* w1, const float* b1, const void* w2, const float* b2, int B, int R);
/* SEBlock + GELU of conv_exp (mci.py:72-81,198): y [B,T,C] bf16 -> out [B,T,C] of out_dtype;
 * pooled: fp32 scratch [B*(C+RD)]; scale: fp32 scratch [B,C]; wr fp32 [RD][C]; we fp32 [C][RD]; RD % 4 == 0. */
int fvhd_op_se_head(fvhd_stream_t stream, const void* y, float* pooled, float* scale, const float* wr, const float* br,
                    const float* we, const float* be, void* out, int out_dtype, int B, int T, int C, int RD);

/* Fused ConvFFN MLP (mci.py:922-926 + 1106-1109): X <- X + ls * (gelu(A.W1^T + b1).W2^T + b2), in place on X [M,C] bf16.
 * C in {96,192,384} (fvhd_ffn_fused_supported).  A [M,C] bf16; b1 fp32 [4C]; b2, ls fp32 [C];
 * w1img / w2img: DEVICE copies of the bf16 chunk images fvhd_ffn_pack writes on the host from fc1.weight [4C][C] and
 * fc2.weight [C][4C] (fp32, the reference's layouts): per chunk of 32 hidden units a 64*C-byte image in the kernel's
 * LDS byte order (XOR-swizzled 16-B slots; fc2's hidden axis permuted inside the chunk so that position 16kb+8half+j
 * holds hidden unit 16kb+8(j>>2)+4half+(j&3)).  Sizes: w1img (4C/32 + 1) * 64*C bytes (last chunk zero), w2img 4C/32 * 64*C.
 * Element types of the images by `precision`: FVHD_FFN_HALF - bf16(fc1 / 4) and IEEE half f16(4 * fc2), the kernel's hidden activation
 * is gelu(x) / 4 in f16 (11 mantissa bits instead of bf16's 8; |Phi error| <= 1.4e-3; saturates at |x| = 262016); FVHD_FFN_BF16 -
 * bf16(fc1), bf16(fc2), f32 GELU, bf16 hidden operand (no range limit).  The images are opaque to callers: pack with fvhd_ffn_pack of
 * the same library build and run them with the SAME precision. */
int fvhd_ffn_fused_supported(int C);
int fvhd_ffn_pack(int C, const float* host_fc1, const float* host_fc2, void* host_w1img, void* host_w2img, int precision);
int fvhd_op_ffn_fused(fvhd_stream_t stream, const void* A, const void* w1img, const float* b1, const void* w2img,
                      const float* b2, const float* ls, void* X, int M, int C, int precision);

/* Image preprocessing of ONE image on the device - `process_images` / `expand2square` (llava/mm_utils.py:154-184) around the
 * tower's CLIPImageProcessor (mobileclip_encoder.py:45-49): canvas of the background colour, Pillow's 8-bit bicubic resample
 * (Resample.c, bit-exact: fixed-point taps with 22 fractional bits, horizontal pass rounded to uint8, then vertical), centre crop,
 * x * (1/255).  src: uint8 HWC RGB [src_h][src_pitch bytes] sitting at (pad_top, pad_left) of the canvas, bg = 0xBBGGRR.
 * hbounds / vbounds: int32 [R][2] (first canvas column / row, tap count) and hcoef / vcoef: int32 [R][hk | vk] for the R cropped
 * output columns / rows (ml_fastvlm_amd/preprocess.py computes them like `precompute_coeffs` + `normalize_coeffs_8bpc`);
 * tmp: nrows * R * 3 bytes of scratch for the canvas rows [row0, row0 + nrows) the vertical taps touch; lut: 256 floats
 * (value * scale as the reference rounds it); out: [3][R][R] of out_dtype.  All pointers are device pointers. */
int fvhd_op_preprocess(fvhd_stream_t stream, const void* src, int src_h, int src_w, int64_t src_pitch, int pad_top, int pad_left,
                       uint32_t bg, const int32_t* hbounds, const int32_t* hcoef, int hk, const int32_t* vbounds, const int32_t* vcoef,
                       int vk, int row0, int nrows, void* tmp, const float* lut, int R, void* out, int out_dtype);

/* ---- multimodal embedding splice --------------------------------------------------
 * The data movement of LlavaMetaForCausalLM.prepare_inputs_labels_for_multimodal (llava_arch.py:233-332) as one gather:
 * out[b, t] = embedding-table row of a text token, a row of the image features, or zeros (padding), plus attention mask,
 * position ids and labels of that position.  The host side (ml_fastvlm_amd/splice.py: splice_plan) supplies, per input
 * position [B, L]: `start` = first output position of the token inside its spliced sequence (non-decreasing; dropped
 * positions carry their successor's value), `feat_row0` = first row of the image in `feats` for a -200 token, -1 for text;
 * `seqlen[b]` = length of the spliced (and truncated) sequence.  table [vocab, H], feats [n_feat_rows, H], out
 * [B, max_len, H] of `dtype`; mask_out (uint8), pos_out, labels_out (int64) [B, max_len], labels_in [B, L], each may be NULL.
 * left_pad != 0 = tokenizer_padding_side "left" (llava_arch.py:306).  All pointers are device pointers. */
int fvhd_op_splice(fvhd_stream_t stream, const int64_t* ids, const int32_t* start, const int32_t* seqlen, const int64_t* feat_row0,
                   const int64_t* labels_in, const void* table, const void* feats, void* out, uint8_t* mask_out, int64_t* pos_out,
                   int64_t* labels_out, int B, int L, int H, int max_len, int64_t vocab, int64_t n_feat_rows, int left_pad, int dtype);

/* GEMM epilogues added for the LLM prefill (fvhd_op_gemm) */
#define FVHD_EPI_RESID 4         /* out = resid + A.W^T                           (Qwen2 o_proj / down_proj + the layer's skip) */
#define FVHD_EPI_SWIGLU 5        /* out[m][j] = silu(acc[m][2j]) * acc[m][2j+1]; out is [M, N/2]; W rows interleaved gate_j, up_j */

/* ---- LLM prefill: Qwen2 decoder stack on the spliced embeddings --------------------
 * Replaces the prefill call the reference makes into the third-party `transformers` Qwen2ForCausalLM (pinned 4.48.3,
 * pyproject.toml:17): `LlavaQwen2ForCausalLM.forward` -> `super().forward(inputs_embeds=...)` (llava/model/language_model/
 * llava_qwen.py:92-103) and the first step of `generate` (:138-143).  One context per (device, model); weights arrive under the
 * model's own state-dict keys.  Arithmetic: bf16 rows, fp32 accumulation / statistics, like the tower.
 *   hidden, n_layers, n_heads, n_kv_heads, head_dim (64 | 128), intermediate, vocab, rms_eps, rope_theta = the fields of Qwen2Config
 *   (Qwen2-0.5B: 896, 24, 14, 2, 64, 4864, 151936, 1e-6, 1e6;  Qwen2-7B: 3584, 28, 28, 4, 128, 18944, 152064). */
typedef struct fvhd_llm fvhd_llm;
int fvhd_llm_create(fvhd_llm** out, int device, int hidden, int n_layers, int n_heads, int n_kv_heads, int head_dim, int intermediate,
                    int vocab, float rms_eps, float rope_theta);
void fvhd_llm_destroy(fvhd_llm* ctx);
/* One tensor of the state dict: key = "model.layers.<l>.{input_layernorm,post_attention_layernorm}.weight",
 * "model.layers.<l>.self_attn.{q,k,v}_proj.{weight,bias}", "model.layers.<l>.self_attn.o_proj.weight",
 * "model.layers.<l>.mlp.{gate,up,down}_proj.weight", "model.norm.weight", "lm_head.weight" (the embedding table when the
 * model ties them; the leading "model." may be absent), and - optional, for the decode of a model that does not tie them -
 * "model.embed_tokens.weight".  host_data: contiguous HOST memory of `dtype` (FVHD_F32 / F16 / BF16) in the
 * reference's [out, in] layout; converted (matrices to bf16, vectors to fp32), packed (q|k|v rows concatenated, gate / up rows
 * interleaved) and uploaded before the call returns.  Any other key is an error. */
int fvhd_llm_set_tensor(fvhd_llm* ctx, const char* key, const void* host_data, int dtype, const int64_t* shape, int ndim);
/* The same tensor from DEVICE memory on the context's device (a model that already lives on the GPU): matrices must be FVHD_BF16 and
 * vectors FVHD_F32, row-major contiguous; packed by one device-to-device (2-D) copy on `stream` - no host round trip.  The caller keeps
 * dev_data alive until `stream` has run the copy.  STREAM CONTRACT (round 5): the copies are asynchronous; fvhd_llm_finalize waits (on the
 * host) for all of them, so after it returns a prefill may run on ANY stream; a tensor re-set after fvhd_llm_finalize is ordered before
 * the next fvhd_llm_prefill by an event (stream wait; a host wait when that prefill's stream is being captured). */
int fvhd_llm_set_tensor_device(fvhd_llm* ctx, const char* key, const void* dev_data, int dtype, const int64_t* shape, int ndim,
                               fvhd_stream_t stream);
int fvhd_llm_finalize(fvhd_llm* ctx);                          /* fails if a tensor is missing */
/* Qwen2Config.max_position_embeddings: rows of the rotary table (default 8192; at most 65536 rows are tabulated).  Position ids beyond
 * the table are legal: the rotary kernel then computes cos / sin itself with the table's formula - it never clamps.  Takes effect at the
 * next workspace allocation: call it before fvhd_llm_reserve / the first prefill. */
int fvhd_llm_set_max_positions(fvhd_llm* ctx, int max_position_embeddings);
int fvhd_llm_reserve(fvhd_llm* ctx, int batch, int seq_len);   /* size the workspace now (synchronises; not during stream capture) */
/* Number of times the workspace has been (re)allocated.  A prefill captured into a CALLER's hipGraph holds workspace pointers: the
 * library never frees a workspace that a capturing stream has used (a later, larger prefill allocates a new one and keeps the old one
 * alive until fvhd_llm_destroy), so such a graph stays valid; a change of this counter tells the caller that a re-capture would pick up
 * the new, larger workspace. */
int fvhd_llm_workspace_generation(const fvhd_llm* ctx);
/* Prefill: embeds [batch, seq_len, hidden] of `dtype` (the `inputs_embeds` of prepare_inputs_labels_for_multimodal / fvhd_op_splice),
 * key_valid uint8 [batch, seq_len] (its attention mask; NULL = all valid), position_ids int64 [batch, seq_len] (NULL = 0..seq_len-1)
 * -> logits_out fp32 [batch, vocab] of the LAST position of every sequence (what generate() samples the first token from).
 * k_cache / v_cache: NULL, or bf16 [n_layers][batch][n_kv_heads][seq_len][head_dim] each - the rotated keys and the values, in the
 * layout of transformers' cache layers, for a decode loop to continue from.  Enqueued on `stream`, capture-safe after fvhd_llm_reserve. */
int fvhd_llm_prefill(fvhd_llm* ctx, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch,
                     int seq_len, float* logits_out, void* k_cache, void* v_cache, fvhd_stream_t stream);
/* tests: hidden states after the last decoder layer (before the final norm) of the previous prefill, [rows, hidden] bf16 */
int fvhd_llm_debug_hidden(fvhd_llm* ctx, void* out, int rows, fvhd_stream_t stream);

/* single ops of the prefill (unit-test entry points) */
/* Qwen2RMSNorm: y = w * x * rsqrt(mean(x^2) + eps); x, y [M, H] bf16 (may alias), w fp32 [H], H % 8 == 0 */
int fvhd_op_rmsnorm(fvhd_stream_t stream, const void* x, void* y, const float* w, int M, int H, float eps);
/* apply_rotary_pos_emb (rotate_half form) in place on the q and k heads of qkv [M, (n_heads + 2 n_kv_heads) * head_dim] bf16;
 * pos int64 [M] or NULL (row % T); table fp32 [table_positions][head_dim / 2][2] = (cos, sin) - a position outside [0, table_positions)
 * is computed in the kernel from rope_theta (inv_freq_i = theta^(-2i / head_dim), fp32), never clamped; k_cache / v_cache as fvhd_llm_prefill
 * for ONE layer ([M / T][n_kv_heads][T][head_dim]) or NULL */
int fvhd_op_rope(fvhd_stream_t stream, void* qkv, const int64_t* pos, const float* table, void* k_cache, void* v_cache, int M, int T,
                 int n_heads, int n_kv_heads, int head_dim, int table_positions, float rope_theta);
/* The q|k|v projection with everything that follows it in Qwen2Attention.forward in ONE launch (round 5): out = A . Wt^T + bias rounded to bf16,
 * then - on the q and k heads of the M real rows - the rotary embedding exactly as fvhd_op_rope applies it, then the KV-cache copies; bit-identical
 * to fvhd_op_gemm(EPI_BIAS) + fvhd_op_rope.  head_dim 64 only (a wave's 64-column block of the output tile is one head, and since the round-5 tile
 * fill a lane holds both members of every rotate_half pair); fvhd_gemm_qkv_rope_supported(Mp, N, K, head_dim, n_heads, n_kv_heads) tells whether a
 * shape takes it (Mp % 128 == 0 rows incl. padding, N = (n_heads + 2 n_kv_heads) * 64, K % 64 == 0, at most one 128 x 128 tile per CU) -
 * fvhd_llm_prefill uses it when FVHD_LLM_FUSEROPE=1 is set at fvhd_llm_create (measured neutral: the launch saved comes back as epilogue time -
 * profiles/r05_ttft_fuserope_ab.log - so the default keeps the two launches).  A [Mp, K], Wt [N, K] bf16; bias fp32 [N]; the rest as fvhd_op_rope. */
int fvhd_gemm_qkv_rope_supported(int Mp, int N, int K, int head_dim, int n_heads, int n_kv_heads);
int fvhd_op_gemm_qkv_rope(fvhd_stream_t stream, const void* A, const void* Wt, const float* bias, void* out, int Mp, int N, int K, const int64_t* pos,
                          const float* table, void* k_cache, void* v_cache, int M, int T, int n_heads, int n_kv_heads, int head_dim,
                          int table_positions, float rope_theta);
/* out = resid + A . Wt^T with K split over `splits` workgroups per output tile (Qwen2 down_proj at prefill: few tiles, long K):
 * A [M, K], Wt [N, K], resid [M, N] or NULL (may alias out), out [M, N] bf16; partial: fp32 scratch [splits][M][N]; the slices are
 * summed in order (deterministic) and rounded once.  N % 128 == 0, K % (64 * splits) == 0. */
int fvhd_op_gemm_splitk(fvhd_stream_t stream, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N,
                        int K, int splits);
/* the same, and norm_out = Qwen2RMSNorm(out) with weight norm_w (fp32 [N]) from the reduce kernel's own pass over the finished rows - the
 * norm the next operation of a decoder layer starts with (transformers Qwen2DecoderLayer.forward: post_attention_layernorm behind o_proj,
 * input_layernorm of the next layer behind down_proj).  Both outputs are bit-identical to fvhd_op_gemm_splitk followed by fvhd_op_rmsnorm.
 * norm_out [M, N] bf16 must not alias out. */
int fvhd_op_gemm_splitk_norm(fvhd_stream_t stream, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N,
                             int K, int splits, const float* norm_w, void* norm_out, float eps);
/* the q|k|v projection of a decoder layer as a split-K GEMM whose reduce finishes the projection: qkv = bf16(A . Wt^T + bias) rows
 * [M, (n_heads + 2 n_kv_heads) * head_dim], then fvhd_op_rope's rotation of the q and k heads and cache copies, in one pass
 * (bit-identical to the separate steps on the same partial sums).  A [Mp, K] bf16 with Mp >= M rows readable (Mp = M rounded up to 128),
 * partial: fp32 scratch [splits][Mp][width]; width % 128 == 0, K % (64 * splits) == 0.  Replaces transformers Qwen2Attention.forward's
 * q_proj / k_proj / v_proj + apply_rotary_pos_emb + DynamicCache.update. */
int fvhd_op_qkv_splitk_rope(fvhd_stream_t stream, const void* A, const void* Wt, const float* bias, float* partial, void* qkv, const int64_t* pos,
                            const float* table, void* k_cache, void* v_cache, int M, int Mp, int K, int T, int n_heads, int n_kv_heads, int head_dim,
                            int table_positions, float rope_theta, int splits);
/* causal grouped-query attention with a key-padding mask: qkv [B*T, (n_heads + 2 n_kv_heads) * head_dim] bf16 ->
 * out [B*T, n_heads * head_dim] bf16; key_valid uint8 [B, T] or NULL; head_dim in {64, 128} */
int fvhd_op_attention_causal(fvhd_stream_t stream, const void* qkv, void* out, const uint8_t* key_valid, int B, int T, int n_heads,
                             int n_kv_heads, int head_dim);

/* ---- LLM decode: generation on the library's own KV cache --------------------------------------------------------------------------
 * After a prefill, one new token per sequence per call, with greedy selection on the device - what transformers' greedy generate loop
 * does after its first forward, on the same packed weights as the prefill (no further weight copy).  Per decoder layer 5 launches:
 * [RMSNorm + q|k|v GEMM + bias + rotary + cache append] [attention over the cache] [o_proj + residual] [RMSNorm + gate|up + silu * up]
 * [down_proj + residual], then [final RMSNorm + lm_head + per-workgroup argmax] [argmax reduce + advance]; the GEMMs stream the weights
 * once (B <= 64 rows: a weight fragment multiplies ceil(B / 16) tiles of 16 rows), fp32 accumulation, deterministic split-K reductions (identical bits run to run).
 * Everything that changes from step to step - the cache slot, the positions, the mask column - lives in device memory and is advanced by
 * the step itself: the host arguments of fvhd_llm_decode are the same for every token, so ONE captured graph replays a whole generation. */
/* The decode's input embedding.  model.embed_tokens.weight [vocab, hidden] (fvhd_llm_set_tensor(_device); optional for the prefill and
 * fvhd_llm_finalize) is used whenever it was set.  Without it, tied != 0 declares that the model ties its embeddings
 * (tie_word_embeddings: Qwen2-0.5B / 1.5B) and the decode embeds through the packed lm_head rows.  Nothing is assumed: until one of the
 * two is done - or after tied == 0 without the embedding table - fvhd_llm_start / fvhd_llm_decode fail with an error. */
int fvhd_llm_set_tied_embeddings(fvhd_llm* ctx, int tied);
/* Allocates the cache: K and V bf16 [n_layers][batch][n_kv_heads][capacity][head_dim] (transformers' per-layer layout with a capacity
 * stride), the key-valid mask [batch][capacity], the next position of every sequence (int64 [batch]), the current length, the last chosen
 * ids, the error word and the decode workspace.  1 <= batch <= 64; hidden, n_heads * head_dim and intermediate multiples of 128.
 * Synchronises (refused while a stream is being captured); replaces an earlier cache (a graph captured on it is then invalid). */
int fvhd_llm_cache_reserve(fvhd_llm* ctx, int batch, int capacity);
/* fvhd_llm_prefill's arithmetic on embeds [batch, seq_len, hidden] (batch <= the reserved batch, seq_len <= capacity), then: its rotated
 * K / V in cache slots [0, seq_len), key_valid (NULL = all valid) as the mask, length = seq_len, next position of sequence b =
 * position_ids[b, seq_len - 1] + 1 (NULL: seq_len), the error word cleared.  logits_out: NULL or fp32 [batch, vocab] of the last
 * position; next_ids_out: NULL or int64 [batch] = their argmax (ties: the lowest index, as torch.argmax). */
int fvhd_llm_start(fvhd_llm* ctx, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch, int seq_len,
                   float* logits_out, int64_t* next_ids_out, fvhd_stream_t stream);
/* One step: token_ids int64 [batch] on the device, or NULL = the ids the previous start / decode chose; appends their k / v at slot
 * `length` with mask 1, advances length and positions by one, and writes logits_out (NULL or fp32 [batch, vocab]) and next_ids_out
 * (NULL or int64 [batch]).  A step past `capacity` (or given an id outside [0, vocab)) writes nothing and sets a sticky error word that the
 * next fvhd_llm_decode reports as an error (fvhd_llm_cache_state reads it at once).  Capture-safe after fvhd_llm_start.
 * token_ids = NULL is refused behind fvhd_llm_cache_rewind / fvhd_llm_cache_gather (see there).  Ends a lookup generation. */
int fvhd_llm_decode(fvhd_llm* ctx, const int64_t* token_ids, float* logits_out, int64_t* next_ids_out, fvhd_stream_t stream);
/* synchronises the device, then: the cache length and the error word (0 = fine, 1 = past capacity, 2 = token id out of range, 3 = a
 * cache reorder's row index out of range, 4 = a cache rewind's keep length out of range) */
int fvhd_llm_cache_state(fvhd_llm* ctx, int* length, int* status);

/* ---- LLM sampling: temperature / top-k / top-p on the device ------------------------------------------------------------------------
 * transformers' multinomial sampling for num_beams = 1 (TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper in that order,
 * min_tokens_to_keep = 1): s = logits / temperature (IEEE fp32 division); top_k >= 1 keeps s >= the min(top_k, V)-th largest value, ties
 * included (0 = off); top_p in [0, 1) keeps a token when the normalised mass of the tokens before it in descending s is < top_p, the top
 * token always (1 = off); then one draw from the softmax over the kept set.  The kept set is {s >= theta, s > -inf}: a -inf logit is
 * never kept, counted or drawn, and tokens tied exactly at the top-p boundary are kept as a group, where transformers' unstable sort may
 * split them.  A row needs at least one finite logit: the result for a row of -inf only (or with a NaN) is undefined, as it is in
 * transformers (softmax of such a row is NaN).  The draw is the inverse CDF in token-index order:
 * the smallest kept index whose prefix mass exceeds u * Z, Z = sum of exp(s - s_max) over the kept set.  u = (x0 >> 8) * 2^-24 of
 * Philox4x32-10 with key (seed low word, seed high word) and counter (row, n, 0, 0), row = the sequence's row in the batch, n = the cache length when the token is chosen (the
 * prompt length for the token fvhd_llm_start chooses, + 1 per decode step).  Only the distribution equals torch.multinomial's, not its
 * draws.  Deterministic: the same logits, settings, seed and n give the same id, eager or replayed from a graph.
 * do_sample = 0 (the default) is greedy, what fvhd_llm_start / fvhd_llm_decode did before: the argmax, bit for bit.  The settings are read
 * when fvhd_llm_start / fvhd_llm_decode enqueue, so a captured graph keeps those it was captured with.  Refused: a temperature that is
 * not finite or not > 0, top_k < 0, top_p outside [0, 1].  With sampling, the step writes its logits to the caller's logits_out or to the
 * context's own buffer, and replaces the argmax reduce by the sampler's launches (llm_sample.hip). */
int fvhd_llm_set_sampling(fvhd_llm* ctx, int do_sample, float temperature, int top_k, float top_p, unsigned long long seed);
/* the sampler on its own (tests): logits fp32 [B, V] (1 <= B <= 16, V >= 1) -> ids int64 [B]; n = the Philox counter's second word;
 * u_override: NULL (Philox) or fp32 [B]; info: NULL or fp32 [B, 4] = (theta, kept count, Z, u).  Allocates a process-wide workspace on
 * first use: eager calls only, not during stream capture. */
int fvhd_op_dec_sample(fvhd_stream_t stream, const float* logits, int B, int V, float temperature, int top_k, float top_p, unsigned long long seed,
                       int n, const float* u_override, int64_t* ids, float* info);
/* the sampler on the T rows of ONE sequence (tests; added under 510): the mode a verify step under sampling uses.  logits fp32 [T, V]
 * (1 <= T <= 16) -> ids int64 [T]; row r draws with the Philox counter (seq_row, n0 + r, 0, 0), so it equals fvhd_op_dec_sample on that row
 * alone (B = 1) at n = n0 + r when seq_row = 0.  u_override / info: as above, indexed by r.  state_last (int64 [T]), state_position (int64
 * [T]) and state_length (int): each NULL or device memory that goes into the launch where a decode step passes its last ids, positions and
 * the length to advance - this mode writes none of them.  Eager calls only. */
int fvhd_op_dec_sample_rows(fvhd_stream_t stream, const float* logits, int T, int V, float temperature, int top_k, float top_p,
                            unsigned long long seed, int seq_row, int n0, const float* u_override, int64_t* ids, float* info,
                            int64_t* state_last, int64_t* state_position, int* state_length);

/* The warpers transformers applies between top-p and the draw, in its order: min_p, typical_p, epsilon_cutoff, eta_cutoff (MinPLogitsWarper,
 * TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper; min_tokens_to_keep = 1).  Each acts on the set K the earlier ones left; with
 * M = s_max of the row, e = expf(s - M), Z = sum of e over K and A = sum of e (s - M) over K / Z:
 *   min_p in (0, 1]          keeps e >= min_p (p >= min_p * p_max);
 *   typical_p in (0, 1)      keeps the tokens of smallest d = |(s - M) - A| (= |-log p - H|) until their mass reaches typical_p * Z: a group of
 *                            equal d is kept iff the mass of the groups before it is < typical_p * Z, the first group always;
 *   epsilon_cutoff in (0, 1) keeps e >= epsilon_cutoff * Z, and the tokens tied at the largest s of K;
 *   eta_cutoff in (0, 1)     the same with eta = min(eta_cutoff, sqrt(eta_cutoff) * exp(-H)), H = log Z - A.
 * Off values: 0, 1, 0, 0 (the default), and then a sampled step enqueues what it did without this call, launch for launch and bit for
 * bit.  Refused, naming the value: min_p outside [0, 1], typical_p outside (0, 1], a cutoff outside [0, 1), a NaN.  The settings are read
 * when start / decode / extend / verify enqueue, like the sampling settings, and have no effect unless do_sample is on; fvhd_llm_set_sampling
 * leaves them alone.  Z and A are sums of 2^-40 fixed-point terms, so they do not depend on the order of the adds: the result is
 * deterministic like the rest of the sampler, and the sampler's workspace is what it was (llm_sample.hip). */
int fvhd_llm_set_sampling_warpers(fvhd_llm* ctx, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff);
/* the sampler with all seven settings on its own (tests).  seq_rows = 0: fvhd_op_dec_sample's mode, logits fp32 [B, V] with 1 <= B <= 64
 * (seq_row is ignored, n = the counter's second word); seq_rows = 1: fvhd_op_dec_sample_rows' mode, B = T <= 16 rows of one sequence, row r
 * draws with the counter (seq_row, n + r, 0, 0).  u_override: NULL or fp32 [B]; info: NULL or fp32 [B, 8] = (lowest kept s, final kept
 * count, Z of the final set, u, highest kept s, kept count behind min_p, behind typical_p, behind epsilon_cutoff).  Eager calls only. */
int fvhd_op_dec_sample_warpers(fvhd_stream_t stream, const float* logits, int B, int V, float temperature, int top_k, float top_p, float min_p,
                               float typical_p, float epsilon_cutoff, float eta_cutoff, unsigned long long seed, int seq_rows, int seq_row, int n,
                               const float* u_override, int64_t* ids, float* info);

/* single ops of the decode step (unit-test entry points); B in [1, 64]; K % 128 == 0; `splits` = workgroups per output tile along K
 * (partial: fp32 scratch [splits][N * 16 * ceil(B / 16)], counters: int [ceil(N / 64)] ZEROED before the first call - each launch leaves them zero)
 * out = epilogue(rmsnorm?(x) . Wt^T): x [B, K] bf16, norm_w fp32 [K] or NULL (no norm), Wt [N, K] bf16; FVHD_EPI_RESID: out [B, N] =
 * resid + acc (resid may alias out); FVHD_EPI_SWIGLU: out [B, N / 2] = silu(acc[2j]) * acc[2j + 1] (gate / up rows interleaved). */
int fvhd_op_dec_gemm(fvhd_stream_t stream, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, int N, int K, const void* resid,
                     void* out, float* partial, int* counters, int splits);
/* the q|k|v projection of one decode step: bf16(rmsnorm?(x) . Wt^T + bias), rotary embedding (fvhd_op_rope's) of the q and k heads at
 * position pos[b] (int64 [B]), q -> q_out [B, n_heads * head_dim], k / v -> k_cache / v_cache [>= B][n_kv_heads][capacity][head_dim] at slot
 * *length (a device int) */
int fvhd_op_dec_qkv(fvhd_stream_t stream, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const float* bias, void* q_out,
                    const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache, void* v_cache, int capacity,
                    const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters, int splits);
/* single-query grouped-query attention over cache keys [0, *length) of every sequence: q [B, n_heads * head_dim] bf16, caches as above,
 * key_valid uint8 [>= B][capacity] -> out [B, n_heads * head_dim] bf16; head_dim 64 / 128.  partial: fp32 [B * n_heads * splits * (head_dim + 2)],
 * counters: int [B * n_heads] zeroed */
int fvhd_op_dec_attention(fvhd_stream_t stream, const void* q, const void* k_cache, const void* v_cache, const uint8_t* key_valid, void* out, int B,
                          int n_heads, int n_kv_heads, int head_dim, int capacity, const int* length, float* partial, int* counters, int splits);
/* final norm + lm_head + argmax: logits (NULL or fp32 [B, V]) = rmsnorm?(x) . Wt^T, ids_out int64 [B] = argmax (lowest index on ties);
 * scratch_v / scratch_i: [ceil(V / 64) * 16 * ceil(B / 16)] each */
int fvhd_op_dec_lm_argmax(fvhd_stream_t stream, const void* x, int B, const float* norm_w, float eps, const void* Wt, int V, int K, float* logits,
                          int64_t* ids_out, float* scratch_v, int* scratch_i);

/* ---- LLM 8-bit weights: the packed matrices as OCP e4m3 codes with one scale per output row (version 504) ---------------------------------
 * Weight-only storage: a matrix W [N, K] (the reference's [out, in] layout) is held as K e4m3 codes (gfx950's e4m3fn: no infinity,
 * maximum 448) per row plus scale[n] (fp32); row n stands for code * scale[n].  The arithmetic does not change: the decode GEMMs convert the
 * codes to bf16 in registers (exact), multiply the same bf16 activation fragments on the same 16 x 16 x 32 MFMA with fp32 accumulation and
 * apply the row scale to the finished accumulator (after the split-K sum, before bias / residual / SwiGLU / logits); the prefill dequantises
 * each matrix into a bf16 scratch (the size of the largest matrix, lm_head included) right before its bf16 GEMM.  The step streams half the
 * bytes and the packed copy occupies half the bytes; no bf16 copy of the matrices is kept.  Vectors (norm weights, biases), the KV cache,
 * the activations and model.embed_tokens.weight (a row gather) stay as they are; a tied model's decode embeds through the dequantised
 * lm_head rows.
 * The library's quantiser uses POWER-OF-TWO scales: scale = 2^ceil(log2(amax_row / 448)) (kept >= 2^-126; an all-zero row: scale 1, codes 0),
 * codes = w / scale rounded to nearest even; amax / scale lies in (224, 448], nothing saturates.  code * scale is then exactly a bf16
 * value, so the prefill (bf16 code * scale) and the decode (scale applied in fp32 to the accumulator) work on identical weight values, and a
 * stock bf16 / fp32 model holding the dequantised weights is an exact-weight oracle.  The single ops below accept any positive finite fp32
 * scale; only powers of two keep that identity. */
#define FVHD_W_BF16 0
#define FVHD_W_E4M3 1
/* The storage format of the packed matrices (lm_head.weight included).  Call it right after fvhd_llm_create: once a tensor was set it fails
 * with an error (both fvhd_llm_set_tensor paths quantise matrices as they arrive).  FVHD_W_E4M3 needs hidden, n_heads * head_dim and
 * intermediate to be multiples of 128; so does FVHD_W_MXFP4 ("LLM 4-bit weights" below).  Re-allocates the weight buffer (and the
 * dequantisation scratch). */
int fvhd_llm_set_weight_format(fvhd_llm* ctx, int format);
/* device bytes held by the packed weights: matrices, row scales, norm weights and biases (not the workspace, the caches, the optional
 * embedding table or the e4m3 dequantisation scratch) */
int fvhd_llm_weight_bytes(const fvhd_llm* ctx, size_t* bytes);
/* tests: one packed matrix of an FVHD_W_E4M3 context in plain [N, K] order (the K order inside the weight buffer is private):
 * codes_out u8 [N][K], scale_out fp32 [N], device pointers.  FVHD_MAT_QKV: q | k | v rows [(n_heads + 2 n_kv_heads) * head_dim, hidden];
 * FVHD_MAT_GATE_UP: gate / up rows interleaved [2 * intermediate, hidden]; FVHD_MAT_LM_HEAD ignores `layer`. */
#define FVHD_MAT_QKV 0
#define FVHD_MAT_O 1
#define FVHD_MAT_GATE_UP 2
#define FVHD_MAT_DOWN 3
#define FVHD_MAT_LM_HEAD 4
int fvhd_llm_debug_packed_e4m3(fvhd_llm* ctx, int layer, int matrix, void* codes_out, float* scale_out, fvhd_stream_t stream);
/* the quantiser on its own: W bf16 [N, K] (K % 8 == 0) -> codes u8 [N, K] (row-major, k order), scale fp32 [N]; codes equal torch's
 * (w / scale).to(torch.float8_e4m3fn) bit for bit */
int fvhd_op_quantize_e4m3(fvhd_stream_t stream, const void* W, int N, int K, void* codes, float* scale);
/* fvhd_op_dec_gemm / _qkv / _lm_argmax on e4m3 weights: the same arguments plus `scale` (fp32 [N]), Wt = plain row-major codes u8 [N, K].
 * With every scale = 1 the output has the bits of the bf16 op on bf16(codes).  The codes are first repacked into a process-wide scratch
 * (allocated on demand): eager calls only, not during stream capture. */
int fvhd_op_dec_gemm_w8(fvhd_stream_t stream, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, const float* scale, int N,
                        int K, const void* resid, void* out, float* partial, int* counters, int splits);
int fvhd_op_dec_qkv_w8(fvhd_stream_t stream, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const float* scale,
                       const float* bias, void* q_out, const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache,
                       void* v_cache, int capacity, const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters,
                       int splits);
int fvhd_op_dec_lm_argmax_w8(fvhd_stream_t stream, const void* x, int B, const float* norm_w, float eps, const void* Wt, const float* scale, int V,
                             int K, float* logits, int64_t* ids_out, float* scratch_v, int* scratch_i);

/* ---- LLM 4-bit weights: the packed matrices as OCP MXFP4 - e2m1 codes with one power-of-two scale per 32 elements (added under 510) ---------
 * Weight-only storage, 4.25 bits per weight.  A matrix W [N, K] (K % 128 == 0, the e4m3 rule), in plain order for the single ops and the
 * read-back:
 *   codes  u8 [N, K / 2]   element k is in byte k / 2, even k in the low nibble; a code is sign (bit 3) + an index (bits 2..0) into
 *                          {0, 0.5, 1, 1.5, 2, 3, 4, 6}
 *   scales u8 [N, K / 32]  byte E stands for 2^(E - 127) (e8m0), one per block of 32 consecutive k of a row
 * and element (n, k) stands for code * 2^(E - 127), which is exactly a bf16 value.  The arithmetic does not change: the decode GEMMs turn a
 * dword of codes and its block scale into the bf16 MFMA fragment in registers (v_cvt_scalef32_pk_bf16_fp4, exact) - the very operand the
 * bf16 kernels load from the dequantised matrix - and run the same MFMAs in the same order; nothing scales the accumulator.  So every op
 * below, and every call on an FVHD_W_MXFP4 context, has the BITS of its bf16 counterpart on the dequantised matrices.  The prefill / extend /
 * score path dequantises each matrix into the bf16 scratch of the e4m3 format (same size rule) right before its GEMM; a tied model's decode
 * embeds through the dequantised lm_head rows.  The K order inside the weight buffer is private.
 * The library's quantiser (both fvhd_llm_set_tensor paths, each source tensor on its own; fvhd_op_quantize_mxfp4), per block:
 * se = ceil(log2(amax / 6)) evaluated exactly from amax's bf16 exponent and mantissa (amax = m 2^e, m in [1, 2): e - 2 + (m > 1.5)), clamped
 * to [-125, 125], 0 for an all-zero block, E = se + 127 in [2, 252]; codes = w / 2^se rounded to the nearest grid value, ties to the even
 * index, saturating at 6 (only at the upper clamp); the sign bit is w's (a small negative becomes -0).  amax / 2^se lies in (3, 6].  This is
 * a COARSE format: the relative L2 error of a Gaussian matrix is about 0.12 (e4m3 with row scales: 0.036). */
#define FVHD_W_MXFP4 2      /* fvhd_llm_set_weight_format: the e4m3 rules (before the first tensor; hidden, n_heads * head_dim, intermediate % 128) */
/* tests: one packed matrix of an FVHD_W_MXFP4 context in plain order: codes_out u8 [N][K / 2], scales_out u8 [N][K / 32], device pointers;
 * layer / matrix as for fvhd_llm_debug_packed_e4m3 */
int fvhd_llm_debug_packed_mxfp4(fvhd_llm* ctx, int layer, int matrix, void* codes_out, void* scales_out, fvhd_stream_t stream);
/* the quantiser on its own: W bf16 [N, K] (K % 32 == 0, 16-byte aligned) -> codes u8 [N, K / 2], scales u8 [N, K / 32] */
int fvhd_op_quantize_mxfp4(fvhd_stream_t stream, const void* W, int N, int K, void* codes, void* scales);
/* fvhd_op_dec_gemm / _qkv / _lm_argmax on MXFP4 weights: the _w8 signatures with `codes, scales` (plain order, 4-byte aligned) in place of
 * `codes, scale`.  Any scale byte whose products stay finite and normal is accepted.  The codes are first repacked into a process-wide scratch
 * (allocated on demand): eager calls only, not during stream capture. */
int fvhd_op_dec_gemm_w4(fvhd_stream_t stream, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, const void* scales, int N,
                        int K, const void* resid, void* out, float* partial, int* counters, int splits);
int fvhd_op_dec_qkv_w4(fvhd_stream_t stream, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const void* scales,
                       const float* bias, void* q_out, const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache,
                       void* v_cache, int capacity, const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters,
                       int splits);
int fvhd_op_dec_lm_argmax_w4(fvhd_stream_t stream, const void* x, int B, const float* norm_w, float eps, const void* Wt, const void* scales, int V,
                             int K, float* logits, int64_t* ids_out, float* scratch_v, int* scratch_i);
/* the layout kernel on its own (tests; K % 128 == 0): mode 0: codes in the private K order + scales -> bf16 [N, K] (dst 16-byte aligned);
 * 1: private order -> plain codes; 2: plain -> private order (scales are in k order either way and may be NULL for modes 1, 2) */
int fvhd_op_w4_unpack(fvhd_stream_t stream, const void* src, const void* scales, void* dst, int N, int K, int mode);

/* ---- LLM beam search: the top continuations and the KV-cache reorder on the device (version 505) -------------------------------------------
 * transformers' `GenerationMixin._beam_search` keeps, per prompt, K = num_beams running hypotheses: K beams of G prompts are G * K rows of
 * the decode step (row g * K + k = beam k of prompt g).  Per step it needs two operations on [rows, vocab] / cache-sized data; the rest is
 * [G, 2 K] bookkeeping that the caller does (ml_fastvlm_amd/beam.py).
 * Top continuations (step b + `_get_top_k_continuations`): acc[k * V + v] = ((logit[g K + k][v] - max_row) - log sum_v exp(logit - max_row))
 * + score[g][k] in fp32, and per prompt its `keep` largest values in descending order with their flat indices k * V + v; equal values: the
 * lower flat index first.  (A row's candidates are pre-selected by their raw logit, ties to the lower index: two logits of one row that
 * differ but round to one accumulated value keep the order of the logits.)  2 <= num_beams <= 16, keep <= 64, keep <= vocab,
 * groups * num_beams <= 64, vocab % 16 == 0, vocab <= 262144.  A row may hold -inf logits; a prompt with fewer than `keep` finite candidates
 * and a row with a NaN are undefined.  A score of -1e9 (a dead beam) is an ordinary input.  Deterministic: fixed summation orders, the same
 * bits eager or replayed.
 * Cache reorder (`Cache.reorder_cache` / index_select of every layer): new row r of K and V of every layer, of the key-valid mask and of
 * the next positions = old row src_rows[r] (int64 [rows_out] on the device, entries in [0, rows_in)), over cache slots [0, length).  Any
 * map is correct (it goes through a scratch, never in place); slots >= length and rows >= rows_out keep their bytes; rows with
 * src_rows[r] == r are not touched.  An index out of range writes nothing and sets the sticky error word to 3.
 * The ids "the previous step chose" are NOT reordered: after the call they belong to the rows as they were before it, so the next call must be
 * fvhd_llm_extend, or fvhd_llm_decode with explicit token_ids; fvhd_llm_decode(token_ids = NULL), fvhd_llm_verify, fvhd_llm_lookup_begin and
 * fvhd_llm_lookup_step are refused, with a message that says so and names the two ways on, until one of those two (or fvhd_llm_start) has
 * been enqueued.  It is an enqueue-time rule of the host, like the settings of the logits processors: a captured step replays as it was
 * captured, whatever was enqueued since.  Ends a lookup generation. */
/* Allocates the reorder's scratch (two layers' K | V of the reserved cache) and the top-K workspace (about 2 MiB), apart from
 * fvhd_llm_cache_reserve's allocation.  Synchronises (refused while a stream is being captured).  fvhd_llm_cache_reserve frees it with
 * the cache it was sized for. */
int fvhd_llm_beam_reserve(fvhd_llm* ctx);
/* The reorder on the context's cache; the later steps run on rows_out sequences (<= the reserved batch; rows_in <= it too).  src_rows =
 * r / num_beams turns G prefilled rows into G * num_beams.  The host arguments are the same every step: capture-safe after
 * fvhd_llm_beam_reserve and fvhd_llm_start.  n_layers + 1 launches.  Refused with logits processors on (their token history is not
 * reordered: the rows would go on with the history of whatever sequence held the row before) - unless fvhd_llm_set_beam_scoring is on, which
 * carries them ("LLM beam search with processors" below). */
int fvhd_llm_cache_gather(fvhd_llm* ctx, const int64_t* src_rows, int rows_in, int rows_out, fvhd_stream_t stream);
/* The top continuations of logits fp32 [groups * num_beams, vocab] (16-byte aligned) and beam_scores fp32 [groups, num_beams] ->
 * cand_scores fp32 [groups, keep], cand_index int64 [groups, keep].  Capture-safe after fvhd_llm_beam_reserve.  3 launches. */
int fvhd_llm_beam_topk(fvhd_llm* ctx, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, float* cand_scores,
                       int64_t* cand_index, fvhd_stream_t stream);
/* the two operations on their own (tests), on plain device pointers; a process-wide scratch, allocated / grown on demand: eager calls
 * only, not during stream capture.  fvhd_op_dec_cache_gather: k_cache / v_cache bf16 [n_layers][batch][n_kv_heads][capacity][head_dim],
 * key_valid uint8 [batch][capacity], positions int64 [batch], length and status device ints (status: as the error word above; nothing
 * happens while *status != 0). */
int fvhd_op_dec_beam_topk(fvhd_stream_t stream, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V,
                          float* cand_scores, int64_t* cand_index);
int fvhd_op_dec_cache_gather(fvhd_stream_t stream, void* k_cache, void* v_cache, uint8_t* key_valid, int64_t* positions, const int64_t* src_rows,
                             int n_layers, int batch, int rows_in, int rows_out, int n_kv_heads, int head_dim, int capacity, const int* length,
                             int* status);

/* ---- LLM beam-search sampling: the top continuations DRAWN, not ranked (added under 510) -----------------------------------------------------
 * transformers' `_beam_search(do_sample=True)` (generate(do_sample=True, num_beams=K)): per step and prompt, log_softmax, then
 * TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper with min_tokens_to_keep = min_keep (n_eos + 1; 2 without an EOS id), +
 * running_beam_scores, and `keep` draws without replacement from softmax over the prompt's K * V values - which is the top `keep` of the values
 * plus independent Gumbel noise - returned in draw order with their UNPERTURBED values.  Per row r = g K + k and token v, x = logits[r][v],
 * M = the row maximum, L = log sum exp(x - M) (the orders of fvhd_llm_beam_topk):
 *   a[k V + v] = (((x - M) - L) / T) + score[g][k], IEEE fp32 in that order (T = 1: fvhd_llm_beam_topk's value, bit for bit);
 *   kept: s = x / T >= max(theta_k', min(theta_p, v_m)) and x > -inf - theta_k' the max(top_k, min_keep)-th largest s (off at top_k = 0),
 *         theta_p the sampler's top-p threshold among the top-k survivors (off at top_p = 1), v_m the min_keep-th largest s; tokens tied at a
 *         threshold are kept as a group; a row with fewer than min_keep finite logits keeps the finite ones;
 *   g = -log(-log u), u = (2 (w >> 9) + 1) 2^-24 with w = word v & 3 of Philox4x32-10 on the counter (r, n, v >> 2, 1), key = the seed's two
 *         words, n = the cache length when the choice is made (fvhd_llm_set_sampling's n; its counter is (row, n, 0, 0));
 *   the `keep` kept candidates of a prompt with the largest a + g, in descending a + g (equal keys: the lower flat index first) ->
 *         cand_scores = their a, cand_index = k V + v; a slot that cannot be filled (fewer than `keep` kept candidates) holds (-inf, 0).
 * A row's candidates are pre-selected by (x / T) + g, which differs from a + g by a row constant and fp32 rounding (DESIGN 4.3 has the bound).
 * The limits are fvhd_llm_beam_topk's, and 1 <= min_keep <= keep.  A score of -1e9 (a dead beam) is an ordinary input.  Deterministic: the same
 * logits, scores, settings, seed and n give the same bits, eager or replayed; no floating-point atomics.  min_p / typical_p / the cutoffs
 * and guidance are not implemented under beams.  Logits processors and a constraint run under beams only with fvhd_llm_set_beam_scoring on
 * ("LLM beam search with processors" below); with it off the calls below are refused with them on where fvhd_llm_beam_topk is. */
/* Allocates (and zeroes) the workspace of fvhd_llm_beam_sample_topk, about 7 MiB, an allocation of its own: fvhd_llm_beam_reserve and
 * fvhd_llm_cache_reserve allocate what they did.  It does not depend on the cache: once per context.  Synchronises (refused while a stream is
 * being captured). */
int fvhd_llm_beam_sample_reserve(fvhd_llm* ctx);
/* logits fp32 [groups * num_beams, vocab] (16-byte aligned), beam_scores fp32 [groups, num_beams] -> cand_scores fp32 [groups, keep],
 * cand_index int64 [groups, keep].  n is read from the context's cache length on the device when the launch runs, so the host arguments are
 * the same every step: capture-safe after fvhd_llm_beam_sample_reserve and fvhd_llm_cache_reserve.  2 launches, 1 + 4 per filter that is on and
 * 1 more per block of 16 rows, then 3. */
int fvhd_llm_beam_sample_topk(fvhd_llm* ctx, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, float temperature,
                              int top_k, float top_p, int min_keep, unsigned long long seed, float* cand_scores, int64_t* cand_index,
                              fvhd_stream_t stream);
/* the operation on its own (tests), on plain device pointers with n given; a process-wide workspace, allocated on first use: eager calls only.
 * noise_override: NULL, or fp32 [rows, V] (16-byte aligned) used as g in place of Philox.  noise_out: NULL, or fp32 [rows, V] (16-byte aligned):
 * every token's g, kept or not.  info: NULL, or fp32 [rows, 4] = (the row's threshold as s, -inf when no filter binds; kept count; M; L). */
int fvhd_op_dec_beam_sample(fvhd_stream_t stream, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V,
                            float temperature, int top_k, float top_p, int min_keep, unsigned long long seed, int n, const float* noise_override,
                            float* noise_out, float* info, float* cand_scores, int64_t* cand_index);

/* ---- LLM logits processors: repetition penalty, no-repeat n-grams, min_new_tokens and token bans inside the step (version 506) ----------
 * transformers' processors for num_beams = 1 (generation/logits_process.py), applied in its order and before temperature / top-k / top-p, to
 * the fp32 logits of fvhd_llm_start / fvhd_llm_decode between the lm_head and the choice.  The HISTORY of a sequence is what transformers'
 * processors see as input_ids when generate() is given inputs_embeds: the tokens fed to the decode steps since fvhd_llm_start (token_ids, or
 * the ids the previous call chose) - not the prompt.  It is empty (g = 0) when fvhd_llm_start chooses the first token and holds g tokens
 * when the g-th decode step chooses.
 *   repetition_penalty p (finite, > 0; 1 = off): for every DISTINCT token t of the history s[t] = s[t] < 0 ? s[t] * p : s[t] / p, an IEEE
 *     fp32 division; a token that occurs many times is penalised once (RepetitionPenaltyLogitsProcessor's gather / scatter).
 *   no_repeat_ngram_size n (0 = off): when g >= n, every window h[i .. i+n-1] whose first n - 1 tokens equal the last n - 1 of the history
 *     sets s[h[i+n-1]] = -inf (NoRepeatNGramLogitsProcessor); n = 1 bans every token of the history.
 *   min_new_tokens m (0 = off) with eos_ids: while g < m every EOS id is -inf (MinNewTokensLengthLogitsProcessor(0, m, eos)) - the first
 *     token included.  Without EOS ids it does nothing.
 *   suppress_ids: always -inf (SuppressTokensLogitsProcessor).
 * Bans are written after the penalty.  Limits: n_eos <= 16, n_suppress <= 256, every id in [0, vocab), the history holds `capacity` tokens per
 * sequence (the cache's own limit); anything else is refused with a message that names the limit.  eos_ids / suppress_ids are HOST int32
 * arrays (NULL with a count of 0), copied into device memory the context owns.  All-off values (1, 0, 0, no lists) switch the feature off.
 * Synchronises (refused while a stream is being captured).  Like the sampling settings, these are read when fvhd_llm_start /
 * fvhd_llm_decode enqueue: a captured graph keeps the ones it was captured with (when other lists are set later, the 1 KiB block
 * its launches read is kept alive until fvhd_llm_destroy; setting the same lists again changes nothing).  Set them BEFORE fvhd_llm_start: a decode step with processors on after a start without them is an error (it has no
 * history), and a step enqueued with processors off appends nothing to the history: g counts the tokens APPENDED (a device word per
 * sequence), not the steps since fvhd_llm_start, so the later steps see a history without that token and without a gap in its place.
 * With any processor on, the call writes its fp32 logits to logits_out or the context's own buffer, edits them in place with one launch of
 * one workgroup per sequence (it appends the step's fed token to the history and touches at most g + 272 logits per sequence, never the
 * whole row; every logit is edited by exactly one lane, so the bits are the same eager or replayed), then chooses: greedy = the argmax of
 * the processed logits (lowest index on ties, two launches as for the first token), sampling = the sampler on them.  logits_out then
 * holds the PROCESSED scores (transformers' `scores`, not its raw `logits`).  A step that hits the sticky error word appends nothing.
 * Beam search is not covered: transformers applies the processors to log-softmaxed scores there, and fvhd_llm_cache_gather does not
 * reorder the history - keep the processors off around fvhd_llm_beam_topk; fvhd_llm_cache_gather is REFUSED while a processor is on
 * ("their token history is not reordered"), as fvhd_llm_cache_rewind, fvhd_llm_extend and fvhd_llm_verify are.
 * With every processor off (the default) nothing changes: no launch, no buffer traffic and no kernel branch is added. */
int fvhd_llm_set_logits_processors(fvhd_llm* ctx, float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens, const int32_t* host_eos_ids,
                                   int n_eos, const int32_t* host_suppress_ids, int n_suppress);
/* the processors on their own (tests): logits fp32 [B, V] edited in place (1 <= B <= 64), history int32 [B, capacity] on the device of which
 * the first g tokens of every row count (0 <= g <= capacity; entries outside [0, V) are ignored), the settings as above (lists on the
 * host).  Builds the first-occurrence records the kernel needs from the history on the device, then runs the step's kernel.  A process-wide
 * scratch, allocated / grown on demand: eager calls only, not during stream capture. */
int fvhd_op_dec_logits_process(fvhd_stream_t stream, float* logits, int B, int V, const int32_t* history, int capacity, int g, float repetition_penalty,
                               int no_repeat_ngram_size, int min_new_tokens, const int32_t* host_eos_ids, int n_eos, const int32_t* host_suppress_ids,
                               int n_suppress);

/* ---- LLM speculative verification: up to 16 tokens of ONE sequence per step, drafts by prompt lookup (version 507) ----------------------
 * A decode step at one sequence uses one of the MFMA tile's 16 columns.  A VERIFY step feeds the last chosen token and T - 1 drafted tokens
 * as the T rows of one step (2 <= T <= 16), takes the argmax of every row, and keeps the longest prefix of drafts the model itself would have
 * chosen: n = the largest value with draft[i] == ids[i] for all i < n, and ids[0 .. n] are emitted - between 1 and T tokens, by construction
 * the greedy output.  Launches: one embed (the capacity check for T slots: error word 1 and nothing written when length + T > capacity; the T
 * token rows; positions position + t; mask bytes [length, length + T) set), then per layer the decode's own q|k|v, o_proj, gate|up and
 * down_proj launches at B = T and ONE attention launch for the T queries on the one cache row, the decode's lm_head + argmax at B = T, and one
 * accept launch (last id, position and length advance by the emitted count, the mask bytes above the new length are cleared again; the k / v
 * of rejected drafts stay in slots above the length, where no later step reads them before it overwrites them).  Nothing depends on the host
 * between steps: a step is capture-safe and replays as one graph.
 * Order contract: row t of a verify step has the BITS of the plain step at length + t + 1.  The GEMM rows are independent MFMA columns; the
 * q|k|v launch writes row t's rotated k and its v into a staging row; the attention kernel reads the keys >= length from staging, lets one
 * workgroup per kv head move them into cache slots [length, length + T), loads every key block once per wave for the wave's queries, and keeps,
 * per query, the key slices, the 64-key blocks per wave, the online-softmax updates, the j order of P.V and the wave and slice combines of
 * the single-query kernel.
 * Scope: the batch of fvhd_llm_start is 1; greedy only unless fvhd_llm_set_verify_sampling (below) is on.  Refused with an error that names the reason: sampling on, logits processors on (the
 * verify step does not maintain their token history), a started batch above 1, rows outside [2, max_rows].  bf16 and e4m3 weights.
 * Prompt lookup (what transformers offers as prompt_lookup_num_tokens; no draft model): the token buffer holds the optional lookup ids
 * (e.g. the prompt's input_ids; negative placeholders such as an image token are allowed, they never match and never become a draft) and
 * then every generated token.  For n = max_ngram .. 1 (n < buffer length) the suffix is the last n tokens; the LARGEST i with
 * buffer[i .. i + n) == suffix and i + n < length wins; the drafts are buffer[i + n ..], at most K, cut at the buffer's end and at the first
 * negative id; missing drafts (no match at any n included) are the buffer's last token.  ml_fastvlm_amd/prompt_lookup.py restates the rule.
 * The choice of drafts never changes the output, only how many steps it takes. */
/* Allocates the step's scratch in one allocation the context owns: T-row activations, the k / v staging rows, per-row positions, the
 * attention partials (max_rows times the single-query size), the token buffer (lookup_capacity + capacity + 16 ids) and the device words.
 * Needs fvhd_llm_cache_reserve first (which also frees this allocation: reserve again), head_dim 64 or 128, 2 <= max_rows <= 16.
 * An allocation that already covers max_rows and lookup_capacity is kept and the call returns at once; otherwise it grows to the larger
 * of the old and the new sizes and synchronises (refused while a stream is being captured). */
int fvhd_llm_spec_reserve(fvhd_llm* ctx, int max_rows, int lookup_capacity);
/* One verify step on draft_ids (device int64 [rows - 1]) after fvhd_llm_start / a decode or verify step: logits_out NULL or fp32
 * [rows, vocab] (row t = the logits after token t of the step), ids_out NULL or int64 [rows] = their argmax, emitted_out NULL or a device
 * int32 = the number of tokens emitted (ids_out[0 .. emitted)).  Capture-safe. */
int fvhd_llm_verify(fvhd_llm* ctx, const int64_t* draft_ids, int rows, float* logits_out, int64_t* ids_out, int32_t* emitted_out, fvhd_stream_t stream);
/* A lookup generation, after fvhd_llm_start: seeds the token buffer with lookup_ids (device int64 [n_lookup], n_lookup <= lookup_capacity;
 * NULL with 0) and the token fvhd_llm_start chose, which is also tokens_out[0].  tokens_out: device int64 [max_new_tokens], written by the
 * later steps; host_eos_ids: host int32 [n_eos <= 16].  One small launch.  The generation belongs to the sequence as the lookup steps left
 * it: fvhd_llm_start, fvhd_llm_extend, fvhd_llm_decode, fvhd_llm_verify, fvhd_llm_cache_rewind, fvhd_llm_cache_gather, fvhd_llm_cache_reserve
 * and a fvhd_llm_spec_reserve that grows the scratch end it when they enqueue (a later fvhd_llm_lookup_step is refused: "no token buffer");
 * fvhd_llm_lookup_begin begins the next one. */
int fvhd_llm_lookup_begin(fvhd_llm* ctx, const int64_t* lookup_ids, int n_lookup, const int32_t* host_eos_ids, int n_eos, int max_new_tokens,
                          int64_t* tokens_out, fvhd_stream_t stream);
/* draft (rows - 1 drafts, 1 <= max_ngram <= 16) + verify + accept: the emitted run is cut after its first EOS id and at max_new_tokens, appended
 * to the token buffer and to tokens_out; after an EOS or at the limit the generation is finished and further steps do nothing.  The host
 * arguments are the same every step: capture-safe, 2 + 5 n_layers + 3 launches (draft, embed; lm_head, argmax reduce, accept). */
int fvhd_llm_lookup_step(fvhd_llm* ctx, int rows, int max_ngram, fvhd_stream_t stream);
/* synchronises the device, then (each optional): tokens written to tokens_out, the finished flag, verify steps run and tokens they emitted */
int fvhd_llm_lookup_state(fvhd_llm* ctx, int* written, int* finished, int* steps, int* tokens);
/* Verify and lookup steps under sampling (added under 510; off by default, and then every call above is refused under sampling with the
 * words it always was, and a greedy step enqueues what it did, launch for launch).  With it on and fvhd_llm_set_sampling on, a step keeps
 * its T fp32 logits rows (logits_out, else scratch that fvhd_llm_spec_reserve makes only when this setting or fvhd_llm_set_logprobs is on)
 * and replaces the argmax reduce by the sampler on the T rows of the one sequence: row t draws with the Philox counter (0, length + 1 + t,
 * 0, 0) - the counter of the decode step that feeds the same token - on logits that have that step's bits, so ids[t] IS the token that
 * step would have sampled.  The accept launch is what it was: a draft is kept when it equals the draw at its position, the first draw that
 * differs is emitted and ends the run.  Against a draft that puts probability 1 on one token that is speculative sampling, exactly: the
 * emitted tokens are those of the sequential sampled run with the same seed, in fewer steps.  Temperature / top-k / top-p / seed are read
 * when the step enqueues.  Logits processors and constraints stay refused.  Switching it on when a scratch exists may allocate and
 * synchronise. */
int fvhd_llm_set_verify_sampling(fvhd_llm* ctx, int on);
/* Log-probabilities of a lookup generation (added under 510), greedy or sampled: call behind fvhd_llm_lookup_begin with fvhd_llm_set_logprobs
 * on since before fvhd_llm_start (started without a logits_out).  token_logprobs_out fp32 [max_new_tokens], top_ids_out int64
 * [max_new_tokens, top_n], top_logprobs_out fp32 [max_new_tokens, top_n] on the device (the last two NULL for top_n = 0), aligned with
 * tokens_out.  The call writes entry 0 - the launch of fvhd_llm_logprobs on the logits fvhd_llm_start left.  Every later fvhd_llm_lookup_step
 * enqueued while the setting is on keeps its T fp32 logits rows, runs the logprobs launch at B = T on them with the step's ids (the values
 * are taken before temperature / top-k / top-p; the slice count depends on the vocabulary alone and each row is merged by its own last
 * workgroup, so row t has the values of the plain step's launch, bit for bit) and, behind the accept, one small launch copies the rows the
 * step emitted to the arrays at the offset of its first token.  No host work: the step still captures into one graph. */
int fvhd_llm_lookup_logprobs(fvhd_llm* ctx, int top_n, float* token_logprobs_out, int64_t* top_ids_out, float* top_logprobs_out, fvhd_stream_t stream);
/* the three new operations on their own (tests), on plain device pointers.
 * fvhd_op_dec_attention_multi: q [T, n_heads * head_dim] bf16, k_cache / v_cache [n_kv_heads][capacity][head_dim] of the one sequence,
 * k_staged / v_staged [T][n_kv_heads][head_dim] = the keys / values of slots *length .. *length + T - 1, key_valid uint8 [capacity] (bytes
 * [*length, *length + T) set by the caller) -> out [T, n_heads * head_dim]; row t = fvhd_op_dec_attention at length *length + t + 1, bit for
 * bit, with the same `splits`; the staged rows are copied into their cache slots.  *length + T > capacity: nothing happens.  partial: fp32
 * [T * n_heads * splits * (head_dim + 2)], counters: int [n_heads] zeroed.
 * fvhd_op_dec_lookup_draft: tokens int32 [*length] on the device -> draft_out int64 [K], 1 <= K <= 15.
 * fvhd_op_dec_lookup_accept: draft int64 [T - 1], ids int64 [T]; words NULL (a bare verify step) or the int32 [24] device words of a
 * generation: [0] token-buffer length, [1] tokens written, [2] finished, [3] steps, [4] tokens emitted, [5] max_new_tokens, [6] n_eos,
 * [8 .. 23] EOS ids; tokens / out: the token buffer and the output (NULL allowed); emitted: NULL or a device int32; then the state of the
 * sequence: last id, next position, length (device words) and its key-valid bytes [capacity]. */
int fvhd_op_dec_attention_multi(fvhd_stream_t stream, const void* q, void* k_cache, void* v_cache, const void* k_staged, const void* v_staged,
                                const uint8_t* key_valid, void* out, int T, int n_heads, int n_kv_heads, int head_dim, int capacity, const int* length,
                                float* partial, int* counters, int splits);
int fvhd_op_dec_lookup_draft(fvhd_stream_t stream, const int32_t* tokens, const int* length, int max_ngram, int K, int64_t* draft_out);
int fvhd_op_dec_lookup_accept(fvhd_stream_t stream, const int64_t* draft, const int64_t* ids, int T, int32_t* words, int32_t* tokens, int tokens_capacity,
                              int64_t* out, int out_capacity, int32_t* emitted, int64_t* last_id, int64_t* position, int* length, uint8_t* key_valid,
                              int capacity);

/* ---- LLM extend: a chunk of T tokens per row onto a started KV cache, and the rewind (version 509) -------------------------------------------
 * fvhd_llm_start prefills an EMPTY cache and fvhd_llm_decode adds one token per row.  fvhd_llm_extend adds a chunk of T >= 1 embedded tokens
 * to every row of a cache that already holds `length` slots: the next turn of a dialogue, one question per row behind a shared prefix
 * (fvhd_llm_cache_gather copies row 0 into N rows first), or the next piece of a prompt longer than one prefill.  What transformers does when
 * forward() is called with past_key_values and T new positions.
 * The decoder stack IS the prefill's (one internal function serves both entry points): the same GEMM launches, split-K choices, fused norms and
 * e4m3 dequantise-into-scratch path on the B * T chunk rows.  Three things differ: the rotary embedding runs without cache pointers; where the
 * prefill launches its attention, one launch per layer copies the chunk's rotated k heads and v heads into slots [length, length + T) of the
 * layer's strided cache (16-byte vector copies; the first layer's launch also writes the mask bytes) and one launch computes causal
 * grouped-query attention of the T chunk queries over slots [0, length + T) - key j is visible to chunk query t of row b iff j <= length + t
 * and the cache's key_valid[b][j]; and without position ids a small launch writes pos[b][t] = next_position[b] + (valid chunk tokens of row b
 * before t), transformers' cumsum(mask) - 1 continued from the row's next position.  `length` is read from the device word by every kernel:
 * the host arguments do not depend on it, and the call composes with replayed decode graphs without a synchronisation.
 * The attention kernel is the prefill's with its keys in the cache: S^T = K . Q^T on the 16x16x32 bf16 MFMA, P in registers, the denominator
 * from a ones fragment, 64-key tiles ALIGNED TO SLOT 0 double-buffered in LDS, 128 queries per workgroup; a query row with no visible key is
 * written as zeros.  With length = 0 it performs the prefill kernel's operations in the same order: fvhd_op_attention_extend(P = 0) has the
 * bits of fvhd_op_attention_causal.  A tiny chunk on a long past runs on ceil(T / 128) * n_heads * batch workgroups that each walk the whole
 * past: the keys are not split across workgroups.
 * length + T > capacity: the first append writes nothing and sets the sticky error word to 1 (the host does not know `length`); every later
 * launch of the call that writes cache state, the chosen ids included, then does nothing, and the next call reports the error. */
/* chunk embeds [batch == the started batch][T][hidden], key_valid uint8 [batch][T] or NULL, position_ids int64 [batch][T] or NULL (continue
 * every row from its next position over the valid chunk tokens) -> K / V of the chunk in slots [len, len + T), mask, len += T, next
 * positions (position of the chunk's last token + 1); logits_out (NULL or fp32 [batch, vocab]) of the chunk's LAST position and next_ids_out
 * through the same argmax / sampler launches as fvhd_llm_start (Philox n = the new length).
 * Capture-safe under fvhd_llm_prefill's rule (the workspace reserved for (batch, T): fvhd_llm_reserve).  Refused, each with a message: no
 * started sequence, T < 1, T > capacity, head_dim other than 64 / 128, a pending error word, logits processors on (their token history has
 * no ids for embedded chunks - the stance of the verify step).  Ends a lookup generation (fvhd_llm_lookup_begin again). */
int fvhd_llm_extend(fvhd_llm* ctx, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int T, float* logits_out,
                    int64_t* next_ids_out, fvhd_stream_t stream);
/* keep_dev: int32 [started batch] on the device.  For every row the slots [keep[b], length) leave the sequence: the row's next position
 * drops by the number of VALID slots among them and their mask bytes are cleared; then length = max_b keep[b].  K / V bytes are not touched
 * (later appends overwrite them).  A keep[b] outside [0, length] changes nothing and sets the sticky error word to 4.  One launch,
 * capture-safe.  Refused with logits processors on (their history is not rewound).  After a rewind the ids "the previous step chose" are
 * stale: the next call must be fvhd_llm_extend, or fvhd_llm_decode with explicit token_ids - anything that would feed the stale ids
 * (fvhd_llm_decode(token_ids = NULL), fvhd_llm_verify, fvhd_llm_lookup_begin / _step) is refused, under fvhd_llm_cache_gather's enqueue-time
 * rule (a captured step replays as captured).  Ends a lookup generation. */
int fvhd_llm_cache_rewind(fvhd_llm* ctx, const int32_t* keep_dev, fvhd_stream_t stream);
/* the kernels on their own (tests), on plain device pointers.
 * fvhd_op_attention_extend: qkv [B*T, (n_heads + 2 n_kv_heads) * head_dim] bf16 (the chunk's packed rows, rope applied; the q heads are
 * read), k_cache / v_cache bf16 [>= B][n_kv_heads][capacity][head_dim] with the chunk already in slots [*past_len, *past_len + T), key_valid
 * uint8 [>= B][capacity] or NULL -> out [B*T, n_heads * head_dim] bf16; head_dim 64 / 128; *past_len + T > capacity: nothing is written.
 * fvhd_op_cache_append: one layer - the k and v heads of the rows -> slots *past_len + t; key_valid (NULL: not written) [>= B][capacity] gets
 * chunk_valid [B][T] (NULL: 1) at the same slots; *past_len + T > capacity: nothing is written and *status = 1; nothing while *status != 0.
 * fvhd_op_extend_positions: pos_out int64 [B][T] from next_positions int64 [B] and chunk_valid [B][T] or NULL.
 * fvhd_op_cache_rewind: fvhd_llm_cache_rewind on key_valid [rows][capacity], positions int64 [rows], *length, *status. */
int fvhd_op_attention_extend(fvhd_stream_t stream, const void* qkv, const void* k_cache, const void* v_cache, const uint8_t* key_valid, void* out, int B,
                             int T, int n_heads, int n_kv_heads, int head_dim, int capacity, const int* past_len);
int fvhd_op_cache_append(fvhd_stream_t stream, const void* qkv, void* k_cache, void* v_cache, uint8_t* key_valid, const uint8_t* chunk_valid, int B, int T,
                         int n_heads, int n_kv_heads, int head_dim, int capacity, const int* past_len, int* status);
int fvhd_op_extend_positions(fvhd_stream_t stream, const int64_t* next_positions, const uint8_t* chunk_valid, int64_t* pos_out, int B, int T);
int fvhd_op_cache_rewind(fvhd_stream_t stream, const int32_t* keep, int rows, uint8_t* key_valid, int64_t* positions, int capacity, int* length,
                         int* status);

/* ---- LLM scoring: the log-probability of GIVEN tokens at every position (added under 510) -------------------------------------------------------
 * fvhd_llm_prefill / _start / _extend project only the last position of every row through lm_head.  Scoring - transformers'
 * forward(labels=...), multiple-choice answers by likelihood, perplexity of a caption - needs log p(target | prefix) at EVERY position:
 *     z = xn . W^T (16x16x32 bf16 MFMA, fp32 accumulation)     lse[m] = log sum_v exp(z[m][v])     logprob[m] = z[m][target[m]] - lse[m]
 * in one kernel that never materialises [rows, vocab] (llm_score.hip): a workgroup owns 128 rows and walks one of S segments of the vocabulary
 * with an online softmax per row (running max: logits of magnitude 1e4 give finite results), a small second launch combines the S segment
 * states of a row in segment order.  Scratch: 16 bytes per (row, segment), not initialised by the caller.
 * Shapes: M >= 1 (rows past M are neither read as valid nor written), V % 8 == 0 (V need not be a multiple of the 128-column tile: columns
 * >= V enter neither the max nor the sum), K % 32 == 0; anything else is refused with a message.
 * target < 0 (transformers' ignore label is -100): logprob = 0.0 exactly, lse is still written.  target >= V: logprob = NaN (no status word).
 * Otherwise the target logit is the very fp32 value that entered the sum, so logprob <= 0 up to the rounding of the log.
 * Bits: the same launch gives the same bits; a row's lse and logprob depend neither on the other rows' contents nor on any target but its
 * own (lse on none); they may depend on (M, V, K) through the plan: fvhd_lm_score_plan returns S (0: the shape is refused). */
size_t fvhd_lm_score_scratch_bytes(int M, int V, int K);
int fvhd_lm_score_plan(int M, int V, int K);
/* xn [M][K] bf16 (rows after the final RMSNorm), Wt [V][K] bf16 (lm_head as stored), targets int64 [M] -> logprob_out fp32 [M], lse_out fp32
 * [M] or NULL.  All pointers on the device, xn / Wt / scratch aligned to 16 bytes; scratch_bytes >= fvhd_lm_score_scratch_bytes(M, V, K). */
int fvhd_op_lm_score(fvhd_stream_t stream, const void* xn, const void* Wt, const int64_t* targets, int M, int V, int K, float* logprob_out,
                     float* lse_out, void* scratch, size_t scratch_bytes);
/* On a context: scores the rows of the LAST fvhd_llm_prefill / fvhd_llm_start / fvhd_llm_extend of this context, whose final hidden states
 * are still in its workspace: the final RMSNorm of all batch * T rows, lm_head (an e4m3 context dequantises it into its scratch first, as
 * the stack does), the score launches.  target_ids int64 [batch][T] on the device: target_ids[b][t] is the id whose probability under the
 * distribution predicted at position t is wanted - the caller shifts.  logprob_out fp32 [batch][T], lse_out NULL or fp32 [batch][T].
 * The score scratch is an allocation of its own that grows on demand; fvhd_llm_score_reserve(rows) sizes it for rows = batch * T ahead
 * (growing it synchronises the device: like fvhd_llm_reserve it then fails with a message while a stream is being captured, and the
 * failed synchronise invalidates that capture - reserve before capturing; a reserve that finds the scratch large enough does nothing
 * and is allowed at any time), after which fvhd_llm_score enqueues without a host synchronisation and is
 * capture-safe; a scratch that a capturing stream used is retired, not freed, when it must grow.  Refused, each with a message: no stack
 * call yet on the current workspace (a stack call that failed part-way leaves none), capture without a sufficient reserve, NULL targets or output. */
int fvhd_llm_score_reserve(fvhd_llm* ctx, int rows);
int fvhd_llm_score(fvhd_llm* ctx, const int64_t* target_ids, float* logprob_out, float* lse_out, fvhd_stream_t stream);

/* ---- LLM log-probabilities: the chosen token's log-probability and the n most likely tokens, per step (added under 510) ----------------------
 * fvhd_llm_start / _decode / _extend return ids; this says how likely they were.  Per row of fp32 logits x [V] and a chosen id:
 *     M = max x     Z = sum_v exp(x[v] - M)     token_logprob = (x[id] - M) - log Z
 *     top_ids[0 .. top_n) = the top_n largest x in descending order, top_logprobs[k] = (x[top_ids[k]] - M) - log Z
 * in ONE launch (llm_logprobs.hip): grid = slices x rows, a slice is ceil(V / S) consecutive ids with S = min(64, ceil(V / 2048)); the
 * slices' (max, sum relative to that max, top_n candidates) meet in the row's last-arriving workgroup.  No floating-point atomics and a fixed
 * order of additions: the same inputs give the same bits, eager or replayed from a graph.
 * Order of top_ids: descending value; equal values by ascending id; -0 and +0 are equal; -inf entries rank last (among them ascending id).
 * The ids depend on comparisons of the input values only: they are exact.  Only the log-probabilities carry rounding.
 * A -inf logit (a suppressed token) contributes 0 to Z and has log-probability -inf - never NaN.  A row without a finite logit, or with
 * +inf or NaN, is undefined (the sampler's rule, "LLM sampling").  id outside [0, V): token_logprob = NaN, nothing is read.
 * top_n in [0, 16]; top_n > V is refused on the host.  V >= 1 (rows need not be 16-byte aligned), row stride V, 1 <= B <= 64.
 * Scratch: fvhd_dec_logprobs_scratch_bytes(B, V, top_n) = 16384 + 2 * pad256(4 B S) + pad256(8 B S top_n) bytes (0: the shape is refused),
 * aligned to 256 bytes.  Its first 16 384 bytes are the rows' arrival counters (one per 256 bytes: 4096 workgroups adding to one cache line
 * wait for each other): zero before the FIRST launch on it, and every launch leaves them zero, so launches of any (B, V, top_n) that fit
 * may follow one another on one scratch; the rest needs no initialisation. */
size_t fvhd_dec_logprobs_scratch_bytes(int B, int V, int top_n);
/* logits fp32 [B][V], ids int64 [B] -> token_logprob_out fp32 [B], top_ids_out int64 [B][top_n], top_logprobs_out fp32 [B][top_n] (both may be
 * NULL when top_n = 0).  All pointers on the device. */
int fvhd_op_dec_logprobs(fvhd_stream_t stream, const float* logits, const int64_t* ids, int B, int V, int top_n, float* token_logprob_out,
                         int64_t* top_ids_out, float* top_logprobs_out, void* scratch, size_t scratch_bytes);
/* On a context.  fvhd_llm_set_logprobs(ctx, 1) reserves the scratch for the batch of fvhd_llm_cache_reserve (an allocation of its own, freed
 * by the next fvhd_llm_cache_reserve, which also switches the setting off) and makes the steps KEEP their logits: a greedy fvhd_llm_decode
 * with logits_out = NULL then stores them into the context's buffer, as it already does under sampling or logits processors (fvhd_llm_start /
 * _extend always do).  The (max, index) pairs still come from the lm_head's fused epilogue: the chosen ids keep their bits.  It synchronises
 * the device and is refused while a stream is being captured; a captured step keeps the setting it was captured with.  With the setting off
 * every call enqueues the launches it did before.
 * fvhd_llm_logprobs enqueues the launch on the logits of the LAST fvhd_llm_start / _decode / _extend and the ids that call chose: logits =
 * NULL reads the context's buffer (the setting must be on and that call must have been given logits_out = NULL), otherwise pass that call's
 * logits_out.  With logits processors on these are the processed scores; they are always the values BEFORE temperature / top-k / top-p (the
 * sampler reads them const, so the launch goes after the choice).  Outputs for the rows of the started batch.  No host synchronisation and host
 * arguments constant per step: capture-safe.  Refused, each with a message: nothing started; logits NULL with the setting off or with no kept
 * logits; no scratch (the setting was never on for this cache); the chosen ids stale (behind fvhd_llm_cache_rewind / _cache_gather, the rule of
 * fvhd_llm_decode(token_ids = NULL)); the error word set; top_n outside [0, 16] or above the vocabulary.  A launch that finds the error word
 * set on the device writes nothing, like the steps. */
int fvhd_llm_set_logprobs(fvhd_llm* ctx, int on);
int fvhd_llm_logprobs(fvhd_llm* ctx, const float* logits, int top_n, float* token_logprob_out, int64_t* top_ids_out, float* top_logprobs_out,
                      fvhd_stream_t stream);

/* ---- LLM constrained decoding: a token-level automaton masks the logits inside the step (added under 510) -----------------------------------
 * The caller hands over an automaton over token ids as CSR data: state s owns the edges offsets[s] .. offsets[s + 1]; tokens[e] (int32,
 * strictly ascending inside a state) is an id the state allows and targets[e] the state it leads to, or -1 = FREE: a FREE row is
 * unconstrained from then on and never leaves FREE.  Every state has at least one edge.  Limits: 16 777 216 states, 268 435 456 edges.
 * The step keeps one int32 state and one int32 flag word per row on the device.  Per step (llm_constrain.hip):
 *   advance  (decode steps only, not the first choice behind fvhd_llm_start / _extend) the token FED to the step - token_ids[b], or the id the
 *            previous call chose when token_ids is NULL: the ids the step embeds and the processors append - is looked up in the sorted edges
 *            of the row's state.  Found: the row takes the edge's target.  Not found: the row goes to FREE and flag bit 0 ("violated") is
 *            set; only ids the caller fed itself can do that.  A FREE row stays FREE.
 *   mask     every id of a non-FREE row that is no edge of its (new) state becomes -inf.  Allowed entries are neither read nor written: they
 *            keep the lm_head's (or the processors') bits, -0.0 included.  A FREE row is not touched.
 * The advance is a small launch of its own in front of the mask launch (grid = slices of fvhd_dec_constrain_slice() ids x rows), so no
 * workgroup can read a state another has replaced; every banned logit is written by one lane with a constant, the new state depends on the
 * old state and the fed id only: the same bits eager or replayed.  A launch that finds the error word set writes nothing, like the steps.
 * This is transformers' PrefixConstrainedLogitsProcessor with the host callback replaced by the tables.  Its place in
 * `_get_logits_processor` is behind repetition penalty, n-gram and min-new-tokens and in front of suppress; bans commute and -inf survives
 * the penalty, so the launches go behind the processors' launch and give the same values.
 *
 * fvhd_llm_set_constraint: n_states = 0 switches the feature off (the other arguments are ignored).  Otherwise host_offsets int32
 * [n_states + 1], host_tokens / host_targets int32 [n_edges], host_start_states int32 [n_start] with n_start = 1 (every row) or the batch of
 * fvhd_llm_cache_reserve; a start state of -1 leaves the row unconstrained.  Validated, each failure with a message naming the state or
 * edge: offsets start at 0, are monotone and end at n_edges; every token in [0, vocab); every target in [-1, n_states); tokens strictly
 * ascending inside a state; no state without an edge; the limits above.  The tables are copied into device memory the context owns.  It
 * synchronises the device and is refused while a stream is being captured.  A captured step keeps the tables it was captured with: tables
 * that a capturing stream has recorded are retired (kept until fvhd_llm_destroy) when OTHER tables are set, never overwritten; switching
 * off keeps the tables, and setting the same tables again uploads nothing.
 * With a constraint on:
 *   fvhd_llm_start / fvhd_llm_extend reset the rows' states to their start states, clear the flags and mask the logits their choice is made
 *     from - behind the processors' launch where those are on, before the argmax or the sampler.  (The start states travel by value in the
 *     launch: a captured start keeps them.)
 *   fvhd_llm_decode advances and masks between the lm_head and the choice.  Greedy: the fused (max, index) pairs saw raw logits, so the pairs
 *     come again from the masked logits, as under the processors - once when both are on.  Sampling: the launches go before the sampler.
 *   The steps keep their logits (the context's buffer when logits_out is NULL); logits_out holds the processed scores, so
 *     fvhd_llm_logprobs renormalises over the allowed set: banned ids have log-probability -inf and rank last.
 *   Refused, each with a message: fvhd_llm_cache_rewind, fvhd_llm_cache_gather, fvhd_llm_beam_topk, fvhd_llm_verify, fvhd_llm_lookup_begin /
 *     _step (none of them carries the rows' states); fvhd_llm_decode behind a start / extend that ran without the constraint (the rows have
 *     no states).  fvhd_llm_score is unaffected.
 *   A row whose processors and constraint together ban every id is undefined (the sampler's rule, "LLM sampling").
 * Off (the default): no launch, no buffer traffic, no allocation: every call enqueues what it did.
 * fvhd_llm_constraint_state synchronises and copies, for the first `rows` rows of the started batch, the state after the last FED token - not
 * advanced by the last chosen one - and the flag words (either output may be NULL); refused while no constraint is on or no sequence was
 * started under it.
 * fvhd_op_dec_constrain is the launches on their own, every pointer on the device: logits fp32 [B][V] with row stride V (aligned to 4 bytes;
 * rows need not be 16-byte aligned), V >= 1, 1 <= B <= 64, tables as above (trusted: validate on the host), states / flags int32 [B], fed_ids
 * int64 [B] or NULL = no advance.  It writes at most 4 V bytes per constrained row, reads only the edges of the rows' current states and
 * never reads the logits. */
int fvhd_dec_constrain_slice(void);
int fvhd_op_dec_constrain(fvhd_stream_t stream, float* logits, int B, int V, const int32_t* offsets, const int32_t* tokens, const int32_t* targets,
                          int n_states, int32_t* states, int32_t* flags, const int64_t* fed_ids);
int fvhd_llm_set_constraint(fvhd_llm* ctx, const int32_t* host_offsets, int n_states, const int32_t* host_tokens, const int32_t* host_targets,
                            int n_edges, const int32_t* host_start_states, int n_start);
int fvhd_llm_constraint_state(fvhd_llm* ctx, int32_t* host_states_out, int32_t* host_flags_out, int rows);

/* ---- LLM classifier-free guidance: the conditional and the unconditional sequence as two rows of one step (added under 510) ------------------
 * transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor (generate(guidance_scale = s, negative_prompt_ids = ...)) runs a second model
 * forward per token.  Here the unconditional sequence rides in the same step: for G prompts the step runs B = 2 G rows (G <= 32), row g the
 * conditional sequence and row G + g the unconditional one (the prompt without the image, say), both fed the same token every step.  Per pair,
 * with lc = log_softmax(x[g]) and lu = log_softmax(x[G + g]) of the step's fp32 logits:
 *     guided[v] = s * (lc[v] - lu[v]) + lu[v]
 * written over row g in front of every other edit: logits processors, the constraint, fvhd_llm_logprobs, temperature / top-k / top-p and the
 * argmax all act on `guided`, and on the G conditional rows only.  The guided scores are not normalised: fvhd_llm_logprobs reports their
 * log-softmax, as it renormalises under a constraint.  The logits must be FINITE: guidance runs before any launch that writes -inf.
 * Kernels (llm_guidance.hip), two launches - the second needs every slice of the first:
 *   statistics  grid = S slices x 2 G rows, S = min(64, ceil(V / 2048)): per slice the maximum m and sum exp(x - m) (a thread adds its elements
 *               in index order, a butterfly over the 256 threads); the row's last-arriving workgroup merges the slices into M = max m_s and
 *               log Z, Z = sum_s sum_s exp(m_s - M) (a butterfly over the slices).  The scheme of the log-probabilities launch: no
 *               floating-point atomics, a fixed order of additions, the same bits eager or replayed.
 *   apply       grid = ceil(V / 2048) slices x G pairs.  In this order, every operation rounded once to fp32, no fused multiply-add:
 *                   lc = (xc - Mc) - log Zc     lu = (xu - Mu) - log Zu     d = lc - lu     p = s * d     guided = p + lu
 *               Identical rows give d = 0 and guided = lc bit for bit, whatever s.  16-byte loads and stores where both rows of a pair are
 *               16-byte aligned (always when V % 4 == 0) with a scalar tail of V % 4 elements; a pair with a misaligned row goes element
 *               by element.  Rows G .. 2 G - 1 are read only: they keep the lm_head's bits.
 * Behind the choice one small launch copies the id row g chose to row G + g (the ids of the last step and next_ids_out) and, in a decode
 * step, advances the positions of rows G .. 2 G - 1; the choice's own launches run on G rows.  Under sampling row g draws with the Philox
 * counter of row g, as without guidance.
 * fvhd_dec_guidance_scratch_bytes(G, V) = 16384 + 2 * pad256(8 G S) + pad256(16 G) bytes (0: the shape is refused), aligned to 256 bytes; its
 * first 16 384 bytes are the rows' arrival counters: zero before the FIRST launch, and every launch leaves them zero.
 * fvhd_op_dec_guidance is the two launches on plain device pointers: logits fp32 [2 G][V], row stride V, aligned to 4 bytes, V >= 1,
 * 1 <= G <= 32, scale finite.
 * fvhd_llm_set_guidance(ctx, scale): scale == 1 is off (the default), any other finite scale is on.  It is read when fvhd_llm_start / _decode /
 * _extend enqueue, like the sampling settings; a captured graph keeps what it was captured with.  The first call that switches guidance on
 * allocates the launches' scratch (an allocation of its own, for 32 pairs of the context's vocabulary, kept until fvhd_llm_destroy); that
 * call synchronises the device and is refused while a stream is being captured.  A context that never switches it on keeps its footprint.
 * With guidance on:
 *   fvhd_llm_start / _decode / _extend run the two launches on the logits their choice is made from (the greedy decode step keeps its logits
 *     and takes its (max, index) pairs from them again, as under the processors), then processors and constraint on the G conditional
 *     rows, the choice on G rows, the mirror launch.  Inside the decode step they obey the error word like the other launches.  logits_out
 *     holds the guided scores in rows [0, G) and the raw logits in rows [G, 2 G); next_ids_out holds 2 G ids (row G + g = row g).
 *     Per-row settings (the constraint's start states, fvhd_llm_constraint_state, fvhd_llm_logprobs' outputs) count G rows.
 *   Refused, each with a message: an odd batch; fvhd_llm_verify, fvhd_llm_lookup_begin / _step; fvhd_llm_beam_topk; fvhd_llm_cache_gather (it
 *     would break the pairing); fvhd_llm_cache_rewind - rows g and G + g would have to keep equal lengths, and the keeps are on the
 *     device, where they cannot be checked without a synchronisation, so the call is refused outright.
 * Off: no launch, no allocation; every call enqueues launch for launch what it did. */
size_t fvhd_dec_guidance_scratch_bytes(int G, int V);
int fvhd_op_dec_guidance(fvhd_stream_t stream, float* logits, int G, int V, float scale, void* scratch, size_t scratch_bytes);
int fvhd_llm_set_guidance(fvhd_llm* ctx, float scale);

/* ---- LLM beam search with processors: logits processors and a constraint on log-softmaxed rows that follow their beams (added under 510) ------
 * Under beams transformers applies its processors to LOG-SOFTMAXED scores, and every beam's history follows its parent:
 *     lp = log_softmax(logits);  lp = processors(flat_running_sequences, lp);  lp += running_beam_scores;  top-K (or a draw) of the K * V values
 * fvhd_llm_set_beam_scoring(ctx, on) switches the context to that order.  Off (the default) every call is what it was, refusals included.  On:
 *   fvhd_llm_start / fvhd_llm_decode with a logits_out first turn every row into x'[v] = (x[v] - M) - L in place - M the row maximum, L = log sum
 *     exp(x - M), both with fvhd_llm_beam_topk's slices and summation order, so an entry no processor edits holds bit for bit what the plain
 *     chain adds to the beam score - then run the processors and the constraint on x' (a log-probability is <= 0: the repetition penalty
 *     multiplies).  Two launches of ceil(V / 4096) x rows workgroups, 16-byte loads and stores on 16-byte-aligned rows; inside the decode step
 *     they obey the error word.  Without a logits_out nothing changes.
 *   fvhd_llm_cache_gather carries, behind K and V and with the same src_rows, the first hist_count[src] history entries with their
 *     first-occurrence marks, the seen-bitmap, the history count and the constraint's state and flag words: two more launches, through a
 *     scratch of their own, rows with src_rows[r] == r skipped, every workgroup checking all of src_rows first (one index out of range: nothing
 *     is written but error word 3).
 *   fvhd_llm_beam_topk / fvhd_llm_beam_sample_topk take the rows as they are: acc = x' + score, a = (x' / T + score); top-k / top-p thresholds
 *     are searched on x' / T; a -inf entry is never a candidate and never counted as kept; a slot that cannot be filled holds (-inf, 0).
 *   Refused, each with a message: guidance, fvhd_llm_set_logprobs (at fvhd_llm_start / _decode), fvhd_llm_extend.  fvhd_llm_verify / _lookup_*
 *     and fvhd_llm_cache_rewind keep their refusals under processors or a constraint.
 * The setting is read when a call enqueues, like the sampling settings; a captured step replays what it captured.  The call that switches it on
 * allocates the normalisation's partials and the reorder's scratch (the reserved batch's histories, bitmaps and states) apart from
 * fvhd_llm_cache_reserve's and fvhd_llm_beam_reserve's allocations - it synchronises and is refused while a stream is being captured;
 * fvhd_llm_cache_reserve frees the scratch with the cache it was sized for and switches the setting off.
 * The operations on their own (tests), on plain device pointers, process-wide scratch, eager calls only:
 *   fvhd_op_dec_beam_norm: logits fp32 [rows][V], row stride V, 4-byte aligned, 1 <= rows <= 64, 1 <= V <= 262144 (rows that are not 16-byte
 *     aligned and a row's last V % 4 entries go element by element); stats_out NULL or fp32 [rows][2] = (M, L).
 *   fvhd_op_dec_hist_gather: history int32 [batch][capacity] (entry = token | 0x80000000 for a repeat), seen uint32 [batch][ceil(V / 32)],
 *     count int32 [batch] - or history NULL; states / flags int32 [batch] - or states NULL; status as in fvhd_op_dec_cache_gather.
 *   fvhd_op_dec_beam_topk_pre / fvhd_op_dec_beam_sample_pre: fvhd_op_dec_beam_topk / _beam_sample on pre-normalised rows (info's M and L are
 *     those of the rows given, which the values do not use). */
int fvhd_llm_set_beam_scoring(fvhd_llm* ctx, int on);
int fvhd_op_dec_beam_norm(fvhd_stream_t stream, float* logits, int rows, int V, float* stats_out);
int fvhd_op_dec_hist_gather(fvhd_stream_t stream, int32_t* history, uint32_t* seen, int32_t* count, int32_t* states, int32_t* flags,
                            const int64_t* src_rows, int batch, int rows_in, int rows_out, int capacity, int V, int* status);
int fvhd_op_dec_beam_topk_pre(fvhd_stream_t stream, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V,
                              float* cand_scores, int64_t* cand_index);
int fvhd_op_dec_beam_sample_pre(fvhd_stream_t stream, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V,
                                float temperature, int top_k, float top_p, int min_keep, unsigned long long seed, int n, const float* noise_override,
                                float* noise_out, float* info, float* cand_scores, int64_t* cand_index);

#ifdef __cplusplus
}
#endif
#endif /* FVHD_H */
