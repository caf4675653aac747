// C ABI of the Qwen2 prefill (include/fvhd.h "LLM prefill"): workspace and the launch sequence of
// transformers' Qwen2ForCausalLM.forward on inputs_embeds (the call the reference makes at llava/model/language_model/
// llava_qwen.py:92-103 after prepare_inputs_labels_for_multimodal, and from generate(), :138-143).  Kernels: llm.hip + gemm.hip.
#include <math.h>

#include "llm_ctx.h"

int ensure_ws(fvhd_llm* c, int B, int T, hipStream_t st, bool check_capture)
{
    const int rows = (int)(((size_t)B * T + 255) / 256 * 256);
    if (c->ws && rows <= c->ws_rows && B <= c->ws_batch && T <= c->ws_pos) return 0;      // (ws_pos >= 8192 once allocated)
    if (check_capture && is_capturing(st))
        return lfail("fvhd_llm_prefill: the workspace must grow for this (batch, length) but the stream is being captured - call fvhd_llm_reserve first");
    // the rotary table covers max_position_embeddings (fvhd_llm_set_max_positions; at most 65536 rows = 16 MB at head_dim 64) or 8192
    // positions: position ids of a prefill are < seq_len, and a caller continuing a longer context may pass larger ones - beyond the
    // table the kernel computes the phases itself (llm.hip: rope_kernel), it never clamps
    const int want_pos = c->max_pos > 0 ? (c->max_pos < 65536 ? c->max_pos : 65536) : 8192;
    const int tpos = T > want_pos ? T : want_pos;
    const int nrows = rows > c->ws_rows ? rows : c->ws_rows, nb = B > c->ws_batch ? B : c->ws_batch, np = tpos > c->ws_pos ? tpos : c->ws_pos;
    const int lb = (nb + 15) / 16 * 16;
    Arena a;
    const size_t o_h = a.take((size_t)nrows * c->H * 2), o_xn = a.take((size_t)nrows * c->H * 2), o_qkv = a.take((size_t)nrows * c->qkvw * 2),
                 o_att = a.take((size_t)nrows * c->nh * c->hd * 2), o_act = a.take((size_t)nrows * c->I * 2), o_last = a.take((size_t)lb * c->H * 2),
                 o_lastn = a.take((size_t)lb * c->H * 2), o_rope = a.take((size_t)np * c->hd * 4),
                 o_part = a.take((size_t)nrows * std::max(kMaxSplits * c->H, 2 * c->qkvw) * 4), o_epos = a.take((size_t)nrows * 8);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return lhip("hipDeviceSynchronize", e);
    if (c->ws) {
        if (c->ws_captured) c->retired.push_back(c->ws);      // a caller's graph may still replay on it
        else (void)hipFree(c->ws);
    }
    c->ws = nullptr;
    c->ws_captured = false;
    ++c->generation;
    e = hipMalloc((void**)&c->ws, a.off);
    if (e != hipSuccess) return lhip("hipMalloc(llm workspace)", e);
    e = hipMemset(c->ws, 0, a.off);           // the padding rows start (and stay) finite
    if (e != hipSuccess) return lhip("hipMemset(llm workspace)", e);
    c->ws_bytes = a.off; c->ws_rows = nrows; c->ws_batch = nb; c->ws_pos = np;
    c->h = c->ws + o_h; c->xn = c->ws + o_xn; c->qkv = c->ws + o_qkv; c->att = c->ws + o_att; c->act = c->ws + o_act;
    c->last = c->ws + o_last; c->lastn = c->ws + o_lastn; c->rope = (float*)(c->ws + o_rope); c->part = (float*)(c->ws + o_part);
    c->epos = (int64_t*)(c->ws + o_epos);
    // rotary table, fp32 like Qwen2RotaryEmbedding.forward: inv_freq_i = theta^(-2i/hd), angle = pos * inv_freq_i, (cos, sin)
    std::vector<float> tab((size_t)np * c->hd);
    for (int p = 0; p < np; ++p)
        for (int i = 0; i < c->hd / 2; ++i) {
            const float inv = 1.0f / powf(c->theta, (float)(2 * i) / (float)c->hd);
            const float ang = (float)p * inv;
            tab[((size_t)p * (c->hd / 2) + i) * 2] = cosf(ang);
            tab[((size_t)p * (c->hd / 2) + i) * 2 + 1] = sinf(ang);
        }
    e = hipMemcpy(c->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
    return e == hipSuccess ? 0 : lhip("hipMemcpy(rope table)", e);
}

// The matrix a GEMM reads: the packed bf16 weights, or - e4m3 / MXFP4 - the bf16 scratch the codes are dequantised into right before it
// (1 byte or 17 / 32 of one in, 2 bytes out per element; the GEMMs run one after the other on `st`, so one scratch of the largest matrix serves them all).  One function
// for the decoder stack and for fvhd_llm_score.
static int stack_weights(fvhd_llm* c, hipStream_t st, int layer, int matrix, const void** p)
{
    const Mat m = mat_of(c, layer, matrix);
    if (c->wfmt == FVHD_W_BF16) { *p = c->wdev + m.off; return 0; }
    *p = c->wscratch;
    if (c->wfmt == FVHD_W_MXFP4) return fvhd_launch_w4_unpack(st, c->wdev + m.off, c->wdev + m.soff, c->wscratch, m.N, m.K, 0);
    return fvhd_launch_w8_unpack(st, c->wdev + m.off, (const float*)(c->wdev + m.soff), c->wscratch, m.N, m.K, 0);
}

// The decoder stack of fvhd_llm_prefill and of fvhd_llm_extend (llm_step.hip) - ONE launch sequence: the GEMMs, their split-K choices, the
// fused norms and the e4m3 dequantise-into-scratch path are the same in both.  extend = false is the prefill, launch for launch what it
// always ran.  extend = true continues the context's started cache: key_valid is the CHUNK's mask [batch][seq_len], the rotary embedding
// runs without cache pointers, and where the prefill launches llm_attention the chunk's k / v are appended to the layer's strided cache at
// slot *len (the first layer's launch writes the mask column) and llm_attention_past reads keys [0, *len + seq_len) under the cache's mask;
// without position ids the chunk's positions are computed on the device into the workspace.  c->epos_used is left pointing at the
// positions the stack used (the caller's, or the workspace's).
int decoder_stack(fvhd_llm* c, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch, int seq_len,
                  float* logits_out, void* k_cache, void* v_cache, hipStream_t st, bool extend)
{
    LLM_ON_DEVICE(c);
    c->last_batch = 0;                          // fvhd_llm_score: from here on c->h is being rewritten; set again when every launch is enqueued
    int e = ensure_ws(c, batch, seq_len, st, true);
    if (e) return e;
    {
        const bool capturing = is_capturing(st);
        if (capturing) c->ws_captured = true;
        // tensors re-set after fvhd_llm_finalize: this prefill runs behind their copies (a captured stream cannot wait on an outside
        // event - there the host waits once)
        if (c->load_pending) {
            // hipEventQuery / hipEventSynchronize are not capture-safe under the default (global) capture mode: while the caller's stream is
            // capturing they run in relaxed mode, so that they cannot invalidate the caller's capture (round 6, advisor)
            hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
            if (capturing) (void)hipThreadExchangeStreamCaptureMode(&mode);
            const hipError_t q = hipEventQuery(c->load_ev);
            if (q == hipSuccess) c->load_pending = false;
            else if (capturing) e = wait_for_loads(c);
            if (capturing) (void)hipThreadExchangeStreamCaptureMode(&mode);
            if (q != hipSuccess && q != hipErrorNotReady) (void)hipGetLastError();
            if (e) return e;
            if (c->load_pending && !capturing && st != c->load_stream) {
                const hipError_t he = hipStreamWaitEvent(st, c->load_ev, 0);
                if (he != hipSuccess) return lhip("hipStreamWaitEvent(llm weights)", he);
            }
        }
    }
    const int B = batch, T = seq_len, M = B * T, Mp = (M + 255) / 256 * 256;
    const int H = c->H, I = c->I, nh = c->nh, nkv = c->nkv, hd = c->hd;
    const char* w = c->wdev;
    if ((size_t)M * H % 4) return lfail("fvhd_llm_prefill / fvhd_llm_extend: batch * seq_len * hidden must be a multiple of 4");
    LCHECK(fvhd_launch_cast_rows(st, embeds, dtype, c->h, (long)M * H), "cast embeds");
    const size_t ext_layer = (size_t)c->dc_batch * nkv * c->dc_cap * hd * 2;      // extend: one layer of the context's strided caches
    if (extend && !position_ids) {
        LCHECK(fvhd_launch_llm_extend_positions(st, c->posv, key_valid, c->epos, B, T, c->status), "chunk positions");
        position_ids = c->epos;
    }
    c->epos_used = position_ids;
    const size_t cache_layer = (size_t)B * nkv * T * hd * 2;
    // split-K factor of a GEMM with few output tiles (Mp / 128 x H / 128) - while the tiles of one slice do not fill the chip twice over, K is
    // split across workgroups (fp32 partials + a deterministic reduce that also adds the residual): down_proj 70 -> ~25 us per layer at the
    // 0.5 B prefill shape (B = 8 x 285 tokens).  The reduce of a split GEMM also applies the RMSNorm the next operation starts with
    // (splitk_reduce_norm_kernel, bit-identical to the separate launch): input_layernorm of layer l + 1 behind down_proj of layer l, and -
    // when o_proj is split too (FVHD_LLM_OSPLIT) - post_attention_layernorm behind o_proj
    // the largest split that still fits ONE round of the streaming 128 x 128 kernel (<= 256 workgroups: gemm.hip v1s) - else, as in round 3, the
    // largest within two v1 workgroups per CU.  0.5 B at B = 8 (126 tiles): down_proj in TWO slices of 38 K steps on v1s instead of four of
    // 19 on v1, 33 -> 16 MB of partials: prefill 3.92 -> 3.77 ms (profiles/r04_ttft_down_split.log)
    const long ncu = cu_count(c);
    auto pick_splits = [&](int N, int K, int max_sp) {
        const long tiles = (long)(Mp / 128) * (N / 128);
        if (N % 128 == 0)
            for (long cap = ncu; cap <= 2 * ncu; cap += ncu)        // one round, then two rounds, of one workgroup per CU (256 / 512 on MI355X)
                for (int sp = kMaxSplits; sp > 1; sp >>= 1)
                    if (sp <= max_sp && tiles * sp <= cap && K % (64 * sp) == 0) return sp;
        return 1;
    };
    const int down_sp = pick_splits(H, I, c->down_splits), o_sp = pick_splits(H, nh * hd, c->o_splits);
    // q|k|v projection: split in two, the reduce applies bias + rotary embedding + the KV-cache copies (splitk_bias_rope_kernel)
    const int qkv_sp = pick_splits(c->qkvw, H, std::min(c->qkv_splits, 2));
    auto weights = [&](int layer, int matrix, const void** p) -> int { return stack_weights(c, st, layer, matrix, p); };
    const void *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wd = nullptr, *wlm = nullptr;
    bool xn_ready = false;                      // c->xn already holds input_layernorm(c->h) of the coming layer
    for (int l = 0; l < c->L; ++l) {
        const LayerOff& o = c->lo[l];
        if (!xn_ready) LCHECK(fvhd_launch_rmsnorm(st, c->h, c->xn, (const float*)(w + o.ln1), Mp, H, c->eps), "rmsnorm 1");
        void* kc = k_cache ? (char*)k_cache + l * cache_layer : nullptr;
        void* vc = v_cache ? (char*)v_cache + l * cache_layer : nullptr;
        LCHECK(weights(l, FVHD_MAT_QKV, &wqkv), "dequantise q|k|v");
        if (qkv_sp > 1) {
            LCHECK(fvhd_launch_gemm_splitk_partials(st, c->xn, wqkv, c->part, Mp, c->qkvw, H, qkv_sp), "qkv gemm (split-K)");
            LCHECK(fvhd_launch_splitk_bias_rope(st, c->part, qkv_sp, Mp, (const float*)(w + o.bqkv), c->qkv, (const long*)position_ids, c->rope, kc, vc,
                                                M, T, nh, nkv, hd, c->ws_pos, c->theta), "qkv reduce + bias + rope");
        } else if (c->fuse_rope && fvhd_gemm_qkv_rope_supported(Mp, c->qkvw, H, hd, nh, nkv)) {
            // round 5: bias + rotary embedding + the KV-cache copies in the projection's own epilogue (head_dim 64; bit-identical to the two launches)
            LCHECK(fvhd_launch_gemm_qkv_rope(st, c->xn, wqkv, (const float*)(w + o.bqkv), c->qkv, Mp, c->qkvw, H, (const long*)position_ids, c->rope, kc, vc,
                                             M, T, nh, nkv, hd, c->ws_pos, c->theta), "qkv gemm + rope");
        } else {
            LCHECK(fvhd_launch_gemm(st, c->xn, wqkv, (const float*)(w + o.bqkv), nullptr, nullptr, c->qkv, Mp, c->qkvw, H, FVHD_EPI_BIAS, FVHD_BF16), "qkv gemm");
            LCHECK(fvhd_launch_rope(st, c->qkv, (const long*)position_ids, c->rope, kc, vc, M, T, nh, nkv, hd, c->ws_pos, c->theta), "rope");
        }
        if (extend) {
            LCHECK(fvhd_launch_llm_cache_append(st, c->qkv, c->kcache + l * ext_layer, c->vcache + l * ext_layer, l == 0 ? c->mask : nullptr, key_valid, B, T, nh,
                                                nkv, hd, c->dc_cap, c->len, c->status, c->status_host_dev), "cache append");
            LCHECK(fvhd_launch_llm_attention_past(st, c->qkv, c->kcache + l * ext_layer, c->vcache + l * ext_layer, c->mask, c->att, B, T, nh, nkv, hd, c->dc_cap,
                                                  c->len, c->status), "attention over the cache");
        } else {
            LCHECK(fvhd_launch_llm_attention(st, c->qkv, c->att, key_valid, B, T, nh, nkv, hd), "attention");
        }
        LCHECK(weights(l, FVHD_MAT_O, &wo), "dequantise o_proj");
        if (o_sp > 1 && c->fuse_norm) {
            LCHECK(fvhd_launch_gemm_splitk_norm(st, c->att, wo, c->h, c->h, c->part, Mp, H, nh * hd, o_sp, (const float*)(w + o.ln2), c->xn, c->eps),
                   "o_proj gemm (split-K + rmsnorm 2)");
        } else {
            if (o_sp > 1) LCHECK(fvhd_launch_gemm_splitk(st, c->att, wo, c->h, c->h, c->part, Mp, H, nh * hd, o_sp), "o_proj gemm (split-K)");
            else LCHECK(fvhd_launch_gemm(st, c->att, wo, nullptr, nullptr, c->h, c->h, Mp, H, nh * hd, FVHD_EPI_RESID, FVHD_BF16), "o_proj gemm");
            LCHECK(fvhd_launch_rmsnorm(st, c->h, c->xn, (const float*)(w + o.ln2), Mp, H, c->eps), "rmsnorm 2");
        }
        LCHECK(weights(l, FVHD_MAT_GATE_UP, &wgu), "dequantise gate|up");
        LCHECK(fvhd_launch_gemm(st, c->xn, wgu, nullptr, nullptr, nullptr, c->act, Mp, 2 * I, H, FVHD_EPI_SWIGLU, FVHD_BF16), "gate_up gemm");
        xn_ready = false;
        LCHECK(weights(l, FVHD_MAT_DOWN, &wd), "dequantise down_proj");
        if (down_sp > 1 && c->fuse_norm && l + 1 < c->L) {
            LCHECK(fvhd_launch_gemm_splitk_norm(st, c->act, wd, c->h, c->h, c->part, Mp, H, I, down_sp, (const float*)(w + c->lo[l + 1].ln1), c->xn, c->eps),
                   "down gemm (split-K + rmsnorm 1 of the next layer)");
            xn_ready = true;
        } else if (down_sp > 1) {
            LCHECK(fvhd_launch_gemm_splitk(st, c->act, wd, c->h, c->h, c->part, Mp, H, I, down_sp), "down gemm (split-K)");
        } else {
            LCHECK(fvhd_launch_gemm(st, c->act, wd, nullptr, nullptr, c->h, c->h, Mp, H, I, FVHD_EPI_RESID, FVHD_BF16), "down gemm");
        }
    }
    // logits of the LAST position of every sequence (what generate() reads: outputs.logits[:, -1, :])
    LCHECK(fvhd_launch_gather_rows(st, c->h, c->last, B, T, T - 1, H), "gather last rows");
    LCHECK(fvhd_launch_rmsnorm(st, c->last, c->lastn, (const float*)(w + c->norm_off), B, H, c->eps), "final norm");
    LCHECK(weights(-1, FVHD_MAT_LM_HEAD, &wlm), "dequantise lm_head");
    LCHECK(fvhd_launch_gemm(st, c->lastn, wlm, nullptr, nullptr, nullptr, logits_out, B, c->V, H, FVHD_EPI_NONE, FVHD_F32), "lm_head gemm");
    c->last_batch = B; c->last_T = T; c->last_gen = c->generation;      // fvhd_llm_score: c->h holds these rows
    return 0;
}

// The score scratch for up to `rows` rows: 16 bytes per (row, segment).  S * M is not monotone in M (S falls as the row blocks grow), so the
// allocation covers every M <= rows: S <= 64, and S <= max(1, 512 / blocks) with M <= 128 blocks.
static size_t score_bytes_for(int rows)
{
    const size_t blocks = ((size_t)rows + 127) / 128;
    return 16 * std::min((size_t)64 * rows, (size_t)65536 + 128 * blocks);
}

static int ensure_score_ws(fvhd_llm* c, int rows, hipStream_t st, bool check_capture)
{
    const size_t need = score_bytes_for(rows);
    if (c->score_ws && need <= c->score_bytes) return 0;
    if (check_capture && is_capturing(st))
        return lfail("fvhd_llm_score: the score scratch must grow for " + std::to_string(rows) + " rows but the stream is being captured - call "
                     "fvhd_llm_score_reserve first");
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess)
        return lfail(std::string(check_capture ? "fvhd_llm_score" : "fvhd_llm_score_reserve") + ": the score scratch must grow, which synchronises the device, "
                     "and that failed - not allowed while a stream is being captured, reserve before the capture begins (hipDeviceSynchronize: " +
                     hipGetErrorString(e) + ")");
    if (c->score_ws) {
        if (c->score_captured) c->retired.push_back(c->score_ws);      // a caller's graph may still replay on it
        else (void)hipFree(c->score_ws);
    }
    c->score_ws = nullptr;
    c->score_bytes = 0;
    c->score_captured = false;
    e = hipMalloc((void**)&c->score_ws, need);
    if (e != hipSuccess) return lhip("hipMalloc(llm score scratch)", e);
    c->score_bytes = need;
    return 0;
}

extern "C" {

int fvhd_llm_set_max_positions(fvhd_llm* c, int max_position_embeddings)
{
    if (!c || max_position_embeddings <= 0) return lfail("fvhd_llm_set_max_positions: bad argument");
    c->max_pos = max_position_embeddings;      // takes effect at the next workspace (re)allocation: call it before fvhd_llm_reserve
    return 0;
}

int fvhd_llm_workspace_generation(const fvhd_llm* c) { return c ? c->generation : -1; }

int fvhd_llm_reserve(fvhd_llm* c, int batch, int seq_len)
{
    if (!c || batch <= 0 || seq_len <= 0) return lfail("fvhd_llm_reserve: bad argument");
    LLM_ON_DEVICE(c);
    return ensure_ws(c, batch, seq_len, nullptr, false);
}

int fvhd_llm_prefill(fvhd_llm* c, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch, int seq_len,
                     float* logits_out, void* k_cache, void* v_cache, fvhd_stream_t stream)
{
    if (!c || !embeds || !logits_out) return lfail("fvhd_llm_prefill: NULL argument");
    if (dtype < 0 || dtype > 2) return lfail("fvhd_llm_prefill: bad dtype");
    if (batch <= 0 || seq_len <= 0) return lfail("fvhd_llm_prefill: batch and seq_len must be positive");
    if ((k_cache == nullptr) != (v_cache == nullptr)) return lfail("fvhd_llm_prefill: k_cache and v_cache come together");
    if (first_missing_tensor(c) >= 0) return lfail("fvhd_llm_prefill: weights incomplete (fvhd_llm_finalize reports the missing tensor)");
    return decoder_stack(c, embeds, dtype, key_valid, position_ids, batch, seq_len, logits_out, k_cache, v_cache, (hipStream_t)stream, false);
}

int fvhd_llm_score_reserve(fvhd_llm* c, int rows)
{
    if (!c || rows <= 0) return lfail("fvhd_llm_score_reserve: bad argument");
    LLM_ON_DEVICE(c);
    if (c->score_ws && score_bytes_for(rows) <= c->score_bytes) return 0;      // nothing to do: allowed at any time
    // Growing synchronises the device.  The call has no stream to ask about a capture (asking the legacy stream invalidates a capture in
    // progress on this runtime: tried), so - like fvhd_llm_reserve - it learns of one from the failed synchronise and says so.
    return ensure_score_ws(c, rows, nullptr, false);
}

// final norm of ALL rows of the last stack call, lm_head, log-softmax and the pick of the target in one kernel (llm_score.hip)
int fvhd_llm_score(fvhd_llm* c, const int64_t* target_ids, float* logprob_out, float* lse_out, fvhd_stream_t stream)
{
    if (!c) return lfail("fvhd_llm_score: NULL context");
    if (!target_ids || !logprob_out) return lfail("fvhd_llm_score: NULL targets or output");
    if (!c->ws || c->last_gen != c->generation || c->last_batch <= 0)
        return lfail("fvhd_llm_score: no fvhd_llm_prefill / fvhd_llm_start / fvhd_llm_extend has run on the current workspace - there are no rows to score");
    LLM_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    const int M = c->last_batch * c->last_T, H = c->H;
    if (!fvhd_lm_score_plan(M, c->V, H))
        return lfail("fvhd_llm_score: needs vocab % 8 == 0 and hidden % 32 == 0 (vocab " + std::to_string(c->V) + ", hidden " + std::to_string(H) + ")");
    if (int e = ensure_score_ws(c, M, st, true)) return e;
    if (is_capturing(st)) { c->score_captured = true; c->ws_captured = true; }
    const char* w = c->wdev;
    LCHECK(fvhd_launch_rmsnorm(st, c->h, c->xn, (const float*)(w + c->norm_off), M, H, c->eps), "final norm (all rows)");
    const void* wlm = nullptr;
    LCHECK(stack_weights(c, st, -1, FVHD_MAT_LM_HEAD, &wlm), "dequantise lm_head");
    LCHECK(fvhd_launch_lm_score(st, c->xn, wlm, target_ids, M, c->V, H, logprob_out, lse_out, c->score_ws), "lm_head score");
    return 0;
}

// hidden states after the decoder stack (before the final norm) of the last prefill: [batch * seq_len, hidden] bf16, for tests
int fvhd_llm_debug_hidden(fvhd_llm* c, void* out, int rows, fvhd_stream_t stream)
{
    if (!c || !out || rows <= 0 || rows > c->ws_rows) return lfail("fvhd_llm_debug_hidden: bad argument");
    DeviceGuard g(c->device);
    hipError_t e = hipMemcpyAsync(out, c->h, (size_t)rows * c->H * 2, hipMemcpyDeviceToDevice, (hipStream_t)stream);
    return e == hipSuccess ? 0 : lhip("hipMemcpyAsync", e);
}

}  // extern "C"
