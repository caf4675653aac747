// C ABI of the Qwen2 decode (include/fvhd.h "LLM decode"): the library's own KV cache, one token per sequence per step.
// Kernels: llm_decode.hip, llm_w8.hip, llm_sample.hip, llm_beam.hip, llm_logits.hip, llm_constrain.hip, llm_guidance.hip, llm_spec.hip, llm_extend.hip.
#include <algorithm>
#include <cmath>

#include "llm_ctx.h"

namespace {

fvhd_llm::Plan dec_plan(int N, int K, int ncu)
{
    // split K until the grid holds about two workgroups per CU (at most 16 slices: the last arriver reads them all)
    const int ntiles = N / 16, ncol = (ntiles + 3) / 4, KC = K / 128;
    const int want = (2 * ncu + ncol - 1) / ncol;
    fvhd_llm::Plan p;
    p.S = std::max(1, std::min(std::min(want, KC), 16));
    p.cpw = (KC + p.S - 1) / p.S;
    p.S = (KC + p.cpw - 1) / p.cpw;
    return p;
}

void att_plan(int cap, int heads, int ncu, int* S, int* chunk)
{
    // key slices until the grid (batch * n_heads * slices) holds ~2 workgroups per CU - at B = 1 the 14 heads of Qwen2-0.5B alone fill
    // 14 of 256 CUs - with at least 64 keys (one block per lane) per slice and at most 32 slices
    const int want = (2 * ncu + heads - 1) / heads;
    const int s = std::max(1, std::min(std::min(want, (cap + 63) / 64), 32));
    *chunk = ((cap + s - 1) / s + 63) / 64 * 64;
    *S = (cap + *chunk - 1) / *chunk;
}

int dec_status_error(const fvhd_llm* c, const char* who)
{
    const int st = *(volatile int*)c->status_host;
    if (st == 1)
        return lfail(std::string(who) + ": the KV cache is full (capacity " + std::to_string(c->dc_cap) +
                     " positions): a decode step past it wrote nothing - reserve a larger cache (fvhd_llm_cache_reserve) and start again");
    if (st == 2) return lfail(std::string(who) + ": a decode step was given a token id outside [0, vocab); it wrote nothing - start again");
    if (st == 3) return lfail(std::string(who) + ": a cache reorder was given a row index outside [0, rows_in); it wrote nothing - start again");
    if (st == 4) return lfail(std::string(who) + ": a cache rewind was given a keep length outside [0, length]; it changed nothing - start again");
    return 0;
}

// the enqueue-time rule behind a cache reorder / rewind: nothing may feed the ids the previous step chose
int stale_ids_error(const fvhd_llm* c, const char* who)
{
    if (!c->ids_stale) return 0;
    return lfail(std::string(who) + ": the ids the previous step chose belong to the rows as they were before the cache reorder / rewind "
                 "(fvhd_llm_cache_gather / fvhd_llm_cache_rewind) - continue with fvhd_llm_extend, or with fvhd_llm_decode on explicit token_ids");
}

DecSampleArgs dec_sample_args(const fvhd_llm* c, const float* logits, int B)
{
    DecSampleArgs a;
    a.logits = logits; a.B = B; a.V = c->V; a.temperature = c->temperature; a.top_k = c->top_k; a.top_p = c->top_p; a.seed = c->seed;
    a.min_p = c->min_p; a.typical_p = c->typical_p; a.epsilon_cutoff = c->epsilon_cutoff; a.eta_cutoff = c->eta_cutoff;
    return a;
}

// the decode's input embedding: model.embed_tokens.weight when it was set, the packed lm_head rows only when the caller said the model ties them
int dec_embedding_error(const fvhd_llm* c, const char* who)
{
    if (c->emb || c->tied == 1) return 0;
    if (c->tied == 0)
        return lfail(std::string(who) + ": this model does not tie its embeddings - set model.embed_tokens.weight (fvhd_llm_set_tensor) before decoding");
    return lfail(std::string(who) + ": the decode's input embedding is unknown - set model.embed_tokens.weight (fvhd_llm_set_tensor), or call "
                 "fvhd_llm_set_tied_embeddings(ctx, 1) for a model whose lm_head IS its embedding table (tie_word_embeddings)");
}

// what a verify step under sampling, or one that keeps log-probabilities, needs beyond fvhd_llm_spec_reserve's scratch (llm_ctx.h `spx`),
// for the rows that scratch covers.  Kept while it covers them; growing synchronises, so it is refused on a capturing stream.
int spec_extra_ensure(fvhd_llm* c, const char* who, hipStream_t st)
{
    if (c->spx && c->spx_rows >= c->spec_rows) return 0;
    if (st && is_capturing(st))
        return lfail(std::string(who) + ": the scratch for the step's logits must grow but the stream is being captured - call fvhd_llm_spec_reserve "
                     "after fvhd_llm_set_verify_sampling / fvhd_llm_set_logprobs, or run one step before capturing");
    hipError_t he = hipDeviceSynchronize();
    if (he != hipSuccess) return lhip("hipDeviceSynchronize", he);
    if (c->spx) {
        if (c->spx_captured) c->retired.push_back(c->spx);       // a captured step replays on the old one
        else (void)hipFree(c->spx);
    }
    c->spx = nullptr;
    c->spx_rows = 0;
    c->spx_captured = false;
    const int T = c->spec_rows;
    Arena a;
    const size_t o_ws = a.take(fvhd_dec_logprobs_scratch_bytes(T, c->V, 16)), o_logits = a.take((size_t)T * c->V * 4), o_tok = a.take(4 * 16),
                 o_ids = a.take(8 * 16 * 16), o_top = a.take(4 * 16 * 16), o_emitted = a.take(4);
    if ((he = hipMalloc((void**)&c->spx, a.off)) != hipSuccess) { c->spx = nullptr; return lhip("hipMalloc(verify step logits scratch)", he); }
    if ((he = hipMemset(c->spx, 0, a.off)) != hipSuccess) return lhip("hipMemset(verify step logits scratch)", he);      // counters start at zero
    char* d = c->spx;
    c->spx_lp_ws = d + o_ws; c->spx_logits = (float*)(d + o_logits); c->spx_tok = (float*)(d + o_tok); c->spx_ids = (int64_t*)(d + o_ids);
    c->spx_top = (float*)(d + o_top); c->spx_emitted = (int*)(d + o_emitted);
    c->spx_rows = T;
    return 0;
}

int constraint_start_error(const fvhd_llm* c, const char* who, int B)
{
    if (c->con_n_start == 1 || c->con_n_start >= B) return 0;
    return lfail(std::string(who) + ": the constraint was set with " + std::to_string(c->con_n_start) + " start states, this call has " + std::to_string(B) +
                 " rows - set it (fvhd_llm_set_constraint) with one start state, or one per row of fvhd_llm_cache_reserve");
}

// classifier-free guidance pairs row g with row B / 2 + g
int guidance_rows_error(const char* who, int B)
{
    if (B % 2 == 0) return 0;
    return lfail(std::string(who) + ": guidance is on (fvhd_llm_set_guidance) and the batch is odd (" + std::to_string(B) + " rows) - row g is the "
                 "conditional sequence and row B / 2 + g its unconditional one, so the batch must be 2 G");
}

// the refusal of a call that would break, or does not carry, the pairing of the rows
int guidance_refusal(const fvhd_llm* c, const char* who, const char* why)
{
    if (!guidance_on(c)) return 0;
    return lfail(std::string(who) + ": guidance is on (fvhd_llm_set_guidance) - " + why + "; switch it off (scale 1) around the call");
}

// a cache rewind / reorder moves K, V, mask and positions only: `done` = "rewound" / "reordered"
int row_state_refusal(const fvhd_llm* c, const char* who, const char* done)
{
    const std::string w(who);
    if (processors_on(c))
        return lfail(w + ": logits processors are on (fvhd_llm_set_logits_processors) - their token history is not " + done + "; switch them off around " + w);
    if (constraint_on(c))
        return lfail(w + ": a constraint is on (fvhd_llm_set_constraint) - the rows' automaton states are not " + done + "; switch it off around " + w);
    return 0;
}

int logprobs_args_error(const fvhd_llm* c, const char* who, int top_n, const float* token_out, const int64_t* top_ids_out, const float* top_out)
{
    const std::string w(who);
    if (!c || !token_out) return lfail(w + ": NULL argument");
    if (top_n < 0 || top_n > 16) return lfail(w + ": top_n must be in [0, 16] (got " + std::to_string(top_n) + ")");
    if (top_n > c->V) return lfail(w + ": top_n = " + std::to_string(top_n) + " exceeds the vocabulary (" + std::to_string(c->V) + ")");
    if (top_n && (!top_ids_out || !top_out)) return lfail(w + ": top_n > 0 needs top_ids_out and top_logprobs_out");
    return 0;
}

// ---- from logits to a chosen token: the ONE place that orders the logits edits ----
struct ChoiceArgs {
    const char* who = nullptr;     // "first-token" / "decode" / "extend": the launches' LCHECK labels begin with it
    const char* reduce_what = nullptr;   // the argmax reduce's whole label (the decode's is spelled without parentheses)
    float* logits = nullptr;       // fp32 [R][V]; under guidance the unconditional rows lie behind them
    int R = 0;                     // the rows the choice is made on: under guidance the G conditional ones
    const int* gate = nullptr;     // non-NULL: the launches do nothing while *gate != 0
    bool step = false;             // a decode step: histories and automaton states advance on `tok` (NULL: on the ids the previous step chose), the
    const int64_t* tok = nullptr;  // choice advances positions and length, and the lm_head left its fused (max, index) pairs of `logits`;
                                   // false (fvhd_llm_start / _extend): the rows take their start states
    int start_T = 0;               // > 0: fvhd_llm_start on a prompt of start_T tokens - the token history begins empty
    int n_add = 0;                 // the sampler's counter is n = length + n_add
    int64_t* ids_out = nullptr;
    bool beam_rows = false;        // beam scoring is on and the caller takes the logits: they become log-probabilities before any edit
};

// what fvhd_llm_set_beam_scoring does not cover, refused when a call enqueues under it
int beam_scoring_refusal(const fvhd_llm* c, const char* who)
{
    if (!c->beam_scoring) return 0;
    const std::string w(who);
    if (guidance_on(c))
        return lfail(w + ": beam scoring is on (fvhd_llm_set_beam_scoring) and so is guidance (fvhd_llm_set_guidance) - beam search does not carry "
                         "the pairing of conditional and unconditional rows; switch one of them off");
    if (c->lp_on)
        return lfail(w + ": beam scoring is on (fvhd_llm_set_beam_scoring) and so are log-probabilities (fvhd_llm_set_logprobs) - the rows would be "
                         "normalised twice; switch one of them off");
    return 0;
}

// guidance, processors, constraint, then the sampler or the argmax, then the guidance mirror - with the host's marks of what the sequence
// was started with.  `state` is fvhd_llm_start's cache-state launch: before the draw, which reads n = the prompt length from the device,
// and behind the argmax reduce.
template <class StateLaunch = int (*)()>
int choose_tokens(fvhd_llm* c, hipStream_t st, const ChoiceArgs& a, StateLaunch state = [] { return 0; })
{
    const std::string w(a.who);
    const bool gd = guidance_on(c), proc = processors_on(c), con = constraint_on(c);
    int64_t* const posv = a.step ? c->posv : nullptr;
    c->guid_rows = gd ? a.R : 0;
    if (a.start_T) c->hist_started = proc;
    if (!a.step) c->con_started = con;
    // guidance first, where transformers puts it: the guided scores replace the conditional rows before anything else reads them
    if (gd) LCHECK(fvhd_launch_dec_guidance(st, a.logits, a.R, c->V, c->guid_scale, c->guid_ws, a.gate), (w + " guidance").c_str());
    // under beams transformers' processors see log_softmax(x): the rows are normalised before the first edit (llm_beam.hip)
    if (a.beam_rows) LCHECK(fvhd_launch_dec_beam_norm(st, a.logits, a.R, c->V, c->beam_proc_norm, nullptr, a.gate), (w + " row normalisation").c_str());
    if (proc) {
        // an empty history: no token is in the bitmap, and the launch zeroes the rows' history counts
        if (a.start_T)
            if (hipError_t he = hipMemsetAsync(c->hist_seen, 0, (size_t)a.R * ((c->V + 31) / 32) * 4, st)) return lhip("history bitmap reset", he);
        DecLogitsArgs pa;
        pa.logits = a.logits; pa.B = a.R; pa.V = c->V; pa.hist = c->hist; pa.cap = c->dc_cap; pa.seen = c->hist_seen; pa.count = c->hist_count;
        pa.penalty = c->proc_penalty; pa.ngram = c->proc_ngram; pa.min_new = c->proc_n_eos ? c->proc_min_new : 0;
        pa.eos = c->proc_lists; pa.n_eos = c->proc_n_eos; pa.sup = c->proc_lists ? c->proc_lists + kMaxEos : nullptr; pa.n_sup = c->proc_n_sup;
        pa.start_T = a.start_T; pa.status = a.gate;
        if (a.step) { pa.tok = a.tok; pa.last = c->last_ids; }
        if (c->proc_lists && is_capturing(st)) c->proc_lists_captured = true;     // the caller's graph now reads the lists: retired, never overwritten
        LCHECK(fvhd_launch_dec_logits_process(st, &pa), (w + " logits processors").c_str());      // one launch over all rows
    }
    if (con) {
        // behind the processors: the advance on the fed ids, then the bans of the rows' states
        DecConstrainArgs ca;
        ca.logits = a.logits; ca.B = a.R; ca.V = c->V; ca.offsets = c->con_tab; ca.tokens = c->con_tab + c->con_n_states + 1;
        ca.targets = ca.tokens + c->con_n_edges; ca.n_states = c->con_n_states; ca.states = c->con_state; ca.flags = c->con_state + 64; ca.status = a.gate;
        if (a.step) { ca.tok = a.tok; ca.last = c->last_ids; }
        else {                                                   // the rows take their start states (by value: a captured launch keeps them), no flags
            ca.reset = 1; ca.n_start = c->con_n_start;
            std::copy(c->con_start, c->con_start + 64, ca.start);
        }
        if (is_capturing(st)) c->con_captured = true;            // the caller's graph now reads the tables: retired, never overwritten
        LCHECK(fvhd_launch_dec_constrain(st, &ca), (w + " constraint").c_str());
    }
    if (c->do_sample) {
        if (int e = state()) return e;
        DecSampleArgs sa = dec_sample_args(c, a.logits, a.R);
        sa.len = c->len; sa.n_add = a.n_add; sa.last = c->last_ids; sa.ids_out = a.ids_out; sa.posv = posv; sa.len_advance = a.step ? c->len : nullptr;
        sa.status = a.gate;
        LCHECK(fvhd_launch_dec_sample(st, &sa, c->sws), (w + " sampling").c_str());
    } else {
        // the (max, index) pairs + reduce of the decode's lm_head (lowest index on ties).  Fused pairs saw the raw logits: the pairs
        // again, ONCE, from the guided, processed and constrained ones.  (vocab % 16 == 0: either way there are (V + 63) / 64 of them)
        if (!a.step || gd || proc || con)
            LCHECK(fvhd_launch_dec_argmax_blocks(st, a.logits, c->V, a.R, c->amax_v, c->amax_i), (w + " argmax (blocks)").c_str());
        LCHECK(fvhd_launch_dec_argmax_finish(st, c->amax_v, c->amax_i, (c->V + 63) / 64, a.R, c->last_ids, a.ids_out, posv, a.step ? c->len : nullptr,
                                             a.gate), a.reduce_what);
        if (int e = state()) return e;
    }
    if (gd) LCHECK(fvhd_launch_dec_guidance_mirror(st, a.R, c->last_ids, a.ids_out, posv, a.gate), (w + " guidance mirror").c_str());
    return 0;
}

// ---- the decoder layers and the lm_head on the decode GEMM, for the rows of a decode step or of a verify step ----
struct DecRows {
    const char* who = nullptr;     // "decode" / "verify": the launches' LCHECK labels begin with it
    const char* lm_head_what = nullptr;  // the lm_head launch's whole label
    void *h = nullptr, *q = nullptr, *att = nullptr, *act = nullptr;      // bf16 rows: hidden (the embedded tokens), q, attention output, MLP activation
    const int64_t* pos = nullptr;  // the rows' positions
    int rows = 0;
    const int* gate = nullptr;     // the launches do nothing while *gate != 0
    float* rstd = nullptr;         // DecGemmArgs::rstd
    void *ks = nullptr, *vs = nullptr;   // a verify step's staging rows: k / v go there (a "cache" of capacity 1 whose length word is 0) and the
                                   // attention appends them; NULL: k / v go to the cache's slot *len
    float* apart = nullptr;        // the attention's partials and counters
    int* acnt = nullptr;
    float* logits = nullptr;       // fp32 [rows][V] or NULL; the (max, index) pairs go to the context's
};

int decode_layers(fvhd_llm* c, hipStream_t st, const DecRows& r)
{
    const int H = c->H, I = c->I, nh = c->nh, nkv = c->nkv, hd = c->hd, cap = c->dc_cap;
    const char* w = c->wdev;
    const bool q8 = c->wfmt == FVHD_W_E4M3, q4 = c->wfmt == FVHD_W_MXFP4;
    const std::string who(r.who);
    const size_t layer_kv = (size_t)c->dc_batch * nkv * cap * hd * 2;
    auto gemm = [&](int epi, const void* x, const float* norm_w, int layer, int matrix) {
        const Mat m = mat_of(c, layer, matrix);
        const fvhd_llm::Plan& p = c->plan[matrix];
        DecGemmArgs a;
        a.wscale = q8 ? (const float*)(w + m.soff) : nullptr;
        a.wblk = q4 ? (const unsigned char*)(w + m.soff) : nullptr;
        a.x = x; a.ldx = m.K; a.norm_w = norm_w; a.eps = c->eps; a.W = w + m.off; a.N = (int)m.N; a.K = m.K; a.B = r.rows; a.S = p.S; a.cpw = p.cpw;
        a.part = c->dpart; a.cnt = c->cnt; a.epi = epi; a.status = r.gate; a.rstd = r.rstd;
        return a;
    };
    for (int l = 0; l < c->L; ++l) {
        const LayerOff& o = c->lo[l];
        char *kl = c->kcache + l * layer_kv, *vl = c->vcache + l * layer_kv;
        DecGemmArgs a = gemm(DEC_EPI_QKV, r.h, (const float*)(w + o.ln1), l, FVHD_MAT_QKV);
        a.bias = (const float*)(w + o.bqkv); a.out = r.q; a.ldo = nh * hd; a.pos = r.pos; a.rope = c->drope; a.P = c->dc_pos; a.theta = c->theta;
        a.nh = nh; a.nkv = nkv; a.hd = hd;
        if (r.ks) {
            a.kc = r.ks; a.vc = r.vs; a.cap = 1; a.len = c->sp_zero;
            LCHECK(fvhd_launch_dec_gemm(st, &a), "verify q|k|v + rope + staging");
            LCHECK(fvhd_launch_spec_attention(st, r.q, kl, vl, r.ks, r.vs, c->mask, r.att, r.rows, nh, nkv, hd, cap, c->len, c->att_S, c->att_chunk, r.apart,
                                              r.acnt, r.gate), "verify attention + cache append");
        } else {
            a.kc = kl; a.vc = vl; a.cap = cap; a.len = c->len;
            LCHECK(fvhd_launch_dec_gemm(st, &a), "decode q|k|v + rope + cache append");
            LCHECK(fvhd_launch_dec_attention(st, r.q, kl, vl, c->mask, r.att, r.rows, nh, nkv, hd, cap, c->len, 1, c->att_S, c->att_chunk, r.apart, r.acnt,
                                             r.gate), "decode attention");
        }
        a = gemm(DEC_EPI_RESID, r.att, nullptr, l, FVHD_MAT_O);
        a.resid = r.h; a.out = r.h; a.ldo = H;
        LCHECK(fvhd_launch_dec_gemm(st, &a), (who + " o_proj + residual").c_str());
        a = gemm(DEC_EPI_SWIGLU, r.h, (const float*)(w + o.ln2), l, FVHD_MAT_GATE_UP);
        a.out = r.act; a.ldo = I;
        LCHECK(fvhd_launch_dec_gemm(st, &a), (who + " rmsnorm + gate|up + silu").c_str());
        a = gemm(DEC_EPI_RESID, r.act, nullptr, l, FVHD_MAT_DOWN);
        a.resid = r.h; a.out = r.h; a.ldo = H;
        LCHECK(fvhd_launch_dec_gemm(st, &a), (who + " down_proj + residual").c_str());
    }
    DecGemmArgs a = gemm(DEC_EPI_ARGMAX, r.h, (const float*)(w + c->norm_off), -1, FVHD_MAT_LM_HEAD);
    a.logits = r.logits; a.amax_v = c->amax_v; a.amax_i = c->amax_i;
    LCHECK(fvhd_launch_dec_gemm(st, &a), r.lm_head_what);
    return 0;
}

}  // namespace

std::string processors_error(float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens, const int32_t* eos_ids, int n_eos,
                             const int32_t* suppress_ids, int n_suppress, int V)
{
    if (!(repetition_penalty > 0.f) || !std::isfinite(repetition_penalty)) return "repetition_penalty must be finite and > 0 (1 = off)";
    if (no_repeat_ngram_size < 0) return "no_repeat_ngram_size must be >= 0 (0 = off)";
    if (min_new_tokens < 0) return "min_new_tokens must be >= 0 (0 = off)";
    if (n_eos < 0 || n_eos > kMaxEos) return "at most " + std::to_string(kMaxEos) + " EOS ids (got " + std::to_string(n_eos) + ")";
    if (n_suppress < 0 || n_suppress > kMaxSuppress)
        return "at most " + std::to_string(kMaxSuppress) + " suppressed ids (got " + std::to_string(n_suppress) + ")";
    if ((n_eos && !eos_ids) || (n_suppress && !suppress_ids)) return "a list with a count > 0 is NULL";
    for (int k = 0; k < 2 && V > 0; ++k) {
        const int32_t* ids = k ? suppress_ids : eos_ids;
        for (int i = 0; i < (k ? n_suppress : n_eos); ++i)
            if (ids[i] < 0 || ids[i] >= V)
                return std::string(k ? "suppressed" : "EOS") + " id " + std::to_string(ids[i]) + " is outside [0, vocab = " + std::to_string(V) + ")";
    }
    return "";
}

const char* sampling_error(float temperature, int top_k, float top_p)
{
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return "temperature must be finite and > 0";
    if (top_k < 0) return "top_k must be >= 0 (0 = off)";
    if (!(top_p >= 0.f && top_p <= 1.f)) return "top_p must be in [0, 1] (1 = off)";
    return nullptr;
}

// fvhd_llm_set_sampling_warpers' rule: "" when the four are valid, else the refusal, which names the value
std::string warpers_error(float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff)
{
    if (!(min_p >= 0.f && min_p <= 1.f)) return "min_p must be in [0, 1] (0 = off), got " + std::to_string(min_p);
    if (!(typical_p > 0.f && typical_p <= 1.f)) return "typical_p must be in (0, 1] (1 = off), got " + std::to_string(typical_p);
    if (!(epsilon_cutoff >= 0.f && epsilon_cutoff < 1.f)) return "epsilon_cutoff must be in [0, 1) (0 = off), got " + std::to_string(epsilon_cutoff);
    if (!(eta_cutoff >= 0.f && eta_cutoff < 1.f)) return "eta_cutoff must be in [0, 1) (0 = off), got " + std::to_string(eta_cutoff);
    return "";
}

extern "C" {

int fvhd_llm_set_tied_embeddings(fvhd_llm* c, int tied)
{
    if (!c) return lfail("fvhd_llm_set_tied_embeddings: ctx is NULL");
    c->tied = tied != 0 ? 1 : 0;
    return 0;
}

int fvhd_llm_cache_reserve(fvhd_llm* c, int batch, int capacity)
{
    if (!c || batch < 1 || batch > 64 || capacity < 1) return lfail("fvhd_llm_cache_reserve: needs a context, 1 <= batch <= 64 and capacity >= 1");
    if (first_missing_tensor(c) >= 0) return lfail("fvhd_llm_cache_reserve: weights incomplete (fvhd_llm_finalize reports the missing tensor)");
    if (c->H % 128 || (c->nh * c->hd) % 128 || c->I % 128)
        return lfail("fvhd_llm_cache_reserve: the decode needs hidden, n_heads * head_dim and intermediate to be multiples of 128");
    LLM_ON_DEVICE(c);
    int e = ensure_ws(c, batch, 1, nullptr, false);              // the rotary table
    if (e) return e;
    const int ncu = cu_count(c);
    const int H = c->H, I = c->I, nh = c->nh, nkv = c->nkv, hd = c->hd, V = c->V, L = c->L;
    att_plan(capacity, batch * nh, ncu, &c->att_S, &c->att_chunk);
    const int NB = (batch + 15) / 16;                            // batch tiles of the decode GEMM: slabs and (max, index) pairs per tile
    size_t part = 0;
    int ncol = 1;
    for (int m = FVHD_MAT_QKV; m <= FVHD_MAT_DOWN; ++m) {
        const Mat d = mat_of(c, 0, m);
        const fvhd_llm::Plan p = c->plan[m] = dec_plan((int)d.N, d.K, ncu);
        if (p.S > 1) part = std::max(part, (size_t)p.S * d.N * 64 * NB);
        ncol = std::max(ncol, ((int)d.N / 16 + 3) / 4);
    }
    c->plan[FVHD_MAT_LM_HEAD] = fvhd_llm::Plan{1, H / 128};
    const int lm_ncol = (V / 16 + 3) / 4;
    c->cnt_att = ncol;
    Arena a;
    const size_t kvb = (size_t)L * batch * nkv * capacity * hd * 2;
    const size_t o_k = a.take(kvb), o_v = a.take(kvb), o_mask = a.take((size_t)batch * capacity), o_pos = a.take(8 * batch), o_last = a.take(8 * batch),
                 o_len = a.take(4), o_status = a.take(4), o_h = a.take((size_t)batch * H * 2), o_q = a.take((size_t)batch * nh * hd * 2),
                 o_att = a.take((size_t)batch * nh * hd * 2), o_act = a.take((size_t)batch * I * 2), o_part = a.take(std::max(part, (size_t)16)),
                 o_apart = a.take((size_t)batch * nh * c->att_S * (hd + 2) * 4), o_cnt = a.take((size_t)(ncol + batch * nh) * 4),
                 o_av = a.take((size_t)lm_ncol * 16 * NB * 4), o_ai = a.take((size_t)lm_ncol * 16 * NB * 4), o_logits = a.take((size_t)batch * V * 4),
                 o_rope = a.take((size_t)c->ws_pos * hd * 4), o_sws = a.take(fvhd_dec_sample_ws_bytes()), o_rstd = a.take(4 * 64),
                 o_hist = a.take((size_t)batch * capacity * 4), o_seen = a.take((size_t)batch * ((V + 31) / 32) * 4), o_hcount = a.take((size_t)batch * 4);
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured (like fvhd_llm_reserve)
    if (he != hipSuccess) return lhip("fvhd_llm_cache_reserve: hipDeviceSynchronize", he);
    if (c->dc) (void)hipFree(c->dc);
    if (c->beam) (void)hipFree(c->beam);                         // sized for the cache it was reserved for: fvhd_llm_beam_reserve again
    if (c->spec) (void)hipFree(c->spec);                         // likewise: fvhd_llm_spec_reserve again
    if (c->lp_ws) (void)hipFree(c->lp_ws);                       // likewise: fvhd_llm_set_logprobs again
    if (c->beam_proc) (void)hipFree(c->beam_proc);               // likewise: fvhd_llm_set_beam_scoring again
    c->dc = c->beam = c->beam_topk = c->spec = c->lp_ws = c->beam_proc = c->beam_proc_norm = c->beam_proc_hist = nullptr;
    c->beam_scoring = 0;
    c->lp_on = 0;
    c->lp_logits = nullptr;
    c->spec_rows = 0;
    c->sp_begun = false;
    c->dc_batch = c->dc_cap = c->run_batch = 0;
    c->hist_started = false;
    c->con_started = false;
    c->ids_stale = false;
    if ((he = hipMalloc((void**)&c->dc, a.off)) != hipSuccess) return lhip("hipMalloc(llm KV cache)", he);
    if ((he = hipMemset(c->dc, 0, a.off)) != hipSuccess) return lhip("hipMemset(llm KV cache)", he);      // counters start at zero
    if (!c->status_host) {
        if ((he = hipHostMalloc((void**)&c->status_host, 4, hipHostMallocMapped)) != hipSuccess) return lhip("hipHostMalloc(status word)", he);
        if ((he = hipHostGetDevicePointer((void**)&c->status_host_dev, c->status_host, 0)) != hipSuccess) return lhip("hipHostGetDevicePointer", he);
    }
    *(volatile int*)c->status_host = 0;
    char* d = c->dc;
    c->kcache = d + o_k; c->vcache = d + o_v; c->mask = (unsigned char*)(d + o_mask); c->posv = (int64_t*)(d + o_pos); c->last_ids = (int64_t*)(d + o_last);
    c->len = (int*)(d + o_len); c->status = (int*)(d + o_status); c->dh = d + o_h; c->dq = d + o_q; c->datt = d + o_att; c->dact = d + o_act;
    c->dpart = (float*)(d + o_part); c->apart = (float*)(d + o_apart); c->cnt = (int*)(d + o_cnt); c->amax_v = (float*)(d + o_av);
    c->amax_i = (int*)(d + o_ai); c->dlogits = (float*)(d + o_logits); c->drope = (float*)(d + o_rope); c->sws = d + o_sws; c->drstd = (float*)(d + o_rstd);
    c->hist = (int*)(d + o_hist); c->hist_seen = (unsigned*)(d + o_seen); c->hist_count = (int*)(d + o_hcount);
    c->dc_bytes = a.off; c->dc_batch = batch; c->dc_cap = capacity; c->dc_pos = c->ws_pos;
    // the decode's own copy of the rotary table: a later, larger prefill may replace the prefill workspace under a captured decode graph
    if ((he = hipMemcpy(c->drope, c->rope, (size_t)c->ws_pos * hd * 4, hipMemcpyDeviceToDevice)) != hipSuccess) return lhip("hipMemcpy(rope table)", he);
    return 0;
}

int fvhd_llm_start(fvhd_llm* c, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch, int seq_len,
                   float* logits_out, int64_t* next_ids_out, fvhd_stream_t stream)
{
    if (!c || !embeds) return lfail("fvhd_llm_start: NULL argument");
    if (!c->dc) return lfail("fvhd_llm_start: no KV cache - call fvhd_llm_cache_reserve first");
    if (batch < 1 || batch > c->dc_batch) return lfail("fvhd_llm_start: batch must be in [1, the batch of fvhd_llm_cache_reserve]");
    if (seq_len < 1 || seq_len > c->dc_cap) return lfail("fvhd_llm_start: seq_len must be in [1, the capacity of fvhd_llm_cache_reserve]");
    if (int e = dec_embedding_error(c, "fvhd_llm_start")) return e;
    if (int e = beam_scoring_refusal(c, "fvhd_llm_start")) return e;
    const bool gd = guidance_on(c);
    if (gd)
        if (int e = guidance_rows_error("fvhd_llm_start", batch)) return e;
    const int R = gd ? batch / 2 : batch;                        // the rows the choice is made on: under guidance the G conditional ones
    const bool con = constraint_on(c);
    if (con)
        if (int e = constraint_start_error(c, "fvhd_llm_start", R)) return e;
    LLM_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    const int L = c->L, nkv = c->nkv, hd = c->hd, T = seq_len, B = batch, cap = c->dc_cap;
    const size_t layer_src = (size_t)B * nkv * T * hd * 2, need = 2 * (size_t)L * layer_src;
    if (need > c->pre_kv_bytes) {
        if (is_capturing(st)) return lfail("fvhd_llm_start: its staging buffer must grow but the stream is being captured");
        hipError_t he = hipDeviceSynchronize();
        if (he != hipSuccess) return lhip("hipDeviceSynchronize", he);
        if (c->pre_kv) (void)hipFree(c->pre_kv);
        c->pre_kv = nullptr;
        c->pre_kv_bytes = 0;
        if ((he = hipMalloc((void**)&c->pre_kv, need)) != hipSuccess) return lhip("hipMalloc(prefill KV staging)", he);
        c->pre_kv_bytes = need;
    }
    *(volatile int*)c->status_host = 0;
    float* logits = logits_out ? logits_out : c->dlogits;
    c->lp_logits = nullptr;
    char* pk = c->pre_kv;
    char* pv = c->pre_kv + (size_t)L * layer_src;
    int e = fvhd_llm_prefill(c, embeds, dtype, key_valid, position_ids, B, T, logits, pk, pv, stream);
    if (e) return e;
    const size_t layer_dst = (size_t)c->dc_batch * nkv * cap * hd * 2;
    for (int l = 0; l < L; ++l) {
        hipError_t he = hipMemcpy2DAsync(c->kcache + l * layer_dst, (size_t)cap * hd * 2, pk + l * layer_src, (size_t)T * hd * 2, (size_t)T * hd * 2,
                                         (size_t)B * nkv, hipMemcpyDeviceToDevice, st);
        if (he == hipSuccess)
            he = hipMemcpy2DAsync(c->vcache + l * layer_dst, (size_t)cap * hd * 2, pv + l * layer_src, (size_t)T * hd * 2, (size_t)T * hd * 2,
                                  (size_t)B * nkv, hipMemcpyDeviceToDevice, st);
        if (he != hipSuccess) return lhip("hipMemcpy2DAsync(KV cache)", he);
    }
    hipError_t he = hipMemsetAsync(c->mask, 0, (size_t)c->dc_batch * cap, st);
    if (he == hipSuccess)
        he = key_valid ? hipMemcpy2DAsync(c->mask, cap, key_valid, T, T, B, hipMemcpyDeviceToDevice, st) : hipMemset2DAsync(c->mask, cap, 1, T, B, st);
    if (he != hipSuccess) return lhip("key mask copy", he);
    // the first token, ungated, of the prefill's logits; the histories and the rows' automaton states begin here
    ChoiceArgs ch;
    ch.who = "first-token"; ch.reduce_what = "first-token argmax (reduce)"; ch.logits = logits; ch.R = R; ch.start_T = T; ch.ids_out = next_ids_out;
    ch.beam_rows = c->beam_scoring && logits_out;
    e = choose_tokens(c, st, ch, [&] {
        LCHECK(fvhd_launch_dec_start_state(st, c->posv, position_ids, B, T, c->len, c->status), "decode state");
        return 0;
    });
    if (e) return e;
    c->run_batch = B;
    c->sp_begun = false;                                         // a lookup generation belongs to the sequence it was begun on
    c->ids_stale = false;                                        // the ids chosen here are these rows'
    c->lp_logits = logits;
    return 0;
}

int fvhd_llm_decode(fvhd_llm* c, const int64_t* token_ids, float* logits_out, int64_t* next_ids_out, fvhd_stream_t stream)
{
    if (!c) return lfail("fvhd_llm_decode: ctx is NULL");
    if (!c->dc || !c->run_batch) return lfail("fvhd_llm_decode: no started sequence - call fvhd_llm_cache_reserve and fvhd_llm_start first");
    if (int e = dec_status_error(c, "fvhd_llm_decode")) return e;
    if (int e = dec_embedding_error(c, "fvhd_llm_decode")) return e;
    if (int e = beam_scoring_refusal(c, "fvhd_llm_decode")) return e;
    if (!token_ids)
        if (int e = stale_ids_error(c, "fvhd_llm_decode(token_ids = NULL)")) return e;
    const bool proc = processors_on(c);
    if (proc && !c->hist_started)
        return lfail("fvhd_llm_decode: logits processors are on but the sequence was started without them (no token history) - set them "
                     "before fvhd_llm_start");
    const bool gd = guidance_on(c);
    if (gd)
        if (int e = guidance_rows_error("fvhd_llm_decode", c->run_batch)) return e;
    const bool con = constraint_on(c);
    if (con && !c->con_started)
        return lfail("fvhd_llm_decode: a constraint is on (fvhd_llm_set_constraint) but the sequence was started without it (the rows have no "
                     "states) - set it before fvhd_llm_start / fvhd_llm_extend");
    LLM_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    const int B = c->run_batch, H = c->H, cap = c->dc_cap;
    const char* w = c->wdev;
    const bool q8 = c->wfmt == FVHD_W_E4M3, q4 = c->wfmt == FVHD_W_MXFP4;
    if (q4 && !c->emb) {
        LCHECK(fvhd_launch_dec_embed_w4(st, token_ids, c->last_ids, w + c->lm_off, w + c->lm_soff, c->V, H, c->dh, c->mask, B, cap, c->len, c->status,
                                        c->status_host_dev), "decode embed (MXFP4 lm_head rows)");
    } else if (q8 && !c->emb) {                                         // a tied model: the token row dequantised from the lm_head codes
        LCHECK(fvhd_launch_dec_embed_w8(st, token_ids, c->last_ids, w + c->lm_off, (const float*)(w + c->lm_soff), c->V, H, c->dh, c->mask, B, cap, c->len,
                                        c->status, c->status_host_dev), "decode embed (e4m3 lm_head rows)");
    } else {
        LCHECK(fvhd_launch_dec_embed(st, token_ids, c->last_ids, c->emb ? c->emb : w + c->lm_off, c->V, H, c->dh, c->mask, B, cap, c->len, c->status,
                                     c->status_host_dev), "decode embed");
    }
    DecRows r;
    r.who = "decode"; r.lm_head_what = c->do_sample ? "decode final norm + lm_head" : "decode final norm + lm_head + argmax";
    r.h = c->dh; r.q = c->dq; r.att = c->datt; r.act = c->dact; r.pos = c->posv; r.rows = B; r.gate = c->status;
    r.rstd = c->dec_rstd_once ? c->drstd : nullptr; r.apart = c->apart; r.acnt = c->cnt + c->cnt_att;
    // the logits are kept where something reads them behind the lm_head: an edit, the sampler, fvhd_llm_set_logprobs
    r.logits = logits_out ? logits_out : proc || con || gd || c->do_sample || c->lp_on ? c->dlogits : nullptr;
    c->lp_logits = nullptr;
    if (int e = decode_layers(c, st, r)) return e;
    // the choice advances positions and length; under sampling it replaces the argmax reduce and draws with n = length + 1 (the cache
    // holds this step's token)
    ChoiceArgs ch;
    ch.who = "decode"; ch.reduce_what = "decode argmax reduce"; ch.logits = r.logits; ch.R = gd ? B / 2 : B; ch.gate = c->status;
    ch.step = true; ch.tok = token_ids; ch.n_add = 1; ch.ids_out = next_ids_out; ch.beam_rows = c->beam_scoring && logits_out;
    if (int e = choose_tokens(c, st, ch)) return e;
    c->sp_begun = false;                                         // a plain step: the token buffer of a lookup generation no longer describes the sequence
    if (token_ids) c->ids_stale = false;                         // the ids chosen on fed ids are these rows'
    c->lp_logits = r.logits;                                     // (NULL: this step kept none)
    return 0;
}

// ---- extend: a chunk of T tokens per row onto the started cache (include/fvhd.h "LLM extend"; kernels: llm_extend.hip) ----
int fvhd_llm_extend(fvhd_llm* c, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int T, float* logits_out,
                    int64_t* next_ids_out, fvhd_stream_t stream)
{
    if (!c || !embeds) return lfail("fvhd_llm_extend: NULL argument");
    if (dtype < 0 || dtype > 2) return lfail("fvhd_llm_extend: bad dtype");
    if (!c->dc || !c->run_batch) return lfail("fvhd_llm_extend: no started sequence - call fvhd_llm_cache_reserve and fvhd_llm_start first");
    if (T < 1) return lfail("fvhd_llm_extend: the chunk length T must be >= 1");
    if (T > c->dc_cap)
        return lfail("fvhd_llm_extend: the chunk length T = " + std::to_string(T) + " exceeds the capacity of fvhd_llm_cache_reserve (" +
                     std::to_string(c->dc_cap) + ")");
    if (c->hd != 64 && c->hd != 128) return lfail("fvhd_llm_extend: the attention over the cache needs head_dim 64 or 128");
    if (int e = dec_status_error(c, "fvhd_llm_extend")) return e;
    if (c->beam_scoring)
        return lfail("fvhd_llm_extend: beam scoring is on (fvhd_llm_set_beam_scoring) - a chunk's logits are not normalised; switch it off around "
                     "fvhd_llm_extend");
    if (processors_on(c))
        return lfail("fvhd_llm_extend: logits processors are on (fvhd_llm_set_logits_processors) - their token history has no ids for an embedded "
                     "chunk; switch them off around fvhd_llm_extend");
    if (first_missing_tensor(c) >= 0) return lfail("fvhd_llm_extend: weights incomplete (fvhd_llm_finalize reports the missing tensor)");
    const bool gd = guidance_on(c);
    if (gd)
        if (int e = guidance_rows_error("fvhd_llm_extend", c->run_batch)) return e;
    const int B = c->run_batch, R = gd ? B / 2 : B;              // R: the rows the choice is made on (under guidance the G conditional ones)
    const bool con = constraint_on(c);
    if (con)
        if (int e = constraint_start_error(c, "fvhd_llm_extend", R)) return e;
    hipStream_t st = (hipStream_t)stream;
    float* logits = logits_out ? logits_out : c->dlogits;
    c->lp_logits = nullptr;
    // the prefill's decoder stack on the chunk rows; per layer the append + the attention over slots [0, length + T) (llm_prefill.hip)
    if (int e = decoder_stack(c, embeds, dtype, key_valid, position_ids, B, T, logits, nullptr, nullptr, st, true)) return e;
    LLM_ON_DEVICE(c);
    // the token: the launches of fvhd_llm_start (the sampler's n = the new length = length + T), then the state; all of them gated by
    // the error word the first append sets when length + T > capacity
    // (a new answer: the rows' start states again, and their bans on the chunk's last logits)
    ChoiceArgs ch;
    ch.who = "extend"; ch.reduce_what = "extend argmax (reduce)"; ch.logits = logits; ch.R = R; ch.gate = c->status; ch.n_add = T; ch.ids_out = next_ids_out;
    if (int e = choose_tokens(c, st, ch)) return e;
    LCHECK(fvhd_launch_llm_extend_state(st, c->posv, c->epos_used, B, T, c->len, c->status), "extend state");
    c->sp_begun = false;                                         // a lookup generation belongs to the sequence it was begun on
    c->ids_stale = false;
    c->lp_logits = logits;
    return 0;
}

int fvhd_llm_cache_rewind(fvhd_llm* c, const int32_t* keep_dev, fvhd_stream_t stream)
{
    if (!c || !keep_dev) return lfail("fvhd_llm_cache_rewind: NULL argument");
    if (!c->dc || !c->run_batch) return lfail("fvhd_llm_cache_rewind: no started sequence - call fvhd_llm_cache_reserve and fvhd_llm_start first");
    if (int e = dec_status_error(c, "fvhd_llm_cache_rewind")) return e;
    if (int e = row_state_refusal(c, "fvhd_llm_cache_rewind", "rewound")) return e;
    // rows g and G + g would need equal keeps; the keeps are on the device, and checking them there needs a synchronisation: refused
    if (int e = guidance_refusal(c, "fvhd_llm_cache_rewind", "rows g and G + g must keep equal lengths, which cannot be checked without a synchronisation"))
        return e;
    LLM_ON_DEVICE(c);
    LCHECK(fvhd_launch_llm_cache_rewind((hipStream_t)stream, keep_dev, c->run_batch, c->mask, c->posv, c->dc_cap, c->len, c->status, c->status_host_dev),
           "cache rewind");
    c->sp_begun = false;
    c->ids_stale = true;                                         // last_ids were chosen behind the slots that just left
    return 0;
}

int fvhd_llm_beam_reserve(fvhd_llm* c)
{
    if (!c || !c->dc) return lfail("fvhd_llm_beam_reserve: no KV cache - call fvhd_llm_cache_reserve first");
    LLM_ON_DEVICE(c);
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured (like fvhd_llm_cache_reserve)
    if (he != hipSuccess) return lhip("fvhd_llm_beam_reserve: hipDeviceSynchronize", he);
    if (c->beam) return 0;                                       // (fvhd_llm_cache_reserve frees it with the cache it was sized for)
    Arena a;
    const size_t o_gather = a.take(fvhd_dec_cache_gather_ws_bytes(c->dc_batch, c->nkv, c->hd, c->dc_cap)), o_topk = a.take(fvhd_dec_beam_topk_ws_bytes());
    if ((he = hipMalloc((void**)&c->beam, a.off)) != hipSuccess) { c->beam = nullptr; return lhip("hipMalloc(beam search scratch)", he); }
    c->beam_topk = c->beam + o_topk;
    (void)o_gather;
    return 0;
}

int fvhd_llm_cache_gather(fvhd_llm* c, const int64_t* src_rows, int rows_in, int rows_out, fvhd_stream_t stream)
{
    if (!c || !src_rows) return lfail("fvhd_llm_cache_gather: NULL argument");
    if (!c->dc || !c->run_batch) return lfail("fvhd_llm_cache_gather: no started sequence - call fvhd_llm_cache_reserve and fvhd_llm_start first");
    if (int e = guidance_refusal(c, "fvhd_llm_cache_gather", "a cache reorder would break the pairing of rows g and G + g")) return e;
    if (!c->beam) return lfail("fvhd_llm_cache_gather: no scratch - call fvhd_llm_beam_reserve first");
    if (rows_in < 1 || rows_in > c->dc_batch || rows_out < 1 || rows_out > c->dc_batch)
        return lfail("fvhd_llm_cache_gather: rows_in and rows_out must be in [1, the batch of fvhd_llm_cache_reserve]");
    if (int e = dec_status_error(c, "fvhd_llm_cache_gather")) return e;
    if (!c->beam_scoring)
        if (int e = row_state_refusal(c, "fvhd_llm_cache_gather", "reordered")) return e;
    LLM_ON_DEVICE(c);
    DecCacheGatherArgs a;
    a.kc = c->kcache; a.vc = c->vcache; a.layers = c->L; a.batch = c->dc_batch; a.mask = c->mask; a.posv = c->posv; a.src = src_rows;
    a.rows_in = rows_in; a.rows_out = rows_out; a.nkv = c->nkv; a.hd = c->hd; a.cap = c->dc_cap; a.len = c->len; a.status = c->status;
    a.status_host = c->status_host_dev; a.ws = c->beam;
    LCHECK(fvhd_launch_dec_cache_gather((hipStream_t)stream, &a), "cache reorder");
    if (c->beam_scoring && (processors_on(c) || constraint_on(c))) {
        // the rows' histories and automaton states follow their K and V (two launches; the same src, the same error word)
        DecHistGatherArgs h;
        if (processors_on(c)) { h.hist = c->hist; h.seen = c->hist_seen; h.count = c->hist_count; }
        if (constraint_on(c)) { h.states = c->con_state; h.flags = c->con_state + 64; }
        h.src = src_rows; h.rows_in = rows_in; h.rows_out = rows_out; h.batch = c->dc_batch; h.cap = c->dc_cap; h.V = c->V; h.status = c->status;
        h.status_host = c->status_host_dev; h.ws = c->beam_proc_hist;
        LCHECK(fvhd_launch_dec_hist_gather((hipStream_t)stream, &h), "history and state reorder");
    }
    c->run_batch = rows_out;
    c->sp_begun = false;                                         // a lookup generation belongs to the row it was begun on
    c->ids_stale = true;                                         // the reorder moves K, V, mask and positions, not last_ids
    return 0;
}

int fvhd_llm_beam_topk(fvhd_llm* c, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, float* cand_scores,
                       int64_t* cand_index, fvhd_stream_t stream)
{
    if (!c || !logits || !beam_scores || !cand_scores || !cand_index) return lfail("fvhd_llm_beam_topk: NULL argument");
    if (int e = guidance_refusal(c, "fvhd_llm_beam_topk", "beam search does not carry the pairing of conditional and unconditional rows")) return e;
    if (!c->beam) return lfail("fvhd_llm_beam_topk: no workspace - call fvhd_llm_beam_reserve first");
    if (constraint_on(c) && !c->beam_scoring)
        return lfail("fvhd_llm_beam_topk: a constraint is on (fvhd_llm_set_constraint) - beam search does not carry the rows' automaton states; "
                     "switch it off for beam search");
    if (!fvhd_dec_beam_topk_supported(groups, num_beams, keep, c->V) || ((uintptr_t)logits & 15))
        return lfail("fvhd_llm_beam_topk: needs groups >= 1, 2 <= num_beams <= 16, 1 <= keep <= 64, keep <= vocab, groups * num_beams <= 64, "
                     "vocab % 16 == 0, vocab <= 262144 and logits aligned to 16 bytes");
    LLM_ON_DEVICE(c);
    LCHECK(fvhd_launch_dec_beam_topk_mode((hipStream_t)stream, logits, beam_scores, groups, num_beams, keep, c->V, c->beam_scoring, cand_scores, cand_index,
                                          c->beam_topk), "beam top-K");
    return 0;
}

// ---- beam-search sampling (include/fvhd.h "LLM beam-search sampling"; kernels: llm_beam.hip on llm_sample.hip's threshold search) ----
int fvhd_llm_beam_sample_reserve(fvhd_llm* c)
{
    if (!c) return lfail("fvhd_llm_beam_sample_reserve: NULL context");
    LLM_ON_DEVICE(c);
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured (like fvhd_llm_beam_reserve)
    if (he != hipSuccess) return lhip("fvhd_llm_beam_sample_reserve: hipDeviceSynchronize", he);
    if (c->beam_sample) return 0;
    const size_t bytes = fvhd_dec_beam_sample_ws_bytes();
    if ((he = hipMalloc((void**)&c->beam_sample, bytes)) != hipSuccess) { c->beam_sample = nullptr; return lhip("hipMalloc(beam sampling workspace)", he); }
    if ((he = hipMemset(c->beam_sample, 0, bytes)) != hipSuccess) return lhip("hipMemset(beam sampling workspace)", he);      // counters start at zero
    return 0;
}

int fvhd_llm_beam_sample_topk(fvhd_llm* c, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, float temperature,
                              int top_k, float top_p, int min_keep, unsigned long long seed, float* cand_scores, int64_t* cand_index, fvhd_stream_t stream)
{
    if (!c || !logits || !beam_scores || !cand_scores || !cand_index) return lfail("fvhd_llm_beam_sample_topk: NULL argument");
    if (int e = guidance_refusal(c, "fvhd_llm_beam_sample_topk", "beam search does not carry the pairing of conditional and unconditional rows")) return e;
    if (!c->dc) return lfail("fvhd_llm_beam_sample_topk: no KV cache - call fvhd_llm_cache_reserve first (the draw's counter is the cache length)");
    if (!c->beam_sample) return lfail("fvhd_llm_beam_sample_topk: no workspace - call fvhd_llm_beam_sample_reserve first");
    if (constraint_on(c) && !c->beam_scoring)
        return lfail("fvhd_llm_beam_sample_topk: a constraint is on (fvhd_llm_set_constraint) - beam search does not carry the rows' automaton states; "
                     "switch it off for beam search");
    if (!fvhd_dec_beam_topk_supported(groups, num_beams, keep, c->V) || ((uintptr_t)logits & 15))
        return lfail("fvhd_llm_beam_sample_topk: needs groups >= 1, 2 <= num_beams <= 16, 1 <= keep <= 64, keep <= vocab, groups * num_beams <= 64, "
                     "vocab % 16 == 0, vocab <= 262144 and logits aligned to 16 bytes");
    if (const char* e = sampling_error(temperature, top_k, top_p)) return lfail(std::string("fvhd_llm_beam_sample_topk: ") + e);
    if (min_keep < 1 || min_keep > keep)
        return lfail("fvhd_llm_beam_sample_topk: min_keep must be in [1, keep] (got " + std::to_string(min_keep) + " with keep = " + std::to_string(keep) + ")");
    LLM_ON_DEVICE(c);
    DecBeamSampleArgs a;
    a.logits = logits; a.scores = beam_scores; a.G = groups; a.K = num_beams; a.keep = keep; a.V = c->V; a.temperature = temperature; a.top_k = top_k;
    a.top_p = top_p; a.min_keep = min_keep; a.seed = seed; a.len = c->len; a.out_v = cand_scores; a.out_i = cand_index;
    a.prenorm = c->beam_scoring;
    LCHECK(fvhd_launch_dec_beam_sample((hipStream_t)stream, &a, c->beam_sample), "beam sampling");
    return 0;
}

// ---- beam search with processors and a constraint (include/fvhd.h "LLM beam search with processors") ----
int fvhd_llm_set_beam_scoring(fvhd_llm* c, int on)
{
    if (!c) return lfail("fvhd_llm_set_beam_scoring: ctx is NULL");
    if (!on) { c->beam_scoring = 0; return 0; }                  // (the scratch stays until fvhd_llm_cache_reserve or fvhd_llm_destroy)
    if (!c->dc) return lfail("fvhd_llm_set_beam_scoring: no KV cache - call fvhd_llm_cache_reserve first (the reorder's scratch is sized for it)");
    if (!fvhd_dec_beam_norm_supported(c->dc_batch, c->V))
        return lfail("fvhd_llm_set_beam_scoring: the row normalisation needs vocab <= 262144");
    if (!c->beam_proc) {
        LLM_ON_DEVICE(c);
        hipError_t he = hipDeviceSynchronize();                  // refused while a stream is being captured (like fvhd_llm_beam_reserve)
        if (he != hipSuccess) return lhip("fvhd_llm_set_beam_scoring: hipDeviceSynchronize", he);
        Arena a;
        const size_t o_norm = a.take(fvhd_dec_beam_norm_ws_bytes()), o_hist = a.take(fvhd_dec_hist_gather_ws_bytes(c->dc_batch, c->dc_cap, c->V));
        if ((he = hipMalloc((void**)&c->beam_proc, a.off)) != hipSuccess) { c->beam_proc = nullptr; return lhip("hipMalloc(beam scoring scratch)", he); }
        c->beam_proc_norm = c->beam_proc + o_norm;
        c->beam_proc_hist = c->beam_proc + o_hist;
    }
    c->beam_scoring = 1;
    return 0;
}

// ---- speculative verification (include/fvhd.h "LLM speculative verification"; kernels: llm_spec.hip) ----
int fvhd_llm_spec_reserve(fvhd_llm* c, int max_rows, int lookup_capacity)
{
    if (!c || !c->dc) return lfail("fvhd_llm_spec_reserve: no KV cache - call fvhd_llm_cache_reserve first");
    if (max_rows < 2 || max_rows > 16 || lookup_capacity < 0)
        return lfail("fvhd_llm_spec_reserve: needs 2 <= max_rows <= 16 (the rows of one verify step) and lookup_capacity >= 0");
    if (c->hd != 64 && c->hd != 128) return lfail("fvhd_llm_spec_reserve: the verify step's attention needs head_dim 64 or 128");
    LLM_ON_DEVICE(c);
    if (c->spec && c->spec_rows >= max_rows && c->spec_seq_cap >= lookup_capacity + c->dc_cap + 16)                  // covered: kept as it is
        return c->verify_sampling || c->lp_on ? spec_extra_ensure(c, "fvhd_llm_spec_reserve", nullptr) : 0;
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured (like fvhd_llm_cache_reserve)
    if (he != hipSuccess) return lhip("fvhd_llm_spec_reserve: hipDeviceSynchronize", he);
    const int T = std::max(max_rows, c->spec ? c->spec_rows : 0), H = c->H, I = c->I, nh = c->nh, nkv = c->nkv, hd = c->hd;
    const int seq_cap = std::max(lookup_capacity + c->dc_cap + 16, c->spec ? c->spec_seq_cap : 0);
    if (c->spec) (void)hipFree(c->spec);
    c->spec = nullptr;
    c->spec_rows = 0;
    c->sp_begun = false;
    Arena a;
    const size_t o_h = a.take((size_t)T * H * 2), o_q = a.take((size_t)T * nh * hd * 2), o_att = a.take((size_t)T * nh * hd * 2),
                 o_act = a.take((size_t)T * I * 2), o_ks = a.take((size_t)T * nkv * hd * 2), o_vs = a.take((size_t)T * nkv * hd * 2),
                 o_pos = a.take(8 * T), o_draft = a.take(8 * 16), o_ids = a.take(8 * 16),
                 o_apart = a.take((size_t)T * nh * c->att_S * (hd + 2) * 4), o_cnt = a.take((size_t)nh * 4), o_zero = a.take(4), o_gate = a.take(4),
                 o_words = a.take(SPEC_WORDS * 4), o_seq = a.take((size_t)seq_cap * 4);
    if ((he = hipMalloc((void**)&c->spec, a.off)) != hipSuccess) { c->spec = nullptr; return lhip("hipMalloc(verify step scratch)", he); }
    if ((he = hipMemset(c->spec, 0, a.off)) != hipSuccess) return lhip("hipMemset(verify step scratch)", he);      // counters and the zero word
    char* d = c->spec;
    c->sp_h = d + o_h; c->sp_q = d + o_q; c->sp_att = d + o_att; c->sp_act = d + o_act; c->sp_ks = d + o_ks; c->sp_vs = d + o_vs;
    c->sp_pos = (int64_t*)(d + o_pos); c->sp_draft = (int64_t*)(d + o_draft); c->sp_ids = (int64_t*)(d + o_ids); c->sp_apart = (float*)(d + o_apart);
    c->sp_cnt = (int*)(d + o_cnt); c->sp_zero = (int*)(d + o_zero); c->sp_gate = (int*)(d + o_gate); c->sp_words = (int*)(d + o_words);
    c->sp_seq = (int*)(d + o_seq);
    c->spec_rows = T; c->spec_seq_cap = seq_cap;
    if (c->verify_sampling || c->lp_on) return spec_extra_ensure(c, "fvhd_llm_spec_reserve", nullptr);      // only then: a greedy user's footprint stays
    return 0;
}

namespace {

int spec_refusal(const fvhd_llm* c, const char* who, int rows)
{
    const std::string w(who);
    if (!c->dc || !c->run_batch) return lfail(w + ": no started sequence - call fvhd_llm_cache_reserve and fvhd_llm_start first");
    if (int e = guidance_refusal(c, who, "the verify step takes one sequence and does not combine a conditional row with an unconditional one")) return e;
    if (!c->spec) return lfail(w + ": no scratch - call fvhd_llm_spec_reserve first");
    if (c->run_batch != 1) return lfail(w + ": the verify step takes ONE sequence (the batch of fvhd_llm_start is " + std::to_string(c->run_batch) + ")");
    if (rows < 2 || rows > c->spec_rows)
        return lfail(w + ": rows must be in [2, the max_rows of fvhd_llm_spec_reserve = " + std::to_string(c->spec_rows) + "]");
    if (c->do_sample && !c->verify_sampling) return lfail(w + ": sampling is on (fvhd_llm_set_sampling) - the verify step is greedy only: it keeps the drafts the argmax confirms");
    if (processors_on(c))
        return lfail(w + ": logits processors are on (fvhd_llm_set_logits_processors) - the verify step does not maintain their token history");
    if (constraint_on(c))
        return lfail(w + ": a constraint is on (fvhd_llm_set_constraint) - the verify step does not advance the rows' automaton states");
    return 0;
}

// one verify step on the drafts at `draft` (device int64 [T - 1]): embed, the decode's launches at B = T, the ids of the T rows.
// Under sampling (the opt-in of fvhd_llm_set_verify_sampling; spec_refusal has passed) the rows' ids are the sampler's draws with the
// counters of the plain steps at their positions; lp_n >= 0: the log-probabilities of the T ids go to the step's scratch (spx_tok ..).
int spec_enqueue(fvhd_llm* c, const int64_t* draft, int T, float* logits_out, int64_t* ids, int* gate, hipStream_t st, int lp_n = -1)
{
    const bool samp = c->do_sample != 0;
    if ((samp && !logits_out) || lp_n >= 0) {
        if (int e = spec_extra_ensure(c, "the verify step", st)) return e;
        if (is_capturing(st)) c->spx_captured = true;
    }
    const char* w = c->wdev;
    const bool q8 = c->wfmt == FVHD_W_E4M3, q4 = c->wfmt == FVHD_W_MXFP4;
    const bool packed = !c->emb;                                 // a tied model: the token rows dequantised from the lm_head codes
    LCHECK(fvhd_launch_spec_embed(st, draft, c->last_ids, c->emb ? c->emb : w + c->lm_off, packed && q8 ? (const float*)(w + c->lm_soff) : nullptr,
                                  packed && q4 ? w + c->lm_soff : nullptr, c->V, c->H, c->sp_h, c->mask, T, c->dc_cap, c->len, c->posv, c->sp_pos, c->status, c->status_host_dev, gate), "verify embed");
    // the decode's launches at B = T: per-row positions, k / v into staging row t
    DecRows r;
    r.who = "verify"; r.lm_head_what = "verify final norm + lm_head + argmax";
    r.h = c->sp_h; r.q = c->sp_q; r.att = c->sp_att; r.act = c->sp_act; r.pos = c->sp_pos; r.rows = T; r.gate = gate; r.ks = c->sp_ks; r.vs = c->sp_vs;
    r.apart = c->sp_apart; r.acnt = c->sp_cnt;
    r.logits = logits_out ? logits_out : samp || lp_n >= 0 ? c->spx_logits : nullptr;      // the T fp32 rows the sampler / the logprobs launch read
    if (int e = decode_layers(c, st, r)) return e;
    if (samp) {
        // row t draws with the counter (0, length + 1 + t): the draw of the decode step that feeds the same token (sa.n_add = 1 there)
        DecSampleArgs sa = dec_sample_args(c, r.logits, T);
        sa.seq_rows = 1; sa.seq_row = 0; sa.len = c->len; sa.n_add = 1; sa.ids_out = ids; sa.status = gate;
        LCHECK(fvhd_launch_dec_sample(st, &sa, c->sws), "verify sampling");
    } else {
        LCHECK(fvhd_launch_dec_argmax_finish(st, c->amax_v, c->amax_i, (c->V / 16 + 3) / 4, T, nullptr, ids, nullptr, nullptr, gate), "verify argmax reduce");
    }
    if (lp_n >= 0)      // of the logits the choice was made from, before temperature / top-k / top-p, as in fvhd_llm_logprobs
        LCHECK(fvhd_launch_dec_logprobs(st, r.logits, ids, T, c->V, lp_n, c->spx_tok, c->spx_ids, c->spx_top, c->spx_lp_ws, gate), "verify logprobs");
    return 0;
}

void spec_accept_args(fvhd_llm* c, const int64_t* draft, int T, int* gate, SpecAcceptArgs& a)
{
    a.draft = draft; a.ids = c->sp_ids; a.T = T; a.last = c->last_ids; a.posv = c->posv; a.len = c->len; a.key_valid = c->mask; a.cap = c->dc_cap;
    a.gate = gate;
}

}  // namespace

int fvhd_llm_verify(fvhd_llm* c, const int64_t* draft_ids, int rows, float* logits_out, int64_t* ids_out, int32_t* emitted_out, fvhd_stream_t stream)
{
    if (!c || !draft_ids) return lfail("fvhd_llm_verify: NULL argument");
    if (int e = spec_refusal(c, "fvhd_llm_verify", rows)) return e;
    if (int e = stale_ids_error(c, "fvhd_llm_verify")) return e;
    if (int e = dec_status_error(c, "fvhd_llm_verify")) return e;
    if (int e = dec_embedding_error(c, "fvhd_llm_verify")) return e;
    LLM_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    c->lp_logits = nullptr;                                      // a verify step's rows are not "the logits of the last step"
    int64_t* ids = ids_out ? ids_out : c->sp_ids;                // the argmax reduce writes them, the accept reads them
    if (int e = spec_enqueue(c, draft_ids, rows, logits_out, ids, c->status, st)) return e;
    SpecAcceptArgs a;
    spec_accept_args(c, draft_ids, rows, c->status, a);
    a.ids = ids;
    a.emitted = emitted_out;
    LCHECK(fvhd_launch_spec_accept(st, &a), "verify accept");
    c->sp_begun = false;                                         // a bare verify step appends nothing to a lookup generation's token buffer
    return 0;
}

int fvhd_llm_lookup_begin(fvhd_llm* c, const int64_t* lookup_ids, int n_lookup, const int32_t* host_eos_ids, int n_eos, int max_new_tokens,
                          int64_t* tokens_out, fvhd_stream_t stream)
{
    if (!c || !tokens_out) return lfail("fvhd_llm_lookup_begin: NULL argument");
    if (int e = spec_refusal(c, "fvhd_llm_lookup_begin", 2)) return e;
    if (int e = stale_ids_error(c, "fvhd_llm_lookup_begin")) return e;
    if (n_lookup < 0 || (n_lookup && !lookup_ids) || n_lookup + c->dc_cap + 16 > c->spec_seq_cap)
        return lfail("fvhd_llm_lookup_begin: n_lookup must be in [0, the lookup_capacity of fvhd_llm_spec_reserve]");
    if (n_eos < 0 || n_eos > kMaxEos || (n_eos && !host_eos_ids)) return lfail("fvhd_llm_lookup_begin: at most " + std::to_string(kMaxEos) + " EOS ids");
    if (max_new_tokens < 1) return lfail("fvhd_llm_lookup_begin: max_new_tokens must be >= 1");
    LLM_ON_DEVICE(c);
    SpecEosList eos;
    eos.n = n_eos;
    for (int i = 0; i < n_eos; ++i) eos.ids[i] = host_eos_ids[i];
    LCHECK(fvhd_launch_spec_begin((hipStream_t)stream, lookup_ids, n_lookup, c->last_ids, c->sp_seq, tokens_out, c->sp_words, max_new_tokens, &eos),
           "lookup begin");
    c->sp_out = tokens_out; c->sp_out_cap = max_new_tokens; c->sp_begun = true;
    c->sp_lp_n = -1;                                             // no log-probability arrays yet: fvhd_llm_lookup_logprobs registers them
    return 0;
}

int fvhd_llm_set_verify_sampling(fvhd_llm* c, int on)
{
    if (!c) return lfail("fvhd_llm_set_verify_sampling: ctx is NULL");
    c->verify_sampling = on != 0;
    if (!on || !c->spec) return 0;                               // (without a scratch yet: fvhd_llm_spec_reserve makes the logits rows)
    LLM_ON_DEVICE(c);
    return spec_extra_ensure(c, "fvhd_llm_set_verify_sampling", nullptr);
}

int fvhd_llm_lookup_logprobs(fvhd_llm* c, int top_n, float* token_logprobs_out, int64_t* top_ids_out, float* top_logprobs_out, fvhd_stream_t stream)
{
    if (int e = logprobs_args_error(c, "fvhd_llm_lookup_logprobs", top_n, token_logprobs_out, top_ids_out, top_logprobs_out)) return e;
    if (!c->spec || !c->sp_begun) return lfail("fvhd_llm_lookup_logprobs: no lookup generation - call fvhd_llm_lookup_begin after fvhd_llm_start");
    if (!c->lp_on || !c->lp_ws || c->lp_logits != c->dlogits)
        return lfail("fvhd_llm_lookup_logprobs: the first token's logits are not in the context's buffer - switch fvhd_llm_set_logprobs on before "
                     "fvhd_llm_start and start without a logits_out");
    if (int e = dec_status_error(c, "fvhd_llm_lookup_logprobs")) return e;
    LLM_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    if (int e = spec_extra_ensure(c, "fvhd_llm_lookup_logprobs", st)) return e;
    // the first token's entry: the launch of fvhd_llm_logprobs on the logits fvhd_llm_start left, into entry 0 of the arrays
    LCHECK(fvhd_launch_dec_logprobs(st, c->dlogits, c->last_ids, 1, c->V, top_n, token_logprobs_out, top_ids_out, top_logprobs_out, c->lp_ws, c->status),
           "lookup first-token logprobs");
    c->sp_lp_n = top_n; c->sp_lp_tok = token_logprobs_out; c->sp_lp_ids = top_ids_out; c->sp_lp_top = top_logprobs_out;
    return 0;
}

int fvhd_llm_lookup_step(fvhd_llm* c, int rows, int max_ngram, fvhd_stream_t stream)
{
    if (!c) return lfail("fvhd_llm_lookup_step: ctx is NULL");
    if (int e = spec_refusal(c, "fvhd_llm_lookup_step", rows)) return e;
    if (int e = stale_ids_error(c, "fvhd_llm_lookup_step")) return e;
    if (!c->sp_begun) return lfail("fvhd_llm_lookup_step: no token buffer - call fvhd_llm_lookup_begin after fvhd_llm_start");
    if (max_ngram < 1 || max_ngram > 16) return lfail("fvhd_llm_lookup_step: max_ngram must be in [1, 16]");
    if (int e = dec_status_error(c, "fvhd_llm_lookup_step")) return e;
    if (int e = dec_embedding_error(c, "fvhd_llm_lookup_step")) return e;
    LLM_ON_DEVICE(c);
    hipStream_t st = (hipStream_t)stream;
    c->lp_logits = nullptr;
    LCHECK(fvhd_launch_spec_draft(st, c->sp_seq, c->sp_words + SPEC_W_SEQ_LEN, max_ngram, rows - 1, c->sp_draft, c->status, c->sp_words, c->sp_gate),
           "lookup draft");
    const int lp_n = c->lp_on ? c->sp_lp_n : -1;                 // >= 0: the generation keeps log-probabilities (fvhd_llm_lookup_logprobs)
    if (int e = spec_enqueue(c, c->sp_draft, rows, nullptr, c->sp_ids, c->sp_gate, st, lp_n)) return e;
    SpecAcceptArgs a;
    spec_accept_args(c, c->sp_draft, rows, c->sp_gate, a);
    a.words = c->sp_words; a.seq = c->sp_seq; a.seq_cap = c->spec_seq_cap; a.out = c->sp_out; a.out_cap = c->sp_out_cap;
    if (lp_n >= 0) a.emitted = c->spx_emitted;
    LCHECK(fvhd_launch_spec_accept(st, &a), "lookup accept");
    if (lp_n >= 0) {
        // the rows the accept emitted, to the generation's arrays at the offset of the step's first token: no host work, one graph
        SpecLogprobsArgs la;
        la.tok = c->spx_tok; la.ids = c->spx_ids; la.top = c->spx_top; la.n = lp_n; la.emitted = c->spx_emitted; la.words = c->sp_words;
        la.out_tok = c->sp_lp_tok; la.out_ids = c->sp_lp_ids; la.out_top = c->sp_lp_top; la.out_cap = c->sp_out_cap; la.gate = c->sp_gate;
        LCHECK(fvhd_launch_spec_logprobs_copy(st, &la), "lookup logprobs copy");
    }
    return 0;
}

int fvhd_llm_lookup_state(fvhd_llm* c, int* written, int* finished, int* steps, int* tokens)
{
    if (!c || !c->spec) return lfail("fvhd_llm_lookup_state: no scratch - call fvhd_llm_spec_reserve first");
    LLM_ON_DEVICE(c);
    int v[SPEC_WORDS] = {};
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(v, c->sp_words, sizeof(v), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return lhip("fvhd_llm_lookup_state", he);
    if (written) *written = v[SPEC_W_WRITTEN];
    if (finished) *finished = v[SPEC_W_FINISHED];
    if (steps) *steps = v[SPEC_W_STEPS];
    if (tokens) *tokens = v[SPEC_W_TOKENS];
    return 0;
}

int fvhd_llm_set_sampling(fvhd_llm* c, int do_sample, float temperature, int top_k, float top_p, unsigned long long seed)
{
    if (!c) return lfail("fvhd_llm_set_sampling: ctx is NULL");
    if (const char* e = sampling_error(temperature, top_k, top_p)) return lfail(std::string("fvhd_llm_set_sampling: ") + e);
    c->do_sample = do_sample != 0;
    c->temperature = temperature;
    c->top_k = top_k;
    c->top_p = top_p;
    c->seed = seed;
    return 0;
}

int fvhd_llm_set_sampling_warpers(fvhd_llm* c, float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff)
{
    if (!c) return lfail("fvhd_llm_set_sampling_warpers: ctx is NULL");
    const std::string err = warpers_error(min_p, typical_p, epsilon_cutoff, eta_cutoff);
    if (!err.empty()) return lfail("fvhd_llm_set_sampling_warpers: " + err);
    c->min_p = min_p;
    c->typical_p = typical_p;
    c->epsilon_cutoff = epsilon_cutoff;
    c->eta_cutoff = eta_cutoff;
    return 0;
}

int fvhd_llm_set_logits_processors(fvhd_llm* c, float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens, const int32_t* eos_ids, int n_eos,
                                   const int32_t* suppress_ids, int n_suppress)
{
    if (!c) return lfail("fvhd_llm_set_logits_processors: ctx is NULL");
    const std::string err = processors_error(repetition_penalty, no_repeat_ngram_size, min_new_tokens, eos_ids, n_eos, suppress_ids, n_suppress, c->V);
    if (!err.empty()) return lfail("fvhd_llm_set_logits_processors: " + err);
    LLM_ON_DEVICE(c);
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured; no enqueued step still reads the lists
    if (he != hipSuccess) return lhip("fvhd_llm_set_logits_processors: hipDeviceSynchronize", he);
    std::vector<int32_t> lists(kMaxEos + kMaxSuppress, 0);
    std::copy(eos_ids, eos_ids + n_eos, lists.begin());
    std::copy(suppress_ids, suppress_ids + n_suppress, lists.begin() + kMaxEos);
    if ((n_eos || n_suppress) && !(c->proc_lists && lists == c->proc_lists_host)) {      // (the same lists again: nothing to upload)
        if (c->proc_lists && c->proc_lists_captured) {           // a captured step replays on the old lists
            c->retired.push_back((char*)c->proc_lists);
            c->proc_lists = nullptr;
        }
        c->proc_lists_captured = false;
        if (!c->proc_lists && (he = hipMalloc((void**)&c->proc_lists, lists.size() * 4)) != hipSuccess) {
            c->proc_lists = nullptr;
            return lhip("hipMalloc(logits processor lists)", he);
        }
        c->proc_lists_host.clear();
        if ((he = hipMemcpy(c->proc_lists, lists.data(), lists.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return lhip("hipMemcpy(id lists)", he);
        if ((he = hipDeviceSynchronize()) != hipSuccess) return lhip("fvhd_llm_set_logits_processors: hipDeviceSynchronize", he);
        c->proc_lists_host = lists;
    }
    c->proc_penalty = repetition_penalty;
    c->proc_ngram = no_repeat_ngram_size;
    c->proc_min_new = min_new_tokens;
    c->proc_n_eos = n_eos;
    c->proc_n_sup = n_suppress;
    return 0;
}

// ---- log-probabilities of the chosen tokens (include/fvhd.h "LLM log-probabilities"; kernel: llm_logprobs.hip) ----
int fvhd_llm_set_logprobs(fvhd_llm* c, int on)
{
    if (!c) return lfail("fvhd_llm_set_logprobs: ctx is NULL");
    if (!c->dc) return lfail("fvhd_llm_set_logprobs: no KV cache - call fvhd_llm_cache_reserve first (the scratch is sized for its batch)");
    LLM_ON_DEVICE(c);
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured (like fvhd_llm_cache_reserve)
    if (he != hipSuccess) return lhip("fvhd_llm_set_logprobs: hipDeviceSynchronize", he);
    if (on && !c->lp_ws) {
        const size_t bytes = fvhd_dec_logprobs_scratch_bytes(c->dc_batch, c->V, 16);
        if ((he = hipMalloc((void**)&c->lp_ws, bytes)) != hipSuccess) { c->lp_ws = nullptr; return lhip("hipMalloc(logprobs scratch)", he); }
        if ((he = hipMemset(c->lp_ws, 0, bytes)) != hipSuccess) return lhip("hipMemset(logprobs scratch)", he);      // counters start at zero
    }
    c->lp_on = on != 0;
    return 0;
}

int fvhd_llm_logprobs(fvhd_llm* c, const float* logits, int top_n, float* token_logprob_out, int64_t* top_ids_out, float* top_logprobs_out,
                      fvhd_stream_t stream)
{
    if (int e = logprobs_args_error(c, "fvhd_llm_logprobs", top_n, token_logprob_out, top_ids_out, top_logprobs_out)) return e;
    if (!c->dc || !c->run_batch) return lfail("fvhd_llm_logprobs: no started sequence - call fvhd_llm_cache_reserve and fvhd_llm_start first");
    if (int e = dec_status_error(c, "fvhd_llm_logprobs")) return e;
    if (int e = stale_ids_error(c, "fvhd_llm_logprobs")) return e;
    if (!logits) {
        if (!c->lp_on)
            return lfail("fvhd_llm_logprobs: logits is NULL and keeping the logits is off - switch it on before the step (fvhd_llm_set_logprobs), or pass "
                         "the logits_out buffer of the step");
        if (c->lp_logits != c->dlogits)
            return lfail("fvhd_llm_logprobs: logits is NULL but the last fvhd_llm_start / _decode / _extend did not leave its logits in the context's "
                         "buffer (none ran since the setting was switched on, or it wrote a logits_out) - pass that buffer");
        logits = c->dlogits;
    }
    if (!c->lp_ws) return lfail("fvhd_llm_logprobs: no scratch - fvhd_llm_set_logprobs(ctx, 1) reserves it (it may be switched off again)");
    LLM_ON_DEVICE(c);
    // (behind a step under guidance: the G conditional rows, whose logits are the guided scores)
    LCHECK(fvhd_launch_dec_logprobs((hipStream_t)stream, logits, c->last_ids, c->guid_rows ? c->guid_rows : c->run_batch, c->V, top_n, token_logprob_out,
                                    top_ids_out, top_logprobs_out, c->lp_ws, c->status), "logprobs");
    return 0;
}

// ---- classifier-free guidance (include/fvhd.h "LLM classifier-free guidance"; kernels: llm_guidance.hip) ----
int fvhd_llm_set_guidance(fvhd_llm* c, float scale)
{
    if (!c) return lfail("fvhd_llm_set_guidance: ctx is NULL");
    if (!std::isfinite(scale)) return lfail("fvhd_llm_set_guidance: scale must be finite (1 = off)");
    if (scale != 1.f && !c->guid_ws) {
        if (c->V < 1) return lfail("fvhd_llm_set_guidance: the context has no vocabulary yet");
        LLM_ON_DEVICE(c);
        hipError_t he = hipDeviceSynchronize();                  // refused while a stream is being captured (like fvhd_llm_set_logprobs)
        if (he != hipSuccess) return lhip("fvhd_llm_set_guidance: hipDeviceSynchronize", he);
        const size_t bytes = fvhd_dec_guidance_scratch_bytes(32, c->V);
        if ((he = hipMalloc((void**)&c->guid_ws, bytes)) != hipSuccess) { c->guid_ws = nullptr; return lhip("hipMalloc(guidance scratch)", he); }
        if ((he = hipMemset(c->guid_ws, 0, bytes)) != hipSuccess) return lhip("hipMemset(guidance scratch)", he);      // counters start at zero
    }
    c->guid_scale = scale;
    return 0;
}

// ---- constrained decoding (include/fvhd.h "LLM constrained decoding"; kernels: llm_constrain.hip) ----
int fvhd_llm_set_constraint(fvhd_llm* c, const int32_t* off, int n_states, const int32_t* tok, const int32_t* tgt, int n_edges, const int32_t* start,
                            int n_start)
{
    const std::string w = "fvhd_llm_set_constraint: ";
    if (!c) return lfail(w + "ctx is NULL");
    if (n_states < 0) return lfail(w + "n_states must be >= 0 (0 = off)");
    if (n_states > 0) {
        if (!off || !tok || !tgt || !start) return lfail(w + "NULL table");
        if (n_states > kMaxConStates) return lfail(w + std::to_string(n_states) + " states exceed the limit of " + std::to_string(kMaxConStates) + " states");
        if (n_edges < 1 || n_edges > kMaxConEdges)
            return lfail(w + "n_edges = " + std::to_string(n_edges) + " must be in [1, the limit of " + std::to_string(kMaxConEdges) + " edges]");
        if (n_start != 1 && (n_start != c->dc_batch || !c->dc))
            return lfail(w + "n_start = " + std::to_string(n_start) + " must be 1 (every row) or the batch of fvhd_llm_cache_reserve (" +
                         std::to_string(c->dc_batch) + ")");
        if (off[0] != 0) return lfail(w + "offsets must start at 0 (offsets[0] = " + std::to_string(off[0]) + ")");
        if (off[n_states] != n_edges)
            return lfail(w + "offsets[n_states] = " + std::to_string(off[n_states]) + " is not n_edges = " + std::to_string(n_edges));
        for (int s = 0; s < n_states; ++s) {
            const int e0 = off[s], e1 = off[s + 1];
            if (e1 < e0 || e1 > n_edges) return lfail(w + "offsets are not monotone at state " + std::to_string(s));
            if (e1 == e0) return lfail(w + "state " + std::to_string(s) + " has no edge - an unsatisfiable state");
            for (int e = e0; e < e1; ++e) {
                if (tok[e] < 0 || tok[e] >= c->V)
                    return lfail(w + "token " + std::to_string(tok[e]) + " of edge " + std::to_string(e) + " (state " + std::to_string(s) +
                                 ") is outside [0, vocab = " + std::to_string(c->V) + ")");
                if (tgt[e] < -1 || tgt[e] >= n_states)
                    return lfail(w + "target " + std::to_string(tgt[e]) + " of edge " + std::to_string(e) + " (state " + std::to_string(s) +
                                 ") is outside [-1, n_states = " + std::to_string(n_states) + ")");
                if (e > e0 && tok[e] <= tok[e - 1])
                    return lfail(w + "the tokens of state " + std::to_string(s) + " are not strictly ascending at edge " + std::to_string(e));
            }
        }
        for (int i = 0; i < n_start; ++i)
            if (start[i] < -1 || start[i] >= n_states)
                return lfail(w + "start state " + std::to_string(start[i]) + " of row " + std::to_string(i) + " is outside [-1, n_states = " +
                             std::to_string(n_states) + ")");
    }
    LLM_ON_DEVICE(c);
    hipError_t he = hipDeviceSynchronize();                      // refused while a stream is being captured; no enqueued step still reads the tables
    if (he != hipSuccess) return lhip("fvhd_llm_set_constraint: hipDeviceSynchronize", he);
    if (n_states == 0) {                                         // off: the tables stay (a captured step may replay on them; the same ones may return)
        c->con_n_states = c->con_n_edges = c->con_n_start = 0;
        return 0;
    }
    if (!c->con_state) {
        if ((he = hipMalloc((void**)&c->con_state, 2 * 64 * 4)) != hipSuccess) { c->con_state = nullptr; return lhip("hipMalloc(constraint states)", he); }
        if ((he = hipMemset(c->con_state, 0xff, 64 * 4)) == hipSuccess) he = hipMemset(c->con_state + 64, 0, 64 * 4);      // FREE, no flags
        if (he != hipSuccess) return lhip("hipMemset(constraint states)", he);
    }
    const size_t words = (size_t)n_states + 1 + 2 * (size_t)n_edges;
    const bool same = c->con_tab && c->con_tab_states == n_states && c->con_tab_edges == n_edges && c->con_host.size() == words &&
                      std::equal(off, off + n_states + 1, c->con_host.begin()) && std::equal(tok, tok + n_edges, c->con_host.begin() + n_states + 1) &&
                      std::equal(tgt, tgt + n_edges, c->con_host.begin() + n_states + 1 + n_edges);
    if (!same) {                                                 // (the same tables again: nothing to upload)
        if (c->con_tab) {
            if (c->con_captured) c->retired.push_back((char*)c->con_tab);      // a captured step replays on the old tables
            else (void)hipFree(c->con_tab);
            c->con_tab = nullptr;
        }
        c->con_captured = false;
        c->con_host.clear();
        c->con_tab_states = c->con_tab_edges = 0;
        c->con_n_states = c->con_n_edges = c->con_n_start = 0;
        if ((he = hipMalloc((void**)&c->con_tab, words * 4)) != hipSuccess) { c->con_tab = nullptr; return lhip("hipMalloc(constraint tables)", he); }
        he = hipMemcpy(c->con_tab, off, ((size_t)n_states + 1) * 4, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(c->con_tab + n_states + 1, tok, (size_t)n_edges * 4, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(c->con_tab + n_states + 1 + n_edges, tgt, (size_t)n_edges * 4, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipDeviceSynchronize();
        if (he != hipSuccess) return lhip("hipMemcpy(constraint tables)", he);
        c->con_host.reserve(words);
        c->con_host.insert(c->con_host.end(), off, off + n_states + 1);
        c->con_host.insert(c->con_host.end(), tok, tok + n_edges);
        c->con_host.insert(c->con_host.end(), tgt, tgt + n_edges);
        c->con_tab_states = n_states;
        c->con_tab_edges = n_edges;
    }
    c->con_n_states = n_states;
    c->con_n_edges = n_edges;
    c->con_n_start = n_start;
    std::fill(c->con_start, c->con_start + 64, -1);
    std::copy(start, start + n_start, c->con_start);
    return 0;
}

int fvhd_llm_constraint_state(fvhd_llm* c, int32_t* states_out, int32_t* flags_out, int rows)
{
    if (!c) return lfail("fvhd_llm_constraint_state: ctx is NULL");
    if (!constraint_on(c)) return lfail("fvhd_llm_constraint_state: no constraint is on (fvhd_llm_set_constraint)");
    if (!c->con_started || !c->run_batch)
        return lfail("fvhd_llm_constraint_state: no sequence was started under the constraint - fvhd_llm_start / fvhd_llm_extend give the rows their states");
    if (rows < 1 || rows > c->run_batch)
        return lfail("fvhd_llm_constraint_state: rows must be in [1, the started batch = " + std::to_string(c->run_batch) + "]");
    LLM_ON_DEVICE(c);
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess && states_out) he = hipMemcpy(states_out, c->con_state, (size_t)rows * 4, hipMemcpyDeviceToHost);
    if (he == hipSuccess && flags_out) he = hipMemcpy(flags_out, c->con_state + 64, (size_t)rows * 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return lhip("fvhd_llm_constraint_state", he);
    return 0;
}

int fvhd_llm_cache_state(fvhd_llm* c, int* length, int* status)
{
    if (!c || !c->dc) return lfail("fvhd_llm_cache_state: no KV cache");
    LLM_ON_DEVICE(c);
    int v[2] = {0, 0};
    hipError_t he = hipDeviceSynchronize();
    if (he == hipSuccess) he = hipMemcpy(&v[0], c->len, 4, hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(&v[1], c->status, 4, hipMemcpyDeviceToHost);
    if (he != hipSuccess) return lhip("fvhd_llm_cache_state", he);
    if (length) *length = v[0];
    if (status) *status = v[1];
    return 0;
}

}  // extern "C"
