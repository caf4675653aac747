// Private header of the Qwen2 C-ABI sources (llm_weights.hip, llm_prefill.hip, llm_step.hip, llm_ops.hip): the context, the descriptor of
// a packed matrix, error reporting and the few helpers one file defines and another calls.
#pragma once
#include <string>
#include <vector>

#include "api_host.h"
#include "launchers.h"

#pragma GCC visibility push(hidden)      // the helpers shared between the four sources are not exported symbols

constexpr int kMaxSplits = 4;
constexpr int kMaxEos = 16, kMaxSuppress = 256;     // list limits of the logits processors (include/fvhd.h)
constexpr int kMaxConStates = 1 << 24, kMaxConEdges = 1 << 28;      // table limits of fvhd_llm_set_constraint (include/fvhd.h)

struct LayerOff { size_t ln1, bqkv, ln2, w[4], s[4]; };     // w, s: by FVHD_MAT_QKV .. FVHD_MAT_DOWN; s: the fp32 row scales of an e4m3 matrix,
                                                            // the block scale bytes of an MXFP4 one

struct __attribute__((visibility("default"))) fvhd_llm {     // (its inline constructor and destructor have always been weak exported symbols)
    int device = 0, H = 0, L = 0, nh = 0, nkv = 0, hd = 0, I = 0, V = 0;
    float eps = 1e-6f, theta = 1e6f;
    int qkvw = 0;
    char* wdev = nullptr;
    size_t wbytes = 0;
    std::vector<LayerOff> lo;
    size_t norm_off = 0, lm_off = 0, lm_soff = 0;
    int wfmt = FVHD_W_BF16;                // fvhd_llm_set_weight_format: FVHD_W_E4M3 = every matrix as e4m3 codes (1 byte, the K order of llm_w8.hip) + one
                                           // fp32 scale per row; vectors and model.embed_tokens.weight are not affected
                                           // FVHD_W_MXFP4 = every matrix as e2m1 codes (two per byte, the K order of w4_layout.h) + one e8m0 scale
                                           // byte per 32 elements of a row
    bool any_set = false;                  // a tensor was set: the format is fixed
    char* wscratch = nullptr;              // e4m3 / MXFP4: bf16 scratch of the largest matrix - the prefill dequantises each matrix into it right before its GEMM
    size_t wscratch_bytes = 0;
    std::vector<char> got;                 // per expected tensor: received?
    std::vector<std::string> names;
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    int ws_rows = 0, ws_batch = 0, ws_pos = 0;
    char *h = nullptr, *xn = nullptr, *qkv = nullptr, *att = nullptr, *act = nullptr, *last = nullptr, *lastn = nullptr;
    float *rope = nullptr, *part = nullptr;
    int64_t* epos = nullptr;               // inside `ws`: the positions [batch][T] of a chunk that fvhd_llm_extend was given without position ids
    const int64_t* epos_used = nullptr;    // the positions the last decoder_stack() call used: the caller's, or `epos`
    int fuse_rope = 0;                     // FVHD_LLM_FUSEROPE=1: rotary embedding + KV-cache copies inside the q|k|v projection's epilogue instead of their own launch (identical bits; measured neutral - prefill 3.421 / 3.410 -> 3.404 / 3.407 ms at B = 8, 2.316 -> 2.342 at B = 1, profiles/r05_ttft_fuserope_ab.log: the 5.4-us launch saved comes back as epilogue time - so off by default)
    int down_splits = kMaxSplits, o_splits = 2, qkv_splits = 0, fuse_norm = 1;     // FVHD_LLM_SPLITK / FVHD_LLM_OSPLIT (largest split of down_proj / o_proj, 0 = never) / FVHD_LLM_QKVSPLIT / FVHD_LLM_FUSENORM
    int max_pos = 0;                       // fvhd_llm_set_max_positions (config.max_position_embeddings): rows of the rotary table
    // A prefill that ran while its stream was being captured put this workspace's pointers into the CALLER's graph.  Such a workspace is
    // never freed when a later call needs a bigger one: it is retired (kept until fvhd_llm_destroy), so the captured graph keeps
    // replaying on valid memory.  `generation` counts workspace replacements (fvhd_llm_workspace_generation).
    bool ws_captured = false;
    std::vector<char*> retired;
    int generation = 0;
    // fvhd_llm_set_tensor_device enqueues its copies on the CALLER's stream: `load_ev` is recorded behind the latest one so that
    // fvhd_llm_finalize (host wait) and fvhd_llm_prefill (stream wait, whatever stream it runs on) are ordered after the packing
    hipEvent_t load_ev = nullptr;
    hipStream_t load_stream = nullptr;
    bool load_pending = false;
    // ---- decode (fvhd_llm_cache_reserve / start / decode) ----
    char* emb = nullptr;                   // model.embed_tokens.weight, bf16 [V][H]: optional, the decode's input table of an untied model
    int tied = -1;                         // fvhd_llm_set_tied_embeddings: 1 = the decode embeds through the packed lm_head rows, 0 = through
                                           // `emb`; -1 = not said - the decode then needs `emb` (it never guesses the lm_head rows)
    char* dc = nullptr;                    // one allocation: caches, mask, device words, decode workspace, rotary table
    size_t dc_bytes = 0;
    int dc_batch = 0, dc_cap = 0, dc_pos = 0;
    int run_batch = 0;                     // batch of the last fvhd_llm_start (the decode steps run on it)
    char *kcache = nullptr, *vcache = nullptr, *dh = nullptr, *dq = nullptr, *datt = nullptr, *dact = nullptr;
    unsigned char* mask = nullptr;
    int64_t *posv = nullptr, *last_ids = nullptr;
    int *len = nullptr, *status = nullptr, *cnt = nullptr, *amax_i = nullptr;
    float *dpart = nullptr, *apart = nullptr, *amax_v = nullptr, *dlogits = nullptr, *drope = nullptr, *drstd = nullptr;
    int dec_rstd_once = 1;                 // a decode GEMM with a folded norm above 16 rows: the row statistics from one small launch (dec_rstd_kernel)
                                           // instead of every workgroup; FVHD_DEC_RSTD_ONCE=0 for the A/B (identical bits)
    int* status_host = nullptr;            // host-mapped copy of the error word: read by every host call without a synchronisation
    int* status_host_dev = nullptr;
    int cnt_att = 0;                       // counters [0, cnt_att) of the GEMMs, then B * nh of the attention
    struct Plan { int S = 1, cpw = 1; } plan[5];      // K split of the decode GEMM of every matrix, by FVHD_MAT_*
    int att_S = 1, att_chunk = 0;
    char* pre_kv = nullptr;                // the prefill's own [n_layers][batch][nkv][seq_len][hd] caches, copied into the strided ones
    size_t pre_kv_bytes = 0;
    // fvhd_llm_set_sampling: read when fvhd_llm_start / fvhd_llm_decode enqueue (a captured graph keeps what it was captured with)
    int do_sample = 0;
    float temperature = 1.f, top_p = 1.f;
    int top_k = 0;
    unsigned long long seed = 0;
    float min_p = 0.f, typical_p = 1.f, epsilon_cutoff = 0.f, eta_cutoff = 0.f;      // fvhd_llm_set_sampling_warpers: read like the sampling settings
    char* sws = nullptr;                   // the sampler's workspace (inside `dc`)
    // fvhd_llm_beam_reserve: one allocation of its own (fvhd_llm_cache_reserve's footprint is what it was), sized for the reserved cache
    char* beam = nullptr;                  // the reorder's scratch (llm_beam.hip: two layers' K | V, the mask, the positions), then the top-K workspace
    char* beam_topk = nullptr;
    char* beam_sample = nullptr;           // fvhd_llm_beam_sample_reserve: the workspace of beam-search sampling, an allocation of its own (no cache size in it)
    // fvhd_llm_set_beam_scoring: with it on, fvhd_llm_start / _decode with a logits_out turn the rows into log-probabilities in front of the
    // processors and the constraint, fvhd_llm_cache_gather carries the rows' histories and automaton states, and the two top-K calls take the
    // rows as they are.  Read when a call enqueues, like the sampling settings.  beam_proc: the normalisation's partials, then the scratch of
    // the history / state reorder - an allocation of its own, made by the call that switches the mode on and sized for the reserved cache
    // (fvhd_llm_cache_reserve frees it and switches the mode off)
    int beam_scoring = 0;
    char* beam_proc = nullptr;
    char* beam_proc_norm = nullptr;        // inside beam_proc: the normalisation's partials ...
    char* beam_proc_hist = nullptr;        // ... and the reorder's scratch
    // fvhd_llm_set_logits_processors (llm_logits.hip): read when fvhd_llm_start / fvhd_llm_decode enqueue, like the sampling settings
    float proc_penalty = 1.f;
    int proc_ngram = 0, proc_min_new = 0, proc_n_eos = 0, proc_n_sup = 0;
    int* proc_lists = nullptr;             // device: EOS ids [16] | suppressed ids [256]; an allocation of its own.  One that a captured step
    bool proc_lists_captured = false;      // has recorded is retired (kept until fvhd_llm_destroy) when OTHER lists are set, not overwritten
    std::vector<int32_t> proc_lists_host;  // what proc_lists holds (setting the same lists again uploads and retires nothing)
    int* hist = nullptr;                   // inside `dc`: per-row token history [dc_batch][dc_cap], the bitmap of its tokens
    unsigned* hist_seen = nullptr;         // [dc_batch][ceil(V / 32)] and per row the number of tokens in its history [dc_batch]: zeroed by a
    int* hist_count = nullptr;             // fvhd_llm_start with processors on (its rows), advanced by every step enqueued with them on
    bool hist_started = false;             // that start has happened: a decode step with processors on has a history to append to
    // fvhd_llm_spec_reserve (llm_spec.hip): one allocation of its own, sized for the reserved cache - the T-row activations, the k / v
    // staging rows [T][nkv][hd], the per-row positions, the attention partials [T][nh][att_S][hd + 2] and counters [nh], the drafts and
    // ids of a step, the token buffer and the device words of a lookup generation (llm_decode.h SPEC_W_*)
    char* spec = nullptr;
    int spec_rows = 0, spec_seq_cap = 0;
    char *sp_h = nullptr, *sp_q = nullptr, *sp_att = nullptr, *sp_act = nullptr, *sp_ks = nullptr, *sp_vs = nullptr;
    int64_t *sp_pos = nullptr, *sp_draft = nullptr, *sp_ids = nullptr;
    float* sp_apart = nullptr;
    int *sp_cnt = nullptr, *sp_zero = nullptr, *sp_gate = nullptr, *sp_words = nullptr, *sp_seq = nullptr;
    int64_t* sp_out = nullptr;             // fvhd_llm_lookup_begin: the caller's output tokens [sp_out_cap]
    int sp_out_cap = 0;
    bool sp_begun = false;
    // fvhd_llm_set_verify_sampling: with it on, verify and lookup steps follow the sampling settings (row t draws with the counter of the
    // plain step at its position) instead of being refused under them.  `spx`: what such a step, or one that keeps log-probabilities,
    // needs beyond `spec` - the fp32 logits [spec_rows][V], the logprobs launch's scratch and outputs for spec_rows rows, the accept's
    // emitted count - in an allocation of its own, made only when either is asked for (a greedy user's footprint is what it was); one
    // that a capturing stream used is retired when it must grow, like the workspace
    int verify_sampling = 0;
    char* spx = nullptr;
    int spx_rows = 0;
    bool spx_captured = false;
    float *spx_logits = nullptr, *spx_tok = nullptr, *spx_top = nullptr;
    int64_t* spx_ids = nullptr;
    char* spx_lp_ws = nullptr;
    int* spx_emitted = nullptr;
    // fvhd_llm_lookup_logprobs: the output arrays of the lookup generation (sp_lp_n < 0: none registered; fvhd_llm_lookup_begin resets it)
    int sp_lp_n = -1;
    float *sp_lp_tok = nullptr, *sp_lp_top = nullptr;
    int64_t* sp_lp_ids = nullptr;
    // fvhd_llm_cache_rewind / fvhd_llm_cache_gather set it: last_ids (the ids "the previous step chose") then belong to the rows as they were
    // before the call.  Cleared by fvhd_llm_start, fvhd_llm_extend and fvhd_llm_decode with explicit token_ids; while it is set every call
    // that would feed last_ids is refused when it enqueues (a captured step replays as captured)
    bool ids_stale = false;
    // fvhd_llm_score (llm_prefill.hip): what the last decoder_stack() call left in `h` - its (batch, T) and the workspace generation it ran
    // on (a workspace replaced since holds no rows) - and the score launch's scratch: an allocation of its own that grows on demand
    // (fvhd_llm_score_reserve); one that a capturing stream used is retired when it must grow, like the workspace
    int last_batch = 0, last_T = 0, last_gen = -1;
    char* score_ws = nullptr;
    size_t score_bytes = 0;
    bool score_captured = false;
    // fvhd_llm_set_logprobs (llm_logprobs.hip): with it on, a greedy step without a logits_out keeps its logits in `dlogits`.  lp_ws: the
    // launch's scratch for (dc_batch, V, 16), an allocation of its own that fvhd_llm_cache_reserve frees with the cache it was sized for;
    // lp_logits: where the last fvhd_llm_start / _decode / _extend left its logits (NULL: nowhere yet)
    int lp_on = 0;
    char* lp_ws = nullptr;
    const float* lp_logits = nullptr;
    // fvhd_llm_set_constraint (llm_constrain.hip): con_n_states > 0 = on.  con_tab: one allocation of its own, offsets [n_states + 1] |
    // tokens [n_edges] | targets [n_edges]; tables that a captured step has recorded are retired (kept until fvhd_llm_destroy) when OTHER
    // tables are set, never overwritten (the proc_lists rule); switching off keeps them, and setting the same tables again uploads nothing.
    // con_state: the rows' states [64] | flags [64], allocated by the first set and kept until destroy.  The start states travel by value
    // in the launch arguments of fvhd_llm_start / _extend.
    int con_n_states = 0, con_n_edges = 0, con_n_start = 0;
    int con_tab_states = 0, con_tab_edges = 0;       // the shape of the tables in con_tab (they stay while the constraint is off)
    int* con_tab = nullptr;
    bool con_captured = false;
    std::vector<int32_t> con_host;         // what con_tab holds
    int* con_state = nullptr;
    int con_start[64] = {};
    bool con_started = false;              // the last fvhd_llm_start / _extend ran with the constraint on: a decode step has states to advance
    // fvhd_llm_set_guidance (llm_guidance.hip): guid_scale != 1 = on, read when fvhd_llm_start / _decode / _extend enqueue, like the sampling
    // settings.  guid_ws: the launches' scratch for 32 pairs of this vocabulary, an allocation of its own made by the first call that
    // switches guidance on and kept until fvhd_llm_destroy.  guid_rows: the conditional rows G of the last start / decode / extend when it
    // ran under guidance (fvhd_llm_logprobs then takes the G conditional rows), else 0
    float guid_scale = 1.f;
    char* guid_ws = nullptr;
    int guid_rows = 0;
};

inline bool constraint_on(const fvhd_llm* c) { return c->con_n_states > 0; }
inline bool guidance_on(const fvhd_llm* c) { return c->guid_scale != 1.f; }

inline bool processors_on(const fvhd_llm* c)
{
    return c->proc_penalty != 1.f || c->proc_ngram > 0 || (c->proc_min_new > 0 && c->proc_n_eos > 0) || c->proc_n_sup > 0;
}

inline int lfail(const std::string& m) { return fvhd_set_error(m.c_str()); }
inline int lhip(const char* what, hipError_t e) { return lfail(std::string(what) + ": " + hipGetErrorString(e)); }
inline int lret(const char* what, int e) { return e ? lhip(what, (hipError_t)e) : 0; }      // e: what a launcher returned

#define LCHECK(expr, what) do { if (int _e = (expr)) return lhip(what, (hipError_t)_e); } while (0)
// the CONTEXT's device is current for the rest of the function; two statements and a local `_guard`, like FVHD_ON_DEVICE: top level of a function body only
#define LLM_ON_DEVICE(c) DeviceGuard _guard((c)->device); if (_guard.err != hipSuccess) return lhip("hipSetDevice", _guard.err)

inline int cu_count(const fvhd_llm* c)      // compute units of the context's device (256 if the query fails)
{
    int n = 0;
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && n > 0 ? n : 256;
}

// one packed matrix: [N][K] elements (bf16, e4m3 codes or MXFP4 codes) at wdev + off; its scales at wdev + soff: e4m3 N fp32 row scales,
// MXFP4 u8 [N][K / 32]
struct Mat { size_t off, soff; long N; int K; };
Mat mat_of(const fvhd_llm* c, int layer, int matrix);             // llm_weights.hip; matrix: FVHD_MAT_* (layer is ignored for FVHD_MAT_LM_HEAD)

int first_missing_tensor(const fvhd_llm* c);                      // llm_weights.hip: index into c->got, -1 when every tensor has arrived
int wait_for_loads(fvhd_llm* c);                                  // llm_weights.hip
int ensure_ws(fvhd_llm* c, int B, int T, hipStream_t st, bool check_capture);     // llm_prefill.hip
// llm_prefill.hip: the launch sequence of fvhd_llm_prefill (extend = false) and of fvhd_llm_extend (extend = true: on the context's started cache)
int decoder_stack(fvhd_llm* c, const void* embeds, int dtype, const uint8_t* key_valid, const int64_t* position_ids, int batch, int seq_len,
                  float* logits_out, void* k_cache, void* v_cache, hipStream_t st, bool extend);
const char* sampling_error(float temperature, int top_k, float top_p);            // llm_step.hip: NULL when the parameters are valid
std::string warpers_error(float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff);   // llm_step.hip: "" when they are valid
// llm_step.hip: "" when the processor settings are valid for a vocabulary of V ids (V <= 0: the id range is not checked); lists: host memory
std::string processors_error(float repetition_penalty, int no_repeat_ngram_size, int min_new_tokens, const int32_t* eos_ids, int n_eos,
                             const int32_t* suppress_ids, int n_suppress, int V);

#pragma GCC visibility pop
