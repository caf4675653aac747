// Arguments of the decode-step weight-streaming GEMM (llm_decode.hip), shared with the launch sequences in llm_step.hip and llm_ops.hip.
#pragma once
#include <stdint.h>

#define DEC_EPI_RESID 4      // out[b][n] = bf16(resid[b][n] + acc)                        (o_proj / down_proj + the skip)
#define DEC_EPI_SWIGLU 5     // out[b][j] = bf16(silu(acc[2j]) * acc[2j + 1])             (gate|up rows interleaved)
#define DEC_EPI_QKV 6        // bias, ONE bf16 rounding, rotary embedding of q / k, q -> out, k / v -> cache slot *len
#define DEC_EPI_ARGMAX 7     // fp32 logits (optional) + per-workgroup (max, index) of every row

struct DecGemmArgs {
    const void* x = nullptr;       // bf16 rows [B][ldx]; the first K columns are the operand
    int ldx = 0;
    const float* norm_w = nullptr; // non-NULL: Qwen2RMSNorm of the x rows (statistics over K) folded into the operand load
    float eps = 1e-6f;
    const void* W = nullptr;       // bf16 [N][K] (the packed layouts of the prefill)
    int N = 0, K = 0, B = 0;
    int S = 1, cpw = 0;            // K split over S workgroups of cpw 128-deep chunks (the last one may hold fewer)
    float* part = nullptr;         // S > 1: fp32 slabs [S][N / 16][NB][64][4], NB = ceil(B / 16) batch tiles
    int* cnt = nullptr;            // S > 1: one arrival counter per workgroup column, zero between launches (the last arriver resets it)
    int epi = 0;
    const void* resid = nullptr;   // RESID: bf16 [B][ldo] (may alias out)
    void* out = nullptr;           // RESID / SWIGLU: bf16 [B][ldo]; QKV: q rows bf16 [B][ldo = n_heads * head_dim]
    int ldo = 0;
    const float* bias = nullptr;   // QKV: fp32 [N]
    const int64_t* pos = nullptr;  // QKV: position of every row's token, int64 [B]
    const float* rope = nullptr;   // QKV: (cos, sin) table [P][hd / 2][2]
    int P = 0;
    float theta = 1e6f;
    int nh = 0, nkv = 0, hd = 0;
    void* kc = nullptr;            // QKV: this layer's caches, bf16 [cache_batch][nkv][cap][hd]
    void* vc = nullptr;
    int cap = 0;
    const int* len = nullptr;      // QKV: the slot the new token's k / v go to (device word)
    float* logits = nullptr;       // ARGMAX: fp32 [B][N] or NULL
    float* amax_v = nullptr;       // ARGMAX: [gridDim][16 * NB] best value / index of every row within the workgroup's columns
    int* amax_i = nullptr;
    const int* status = nullptr;   // non-NULL: the launch does nothing while *status != 0 (a step past the cache's capacity)
    float* rstd = nullptr;         // B > 16 with norm_w: scratch [B]; the row statistics are computed once, by a launch of their own, instead of
                                   // in every workgroup (NULL: every workgroup recomputes them, as at B <= 16; the bits are the same)
    const float* wscale = nullptr; // non-NULL: W holds OCP e4m3 codes [N][K], one byte each, in the packed K order of llm_w8.hip, and row n
                                   // stands for code * wscale[n] (fp32 [N]); the launch goes to dec_gemm_w8_kernel
    const unsigned char* wblk = nullptr;   // non-NULL (wscale is NULL then): W holds MXFP4 codes [N][K / 2] in the packed K order of w4_layout.h and
                                   // wblk the e8m0 block scales u8 [N][K / 32]; the launch goes to dec_gemm_w4_kernel (llm_w4.hip)
};

// Arguments of the sampler (llm_sample.hip): temperature / top-k / top-p over fp32 logits [B][V], one draw per row.
struct DecSampleArgs {
    const float* logits = nullptr;
    int B = 0, V = 0;              // B in [1, 64]: launched in blocks of 16 rows
    int row0 = 0;                  // set per block by the launcher: first row of the block (logits, ids, positions, u and the Philox
                                   // counter are indexed by the global row row0 + r, the workspace by r)
    float temperature = 1.f;       // > 0
    int top_k = 0;                 // 0 = off
    float top_p = 1.f;             // 1 = off
    float min_p = 0.f;             // the warpers behind top-p, in transformers' order (fvhd_llm_set_sampling_warpers): 0 = off
    float typical_p = 1.f;         // 1 = off
    float epsilon_cutoff = 0.f;    // 0 = off
    float eta_cutoff = 0.f;        // 0 = off
    float* info8 = nullptr;        // [B][8]: lowest kept s, kept count, Z, u, highest kept s, kept counts behind min_p / typical_p / epsilon_cutoff
    unsigned long long seed = 0;   // Philox key: low word, high word
    const int* len = nullptr;      // Philox counter (row, n = (len ? *len : 0) + n_add, 0, 0)
    int n_add = 0;
    const float* u_override = nullptr;   // non-NULL: u [B] instead of Philox
    int64_t* last = nullptr;       // chosen ids [B] (each optional)
    int64_t* ids_out = nullptr;
    float* info = nullptr;         // [B][4]: theta, kept count, Z, u
    int64_t* posv = nullptr;       // non-NULL: positions += 1
    int* len_advance = nullptr;    // non-NULL: *len_advance += 1 once every row (of the last block) has read n
    const int* status = nullptr;
    int seq_rows = 0;              // 1: the B <= 16 rows are consecutive positions of ONE sequence (a verify step, llm_spec.hip): logits, ids_out,
    int seq_row = 0;               // info and u_override are indexed by the row r, the Philox counter is (seq_row, n + r, 0, 0) - the counter of
                                   // the plain step at that position; the launch writes ids_out / info only, never last, posv or the length
};

// Arguments of the KV-cache reorder (llm_beam.hip): row r of every layer's K / V (slots [0, *len)), of the mask and of the positions = row src[r].
struct DecCacheGatherArgs {
    char* kc = nullptr;            // K and V of all layers, bf16 [layers][batch][nkv][cap][hd]
    char* vc = nullptr;
    int layers = 0, batch = 0;     // batch: rows of the allocation (the layer stride)
    unsigned char* mask = nullptr; // key-valid [batch][cap]
    int64_t* posv = nullptr;       // next positions [batch]
    const int64_t* src = nullptr;  // int64 [rows_out] on the device, every entry in [0, rows_in)
    int rows_in = 0, rows_out = 0; // both <= batch
    int nkv = 0, hd = 0, cap = 0;
    const int* len = nullptr;      // device word: slots [0, *len) move
    int* status = nullptr;         // the launches do nothing while *status != 0; an index out of range sets it (and *status_host, optional) to 3
    int* status_host = nullptr;
    char* ws = nullptr;            // fvhd_dec_cache_gather_ws_bytes(batch, nkv, hd, cap) bytes
};

// Arguments of the reorder of the rows' processor histories and automaton states (llm_beam.hip), behind the KV reorder with the same src.
struct DecHistGatherArgs {
    int* hist = nullptr;           // [batch][cap] history entries (DecLogitsArgs::hist), or NULL: no histories move
    unsigned* seen = nullptr;      // [batch][ceil(V / 32)]
    int* count = nullptr;          // [batch]
    int* states = nullptr;         // the constraint's states [batch] and flags [batch], or NULL: no states move
    int* flags = nullptr;
    const int64_t* src = nullptr;  // int64 [rows_out] on the device, every entry in [0, rows_in)
    int rows_in = 0, rows_out = 0, batch = 0, cap = 0, V = 0;
    int* status = nullptr;         // as DecCacheGatherArgs::status
    int* status_host = nullptr;
    char* ws = nullptr;            // fvhd_dec_hist_gather_ws_bytes(batch, cap, V) bytes, 16-byte aligned
};

// Arguments of beam-search sampling (llm_beam.hip): per prompt the `keep` kept candidates with the largest a + g (include/fvhd.h "LLM beam-search
// sampling"), logits fp32 [G * K][V] 16-byte aligned, scores fp32 [G][K].
struct DecBeamSampleArgs {
    const float* logits = nullptr;
    const float* scores = nullptr;
    int G = 0, K = 0, keep = 0, V = 0;
    float temperature = 1.f;       // > 0
    int top_k = 0;                 // 0 = off
    float top_p = 1.f;             // 1 = off
    int min_keep = 1;              // transformers' min_tokens_to_keep under beams, in [1, keep]
    unsigned long long seed = 0;   // Philox key: low word, high word
    const int* len = nullptr;      // Philox counter (row, n = (len ? *len : 0) + n_add, v >> 2, 1)
    int n_add = 0;
    const float* noise_override = nullptr;   // non-NULL: g [G * K][V] instead of Philox
    float* noise_out = nullptr;    // non-NULL: [G * K][V], every token's g
    float* info = nullptr;         // non-NULL: [G * K][4]: theta as s (-inf: no filter binds), kept count, row maximum M, L = log sum exp(x - M)
    float* out_v = nullptr;        // [G][keep]: the unperturbed a of the picks, in descending a + g
    int64_t* out_i = nullptr;      // [G][keep]: beam * V + token
    int prenorm = 0;               // 1: the rows hold processed log-probabilities x' - a = x' / T + score, no M or L subtracted
};

// Arguments of the logits processors (llm_logits.hip): sparse in-place edits of fp32 logits [B][V] from a per-row token history, one
// workgroup per row (include/fvhd.h "LLM logits processors").
struct DecLogitsArgs {
    float* logits = nullptr;
    int B = 0, V = 0;
    int* hist = nullptr;           // [B][cap]: entry = token | 0x80000000 when an earlier entry of the row holds the same token
    int cap = 0;
    unsigned* seen = nullptr;      // [B][ceil(V / 32)] bits: token occurs in the row's history (tested and set by the append)
    const int64_t* tok = nullptr;  // the step's fed ids: tok, else last; both NULL = nothing to append (the first token, the single op)
    const int64_t* last = nullptr;
    int* count = nullptr;          // device words [B]: the tokens in each row's history - read before the append, written back behind it
                                   // (NOT the cache length less the prompt: a step enqueued with processors off appends and counts nothing)
    int start_T = 0;               // > 0: fvhd_llm_start's launch - the history is empty: count[b] = 0
    int g_fixed = -1;              // >= 0: the history length itself (the single op)
    float penalty = 1.f;           // repetition_penalty (1 = off)
    int ngram = 0, min_new = 0;    // no_repeat_ngram_size, min_new_tokens (0 = off)
    const int* eos = nullptr;      // int32 [n_eos] / [n_sup] on the device, every id in [0, V)
    const int* sup = nullptr;
    int n_eos = 0, n_sup = 0;
    const int* status = nullptr;   // non-NULL: the launch does nothing (appends nothing) while *status != 0
};

// Speculative verification (llm_spec.hip).  The device words of a lookup generation, int32 [SPEC_WORDS]:
#define SPEC_W_SEQ_LEN 0     // tokens in the token buffer (lookup ids, then every generated token)
#define SPEC_W_WRITTEN 1     // tokens written to the output buffer
#define SPEC_W_FINISHED 2    // an EOS id was emitted, or the token limit was reached: later steps do nothing
#define SPEC_W_STEPS 3       // verify steps that ran
#define SPEC_W_TOKENS 4      // tokens those steps emitted
#define SPEC_W_LIMIT 5       // max_new_tokens
#define SPEC_W_N_EOS 6
#define SPEC_W_EOS 8         // .. 23: the EOS ids
#define SPEC_WORDS 24

struct SpecEosList { int n = 0; int ids[16] = {}; };

// Arguments of the accept launch: drafts int64 [T - 1] against the step's argmax ids int64 [T]
struct SpecAcceptArgs {
    const int64_t* draft = nullptr;
    const int64_t* ids = nullptr;
    int T = 0;
    int* words = nullptr;          // NULL: a bare verify step - no EOS cut, no limit, nothing appended
    int* seq = nullptr;            // the token buffer int32 [seq_cap]
    int seq_cap = 0;
    int64_t* out = nullptr;        // the output tokens int64 [out_cap]
    int out_cap = 0;
    int* emitted = nullptr;        // optional: the number of tokens this step emitted (1 .. T)
    int64_t* last = nullptr;       // the cache state of sequence 0: last id, next position, length, key-valid mask [cap]
    int64_t* posv = nullptr;
    int* len = nullptr;
    unsigned char* key_valid = nullptr;
    int cap = 0;
    const int* gate = nullptr;     // non-NULL: the launch does nothing while *gate != 0
};

// Arguments of the log-probability copy behind the accept of a lookup step: the rows the step emitted go from the step's scratch to the
// generation's arrays at the offset of its first emitted token (read from the accept's words on the device)
struct SpecLogprobsArgs {
    const float* tok = nullptr;    // the step's scratch: [T], [T][n], [T][n]
    const int64_t* ids = nullptr;
    const float* top = nullptr;
    int n = 0;                     // top_n, 0 .. 16
    const int* emitted = nullptr;  // the accept's count of this step (1 .. T)
    const int* words = nullptr;    // SPEC_W_WRITTEN behind the accept = the offset of the first emitted token + emitted
    float* out_tok = nullptr;      // the generation's arrays: [out_cap], [out_cap][n], [out_cap][n]
    int64_t* out_ids = nullptr;
    float* out_top = nullptr;
    int out_cap = 0;
    const int* gate = nullptr;     // the step's gate word
};

// Constrained decoding (llm_constrain.hip): the automaton's CSR tables, the rows' states and the step's fed ids
#define DEC_CON_SLICE 4096   // ids per workgroup of the mask launch (fvhd_dec_constrain_slice)

struct DecConstrainArgs {
    float* logits = nullptr;       // fp32 [B][V], row stride V, any 4-byte alignment
    int B = 0, V = 0;
    const int* offsets = nullptr;  // int32 [n_states + 1]
    const int* tokens = nullptr;   // int32 [n_edges], strictly ascending inside a state
    const int* targets = nullptr;  // int32 [n_edges]: the next state, or -1 (FREE)
    int n_states = 0;
    int* states = nullptr;         // int32 [B]: -1 = FREE
    int* flags = nullptr;          // int32 [B]: bit 0 = the row was fed a token its state does not list
    const int64_t* tok = nullptr;  // the step's fed ids: tok, else last; both NULL = no advance
    const int64_t* last = nullptr;
    int reset = 0;                 // 1: states[b] = start[n_start == 1 ? 0 : b], flags[b] = 0 (fvhd_llm_start / _extend) instead of an advance
    int n_start = 0;
    int start[64] = {};            // by value: a captured launch keeps the start states it was captured with
    const int* status = nullptr;   // non-NULL: the launches write nothing while *status != 0
};
