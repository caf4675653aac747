// Every internal extern "C" symbol of the library that crosses a translation unit, declared ONCE: the file that defines a launcher and
// every file that calls it include this header, so a prototype that drifts from its definition is a compile error (the symbols are
// unmangled - a mismatch would still link and pass garbage).  Launchers return a hipError_t as int.  The public functions that kernel files
// define (fvhd_gemm_splitk_plan, fvhd_gemm_qkv_rope_supported, fvhd_dw3_dw7_supported, ...) get the same check from include/fvhd.h, included here.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/fvhd.h"
#include "llm_decode.h"

extern "C" {
int fvhd_set_error(const char* msg);     // fvhd_api.hip: the library's one thread-local error string; returns 1
// dwconv.hip
int fvhd_launch_dwconv(hipStream_t st, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int Cin, int K, int stride, int mult, int gelu,
                       int flags, unsigned* amax);
// dwconv_mfma.hip
int fvhd_dw7_mfma_supported(int B, int H, int W, int C, int force);
int fvhd_launch_dw7_mfma(hipStream_t st, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int C, unsigned* amax);
// dwconv_down.hip
int fvhd_launch_dw7s2_mfma(hipStream_t st, const void* x, void* y, const float* w, const float* bias, int B, int H, int W, int Cin, int gelu);
// dwconv_fused.hip
int fvhd_launch_dw3_dw7(hipStream_t st, const void* x, void* y, void* a, const float* w3, const float* b3, const float* w7, const float* b7, int B, int H, int W, int C,
                        unsigned* amax);
// gemm.hip
int fvhd_launch_gemm(hipStream_t st, const void* A, const void* Wt, const float* bias, const float* ls, const void* resid, void* out, int M, int N, int K, int epi,
                     int out_dtype);
int fvhd_launch_gemm_splitk(hipStream_t st, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N, int K, int splits);
int fvhd_launch_gemm_splitk_ls(hipStream_t st, const void* A, const void* Wt, const float* bias, const float* ls, const void* resid, void* out, float* partial, int M,
                               int N, int K, int splits);
int fvhd_launch_gemm_splitk_partials(hipStream_t st, const void* A, const void* Wt, float* partial, int M, int N, int K, int splits);
int fvhd_launch_gemm_splitk_norm(hipStream_t st, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N, int K, int splits,
                                 const float* norm_w, void* norm_out, float eps);
int fvhd_launch_gemm_qkv_rope(hipStream_t st, const void* A, const void* Wt, const float* bias, void* out, int Mp, int N, int K, const long* pos, const float* table,
                              void* kcache, void* vcache, int M, int T, int nh, int nkv, int HD, int P, float theta);
// attention.hip
int fvhd_launch_layernorm(hipStream_t st, const void* x, void* y, const float* w, const float* b, int M, int C, float eps);
int fvhd_launch_attention(hipStream_t st, const void* qkv, void* out, int B, int N, int C, int fp8);
// stem_head.hip
int fvhd_launch_stem_conv(hipStream_t st, const void* img, int dtype, void* out, const float* w, const float* bias, int B, int R);
int fvhd_launch_stem_fused(hipStream_t st, const void* img, int dtype, void* out, const float* w0, const float* b0, const float* w1, const float* b1, const void* w2,
                           const float* b2, int B, int R);
int fvhd_launch_se_head(hipStream_t st, const void* y, float* pooled, float* scale, const float* wr, const float* br, const float* we, const float* be, void* out,
                        int out_dtype, int B, int T, int C, int RD);
int fvhd_launch_cast_to_bf16(hipStream_t st, const void* x, int dtype, void* y, long n);
// ffn_fused.hip
int fvhd_ffn_pack_host(int C, const float* fc1, const float* fc2, uint16_t* w1img, uint16_t* w2img, int precision);
float fvhd_ffn_half_w2_limit(void);
int fvhd_launch_ffn_fused(hipStream_t st, const void* A, const void* w1img, const float* b1, const void* w2img, const float* b2, const float* ls, void* X, int M, int C,
                          int precision);
// splice.hip
int fvhd_launch_splice(hipStream_t st, const long* ids, const int* start, const int* seqlen, const long* feat_row0, const long* labels_in, const void* table,
                       const void* feats, void* out, unsigned char* mask_out, long* pos_out, long* labels_out, int B, int L, int H, int max_len, long vocab,
                       long n_feat_rows, int left_pad, int dtype);
// preprocess.hip
int fvhd_launch_preprocess(hipStream_t st, const void* src, int src_h, int src_w, long src_pitch, int pad_top, int pad_left, unsigned bg, const int* hb, const int* hc,
                           int hk, const int* vb, const int* vc, int vk, int row0, int nrows, void* tmp, const float* lut, int R, void* out, int out_dtype);
// llm.hip
int fvhd_launch_rmsnorm(hipStream_t st, const void* x, void* y, const float* w, int M, int H, float eps);
int fvhd_launch_rope(hipStream_t st, void* qkv, const long* pos, const float* table, void* kcache, void* vcache, int M, int T, int nh, int nkv, int HD, int P, float theta);
int fvhd_launch_splitk_bias_rope(hipStream_t st, const float* partial, int splits, int Mp, const float* bias, void* qkv, const long* pos, const float* table, void* kcache,
                                 void* vcache, int M, int T, int nh, int nkv, int HD, int P, float theta);
int fvhd_launch_llm_attention(hipStream_t st, const void* qkv, void* out, const unsigned char* key_valid, int B, int T, int nh, int nkv, int HD);
int fvhd_launch_cast_rows(hipStream_t st, const void* src, int dtype, void* dst, long n);
int fvhd_launch_gather_rows(hipStream_t st, const void* src, void* dst, int B, int T, int t_sel, int H);
// llm_extend.hip
int fvhd_launch_llm_attention_past(hipStream_t st, const void* qkv, const void* kc, const void* vc, const unsigned char* key_valid, void* out, int B, int T, int nh,
                                   int nkv, int HD, int cap, const int* past_len, const int* status);
int fvhd_launch_llm_cache_append(hipStream_t st, const void* qkv, void* kc, void* vc, unsigned char* key_valid, const unsigned char* chunk_valid, int B, int T, int nh,
                                 int nkv, int HD, int cap, const int* past_len, int* status, int* status_host);
int fvhd_launch_llm_extend_positions(hipStream_t st, const int64_t* next, const unsigned char* chunk_valid, int64_t* pos, int B, int T, const int* status);
int fvhd_launch_llm_extend_state(hipStream_t st, int64_t* next, const int64_t* pos, int B, int T, int* len, const int* status);
int fvhd_launch_llm_cache_rewind(hipStream_t st, const int* keep, int rows, unsigned char* key_valid, int64_t* next, int cap, int* len, int* status, int* status_host);
// llm_decode.hip
int fvhd_launch_dec_gemm(hipStream_t st, const DecGemmArgs* a);
int fvhd_launch_dec_attention(hipStream_t st, const void* q, const void* kc, const void* vc, const unsigned char* key_valid, void* out, int B, int nh, int nkv, int hd,
                              int cap, const int* len, int len_add, int S, int chunk, float* part, int* cnt, const int* status);
int fvhd_launch_dec_embed(hipStream_t st, const int64_t* tok, const int64_t* last, const void* table, int V, int H, void* h, unsigned char* key_valid, int B, int cap,
                          const int* len, int* status, int* status_host);
int fvhd_launch_dec_argmax_finish(hipStream_t st, const float* av, const int* ai, int nblk, int B, int64_t* last, int64_t* ids_out, int64_t* posv, int* len,
                                  const int* status);
int fvhd_launch_dec_argmax_blocks(hipStream_t st, const float* logits, int V, int B, float* av, int* ai);
int fvhd_launch_dec_start_state(hipStream_t st, int64_t* posv, const int64_t* position_ids, int B, int T, int* len, int* status);
// llm_w8.hip
int fvhd_launch_dec_gemm_w8(hipStream_t st, const DecGemmArgs* a);
int fvhd_launch_quantize_e4m3(hipStream_t st, const void* w, int rows, int K, void* codes, long pitch, float* scale, int sstride, int packed);
int fvhd_launch_w8_unpack(hipStream_t st, const void* src, const float* scale, void* dst, long N, int K, int mode);
int fvhd_launch_dec_embed_w8(hipStream_t st, const int64_t* tok, const int64_t* last, const void* table, const float* scale, int V, int H, void* h,
                             unsigned char* key_valid, int B, int cap, const int* len, int* status, int* status_host);
// llm_w4.hip
int fvhd_launch_dec_gemm_w4(hipStream_t st, const DecGemmArgs* a);
int fvhd_launch_quantize_mxfp4(hipStream_t st, const void* w, int rows, int K, void* codes, long pitch, void* scales, long spitch, int packed);
int fvhd_launch_w4_unpack(hipStream_t st, const void* src, const void* scales, void* dst, long N, int K, int mode);
int fvhd_launch_dec_embed_w4(hipStream_t st, const int64_t* tok, const int64_t* last, const void* table, const void* scales, int V, int H, void* h,
                             unsigned char* key_valid, int B, int cap, const int* len, int* status, int* status_host);
// llm_sample.hip
size_t fvhd_dec_sample_ws_bytes(void);
int fvhd_launch_dec_sample(hipStream_t st, const DecSampleArgs* a, void* ws);
int fvhd_launch_dec_sample_theta(hipStream_t st, const DecSampleArgs* a, void* ws, unsigned* theta_key);
// llm_beam.hip
size_t fvhd_dec_beam_topk_ws_bytes(void);
int fvhd_dec_beam_topk_supported(int G, int K, int C, int V);
int fvhd_launch_dec_beam_topk(hipStream_t st, const float* logits, const float* scores, int G, int K, int C, int V, float* out_v, int64_t* out_i, void* ws);
int fvhd_launch_dec_beam_topk_mode(hipStream_t st, const float* logits, const float* scores, int G, int K, int C, int V, int prenorm, float* out_v, int64_t* out_i,
                                   void* ws);
size_t fvhd_dec_beam_norm_ws_bytes(void);
int fvhd_dec_beam_norm_supported(int rows, int V);
// stats: NULL, or fp32 [rows][2] = the (M, L) that were subtracted; status: NULL, or the launches do nothing while *status != 0
int fvhd_launch_dec_beam_norm(hipStream_t st, float* logits, int rows, int V, void* ws, float* stats, const int* status);
size_t fvhd_dec_hist_gather_ws_bytes(int batch, int cap, int V);
int fvhd_launch_dec_hist_gather(hipStream_t st, const DecHistGatherArgs* a);
size_t fvhd_dec_beam_sample_ws_bytes(void);      // zeroed once by the owner: it holds the sampler's arrival counters
int fvhd_launch_dec_beam_sample(hipStream_t st, const DecBeamSampleArgs* a, void* ws);
size_t fvhd_dec_cache_gather_ws_bytes(int rows, int nkv, int hd, int cap);
int fvhd_launch_dec_cache_gather(hipStream_t st, const DecCacheGatherArgs* a);
// llm_spec.hip
int fvhd_launch_spec_draft(hipStream_t st, const int* seq, const int* seq_len, int max_ngram, int K, int64_t* draft, const int* status, const int* words,
                           int* gate);
int fvhd_launch_spec_embed(hipStream_t st, const int64_t* draft, const int64_t* last, const void* table, const float* scale, const void* wblk, int V, int H,
                           void* h, unsigned char* key_valid, int T, int cap, const int* len, const int64_t* posv, int64_t* pos, int* status,
                           int* status_host, int* gate);
int fvhd_launch_spec_attention(hipStream_t st, const void* q, void* kc, void* vc, const void* ks, const void* vs, const unsigned char* key_valid, void* out,
                               int T, int nh, int nkv, int hd, int cap, const int* len, int S, int chunk, float* part, int* cnt, const int* status);
int fvhd_launch_spec_accept(hipStream_t st, const SpecAcceptArgs* a);
int fvhd_launch_spec_logprobs_copy(hipStream_t st, const SpecLogprobsArgs* a);
int fvhd_launch_spec_begin(hipStream_t st, const int64_t* lookup, int n, const int64_t* last, int* seq, int64_t* out, int* words, int limit,
                           const SpecEosList* eos);
// llm_score.hip (the shape is valid when fvhd_lm_score_plan(M, V, K) != 0; scratch: fvhd_lm_score_scratch_bytes, 16-byte aligned)
int fvhd_launch_lm_score(hipStream_t st, const void* xn, const void* Wt, const int64_t* target, int M, int V, int K, float* logprob, float* lse, void* scratch);
// llm_logits.hip
int fvhd_launch_dec_logits_process(hipStream_t st, const DecLogitsArgs* a);
int fvhd_launch_dec_logits_history(hipStream_t st, const int* tokens, int* hist, unsigned* seen, int B, int V, int cap, int g);
// llm_logprobs.hip (scratch: fvhd_dec_logprobs_scratch_bytes, its first 16 384 bytes zero before the first launch; status: NULL or the error word)
int fvhd_launch_dec_logprobs(hipStream_t st, const float* logits, const int64_t* ids, int B, int V, int top_n, float* token_logprob, int64_t* top_ids,
                             float* top_logprobs, void* scratch, const int* status);
// llm_constrain.hip (the advance / reset launch when the arguments ask for one, then the mask launch)
int fvhd_launch_dec_constrain(hipStream_t st, const DecConstrainArgs* a);
// llm_guidance.hip (logits fp32 [2 G][V], finite; scratch: fvhd_dec_guidance_scratch_bytes, its first 16 384 bytes zero before the first launch;
// status: NULL or the error word).  The statistics launch and the apply launch; the mirror: ids of rows [0, G) -> rows [G, 2 G), posv (optional) + 1 there
size_t fvhd_dec_guidance_scratch_bytes(int G, int V);
int fvhd_launch_dec_guidance(hipStream_t st, float* logits, int G, int V, float scale, void* scratch, const int* status);
int fvhd_launch_dec_guidance_mirror(hipStream_t st, int G, int64_t* last, int64_t* ids_out, int64_t* posv, const int* status);
}
