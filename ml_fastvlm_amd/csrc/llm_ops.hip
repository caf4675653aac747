// C ABI of the Qwen2 kernels one at a time (include/fvhd.h fvhd_op_*): the unit tests' entry points.  None of them takes a context.
#include <cmath>

#include "llm_ctx.h"

extern "C" {

int fvhd_op_rmsnorm(fvhd_stream_t st, const void* x, void* y, const float* w, int M, int H, float eps)
{
    if (!x || !y || !w) return lfail("fvhd_op_rmsnorm: NULL pointer");
    return lret("fvhd_op_rmsnorm", fvhd_launch_rmsnorm((hipStream_t)st, x, y, w, M, H, eps));
}

int fvhd_op_rope(fvhd_stream_t st, void* qkv, const int64_t* pos, const float* table, void* k_cache, void* v_cache, int M, int T, int n_heads,
                 int n_kv_heads, int head_dim, int table_positions, float rope_theta)
{
    if (!qkv || !table) return lfail("fvhd_op_rope: NULL pointer");
    return lret("fvhd_op_rope", fvhd_launch_rope((hipStream_t)st, qkv, (const long*)pos, table, k_cache, v_cache, M, T, n_heads, n_kv_heads, head_dim,
                                                 table_positions, rope_theta));
}

int fvhd_op_gemm_qkv_rope(fvhd_stream_t st, const void* A, const void* Wt, const float* bias, void* out, int Mp, int N, int K, const int64_t* pos,
                          const float* table, void* k_cache, void* v_cache, int M, int T, int n_heads, int n_kv_heads, int head_dim, int table_positions,
                          float rope_theta)
{
    if (!A || !Wt || !bias || !out || !table) return lfail("fvhd_op_gemm_qkv_rope: NULL pointer");
    if (!fvhd_gemm_qkv_rope_supported(Mp, N, K, head_dim, n_heads, n_kv_heads))
        return lfail("fvhd_op_gemm_qkv_rope: needs head_dim 64, N = (n_heads + 2 n_kv_heads) * 64, Mp % 128 == 0, N % 128 == 0, K % 64 == 0 and at most one "
                     "128 x 128 tile per CU (fvhd_gemm_qkv_rope_supported); other shapes run fvhd_op_gemm + fvhd_op_rope");
    int e = fvhd_launch_gemm_qkv_rope((hipStream_t)st, A, Wt, bias, out, Mp, N, K, (const long*)pos, table, k_cache, v_cache, M, T, n_heads, n_kv_heads,
                                      head_dim, table_positions, rope_theta);
    return e ? lhip("fvhd_op_gemm_qkv_rope", (hipError_t)e) : 0;
}

int fvhd_op_gemm_splitk(fvhd_stream_t st, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N, int K, int splits)
{
    if (!A || !Wt || !out || !partial) return lfail("fvhd_op_gemm_splitk: NULL pointer");
    if (splits < 1 || N % 128 || K % (64 * splits)) return lfail("fvhd_op_gemm_splitk: needs N % 128 == 0 and K % (64 * splits) == 0");
    return lret("fvhd_op_gemm_splitk", fvhd_launch_gemm_splitk((hipStream_t)st, A, Wt, resid, out, partial, M, N, K, splits));
}

int fvhd_op_gemm_splitk_norm(fvhd_stream_t st, const void* A, const void* Wt, const void* resid, void* out, float* partial, int M, int N, int K, int splits,
                             const float* norm_w, void* norm_out, float eps)
{
    if (!A || !Wt || !out || !partial || !norm_w || !norm_out) return lfail("fvhd_op_gemm_splitk_norm: NULL pointer");
    if (norm_out == out) return lfail("fvhd_op_gemm_splitk_norm: norm_out must not alias out");
    if (splits < 1 || N % 128 || K % (64 * splits)) return lfail("fvhd_op_gemm_splitk_norm: needs N % 128 == 0 and K % (64 * splits) == 0");
    return lret("fvhd_op_gemm_splitk_norm", fvhd_launch_gemm_splitk_norm((hipStream_t)st, A, Wt, resid, out, partial, M, N, K, splits, norm_w, norm_out, eps));
}

int fvhd_op_qkv_splitk_rope(fvhd_stream_t st, const void* A, const void* Wt, const float* bias, float* partial, void* qkv, const int64_t* pos,
                            const float* table, void* k_cache, void* v_cache, int M, int Mp, int K, int T, int n_heads, int n_kv_heads, int head_dim,
                            int table_positions, float rope_theta, int splits)
{
    if (!A || !Wt || !partial || !qkv || !table) return lfail("fvhd_op_qkv_splitk_rope: NULL pointer");
    const int width = (n_heads + 2 * n_kv_heads) * head_dim;
    if (splits < 1 || width % 128 || K % (64 * splits) || Mp < M) return lfail("fvhd_op_qkv_splitk_rope: needs width % 128 == 0, K % (64 * splits) == 0, Mp >= M");
    int e = fvhd_launch_gemm_splitk_partials((hipStream_t)st, A, Wt, partial, Mp, width, K, splits);
    if (e) return lhip("fvhd_op_qkv_splitk_rope (gemm)", (hipError_t)e);
    e = fvhd_launch_splitk_bias_rope((hipStream_t)st, partial, splits, Mp, bias, qkv, (const long*)pos, table, k_cache, v_cache, M, T, n_heads, n_kv_heads,
                                     head_dim, table_positions, rope_theta);
    return e ? lhip("fvhd_op_qkv_splitk_rope (reduce)", (hipError_t)e) : 0;
}

int fvhd_op_attention_causal(fvhd_stream_t st, const void* qkv, void* out, const uint8_t* key_valid, int B, int T, int n_heads, int n_kv_heads, int head_dim)
{
    if (!qkv || !out) return lfail("fvhd_op_attention_causal: NULL pointer");
    return lret("fvhd_op_attention_causal", fvhd_launch_llm_attention((hipStream_t)st, qkv, out, key_valid, B, T, n_heads, n_kv_heads, head_dim));
}

// ---- single ops of fvhd_llm_extend / fvhd_llm_cache_rewind (llm_extend.hip) ----
int fvhd_op_attention_extend(fvhd_stream_t st, const void* qkv, const void* k_cache, const void* v_cache, const uint8_t* key_valid, void* out, int B, int T,
                             int n_heads, int n_kv_heads, int head_dim, int capacity, const int* past_len)
{
    if (!qkv || !k_cache || !v_cache || !out || !past_len) return lfail("fvhd_op_attention_extend: NULL pointer");
    if (head_dim != 64 && head_dim != 128) return lfail("fvhd_op_attention_extend: head_dim must be 64 or 128");
    if (B < 1 || T < 1 || capacity < 1 || T > capacity || n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads)
        return lfail("fvhd_op_attention_extend: needs B >= 1, 1 <= T <= capacity and n_heads a multiple of n_kv_heads");
    return lret("fvhd_op_attention_extend", fvhd_launch_llm_attention_past((hipStream_t)st, qkv, k_cache, v_cache, key_valid, out, B, T, n_heads, n_kv_heads, head_dim,
                                                                           capacity, past_len, nullptr));
}

int fvhd_op_cache_append(fvhd_stream_t st, const void* qkv, void* k_cache, void* v_cache, uint8_t* key_valid, const uint8_t* chunk_valid, int B, int T, int n_heads,
                         int n_kv_heads, int head_dim, int capacity, const int* past_len, int* status)
{
    if (!qkv || !k_cache || !v_cache || !past_len || !status) return lfail("fvhd_op_cache_append: NULL pointer");
    if (B < 1 || T < 1 || capacity < 1 || T > capacity || n_heads < 1 || n_kv_heads < 1 || head_dim < 8 || head_dim % 8 || ((uintptr_t)qkv & 15) ||
        ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15))
        return lfail("fvhd_op_cache_append: needs B >= 1, 1 <= T <= capacity, head_dim % 8 == 0 and rows and caches aligned to 16 bytes");
    return lret("fvhd_op_cache_append", fvhd_launch_llm_cache_append((hipStream_t)st, qkv, k_cache, v_cache, key_valid, chunk_valid, B, T, n_heads, n_kv_heads,
                                                                     head_dim, capacity, past_len, status, nullptr));
}

int fvhd_op_extend_positions(fvhd_stream_t st, const int64_t* next_positions, const uint8_t* chunk_valid, int64_t* pos_out, int B, int T)
{
    if (!next_positions || !pos_out) return lfail("fvhd_op_extend_positions: NULL pointer");
    if (B < 1 || T < 1) return lfail("fvhd_op_extend_positions: needs B >= 1 and T >= 1");
    return lret("fvhd_op_extend_positions", fvhd_launch_llm_extend_positions((hipStream_t)st, next_positions, chunk_valid, pos_out, B, T, nullptr));
}

int fvhd_op_cache_rewind(fvhd_stream_t st, const int32_t* keep, int rows, uint8_t* key_valid, int64_t* positions, int capacity, int* length, int* status)
{
    if (!keep || !key_valid || !positions || !length || !status) return lfail("fvhd_op_cache_rewind: NULL pointer");
    if (rows < 1 || rows > 64 || capacity < 1) return lfail("fvhd_op_cache_rewind: needs 1 <= rows <= 64 and capacity >= 1");
    return lret("fvhd_op_cache_rewind", fvhd_launch_llm_cache_rewind((hipStream_t)st, keep, rows, key_valid, positions, capacity, length, status, nullptr));
}

// ---- scoring given tokens (llm_score.hip) ----
int fvhd_op_lm_score(fvhd_stream_t st, const void* xn, const void* Wt, const int64_t* targets, int M, int V, int K, float* logprob_out, float* lse_out,
                     void* scratch, size_t scratch_bytes)
{
    if (!xn || !Wt || !targets || !logprob_out || !scratch) return lfail("fvhd_op_lm_score: NULL pointer");
    if (M < 1) return lfail("fvhd_op_lm_score: needs M >= 1");
    if (V < 8 || V % 8) return lfail("fvhd_op_lm_score: the vocabulary V = " + std::to_string(V) + " must be a positive multiple of 8 (V % 8 == 0)");
    if (K < 32 || K % 32) return lfail("fvhd_op_lm_score: the hidden size K = " + std::to_string(K) + " must be a positive multiple of 32 (K % 32 == 0)");
    if (((uintptr_t)xn & 15) || ((uintptr_t)Wt & 15) || ((uintptr_t)scratch & 15)) return lfail("fvhd_op_lm_score: xn, Wt and scratch must be aligned to 16 bytes");
    const size_t need = fvhd_lm_score_scratch_bytes(M, V, K);
    if (scratch_bytes < need)
        return lfail("fvhd_op_lm_score: scratch too small: " + std::to_string(scratch_bytes) + " bytes, fvhd_lm_score_scratch_bytes(M, V, K) = " + std::to_string(need));
    return lret("fvhd_op_lm_score", fvhd_launch_lm_score((hipStream_t)st, xn, Wt, targets, M, V, K, logprob_out, lse_out, scratch));
}

// ---- single ops of the decode step (unit tests) ----
// One builder per epilogue family fills DecGemmArgs; `scale` is NULL for a bf16 matrix, the fp32 row scales of an e4m3 one (the *_w8 entry points)
static DecGemmArgs dec_args(int epi, const void* x, int B, const float* norm_w, float eps, const void* W, const float* scale, int N, int K, int splits)
{
    DecGemmArgs a;
    a.x = x; a.ldx = K; a.norm_w = norm_w; a.eps = eps; a.W = W; a.wscale = scale; a.N = N; a.K = K; a.B = B; a.epi = epi;
    a.cpw = (K / 128 + splits - 1) / splits;
    if (a.cpw) a.S = (K / 128 + a.cpw - 1) / a.cpw;      // (K < 128: the launcher refuses cpw = 0)
    return a;
}

static DecGemmArgs dec_gemm_args(int epi, const void* x, int B, const float* norm_w, float eps, const void* W, const float* scale, int N, int K,
                                 const void* resid, void* out, float* partial, int* counters, int splits)
{
    DecGemmArgs a = dec_args(epi, x, B, norm_w, eps, W, scale, N, K, splits);
    a.part = partial; a.cnt = counters; a.resid = resid; a.out = out; a.ldo = epi == FVHD_EPI_SWIGLU ? N / 2 : N;
    return a;
}

static DecGemmArgs dec_qkv_args(const void* x, int B, int K, const float* norm_w, float eps, const void* W, const float* scale, const float* bias, void* q_out,
                                const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache, void* v_cache, int capacity,
                                const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters, int splits)
{
    DecGemmArgs a = dec_args(DEC_EPI_QKV, x, B, norm_w, eps, W, scale, (n_heads + 2 * n_kv_heads) * head_dim, K, splits);
    a.part = partial; a.cnt = counters; a.bias = bias; a.out = q_out; a.ldo = n_heads * head_dim; a.pos = pos; a.rope = table; a.P = table_positions;
    a.theta = rope_theta; a.nh = n_heads; a.nkv = n_kv_heads; a.hd = head_dim; a.kc = k_cache; a.vc = v_cache; a.cap = capacity; a.len = length;
    return a;
}

static DecGemmArgs dec_argmax_args(const void* x, int B, const float* norm_w, float eps, const void* W, const float* scale, int V, int K, float* logits,
                                   float* scratch_v, int* scratch_i)
{
    DecGemmArgs a = dec_args(DEC_EPI_ARGMAX, x, B, norm_w, eps, W, scale, V, K, 1);
    a.logits = logits; a.amax_v = scratch_v; a.amax_i = scratch_i;
    return a;
}

// e4m3 = a.wscale set: only the *_w8 entry points pass a scale (and refuse a NULL one), the bf16 ones pass nullptr and skip this.  a.W arrives as
// plain row-major codes u8 [N][K]; the kernels read the packed K order of llm_w8.hip, so the codes are repacked into a process-wide scratch first,
// grown on demand (eager calls only, like fvhd_op_dec_sample's workspace).  MXFP4 = a.wblk set (the *_w4 entry points): plain codes u8
// [N][K / 2] repacked into the same scratch, the block scales read where they are.  Then the launch; ARGMAX also reduces the (max, index)
// pairs to ids.
static int dec_run(hipStream_t st, const char* who, DecGemmArgs a, int64_t* ids_out = nullptr)
{
    if (a.wscale || a.wblk) {
        static char* buf[64] = {};
        static size_t cap[64] = {};
        int dev = 0;
        hipError_t he = hipGetDevice(&dev);
        if (he != hipSuccess) return lhip("hipGetDevice", he);
        if (dev < 0 || dev >= 64) return lfail(std::string(who) + ": device index out of range");
        const size_t need = a.wblk ? (size_t)a.N * a.K / 2 : (size_t)a.N * a.K;
        if (need > cap[dev]) {
            if (buf[dev]) (void)hipFree(buf[dev]);                  // (synchronises: no earlier launch still reads it)
            buf[dev] = nullptr;
            cap[dev] = 0;
            if ((he = hipMalloc((void**)&buf[dev], need)) != hipSuccess) { buf[dev] = nullptr; return lhip("hipMalloc(repack scratch)", he); }
            cap[dev] = need;
        }
        if (int e = a.wblk ? fvhd_launch_w4_unpack(st, a.W, nullptr, buf[dev], a.N, a.K, 2) : fvhd_launch_w8_unpack(st, a.W, nullptr, buf[dev], a.N, a.K, 2))
            return lhip(who, (hipError_t)e);
        a.W = buf[dev];
    }
    int e = fvhd_launch_dec_gemm(st, &a);
    if (!e && a.epi == DEC_EPI_ARGMAX) e = fvhd_launch_dec_argmax_finish(st, a.amax_v, a.amax_i, (a.N / 16 + 3) / 4, a.B, nullptr, ids_out, nullptr, nullptr, nullptr);
    return lret(who, e);
}

int fvhd_op_dec_gemm(fvhd_stream_t st, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, int N, int K, const void* resid,
                     void* out, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !out || (epi == FVHD_EPI_RESID && !resid)) return lfail("fvhd_op_dec_gemm: NULL pointer");
    if (epi != FVHD_EPI_RESID && epi != FVHD_EPI_SWIGLU) return lfail("fvhd_op_dec_gemm: epi must be FVHD_EPI_RESID or FVHD_EPI_SWIGLU");
    if (B < 1 || B > 64 || N % 16 || K % 128 || splits < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_gemm: needs 1 <= B <= 64, N % 16 == 0, K % 128 == 0, splits >= 1 (and scratch when splits > 1)");
    return dec_run((hipStream_t)st, "fvhd_op_dec_gemm", dec_gemm_args(epi, x, B, norm_w, eps, Wt, nullptr, N, K, resid, out, partial, counters, splits));
}

int fvhd_op_dec_gemm_w8(fvhd_stream_t st, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, const float* scale, int N, int K,
                        const void* resid, void* out, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !scale || !out || (epi == FVHD_EPI_RESID && !resid)) return lfail("fvhd_op_dec_gemm_w8: NULL pointer");
    if (epi != FVHD_EPI_RESID && epi != FVHD_EPI_SWIGLU) return lfail("fvhd_op_dec_gemm_w8: epi must be FVHD_EPI_RESID or FVHD_EPI_SWIGLU");
    if (B < 1 || B > 64 || N < 16 || N % 16 || K < 128 || K % 128 || splits < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_gemm_w8: needs 1 <= B <= 64, N % 16 == 0, K % 128 == 0, splits >= 1 (and scratch when splits > 1)");
    return dec_run((hipStream_t)st, "fvhd_op_dec_gemm_w8", dec_gemm_args(epi, x, B, norm_w, eps, Wt, scale, N, K, resid, out, partial, counters, splits));
}

int fvhd_op_dec_qkv(fvhd_stream_t st, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const float* bias, void* q_out,
                    const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache, void* v_cache, int capacity,
                    const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !bias || !q_out || !pos || !table || !k_cache || !v_cache || !length) return lfail("fvhd_op_dec_qkv: NULL pointer");
    if (B < 1 || B > 64 || K % 128 || splits < 1 || head_dim % 16 || n_heads < 1 || n_kv_heads < 1 || capacity < 1 || table_positions < 1 ||
        (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_qkv: needs 1 <= B <= 64, K % 128 == 0, head_dim % 16 == 0, splits >= 1 (and scratch when splits > 1)");
    return dec_run((hipStream_t)st, "fvhd_op_dec_qkv", dec_qkv_args(x, B, K, norm_w, eps, Wt, nullptr, bias, q_out, pos, table, table_positions, rope_theta, k_cache,
                                                                    v_cache, capacity, length, n_heads, n_kv_heads, head_dim, partial, counters, splits));
}

int fvhd_op_dec_qkv_w8(fvhd_stream_t st, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const float* scale, const float* bias,
                       void* q_out, const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache, void* v_cache, int capacity,
                       const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !scale || !bias || !q_out || !pos || !table || !k_cache || !v_cache || !length) return lfail("fvhd_op_dec_qkv_w8: NULL pointer");
    if (B < 1 || B > 64 || K < 128 || K % 128 || splits < 1 || head_dim < 16 || head_dim % 16 || n_heads < 1 || n_kv_heads < 1 || capacity < 1 ||
        table_positions < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_qkv_w8: needs 1 <= B <= 64, K % 128 == 0, head_dim % 16 == 0, splits >= 1 (and scratch when splits > 1)");
    return dec_run((hipStream_t)st, "fvhd_op_dec_qkv_w8", dec_qkv_args(x, B, K, norm_w, eps, Wt, scale, bias, q_out, pos, table, table_positions, rope_theta, k_cache,
                                                                       v_cache, capacity, length, n_heads, n_kv_heads, head_dim, partial, counters, splits));
}

int fvhd_op_dec_attention(fvhd_stream_t st, const void* q, const void* k_cache, const void* v_cache, const uint8_t* key_valid, void* out, int B, int n_heads,
                          int n_kv_heads, int head_dim, int capacity, const int* length, float* partial, int* counters, int splits)
{
    if (!q || !k_cache || !v_cache || !key_valid || !out || !length) return lfail("fvhd_op_dec_attention: NULL pointer");
    if (B < 1 || B > 64) return lfail("fvhd_op_dec_attention: needs 1 <= B <= 64");
    if (splits < 1 || capacity < 1 || (splits > 1 && (!partial || !counters))) return lfail("fvhd_op_dec_attention: splits >= 1 (and scratch when splits > 1)");
    const int chunk = ((capacity + splits - 1) / splits + 63) / 64 * 64, S = (capacity + chunk - 1) / chunk;
    return lret("fvhd_op_dec_attention", fvhd_launch_dec_attention((hipStream_t)st, q, k_cache, v_cache, key_valid, out, B, n_heads, n_kv_heads, head_dim, capacity,
                                                                   length, 0, S, chunk, partial, counters, nullptr));
}

int fvhd_op_dec_lm_argmax(fvhd_stream_t st, const void* x, int B, const float* norm_w, float eps, const void* Wt, int V, int K, float* logits, int64_t* ids_out,
                          float* scratch_v, int* scratch_i)
{
    if (!x || !Wt || !ids_out || !scratch_v || !scratch_i) return lfail("fvhd_op_dec_lm_argmax: NULL pointer");
    if (B < 1 || B > 64 || V % 16 || K % 128) return lfail("fvhd_op_dec_lm_argmax: needs 1 <= B <= 64, V % 16 == 0, K % 128 == 0");
    return dec_run((hipStream_t)st, "fvhd_op_dec_lm_argmax", dec_argmax_args(x, B, norm_w, eps, Wt, nullptr, V, K, logits, scratch_v, scratch_i), ids_out);
}

int fvhd_op_dec_lm_argmax_w8(fvhd_stream_t st, const void* x, int B, const float* norm_w, float eps, const void* Wt, const float* scale, int V, int K,
                             float* logits, int64_t* ids_out, float* scratch_v, int* scratch_i)
{
    if (!x || !Wt || !scale || !ids_out || !scratch_v || !scratch_i) return lfail("fvhd_op_dec_lm_argmax_w8: NULL pointer");
    if (B < 1 || B > 64 || V < 16 || V % 16 || K < 128 || K % 128) return lfail("fvhd_op_dec_lm_argmax_w8: needs 1 <= B <= 64, V % 16 == 0, K % 128 == 0");
    return dec_run((hipStream_t)st, "fvhd_op_dec_lm_argmax_w8", dec_argmax_args(x, B, norm_w, eps, Wt, scale, V, K, logits, scratch_v, scratch_i), ids_out);
}

// ---- the same single ops on MXFP4 weights (llm_w4.hip): Wt = plain codes u8 [N][K / 2], scales = block scales u8 [N][K / 32] ----
static bool misaligned4(const void* codes, const void* scales) { return ((uintptr_t)codes & 3) || ((uintptr_t)scales & 3); }

int fvhd_op_dec_gemm_w4(fvhd_stream_t st, int epi, const void* x, int B, const float* norm_w, float eps, const void* Wt, const void* scales, int N, int K,
                        const void* resid, void* out, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !scales || !out || (epi == FVHD_EPI_RESID && !resid)) return lfail("fvhd_op_dec_gemm_w4: NULL pointer");
    if (epi != FVHD_EPI_RESID && epi != FVHD_EPI_SWIGLU) return lfail("fvhd_op_dec_gemm_w4: epi must be FVHD_EPI_RESID or FVHD_EPI_SWIGLU");
    if (B < 1 || B > 64 || N < 16 || N % 16 || K < 128 || K % 128 || splits < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_gemm_w4: needs 1 <= B <= 64, N % 16 == 0, K % 128 == 0, splits >= 1 (and scratch when splits > 1)");
    if (misaligned4(Wt, scales)) return lfail("fvhd_op_dec_gemm_w4: codes and scales must be aligned to 4 bytes");
    DecGemmArgs a = dec_gemm_args(epi, x, B, norm_w, eps, Wt, nullptr, N, K, resid, out, partial, counters, splits);
    a.wblk = (const unsigned char*)scales;
    return dec_run((hipStream_t)st, "fvhd_op_dec_gemm_w4", a);
}

int fvhd_op_dec_qkv_w4(fvhd_stream_t st, const void* x, int B, int K, const float* norm_w, float eps, const void* Wt, const void* scales, const float* bias,
                       void* q_out, const int64_t* pos, const float* table, int table_positions, float rope_theta, void* k_cache, void* v_cache, int capacity,
                       const int* length, int n_heads, int n_kv_heads, int head_dim, float* partial, int* counters, int splits)
{
    if (!x || !Wt || !scales || !bias || !q_out || !pos || !table || !k_cache || !v_cache || !length) return lfail("fvhd_op_dec_qkv_w4: NULL pointer");
    if (B < 1 || B > 64 || K < 128 || K % 128 || splits < 1 || head_dim < 16 || head_dim % 16 || n_heads < 1 || n_kv_heads < 1 || capacity < 1 ||
        table_positions < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_qkv_w4: needs 1 <= B <= 64, K % 128 == 0, head_dim % 16 == 0, splits >= 1 (and scratch when splits > 1)");
    if (misaligned4(Wt, scales)) return lfail("fvhd_op_dec_qkv_w4: codes and scales must be aligned to 4 bytes");
    DecGemmArgs a = dec_qkv_args(x, B, K, norm_w, eps, Wt, nullptr, bias, q_out, pos, table, table_positions, rope_theta, k_cache, v_cache, capacity, length,
                                 n_heads, n_kv_heads, head_dim, partial, counters, splits);
    a.wblk = (const unsigned char*)scales;
    return dec_run((hipStream_t)st, "fvhd_op_dec_qkv_w4", a);
}

int fvhd_op_dec_lm_argmax_w4(fvhd_stream_t st, const void* x, int B, const float* norm_w, float eps, const void* Wt, const void* scales, int V, int K,
                             float* logits, int64_t* ids_out, float* scratch_v, int* scratch_i)
{
    if (!x || !Wt || !scales || !ids_out || !scratch_v || !scratch_i) return lfail("fvhd_op_dec_lm_argmax_w4: NULL pointer");
    if (B < 1 || B > 64 || V < 16 || V % 16 || K < 128 || K % 128) return lfail("fvhd_op_dec_lm_argmax_w4: needs 1 <= B <= 64, V % 16 == 0, K % 128 == 0");
    if (misaligned4(Wt, scales)) return lfail("fvhd_op_dec_lm_argmax_w4: codes and scales must be aligned to 4 bytes");
    DecGemmArgs a = dec_argmax_args(x, B, norm_w, eps, Wt, nullptr, V, K, logits, scratch_v, scratch_i);
    a.wblk = (const unsigned char*)scales;
    return dec_run((hipStream_t)st, "fvhd_op_dec_lm_argmax_w4", a, ids_out);
}

int fvhd_op_quantize_mxfp4(fvhd_stream_t st, const void* W, int N, int K, void* codes, void* scales)
{
    if (!W || !codes || !scales) return lfail("fvhd_op_quantize_mxfp4: NULL pointer");
    if (N < 1 || K < 32 || K % 32) return lfail("fvhd_op_quantize_mxfp4: needs N >= 1, K >= 32 and K % 32 == 0");
    if (((uintptr_t)W & 15) || ((uintptr_t)codes & 3)) return lfail("fvhd_op_quantize_mxfp4: W must be aligned to 16 bytes, codes to 4");
    return lret("fvhd_op_quantize_mxfp4", fvhd_launch_quantize_mxfp4((hipStream_t)st, W, N, K, codes, K / 2, scales, K / 32, 0));
}

// the layout kernel on its own (tests): mode 0: packed codes + scales -> bf16 [N][K] (the prefill's dequantise); 1: packed -> plain codes;
// 2: plain -> packed codes.  K % 128 == 0.
int fvhd_op_w4_unpack(fvhd_stream_t st, const void* src, const void* scales, void* dst, int N, int K, int mode)
{
    if (!src || !dst || (mode == 0 && !scales)) return lfail("fvhd_op_w4_unpack: NULL pointer");
    if (N < 1 || K < 128 || K % 128 || mode < 0 || mode > 2) return lfail("fvhd_op_w4_unpack: needs N >= 1, K % 128 == 0 and mode in 0 .. 2");
    if (((uintptr_t)src & 3) || ((uintptr_t)dst & 15)) return lfail("fvhd_op_w4_unpack: src must be aligned to 4 bytes, dst to 16");
    return lret("fvhd_op_w4_unpack", fvhd_launch_w4_unpack((hipStream_t)st, src, scales, dst, N, K, mode));
}

int fvhd_op_quantize_e4m3(fvhd_stream_t st, const void* W, int N, int K, void* codes, float* scale)
{
    if (!W || !codes || !scale) return lfail("fvhd_op_quantize_e4m3: NULL pointer");
    if (N < 1 || K < 8 || K % 8) return lfail("fvhd_op_quantize_e4m3: needs N >= 1, K >= 8 and K % 8 == 0");
    return lret("fvhd_op_quantize_e4m3", fvhd_launch_quantize_e4m3((hipStream_t)st, W, N, K, codes, K, scale, 1, 0));
}

// the sampler on its own: a process-wide workspace, allocated (and its counters zeroed) on first use - eager calls only
static int op_sample(const char* who, fvhd_stream_t st, DecSampleArgs& a)
{
    const std::string w(who);
    if (!a.logits || !a.ids_out) return lfail(w + ": NULL pointer");
    const int bmax = a.info8 && !a.seq_rows ? 64 : 16;                         // fvhd_op_dec_sample_warpers takes the wide batch too
    if (a.B < 1 || a.B > bmax || a.V < 1) return lfail(w + ": needs 1 <= B <= " + std::to_string(bmax) + " and V >= 1");
    if (const char* e = sampling_error(a.temperature, a.top_k, a.top_p)) return lfail(w + ": " + e);
    const std::string we = warpers_error(a.min_p, a.typical_p, a.epsilon_cutoff, a.eta_cutoff);
    if (!we.empty()) return lfail(w + ": " + we);
    static char* ws[64] = {};
    int dev = 0;
    hipError_t he = hipGetDevice(&dev);
    if (he != hipSuccess) return lhip("hipGetDevice", he);
    if (dev < 0 || dev >= 64) return lfail(w + ": device index out of range");
    if (!ws[dev]) {
        const size_t bytes = fvhd_dec_sample_ws_bytes();
        if ((he = hipMalloc((void**)&ws[dev], bytes)) != hipSuccess) { ws[dev] = nullptr; return lhip("hipMalloc(sampler workspace)", he); }
        if ((he = hipMemset(ws[dev], 0, bytes)) != hipSuccess) return lhip("hipMemset(sampler workspace)", he);
    }
    return lret(who, fvhd_launch_dec_sample((hipStream_t)st, &a, ws[dev]));
}

int fvhd_op_dec_sample(fvhd_stream_t st, const float* logits, int B, int V, float temperature, int top_k, float top_p, unsigned long long seed, int n,
                       const float* u_override, int64_t* ids, float* info)
{
    DecSampleArgs a;
    a.logits = logits; a.B = B; a.V = V; a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.n_add = n;
    a.u_override = u_override; a.ids_out = ids; a.info = info;
    return op_sample("fvhd_op_dec_sample", st, a);
}

// the T rows of ONE sequence (the verify step's mode): row r draws with the counter (seq_row, n0 + r).  state_last / state_position /
// state_length go into the launch where a decode step passes last ids, positions and the length to advance: the mode must leave them alone
int fvhd_op_dec_sample_rows(fvhd_stream_t st, const float* logits, int T, int V, float temperature, int top_k, float top_p, unsigned long long seed,
                            int seq_row, int n0, const float* u_override, int64_t* ids, float* info, int64_t* state_last, int64_t* state_position,
                            int* state_length)
{
    if (seq_row < 0 || n0 < 0) return lfail("fvhd_op_dec_sample_rows: seq_row and n0 must be >= 0");
    DecSampleArgs a;
    a.logits = logits; a.B = T; a.V = V; a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.n_add = n0;
    a.u_override = u_override; a.ids_out = ids; a.info = info; a.seq_rows = 1; a.seq_row = seq_row;
    a.last = state_last; a.posv = state_position; a.len_advance = state_length;
    return op_sample("fvhd_op_dec_sample_rows", st, a);
}

int fvhd_op_dec_sample_warpers(fvhd_stream_t st, const float* logits, int B, int V, float temperature, int top_k, float top_p, float min_p,
                               float typical_p, float epsilon_cutoff, float eta_cutoff, unsigned long long seed, int seq_rows, int seq_row, int n,
                               const float* u_override, int64_t* ids, float* info)
{
    if (!info) return lfail("fvhd_op_dec_sample_warpers: NULL pointer");
    if (seq_row < 0 || n < 0) return lfail("fvhd_op_dec_sample_warpers: seq_row and n must be >= 0");
    DecSampleArgs a;
    a.logits = logits; a.B = B; a.V = V; a.temperature = temperature; a.top_k = top_k; a.top_p = top_p; a.seed = seed; a.n_add = n;
    a.min_p = min_p; a.typical_p = typical_p; a.epsilon_cutoff = epsilon_cutoff; a.eta_cutoff = eta_cutoff;
    a.u_override = u_override; a.ids_out = ids; a.info8 = info; a.seq_rows = seq_rows != 0; a.seq_row = seq_rows ? seq_row : 0;
    return op_sample("fvhd_op_dec_sample_warpers", st, a);
}

int fvhd_op_dec_logprobs(fvhd_stream_t st, const float* logits, const int64_t* ids, int B, int V, int top_n, float* token_logprob_out,
                         int64_t* top_ids_out, float* top_logprobs_out, void* scratch, size_t scratch_bytes)
{
    if (!logits || !ids || !token_logprob_out || !scratch) return lfail("fvhd_op_dec_logprobs: NULL pointer");
    if (B < 1 || B > 64 || V < 1) return lfail("fvhd_op_dec_logprobs: needs 1 <= B <= 64 and V >= 1");
    if (top_n < 0 || top_n > 16) return lfail("fvhd_op_dec_logprobs: top_n must be in [0, 16] (got " + std::to_string(top_n) + ")");
    if (top_n > V) return lfail("fvhd_op_dec_logprobs: top_n = " + std::to_string(top_n) + " exceeds V = " + std::to_string(V));
    if (top_n && (!top_ids_out || !top_logprobs_out)) return lfail("fvhd_op_dec_logprobs: top_n > 0 needs top_ids_out and top_logprobs_out");
    if (scratch_bytes < fvhd_dec_logprobs_scratch_bytes(B, V, top_n))
        return lfail("fvhd_op_dec_logprobs: scratch_bytes = " + std::to_string(scratch_bytes) + " is below fvhd_dec_logprobs_scratch_bytes(B, V, top_n) = " +
                     std::to_string(fvhd_dec_logprobs_scratch_bytes(B, V, top_n)));
    return lret("fvhd_op_dec_logprobs", fvhd_launch_dec_logprobs((hipStream_t)st, logits, ids, B, V, top_n, token_logprob_out, top_ids_out, top_logprobs_out,
                                                                 scratch, nullptr));
}

// the constraint's launches on their own: the advance when fed_ids is given, then the mask
int fvhd_op_dec_constrain(fvhd_stream_t st, float* logits, int B, int V, const int32_t* offsets, const int32_t* tokens, const int32_t* targets, int n_states,
                          int32_t* states, int32_t* flags, const int64_t* fed_ids)
{
    if (!logits || !offsets || !tokens || !targets || !states || !flags) return lfail("fvhd_op_dec_constrain: NULL pointer");
    if (B < 1 || B > 64 || V < 1) return lfail("fvhd_op_dec_constrain: needs 1 <= B <= 64 and V >= 1");
    if (n_states < 1) return lfail("fvhd_op_dec_constrain: needs n_states >= 1");
    if ((uintptr_t)logits & 3) return lfail("fvhd_op_dec_constrain: logits must be aligned to 4 bytes");
    DecConstrainArgs a;
    a.logits = logits; a.B = B; a.V = V; a.offsets = offsets; a.tokens = tokens; a.targets = targets; a.n_states = n_states; a.states = states;
    a.flags = flags; a.tok = fed_ids;
    return lret("fvhd_op_dec_constrain", fvhd_launch_dec_constrain((hipStream_t)st, &a));
}

// classifier-free guidance on its own: the statistics launch and the apply launch (llm_guidance.hip)
int fvhd_op_dec_guidance(fvhd_stream_t st, float* logits, int G, int V, float scale, void* scratch, size_t scratch_bytes)
{
    if (!logits || !scratch) return lfail("fvhd_op_dec_guidance: NULL pointer");
    if (G < 1 || G > 32 || V < 1) return lfail("fvhd_op_dec_guidance: needs 1 <= G <= 32 pairs and V >= 1");
    if (!std::isfinite(scale)) return lfail("fvhd_op_dec_guidance: scale must be finite");
    if ((uintptr_t)logits & 3) return lfail("fvhd_op_dec_guidance: logits must be aligned to 4 bytes");
    if (scratch_bytes < fvhd_dec_guidance_scratch_bytes(G, V))
        return lfail("fvhd_op_dec_guidance: scratch_bytes = " + std::to_string(scratch_bytes) + " is below fvhd_dec_guidance_scratch_bytes(G, V) = " +
                     std::to_string(fvhd_dec_guidance_scratch_bytes(G, V)));
    return lret("fvhd_op_dec_guidance", fvhd_launch_dec_guidance((hipStream_t)st, logits, G, V, scale, scratch, nullptr));
}

// process-wide scratch of a single op, allocated / grown on demand - eager calls only
static int op_scratch(const char* who, char* (&buf)[64], size_t (&cap)[64], size_t need, char** out)
{
    int dev = 0;
    hipError_t he = hipGetDevice(&dev);
    if (he != hipSuccess) return lhip("hipGetDevice", he);
    if (dev < 0 || dev >= 64) return lfail(std::string(who) + ": device index out of range");
    if (need > cap[dev]) {
        if (buf[dev]) (void)hipFree(buf[dev]);                      // (synchronises: no earlier launch still uses it)
        buf[dev] = nullptr;
        cap[dev] = 0;
        if ((he = hipMalloc((void**)&buf[dev], need)) != hipSuccess) { buf[dev] = nullptr; return lhip((std::string(who) + ": hipMalloc(scratch)").c_str(), he); }
        cap[dev] = need;
    }
    *out = buf[dev];
    return 0;
}

static int op_beam_topk(const char* who, fvhd_stream_t st, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V,
                        int prenorm, float* cand_scores, int64_t* cand_index)
{
    const std::string w(who);
    if (!logits || !beam_scores || !cand_scores || !cand_index) return lfail(w + ": NULL pointer");
    if (!fvhd_dec_beam_topk_supported(groups, num_beams, keep, V) || ((uintptr_t)logits & 15))
        return lfail(w + ": needs groups >= 1, 2 <= num_beams <= 16, 1 <= keep <= 64, keep <= V, groups * num_beams <= 64, V % 16 == 0, "
                     "V <= 262144 and logits aligned to 16 bytes");
    static char* buf[64] = {};
    static size_t cap[64] = {};
    char* ws = nullptr;
    if (int e = op_scratch(who, buf, cap, fvhd_dec_beam_topk_ws_bytes(), &ws)) return e;
    return lret(who, fvhd_launch_dec_beam_topk_mode((hipStream_t)st, logits, beam_scores, groups, num_beams, keep, V, prenorm, cand_scores, cand_index, ws));
}

int fvhd_op_dec_beam_topk(fvhd_stream_t st, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V, float* cand_scores,
                          int64_t* cand_index)
{
    return op_beam_topk("fvhd_op_dec_beam_topk", st, logits, beam_scores, groups, num_beams, keep, V, 0, cand_scores, cand_index);
}

int fvhd_op_dec_beam_topk_pre(fvhd_stream_t st, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V, float* cand_scores,
                              int64_t* cand_index)
{
    return op_beam_topk("fvhd_op_dec_beam_topk_pre", st, logits, beam_scores, groups, num_beams, keep, V, 1, cand_scores, cand_index);
}

// beam-search sampling on its own: a process-wide workspace, allocated and zeroed (the sampler's arrival counters) on first use - eager calls only
static int op_beam_sample(const char* who, fvhd_stream_t st, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V,
                          float temperature, int top_k, float top_p, int min_keep, unsigned long long seed, int n, const float* noise_override, float* noise_out,
                          float* info, float* cand_scores, int64_t* cand_index, int prenorm)
{
    const std::string w(who);
    if (!logits || !beam_scores || !cand_scores || !cand_index) return lfail(w + ": NULL pointer");
    if (!fvhd_dec_beam_topk_supported(groups, num_beams, keep, V) || ((uintptr_t)logits & 15))
        return lfail(w + ": needs groups >= 1, 2 <= num_beams <= 16, 1 <= keep <= 64, keep <= V, groups * num_beams <= 64, V % 16 == 0, "
                     "V <= 262144 and logits aligned to 16 bytes");
    if (const char* e = sampling_error(temperature, top_k, top_p)) return lfail(w + ": " + e);
    if (min_keep < 1 || min_keep > keep)
        return lfail(w + ": min_keep must be in [1, keep] (got " + std::to_string(min_keep) + " with keep = " + std::to_string(keep) + ")");
    if (n < 0) return lfail(w + ": n must be >= 0");
    if (((uintptr_t)noise_override & 15) || ((uintptr_t)noise_out & 15)) return lfail(w + ": noise_override and noise_out must be aligned to 16 bytes");
    static char* ws[64] = {};
    int dev = 0;
    hipError_t he = hipGetDevice(&dev);
    if (he != hipSuccess) return lhip("hipGetDevice", he);
    if (dev < 0 || dev >= 64) return lfail(w + ": device index out of range");
    if (!ws[dev]) {
        const size_t bytes = fvhd_dec_beam_sample_ws_bytes();
        if ((he = hipMalloc((void**)&ws[dev], bytes)) != hipSuccess) { ws[dev] = nullptr; return lhip("hipMalloc(beam sampling workspace)", he); }
        if ((he = hipMemset(ws[dev], 0, bytes)) != hipSuccess) return lhip("hipMemset(beam sampling workspace)", he);
    }
    DecBeamSampleArgs a;
    a.logits = logits; a.scores = beam_scores; a.G = groups; a.K = num_beams; a.keep = keep; a.V = V; a.temperature = temperature; a.top_k = top_k;
    a.top_p = top_p; a.min_keep = min_keep; a.seed = seed; a.n_add = n; a.noise_override = noise_override; a.noise_out = noise_out; a.info = info;
    a.out_v = cand_scores; a.out_i = cand_index; a.prenorm = prenorm;
    return lret(who, fvhd_launch_dec_beam_sample((hipStream_t)st, &a, ws[dev]));
}

int fvhd_op_dec_beam_sample(fvhd_stream_t st, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V, float temperature,
                            int top_k, float top_p, int min_keep, unsigned long long seed, int n, const float* noise_override, float* noise_out, float* info,
                            float* cand_scores, int64_t* cand_index)
{
    return op_beam_sample("fvhd_op_dec_beam_sample", st, logits, beam_scores, groups, num_beams, keep, V, temperature, top_k, top_p, min_keep, seed, n,
                          noise_override, noise_out, info, cand_scores, cand_index, 0);
}

int fvhd_op_dec_beam_sample_pre(fvhd_stream_t st, const float* logits, const float* beam_scores, int groups, int num_beams, int keep, int V, float temperature,
                                int top_k, float top_p, int min_keep, unsigned long long seed, int n, const float* noise_override, float* noise_out, float* info,
                                float* cand_scores, int64_t* cand_index)
{
    return op_beam_sample("fvhd_op_dec_beam_sample_pre", st, logits, beam_scores, groups, num_beams, keep, V, temperature, top_k, top_p, min_keep, seed, n,
                          noise_override, noise_out, info, cand_scores, cand_index, 1);
}

// the row normalisation on its own: stats_out NULL, or fp32 [rows][2] = the (M, L) subtracted from every row
int fvhd_op_dec_beam_norm(fvhd_stream_t st, float* logits, int rows, int V, float* stats_out)
{
    if (!logits) return lfail("fvhd_op_dec_beam_norm: NULL pointer");
    if (!fvhd_dec_beam_norm_supported(rows, V) || ((uintptr_t)logits & 3))
        return lfail("fvhd_op_dec_beam_norm: needs 1 <= rows <= 64, 1 <= V <= 262144 and logits aligned to 4 bytes");
    static char* buf[64] = {};
    static size_t cap[64] = {};
    char* ws = nullptr;
    if (int e = op_scratch("fvhd_op_dec_beam_norm", buf, cap, fvhd_dec_beam_norm_ws_bytes(), &ws)) return e;
    return lret("fvhd_op_dec_beam_norm", fvhd_launch_dec_beam_norm((hipStream_t)st, logits, rows, V, ws, stats_out, nullptr));
}

// the history / state reorder on its own: history NULL (no histories move) or int32 [batch][capacity] entries as the step keeps them, seen
// uint32 [batch][ceil(V / 32)], count int32 [batch]; states NULL (no states move) or int32 [batch] with flags int32 [batch]
int fvhd_op_dec_hist_gather(fvhd_stream_t st, int32_t* history, uint32_t* seen, int32_t* count, int32_t* states, int32_t* flags, const int64_t* src_rows,
                            int batch, int rows_in, int rows_out, int capacity, int V, int* status)
{
    if (!src_rows || !status) return lfail("fvhd_op_dec_hist_gather: NULL pointer");
    if (batch < 1 || batch > 64 || rows_in < 1 || rows_in > batch || rows_out < 1 || rows_out > batch || capacity < 1 || V < 1 ||
        (history && (!seen || !count)) || (states && !flags))
        return lfail("fvhd_op_dec_hist_gather: needs 1 <= rows_in, rows_out <= batch <= 64, capacity >= 1, V >= 1, seen and count with a history, flags "
                     "with states");
    static char* buf[64] = {};
    static size_t cap[64] = {};
    char* ws = nullptr;
    if (int e = op_scratch("fvhd_op_dec_hist_gather", buf, cap, fvhd_dec_hist_gather_ws_bytes(batch, capacity, V), &ws)) return e;
    DecHistGatherArgs a;
    a.hist = history; a.seen = seen; a.count = count; a.states = states; a.flags = flags; a.src = src_rows; a.rows_in = rows_in; a.rows_out = rows_out;
    a.batch = batch; a.cap = capacity; a.V = V; a.status = status; a.ws = ws;
    return lret("fvhd_op_dec_hist_gather", fvhd_launch_dec_hist_gather((hipStream_t)st, &a));
}

int fvhd_op_dec_cache_gather(fvhd_stream_t st, void* k_cache, void* v_cache, uint8_t* key_valid, int64_t* positions, const int64_t* src_rows, int n_layers,
                             int batch, int rows_in, int rows_out, int n_kv_heads, int head_dim, int capacity, const int* length, int* status)
{
    if (!k_cache || !v_cache || !key_valid || !positions || !src_rows || !length || !status) return lfail("fvhd_op_dec_cache_gather: NULL pointer");
    if (n_layers < 1 || batch < 1 || batch > 64 || rows_in < 1 || rows_in > batch || rows_out < 1 || rows_out > batch || n_kv_heads < 1 || head_dim < 8 ||
        head_dim % 8 || capacity < 1 || ((uintptr_t)k_cache & 15) || ((uintptr_t)v_cache & 15))
        return lfail("fvhd_op_dec_cache_gather: needs n_layers >= 1, 1 <= rows_in, rows_out <= batch <= 64, head_dim % 8 == 0, capacity >= 1 and caches "
                     "aligned to 16 bytes");
    static char* buf[64] = {};
    static size_t cap[64] = {};
    char* ws = nullptr;
    if (int e = op_scratch("fvhd_op_dec_cache_gather", buf, cap, fvhd_dec_cache_gather_ws_bytes(batch, n_kv_heads, head_dim, capacity), &ws)) return e;
    DecCacheGatherArgs a;
    a.kc = (char*)k_cache; a.vc = (char*)v_cache; a.layers = n_layers; a.batch = batch; a.mask = key_valid; a.posv = positions; a.src = src_rows;
    a.rows_in = rows_in; a.rows_out = rows_out; a.nkv = n_kv_heads; a.hd = head_dim; a.cap = capacity; a.len = length; a.status = status; a.ws = ws;
    return lret("fvhd_op_dec_cache_gather", fvhd_launch_dec_cache_gather((hipStream_t)st, &a));
}

// the logits processors on their own: the history's first-occurrence records and bitmap are built on the device from the plain tokens
// (process-wide scratch, grown on demand - eager calls only), then the step's kernel runs on them
int fvhd_op_dec_logits_process(fvhd_stream_t st, float* logits, int B, int V, const int32_t* history, int capacity, int g, float repetition_penalty,
                               int no_repeat_ngram_size, int min_new_tokens, const int32_t* host_eos_ids, int n_eos, const int32_t* host_suppress_ids,
                               int n_suppress)
{
    if (!logits || !history) return lfail("fvhd_op_dec_logits_process: NULL pointer");
    if (B < 1 || B > 64 || V < 1 || capacity < 1 || g < 0 || g > capacity)
        return lfail("fvhd_op_dec_logits_process: needs 1 <= B <= 64, V >= 1, capacity >= 1 and 0 <= g <= capacity");
    const std::string err = processors_error(repetition_penalty, no_repeat_ngram_size, min_new_tokens, host_eos_ids, n_eos, host_suppress_ids, n_suppress, V);
    if (!err.empty()) return lfail("fvhd_op_dec_logits_process: " + err);
    static char* buf[64] = {};
    static size_t cap[64] = {};
    const size_t hist_bytes = ((size_t)B * capacity * 4 + 255) & ~(size_t)255, seen_bytes = ((size_t)B * ((V + 31) / 32) * 4 + 255) & ~(size_t)255;
    char* ws = nullptr;
    if (int e = op_scratch("fvhd_op_dec_logits_process", buf, cap, hist_bytes + seen_bytes + (kMaxEos + kMaxSuppress) * 4, &ws)) return e;
    hipStream_t s = (hipStream_t)st;
    DecLogitsArgs a;
    a.logits = logits; a.B = B; a.V = V; a.hist = (int*)ws; a.cap = capacity; a.seen = (unsigned*)(ws + hist_bytes); a.g_fixed = g;
    a.penalty = repetition_penalty; a.ngram = no_repeat_ngram_size; a.min_new = n_eos ? min_new_tokens : 0;
    int* lists = (int*)(ws + hist_bytes + seen_bytes);
    a.eos = lists; a.n_eos = n_eos; a.sup = lists + kMaxEos; a.n_sup = n_suppress;
    hipError_t he = hipMemsetAsync(a.seen, 0, seen_bytes, s);
    if (he == hipSuccess && n_eos) he = hipMemcpyAsync(lists, host_eos_ids, (size_t)n_eos * 4, hipMemcpyHostToDevice, s);
    if (he == hipSuccess && n_suppress) he = hipMemcpyAsync(lists + kMaxEos, host_suppress_ids, (size_t)n_suppress * 4, hipMemcpyHostToDevice, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);          // the host lists are the caller's again
    if (he != hipSuccess) return lhip("fvhd_op_dec_logits_process: list copy", he);
    if (int e = fvhd_launch_dec_logits_history(s, history, a.hist, a.seen, B, V, capacity, g)) return lhip("fvhd_op_dec_logits_process (history)", (hipError_t)e);
    return lret("fvhd_op_dec_logits_process", fvhd_launch_dec_logits_process(s, &a));
}

// ---- single ops of the verify step (llm_spec.hip) ----
int fvhd_op_dec_attention_multi(fvhd_stream_t st, const void* q, void* k_cache, void* v_cache, const void* k_staged, const void* v_staged,
                                const uint8_t* key_valid, void* out, int T, int n_heads, int n_kv_heads, int head_dim, int capacity, const int* length,
                                float* partial, int* counters, int splits)
{
    if (!q || !k_cache || !v_cache || !k_staged || !v_staged || !key_valid || !out || !length) return lfail("fvhd_op_dec_attention_multi: NULL pointer");
    if (T < 2 || T > 16) return lfail("fvhd_op_dec_attention_multi: needs 2 <= T <= 16");
    if (head_dim != 64 && head_dim != 128) return lfail("fvhd_op_dec_attention_multi: head_dim must be 64 or 128");
    if (n_heads < 1 || n_kv_heads < 1 || n_heads % n_kv_heads) return lfail("fvhd_op_dec_attention_multi: n_heads must be a multiple of n_kv_heads");
    if (splits < 1 || capacity < 1 || (splits > 1 && (!partial || !counters)))
        return lfail("fvhd_op_dec_attention_multi: splits >= 1 (and scratch when splits > 1)");
    const int chunk = ((capacity + splits - 1) / splits + 63) / 64 * 64, S = (capacity + chunk - 1) / chunk;
    return lret("fvhd_op_dec_attention_multi", fvhd_launch_spec_attention((hipStream_t)st, q, k_cache, v_cache, k_staged, v_staged, key_valid, out, T, n_heads,
                                                                          n_kv_heads, head_dim, capacity, length, S, chunk, partial, counters, nullptr));
}

int fvhd_op_dec_lookup_draft(fvhd_stream_t st, const int32_t* tokens, const int* length, int max_ngram, int K, int64_t* draft_out)
{
    if (!tokens || !length || !draft_out) return lfail("fvhd_op_dec_lookup_draft: NULL pointer");
    if (max_ngram < 1 || max_ngram > 16 || K < 1 || K > 15) return lfail("fvhd_op_dec_lookup_draft: needs 1 <= max_ngram <= 16 and 1 <= K <= 15");
    return lret("fvhd_op_dec_lookup_draft", fvhd_launch_spec_draft((hipStream_t)st, tokens, length, max_ngram, K, draft_out, nullptr, nullptr, nullptr));
}

int fvhd_op_dec_lookup_accept(fvhd_stream_t st, const int64_t* draft, const int64_t* ids, int T, int32_t* words, int32_t* tokens, int tokens_capacity,
                              int64_t* out, int out_capacity, int32_t* emitted, int64_t* last_id, int64_t* position, int* length, uint8_t* key_valid,
                              int capacity)
{
    if (!draft || !ids || !last_id || !position || !length || !key_valid) return lfail("fvhd_op_dec_lookup_accept: NULL pointer");
    if (T < 2 || T > 16 || capacity < 1 || tokens_capacity < 0 || out_capacity < 0) return lfail("fvhd_op_dec_lookup_accept: needs 2 <= T <= 16 and capacity >= 1");
    SpecAcceptArgs a;
    a.draft = draft; a.ids = ids; a.T = T; a.words = words; a.seq = tokens; a.seq_cap = tokens_capacity; a.out = out; a.out_cap = out_capacity;
    a.emitted = emitted; a.last = last_id; a.posv = position; a.len = length; a.key_valid = key_valid; a.cap = capacity;
    return lret("fvhd_op_dec_lookup_accept", fvhd_launch_spec_accept((hipStream_t)st, &a));
}

}  // extern "C"
