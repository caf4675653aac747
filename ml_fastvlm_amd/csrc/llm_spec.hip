// Speculative verification for the Qwen2 decode (include/fvhd.h "LLM speculative verification"): the last chosen token and T - 1 drafted
// tokens of ONE sequence run as the T rows of one step, and the longest prefix of drafts the model itself would have chosen is kept.
//   spec_draft_kernel      prompt lookup: the drafts are what followed the latest earlier occurrence of the token buffer's last n-gram
//   spec_embed_kernel      the capacity check for T slots, the T token rows, per-row positions, mask bytes [*len, *len + T)
//   spec_attention_kernel  T queries over the one cache row: query t sees keys [0, *len + t + 1); the T new k / v rows come from the
//                          staging rows the q|k|v launch wrote and are moved into their cache slots by one workgroup per kv head
//   spec_accept_kernel     the accepted prefix, the cut at EOS / at the token limit, the state advance, the mask bytes cleared again
//   spec_begin_kernel      seeds the token buffer and the counters of a lookup generation
// The GEMMs of the step are the decode's own launches at B = T (llm_decode.hip, llm_w8.hip): a row is one MFMA column there, so its bits
// do not depend on the other rows.  spec_attention_kernel keeps dec_attention_kernel's arithmetic per query - the key slices, the 64-key
// blocks a wave takes, the online-softmax updates, the j order of P.V, the wave and slice combines - so row t of a verify step has the
// bits of the plain step at length *len + t + 1.
#include "fvhd_common.h"
#include "launchers.h"
#include "split_handoff.h"  // arrive_last
#include "w4_layout.h"  // w4_pos, w4_scale, fp4x8_to_bf8
#include "w8_layout.h"  // w8_pos, e4m3x8_to_f32

namespace {

typedef unsigned char u8;
}  // namespace

// ---------------------------------------------------------------------------------------------------
// One workgroup.  seq[0 .. *seq_len) = the lookup ids, then every generated token.  For n = max_ngram .. 1 (n < length) the suffix is the
// last n tokens; the LARGEST i with seq[i .. i + n) == suffix and i + n < length wins, and the drafts are seq[i + n ..], cut at the
// buffer's end and at the first negative id.  A negative id never matches.  Missing drafts = the last token.  In the step (gate given) it
// also sets the step's gate word: *status, or 1 once the generation has finished.
__global__ __launch_bounds__(256) void spec_draft_kernel(const int* __restrict__ seq, const int* seq_len, int max_ngram, int K, int64_t* __restrict__ draft,
                                                         const int* status, const int* words, int* gate)
{
    __shared__ int best[256];
    __shared__ int suf[16];
    const int tid = threadIdx.x;
    if (gate) {
        const int g = (*status != 0 || words[SPEC_W_FINISHED] != 0) ? 1 : 0;
        if (tid == 0) *gate = g;
        if (g) return;
    }
    const int n_seq = *seq_len;
    if (n_seq < 1) {
        for (int k = tid; k < K; k += 256) draft[k] = 0;
        return;
    }
    int found = -1, fn = 0;
    for (int n = min(max_ngram, n_seq - 1); n >= 1; --n) {
        __syncthreads();
        if (tid < n) suf[tid] = seq[n_seq - n + tid];
        __syncthreads();
        bool ok = true;
        for (int k = 0; k < n; ++k) ok = ok && suf[k] >= 0;
        int mine = -1;
        if (ok)
            for (int i = tid; i + n < n_seq; i += 256) {
                bool eq = true;
                for (int k = 0; k < n; ++k) eq = eq && seq[i + k] == suf[k];
                if (eq) mine = i;                                // ascending i: the last hit of this thread is its largest
            }
        best[tid] = mine;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) best[tid] = max(best[tid], best[tid + o]);
            __syncthreads();
        }
        if (best[0] >= 0) { found = best[0]; fn = n; break; }    // (uniform: every thread reads the same word)
    }
    if (tid == 0) {
        const int fill = seq[n_seq - 1];
        int k = 0;
        if (found >= 0)
            for (int i = found + fn; k < K && i < n_seq && seq[i] >= 0; ++i) draft[k++] = seq[i];
        for (; k < K; ++k) draft[k] = fill;
    }
}

// ---------------------------------------------------------------------------------------------------
// The step's token rows.  Workgroup = row t: row 0 = the token the previous step chose, row t = draft[t - 1].  Nothing is written when the
// T slots do not fit (error 1, sticky); an id outside [0, V) is error 2.  scale != NULL: the table holds packed e4m3 lm_head rows;
// wblk != NULL: packed MXFP4 lm_head rows and these block scales (w4_layout.h).
__global__ __launch_bounds__(256) void spec_embed_kernel(const int64_t* __restrict__ draft, const int64_t* __restrict__ last, const void* __restrict__ table,
                                                         const float* __restrict__ scale, const u8* __restrict__ wblk, int V, int H, bf16* __restrict__ h,
                                                         unsigned char* __restrict__ key_valid, int T, int cap, const int* len, const int64_t* posv, int64_t* __restrict__ pos, int* status,
                                                         int* status_host, int* gate)
{
    if (*gate) return;
    const int t = blockIdx.x;
    const int L = *len;
    if (L < 0 || L + T > cap) {
        if (t == 0 && threadIdx.x == 0) { *gate = 1; *status = 1; *status_host = 1; }      // (a bare verify step: gate IS status)
        return;
    }
    const int64_t id = t == 0 ? last[0] : draft[t - 1];
    if (id < 0 || id >= V) {
        if (threadIdx.x == 0) { *gate = 1; *status = 2; *status_host = 2; }
        return;
    }
    if (scale) {
        const u8* src = (const u8*)table + (size_t)id * H;
        const float s = scale[id];
        for (int c = threadIdx.x * 8; c < H; c += 256 * 8) {
            const u32x2 q = *(const u32x2*)(src + w8_pos(c));
            f32x8 v = e4m3x8_to_f32(q[0], q[1]);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] *= s;
            *(bf16x8*)(h + (size_t)t * H + c) = f32_to_bf8(v);
        }
    } else if (wblk) {
        const u8* src = (const u8*)table + (size_t)id * (H / 2);
        const u8* sr = wblk + (size_t)id * (H / 32);
        for (int c = threadIdx.x * 8; c < H; c += 256 * 8)
            *(bf16x8*)(h + (size_t)t * H + c) = fp4x8_to_bf8(*(const uint32_t*)(src + w4_pos(c)), w4_scale(sr[c >> 5]));
    } else {
        const bf16* src = (const bf16*)table + (size_t)id * H;
        for (int c = threadIdx.x * 8; c < H; c += 256 * 8) *(u32x4*)(h + (size_t)t * H + c) = *(const u32x4*)(src + c);
    }
    if (threadIdx.x == 0) {
        key_valid[L + t] = 1;
        pos[t] = posv[0] + t;
    }
}

// ---------------------------------------------------------------------------------------------------
// q [T][nh * HD]; kc / vc: cache row 0 [nkv][cap][HD]; ks / vs: the staged new rows [T][nkv][HD] (key *len + t); key_valid [cap];
// out [T][nh * HD].  Workgroup = (head, key slice) with 16 waves: wave = (lw, qg), lw = the wave of dec_attention_kernel whose 64-key
// blocks it takes, qg = its queries t = qg, qg + 4, qg + 8, qg + 12.  A key block's K row (one per lane) and its V rows are loaded once
// per wave and used for that wave's queries; per query the arithmetic is dec_attention_kernel's at Lk = *len + t + 1.  Partials
// [T][nh][S][HD + 2], one counter per head.
template <int HD>
__global__ __launch_bounds__(1024) void spec_attention_kernel(const bf16* __restrict__ q, bf16* __restrict__ kc, bf16* __restrict__ vc,
                                                              const bf16* __restrict__ ks, const bf16* __restrict__ vs,
                                                              const unsigned char* __restrict__ key_valid, bf16* __restrict__ out, int T, int nh, int nkv,
                                                              int cap, const int* len, int S, int chunk, float* part, int* cnt, const int* status, float scale)
{
    constexpr int DPL = HD / 64, QW = 4;
    if (status && *status) return;
    extern __shared__ float sh[];
    float* qs = sh;                                              // [T][HD]
    float* ws = sh + T * HD;                                     // [4 lw][T][HD + 2]: m, l, o[HD]
    int* flag = (int*)(ws + 4 * T * (HD + 2));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lw = wave & 3, qg = wave >> 2;
    const int h = blockIdx.x / S, s = blockIdx.x % S, kvh = h / (nh / nkv);
    const int L0 = *len;
    if (L0 < 0 || L0 + T > cap) return;                          // (the step's embed has set the error word; the single op: nothing to do)
    const int k0 = s * chunk;
    for (int i = tid; i < T * HD; i += 1024) qs[i] = (float)q[(size_t)(i / HD) * nh * HD + h * HD + i % HD];
    __syncthreads();
    bf16* kb_ = kc + (size_t)kvh * cap * HD;
    bf16* vb_ = vc + (size_t)kvh * cap * HD;
    const bf16* ksb = ks + (size_t)kvh * HD;                     // staged row t: + t * nkv * HD
    const bf16* vsb = vs + (size_t)kvh * HD;
    float m[QW], l[QW], o[QW][DPL], p[QW];
    int k1[QW];
    int k1w = 0;                                                 // the end of this wave's keys: its last query's
#pragma unroll
    for (int u = 0; u < QW; ++u) {
        const int t = qg + 4 * u;
        m[u] = -INFINITY; l[u] = 0.f;
#pragma unroll
        for (int i = 0; i < DPL; ++i) o[u][i] = 0.f;
        k1[u] = t < T ? min(k0 + chunk, min(L0 + t + 1, cap)) : 0;
        k1w = max(k1w, k1[u]);
    }
    for (int kb = k0 + lw * 64; kb < k1w; kb += 256) {
        const int key = kb + lane;
        const bool live = key < k1w && key_valid[min(key, cap - 1)] != 0;
        float acc[QW];
#pragma unroll
        for (int u = 0; u < QW; ++u) acc[u] = 0.f;
        if (live) {
            const bf16* kr = key >= L0 ? ksb + (size_t)(key - L0) * nkv * HD : kb_ + (size_t)key * HD;
#pragma unroll
            for (int c = 0; c < HD; c += 8) {
                const f32x8 kv = bf8_to_f32(*(const bf16x8*)(kr + c));
#pragma unroll
                for (int u = 0; u < QW; ++u) {
                    if (qg + 4 * u < T) {
                        const float* qr = qs + (qg + 4 * u) * HD;
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[u] = __builtin_fmaf(kv[e], qr[c + e], acc[u]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QW; ++u) {
            p[u] = 0.f;
            if (kb >= k1[u]) continue;                           // beyond this query's keys (wave-uniform): its loop has ended
            const bool valid = live && key < k1[u];
            float sc = -INFINITY;
            if (valid) sc = acc[u] * scale;
            float mb = sc;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mb = fmaxf(mb, __shfl_xor(mb, off, 64));
            if (mb == -INFINITY) continue;                       // no valid key in this block (wave-uniform)
            const float mn = fmaxf(m[u], mb);
            const float alpha = m[u] == -INFINITY ? 0.f : expf(m[u] - mn);
            p[u] = valid ? expf(sc - mn) : 0.f;
            l[u] = l[u] * alpha + wave_sum(p[u]);
#pragma unroll
            for (int i = 0; i < DPL; ++i) o[u][i] *= alpha;
            m[u] = mn;
        }
        const int jn = min(64, k1w - kb);
        for (int j = 0; j < jn; ++j) {
            float pj[QW];
            bool any = false;
#pragma unroll
            for (int u = 0; u < QW; ++u) { pj[u] = __shfl(p[u], j, 64); any = any || pj[u] != 0.f; }
            if (!any) continue;                                  // masked for every query of the wave (wave-uniform): its row is never read
            const int kj = kb + j;
            const bf16* vr = (kj >= L0 ? vsb + (size_t)(kj - L0) * nkv * HD : vb_ + (size_t)kj * HD) + lane * DPL;
            float v0, v1 = 0.f;
            if constexpr (DPL == 1) v0 = (float)vr[0];
            else {
                const bf16x2 vv = *(const bf16x2*)vr;
                v0 = (float)vv[0]; v1 = (float)vv[1];
            }
#pragma unroll
            for (int u = 0; u < QW; ++u) {
                if (pj[u] == 0.f) continue;
                o[u][0] = __builtin_fmaf(pj[u], v0, o[u][0]);
                if constexpr (DPL == 2) o[u][1] = __builtin_fmaf(pj[u], v1, o[u][1]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < QW; ++u) {
        const int t = qg + 4 * u;
        if (t < T) {
            float* mine = ws + ((size_t)lw * T + t) * (HD + 2);
            if (lane == 0) { mine[0] = m[u]; mine[1] = l[u]; }
#pragma unroll
            for (int i = 0; i < DPL; ++i) mine[2 + lane * DPL + i] = o[u][i];
        }
    }
    __syncthreads();
    // waves -> one (m, l, o) per query of this slice, in wave order: wave t combines query t
    const int t = wave;
    const size_t wstride = (size_t)T * (HD + 2);
    float M = -INFINITY, L = 0.f, O[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) O[i] = 0.f;
    if (t < T) {
        const float* wq = ws + (size_t)t * (HD + 2);
        for (int w = 0; w < 4; ++w) M = fmaxf(M, wq[w * wstride]);
        if (M != -INFINITY)
            for (int w = 0; w < 4; ++w) {
                const float wm = wq[w * wstride];
                if (wm == -INFINITY) continue;
                const float f = expf(wm - M);
                L += wq[w * wstride + 1] * f;
#pragma unroll
                for (int i = 0; i < DPL; ++i) O[i] += wq[w * wstride + 2 + lane * DPL + i] * f;
            }
    }
    // the staged k / v rows of this kv head -> cache slots [*len, *len + T): one workgroup per kv head (no workgroup of this launch reads them)
    if (s == 0 && h % (nh / nkv) == 0) {
        for (int i = tid; i < 2 * T * (HD / 8); i += 1024) {
            const int kv = i / (T * (HD / 8)), r = i % (T * (HD / 8)), tt = r / (HD / 8), c = r % (HD / 8) * 8;
            const bf16* src = (kv ? vsb : ksb) + (size_t)tt * nkv * HD + c;
            bf16* dst = (kv ? vb_ : kb_) + (size_t)(L0 + tt) * HD + c;
            *(u32x4*)dst = *(const u32x4*)src;
        }
    }
    if (S > 1) {
        if (t < T) {
            float* slab = part + (((size_t)t * nh + h) * S + s) * (HD + 2);
            if (lane == 0) { slab[0] = M; slab[1] = L; }
#pragma unroll
            for (int i = 0; i < DPL; ++i) slab[2 + lane * DPL + i] = O[i];
        }
        if (!arrive_last(cnt + h, S, flag)) return;              // every wave joins the hand-off's barriers
        if (t >= T) return;
        const float* pq = part + ((size_t)t * nh + h) * S * (HD + 2);
        M = -INFINITY;
        for (int u = 0; u < S; ++u) M = fmaxf(M, pq[(size_t)u * (HD + 2)]);
        L = 0.f;
#pragma unroll
        for (int i = 0; i < DPL; ++i) O[i] = 0.f;
        if (M != -INFINITY)
            for (int u = 0; u < S; ++u) {
                const float* sl = pq + (size_t)u * (HD + 2);
                if (sl[0] == -INFINITY) continue;
                const float f = expf(sl[0] - M);
                L += sl[1] * f;
#pragma unroll
                for (int i = 0; i < DPL; ++i) O[i] += sl[2 + lane * DPL + i] * f;
            }
    } else if (t >= T) {
        return;
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;
#pragma unroll
    for (int i = 0; i < DPL; ++i) out[(size_t)t * nh * HD + h * HD + lane * DPL + i] = (bf16)(O[i] * inv);
}

// ---------------------------------------------------------------------------------------------------
// One workgroup.  n = the drafts the model confirmed (draft[i] == ids[i] for all i < n): ids[0 .. n] are emitted.  With a token buffer
// (words given) the run is cut after the first EOS id and at the token limit, appended to the buffers, and the counters advance.  Then
// the state: last id, position and length + emitted, mask bytes [new length, old length + T) cleared.
__global__ __launch_bounds__(64) void spec_accept_kernel(const SpecAcceptArgs a)
{
    if (a.gate && *a.gate) return;
    __shared__ int se, sL;
    const int T = a.T;
    if (threadIdx.x == 0) {
        int n = 0;
        while (n < T - 1 && a.draft[n] == a.ids[n]) ++n;
        int e = n + 1;
        if (a.words) {
            int* w = a.words;
            int fin = 0;
            const int n_eos = min(max(w[SPEC_W_N_EOS], 0), 16);
            for (int i = 0; i < e && !fin; ++i)
                for (int k = 0; k < n_eos; ++k)
                    if (a.ids[i] == (int64_t)w[SPEC_W_EOS + k]) { e = i + 1; fin = 1; break; }
            const int written = w[SPEC_W_WRITTEN], room = max(w[SPEC_W_LIMIT] - written, 1);
            if (e >= room) { e = room; fin = 1; }                 // the token limit: the run ends there, whatever lay beyond
            const int sl = w[SPEC_W_SEQ_LEN];
            for (int i = 0; i < e; ++i) {
                if (a.out && written + i < a.out_cap) a.out[written + i] = a.ids[i];
                if (a.seq && sl + i < a.seq_cap) a.seq[sl + i] = (int)a.ids[i];
            }
            w[SPEC_W_WRITTEN] = written + e;
            w[SPEC_W_SEQ_LEN] = min(sl + e, a.seq_cap);
            w[SPEC_W_FINISHED] = fin;
            w[SPEC_W_STEPS] += 1;
            w[SPEC_W_TOKENS] += e;
        }
        if (a.emitted) *a.emitted = e;
        a.last[0] = a.ids[e - 1];
        a.posv[0] += e;
        const int L = *a.len;
        *a.len = L + e;
        se = e; sL = L;
    }
    __syncthreads();
    for (int k = sL + se + threadIdx.x; k < min(sL + T, a.cap); k += 64) a.key_valid[k] = 0;
}

// One workgroup behind the accept of a lookup step: thread (i, k) = (tid / 16, tid % 16) moves entry k of emitted row i.  The accept has
// advanced SPEC_W_WRITTEN by the count it left in *emitted, so the step's first token sits at written - emitted.
__global__ __launch_bounds__(256) void spec_logprobs_copy_kernel(const SpecLogprobsArgs a)
{
    if (a.gate && *a.gate) return;
    const int e = min(max(*a.emitted, 0), 16), first = a.words[SPEC_W_WRITTEN] - e;
    const int i = threadIdx.x >> 4, k = threadIdx.x & 15, o = first + i;
    if (i >= e || o < 0 || o >= a.out_cap) return;
    if (k == 0) a.out_tok[o] = a.tok[i];
    if (k < a.n) {
        a.out_ids[(size_t)o * a.n + k] = a.ids[i * a.n + k];
        a.out_top[(size_t)o * a.n + k] = a.top[i * a.n + k];
    }
}

// the token buffer of a lookup generation: the lookup ids (int64 -> int32, negative placeholders kept), then the first token
__global__ __launch_bounds__(256) void spec_begin_kernel(const int64_t* __restrict__ lookup, int n, const int64_t* last, int* __restrict__ seq, int64_t* out,
                                                         int* words, int limit, const SpecEosList eos)
{
    for (int i = threadIdx.x; i < n; i += 256) seq[i] = (int)max((int64_t)-0x7fffffff, min(lookup[i], (int64_t)0x7fffffff));
    if (threadIdx.x == 0) {
        const int64_t id = last[0];
        seq[n] = (int)id;
        if (out) out[0] = id;
        int fin = limit <= 1;
        for (int k = 0; k < eos.n; ++k) fin = fin || id == (int64_t)eos.ids[k];
        words[SPEC_W_SEQ_LEN] = n + 1; words[SPEC_W_WRITTEN] = 1; words[SPEC_W_FINISHED] = fin; words[SPEC_W_STEPS] = 0; words[SPEC_W_TOKENS] = 0;
        words[SPEC_W_LIMIT] = limit; words[SPEC_W_N_EOS] = eos.n;
        for (int k = 0; k < 16; ++k) words[SPEC_W_EOS + k] = k < eos.n ? eos.ids[k] : -1;
    }
}

// ---------------------------------------------------------------------------------------------------
extern "C" int fvhd_launch_spec_draft(hipStream_t st, const int* seq, const int* seq_len, int max_ngram, int K, int64_t* draft, const int* status,
                                      const int* words, int* gate)
{
    if (max_ngram < 1 || max_ngram > 16 || K < 1 || K > 15 || (gate && (!status || !words))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_draft_kernel, dim3(1), dim3(256), 0, st, seq, seq_len, max_ngram, K, draft, status, words, gate);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_spec_embed(hipStream_t st, const int64_t* draft, const int64_t* last, const void* table, const float* scale, const void* wblk, int V, int H,
                                      void* h, unsigned char* key_valid, int T, int cap, const int* len, const int64_t* posv, int64_t* pos, int* status,
                                      int* status_host, int* gate)
{
    if (T < 2 || T > 16 || H % 8 || (wblk && (scale || H % 128))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_embed_kernel, dim3(T), dim3(256), 0, st, draft, last, table, scale, (const u8*)wblk, V, H, (bf16*)h, key_valid, T, cap, len, posv, pos, status,
                       status_host, gate);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_spec_attention(hipStream_t st, const void* q, void* kc, void* vc, const void* ks, const void* vs, const unsigned char* key_valid,
                                          void* out, int T, int nh, int nkv, int hd, int cap, const int* len, int S, int chunk, float* part, int* cnt,
                                          const int* status)
{
    if (T < 2 || T > 16 || nh < 1 || nkv < 1 || nh % nkv || cap < 1 || S < 1 || chunk < 1 || (long)S * chunk < cap || (S > 1 && (!part || !cnt)))
        return (int)hipErrorInvalidValue;
    const float scale = 1.0f / sqrtf((float)hd);
    const dim3 grid((unsigned)((long)nh * S)), block(1024);
    const size_t lds = ((size_t)T * hd + 4 * (size_t)T * (hd + 2) + 4) * 4;
    if (hd == 64)
        hipLaunchKernelGGL(spec_attention_kernel<64>, grid, block, lds, st, (const bf16*)q, (bf16*)kc, (bf16*)vc, (const bf16*)ks, (const bf16*)vs, key_valid,
                           (bf16*)out, T, nh, nkv, cap, len, S, chunk, part, cnt, status, scale);
    else if (hd == 128)
        hipLaunchKernelGGL(spec_attention_kernel<128>, grid, block, lds, st, (const bf16*)q, (bf16*)kc, (bf16*)vc, (const bf16*)ks, (const bf16*)vs, key_valid,
                           (bf16*)out, T, nh, nkv, cap, len, S, chunk, part, cnt, status, scale);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_spec_accept(hipStream_t st, const SpecAcceptArgs* a)
{
    if (a->T < 2 || a->T > 16 || !a->draft || !a->ids || !a->last || !a->posv || !a->len || !a->key_valid) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(64), 0, st, *a);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_spec_logprobs_copy(hipStream_t st, const SpecLogprobsArgs* a)
{
    if (!a->tok || !a->emitted || !a->words || !a->out_tok || a->n < 0 || a->n > 16 || a->out_cap < 1 ||
        (a->n && (!a->ids || !a->top || !a->out_ids || !a->out_top)))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_logprobs_copy_kernel, dim3(1), dim3(256), 0, st, *a);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_spec_begin(hipStream_t st, const int64_t* lookup, int n, const int64_t* last, int* seq, int64_t* out, int* words, int limit,
                                      const SpecEosList* eos)
{
    if (n < 0 || (n && !lookup) || eos->n < 0 || eos->n > 16) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_begin_kernel, dim3(1), dim3(256), 0, st, lookup, n, last, seq, out, words, limit, *eos);
    return (int)hipGetLastError();
}
