// Logits processors inside the decode step: repetition penalty, no-repeat n-grams, min_new_tokens and token bans as sparse in-place
// edits of the fp32 logits [B][V] between the lm_head and the choice (include/fvhd.h "LLM logits processors").
//
// transformers' processors for num_beams = 1, in the order of its `_get_logits_processor`, over the history h[0 .. g) of a row = the
// tokens fed to the decode steps since fvhd_llm_start:
//   RepetitionPenaltyLogitsProcessor(p)      every DISTINCT token t of h: s[t] = s[t] < 0 ? s[t] * p : s[t] / p (IEEE division)
//   NoRepeatNGramLogitsProcessor(n)          g >= n: every window h[i .. i+n-1] whose first n-1 tokens equal the last n-1 of h bans
//                                            its last token (s = -inf)
//   MinNewTokensLengthLogitsProcessor(0, m)  g < m: every EOS id banned
//   SuppressTokensLogitsProcessor            the ids banned, always
// One workgroup per row, one launch:
//   append   thread 0 adds the step's fed token to the row's history, at the row's own count (a device word per row that only these
//            launches advance: a step enqueued with processors off appends nothing, counts nothing and leaves no gap).  A bitmap of V
//            bits per row ("token is in the history") is tested and set there, and the entry records whether it is the token's first
//            occurrence (sign bit clear) or a repeat (sign bit set)
//   penalty  lanes walk the history in strides of 256; only a first occurrence edits its logit, so each distinct token is read, scaled
//            and written by exactly one lane: no atomics, the same bits eager or replayed, however often a token repeats
//   barrier  the bans come after every penalty (a token both penalised and banned ends up banned)
//   bans     the same walk over the n-gram windows, then the EOS and suppress lists; lanes that ban the same token store the same -inf
// At most g + 272 logits of a row are touched; the row itself is never read or written as a whole.
#include "fvhd_common.h"
#include "launchers.h"      // (with llm_decode.h: DecLogitsArgs)

namespace {

constexpr unsigned kRepeat = 0x80000000u;        // history entry: an earlier entry of the row holds the same token

// entry i of a row's history = `id`, with the first-occurrence record; an id outside [0, V) (never from the step: dec_embed refuses it
// first) is stored as -1: a repeat of a token >= V, which no phase turns into a logit index
FVHD_DEV void history_append(int* h, unsigned* seen, int i, long id, int V)
{
    if (id < 0 || id >= V) { h[i] = -1; return; }
    const unsigned bit = 1u << (id & 31), word = seen[id >> 5];
    seen[id >> 5] = word | bit;
    h[i] = (int)((unsigned)id | ((word & bit) ? kRepeat : 0u));
}

}  // namespace

__global__ __launch_bounds__(256) void dec_logits_process_kernel(const DecLogitsArgs a)
{
    if (a.status && *a.status) return;                           // a step that hit the sticky error appends nothing
    __shared__ int g_s;
    const int tid = threadIdx.x, b = blockIdx.x, V = a.V;
    int* h = a.hist + (size_t)b * a.cap;
    float* x = a.logits + (size_t)b * V;
    if (tid == 0) {
        int g = a.g_fixed >= 0 ? a.g_fixed : a.start_T > 0 ? 0 : a.count[b];
        g = max(0, min(g, a.cap));
        if ((a.tok || a.last) && g < a.cap) {
            history_append(h, a.seen + (size_t)b * ((V + 31) / 32), g, a.tok ? a.tok[b] : a.last[b], V);
            ++g;
        }
        if (a.g_fixed < 0) a.count[b] = g;                       // the row's own word: only this workgroup reads or writes it
        g_s = g;
    }
    __syncthreads();
    const int g = g_s;
    if (a.penalty != 1.f) {
        const float p = a.penalty;
        for (int i = tid; i < g; i += 256) {
            const int t = h[i];
            if (t >= 0 && t < V) {                               // a first occurrence: this lane alone owns logit t
                const float s = x[t];
                x[t] = s < 0.f ? s * p : __fdiv_rn(s, p);
            }
        }
    }
    __syncthreads();
    const int n = a.ngram;
    if (n > 0 && g >= n) {
        const int* suffix = h + g - (n - 1);                     // the last n - 1 tokens
        for (int i = tid; i + n <= g; i += 256) {
            bool match = true;
            for (int j = 0; j < n - 1 && match; ++j) match = ((h[i + j] ^ suffix[j]) & ~kRepeat) == 0;
            const unsigned t = (unsigned)h[i + n - 1] & ~kRepeat;
            if (match && t < (unsigned)V) x[t] = -INFINITY;
        }
    }
    if (g < a.min_new)
        for (int j = tid; j < a.n_eos; j += 256)
            if ((unsigned)a.eos[j] < (unsigned)V) x[a.eos[j]] = -INFINITY;
    for (int j = tid; j < a.n_sup; j += 256)
        if ((unsigned)a.sup[j] < (unsigned)V) x[a.sup[j]] = -INFINITY;
}

// the single op's history: `tokens` int32 [B][cap] -> hist / seen as g appends of the step would have left them (seen zeroed by the caller)
__global__ __launch_bounds__(64) void dec_logits_history_kernel(const int* __restrict__ tokens, int* __restrict__ hist, unsigned* __restrict__ seen, int V,
                                                                int cap, int g)
{
    if (threadIdx.x) return;
    const int b = blockIdx.x;
    for (int i = 0; i < g; ++i) history_append(hist + (size_t)b * cap, seen + (size_t)b * ((V + 31) / 32), i, tokens[(size_t)b * cap + i], V);
}

// ---------------------------------------------------------------------------------------------------
extern "C" int fvhd_launch_dec_logits_process(hipStream_t st, const DecLogitsArgs* a)
{
    if (!a->logits || !a->hist || a->B < 1 || a->B > 64 || a->V < 1 || a->cap < 1 || a->g_fixed > a->cap || !(a->penalty > 0.f) || a->ngram < 0 ||
        a->min_new < 0 || a->n_eos < 0 || a->n_sup < 0 || (a->n_eos && !a->eos) || (a->n_sup && !a->sup))
        return (int)hipErrorInvalidValue;
    if ((a->tok || a->last) && !a->seen) return (int)hipErrorInvalidValue;
    if (a->g_fixed < 0 && !a->count) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_logits_process_kernel, dim3(a->B), dim3(256), 0, st, *a);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_logits_history(hipStream_t st, const int* tokens, int* hist, unsigned* seen, int B, int V, int cap, int g)
{
    if (!tokens || !hist || !seen || B < 1 || B > 64 || V < 1 || cap < 1 || g < 0 || g > cap) return (int)hipErrorInvalidValue;
    if (g) hipLaunchKernelGGL(dec_logits_history_kernel, dim3(B), dim3(64), 0, st, tokens, hist, seen, V, cap, g);
    return (int)hipGetLastError();
}
