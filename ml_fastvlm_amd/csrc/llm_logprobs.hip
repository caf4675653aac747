// Log-probabilities of chosen tokens with the n most likely alternatives, over the fp32 logits [B][V] of the lm_head (include/fvhd.h
// "LLM log-probabilities").
//
// Per row:  M = max x,  Z = sum exp(x - M),  token_logprob = (x[id] - M) - log Z,  and the top_n largest logits in descending order (equal
// values by ascending id, -0 = +0, -inf last) with their log-probabilities.  A -inf logit (a suppressed token) adds 0 to Z and has
// log-probability -inf; a row without a finite logit, or with +inf / NaN, is undefined (the sampler's rule, llm_sample.hip).
//
// ONE launch, grid = S slices x B rows, 256 threads; slice s owns the indices [s L, s L + L), L = ceil(V / S), thread t of it the indices
// s L + t + 256 j (coalesced 4-byte loads: the rows of a V that is no multiple of 4 are not 16-byte aligned).  A workgroup makes three passes
// over its slice (9.5 KB at V = 152 064: the second and third come from the cache):
//   A  every thread's best element as ONE 64-bit word (the order-preserving key of the value, ~index): the block maximum is the slice's
//      first candidate and gives the slice maximum m
//   B  sum exp(x - m): a thread adds its elements in index order, the 256 thread sums meet in a butterfly (wave, then the 4 waves) - a fixed
//      order of additions, no floating-point atomics
//   C  top_n rounds of "block maximum of the threads' bests": the thread that owned the winner looks through its elements again for its best
//      below it, every other thread's best is still valid
// Slice partials (m, sum, the top_n candidate words) go to the scratch; the last-arriving workgroup of a row (the in-launch hand-off of
// split_handoff.h, which leaves the counter at zero: `arrive_last_published`, the protocol with the lighter producer side) merges them: M, Z = sum_s sum_s exp(m_s - M) in a butterfly over the
// slices, and top_n rounds of block maximum over the S * top_n candidates, which sit in registers (4 per thread).  The ids depend on
// comparisons of the input values only: they are exact.  The same inputs give the same bits, eager or replayed.
#include "fvhd_common.h"
#include "launchers.h"
#include "split_handoff.h"  // publish, arrive_last_published

namespace {

constexpr int LP_SMAX = 64;                      // slices per row (one wave merges them)
constexpr int LP_NMAX = 16;                      // top_n
constexpr int LP_BMAX = 64;                      // rows per launch: their arrival counters are the head of the scratch
constexpr int LP_CNT_STRIDE = 64;                // ints between two rows' counters: a 256-byte line each (the adds of 64 rows on one line wait for each other)
constexpr int LP_SLICE = 2048;                   // a row shorter than LP_SMAX slices of this many elements gets fewer slices

typedef unsigned long long u64;

struct LpArgs {
    const float* logits;
    const int64_t* ids;
    int V, top_n;
    float* token_lp;
    int64_t* top_ids;
    float* top_lp;
    const int* status;
};

struct LpWs {
    int* cnt;                                    // [LP_BMAX] arrival counters, one per LP_CNT_STRIDE ints (zero between launches)
    float* pm;                                   // [B][S] slice maximum
    float* ps;                                   // [B][S] sum of exp(x - slice maximum)
    u64* cand;                                   // [B][S][top_n] the slice's candidates, best first (0: none)
};

size_t al256l(size_t x) { return (x + 255) & ~(size_t)255; }

int slices_of(int V) { return V >= LP_SMAX * LP_SLICE ? LP_SMAX : (V + LP_SLICE - 1) / LP_SLICE; }

LpWs carve(void* base, int B, int S)
{
    char* p = (char*)base;
    LpWs w;
    w.cnt = (int*)p;
    p += al256l(4 * LP_BMAX * LP_CNT_STRIDE);
    w.pm = (float*)p;
    p += al256l((size_t)4 * B * S);
    w.ps = (float*)p;
    p += al256l((size_t)4 * B * S);
    w.cand = (u64*)p;
    return w;
}

// order-preserving key of an fp32 value (order_key of llm_sample.hip): a > b <=> key(a) > key(b); -0 and +0 share one key
FVHD_DEV unsigned okey(float s)
{
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

FVHD_DEV float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// value and index as one word: a larger word = a larger value, or an equal value at a lower index.  Never 0 for a value that is no NaN.
FVHD_DEV u64 word_of(float v, int i) { return ((u64)okey(v) << 32) | (unsigned)~i; }
FVHD_DEV float word_value(u64 w) { return key_value((unsigned)(w >> 32)); }
FVHD_DEV int word_index(u64 w) { return (int)~(unsigned)w; }

FVHD_DEV u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

// the maximum over the 256 threads, in every thread; `buf`: 4 words that no thread still reads (the callers alternate two)
FVHD_DEV u64 block_max(u64 v, u64* buf)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = umax64(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    return umax64(umax64(buf[0], buf[1]), umax64(buf[2], buf[3]));
}

}  // namespace

__global__ __launch_bounds__(256) void dec_logprobs_kernel(const LpArgs a, const LpWs w)
{
    if (a.status && *a.status) return;
    __shared__ u64 redk[2][4];
    __shared__ float redf[4];
    __shared__ float row_m, row_logz;
    __shared__ int flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const int V = a.V, n = a.top_n;
    const float* x = a.logits + (size_t)b * V;
    const int L = (V + S - 1) / S;
    const int i0 = min(s * L, V), i1 = min(i0 + L, V);
    // A: the thread's best element; the block's is the slice maximum
    u64 best = 0;
    for (int i = i0 + tid; i < i1; i += 256) best = umax64(best, word_of(x[i], i));
    u64 pick = block_max(best, redk[0]);
    const float m = pick ? word_value(pick) : -INFINITY;
    // B: sum exp(x - m) (a slice of -inf only: 0, never exp(-inf - -inf))
    float acc = 0.f;
    if (m > -INFINITY)
        for (int i = i0 + tid; i < i1; i += 256) acc += expf(x[i] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) redf[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        publish(w.pm + b * S + s, m);
        publish(w.ps + b * S + s, (redf[0] + redf[1]) + (redf[2] + redf[3]));
    }
    // C: the slice's top_n, best first (round 0 is the maximum found above)
    u64* cand = w.cand + ((size_t)b * S + s) * n;
    for (int k = 0; k < n; ++k) {
        if (k) pick = block_max(best, redk[k & 1]);
        if (tid == 0) publish(cand + k, pick);
        if (best == pick && pick) {                                                 // the one owner: its best below the winner
            u64 nb = 0;
            for (int i = i0 + tid; i < i1; i += 256) {
                const u64 c = word_of(x[i], i);
                if (c < pick) nb = umax64(nb, c);
            }
            best = nb;
        }
    }
    if (!arrive_last_published(w.cnt + b * LP_CNT_STRIDE, S, &flag)) return;
    // ---- the row's last workgroup: merge the slices ----
    if (wave == 0) {
        const float ms = lane < S ? w.pm[b * S + lane] : -INFINITY;
        const float ss = lane < S ? w.ps[b * S + lane] : 0.f;
        float M = ms;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
        float z = ms > -INFINITY ? ss * expf(ms - M) : 0.f;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if (lane == 0) {
            row_m = M;
            row_logz = logf(z);
        }
    }
    // the S * n candidates: 4 per thread, in registers
    u64 c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = tid + 256 * q;
        c[q] = j < S * n ? w.cand[(size_t)b * S * n + j] : 0;
    }
    __syncthreads();
    const float M = row_m, logz = row_logz;
    if (tid == 0) {
        const int64_t id = a.ids[b];
        a.token_lp[b] = id >= 0 && id < V ? (x[id] - M) - logz : __uint_as_float(0x7fc00000u);
    }
    for (int k = 0; k < n; ++k) {
        const u64 mine = umax64(umax64(c[0], c[1]), umax64(c[2], c[3]));
        pick = block_max(mine, redk[k & 1]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (c[q] == pick) c[q] = 0;
        if (tid == 0) {
            a.top_ids[(size_t)b * n + k] = word_index(pick);
            a.top_lp[(size_t)b * n + k] = (word_value(pick) - M) - logz;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
extern "C" size_t fvhd_dec_logprobs_scratch_bytes(int B, int V, int top_n)
{
    if (B < 1 || B > LP_BMAX || V < 1 || top_n < 0 || top_n > LP_NMAX) return 0;
    const int S = slices_of(V);
    return al256l(4 * LP_BMAX * LP_CNT_STRIDE) + 2 * al256l((size_t)4 * B * S) + al256l((size_t)8 * B * S * top_n);
}

extern "C" int fvhd_launch_dec_logprobs(hipStream_t st, const float* logits, const int64_t* ids, int B, int V, int top_n, float* token_logprob,
                                        int64_t* top_ids, float* top_logprobs, void* scratch, const int* status)
{
    if (!logits || !ids || !token_logprob || !scratch || B < 1 || B > LP_BMAX || V < 1 || top_n < 0 || top_n > LP_NMAX || top_n > V ||
        (top_n && (!top_ids || !top_logprobs)))
        return (int)hipErrorInvalidValue;
    const int S = slices_of(V);
    LpArgs a;
    a.logits = logits; a.ids = ids; a.V = V; a.top_n = top_n; a.token_lp = token_logprob; a.top_ids = top_ids; a.top_lp = top_logprobs; a.status = status;
    hipLaunchKernelGGL(dec_logprobs_kernel, dim3((unsigned)S, (unsigned)B), dim3(256), 0, st, a, carve(scratch, B, S));
    return (int)hipGetLastError();
}
