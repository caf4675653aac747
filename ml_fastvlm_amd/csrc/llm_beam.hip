// Beam search on the device (include/fvhd.h "LLM beam search"): the top continuations of every prompt and the KV-cache reorder.
//
// dec_beam_topk: per prompt g the C largest of acc[k * V + v] = ((logit[g K + k][v] - max_row) - log sum_v exp(logit - max_row)) + score[g][k]
// over its K beams (transformers' `_beam_search` step b + `_get_top_k_continuations`: log_softmax, + running_beam_scores, topk), without
// sorting or even writing the K * V values: the term added to a row's logits is one constant, so a prompt's top C lie inside the per-row
// top C of the RAW logits.  Three launches, 256 threads each:
//   beam_slice   grid (S, rows): a slice of 4096 logits in registers (16 per thread) -> the slice's (max, sum exp(x - max)) and its top C
//   beam_row     grid (rows):    the S * C survivors of a row -> the row's top C, and (max, log sum exp) from the slices in slice order
//   beam_group   grid (G):       the K * C survivors of a prompt with their accumulated values -> the C best (value, flat index)
// A candidate is ONE 64-bit key: the order-preserving image of its fp32 value in the high word, ~index in the low word - the larger key
// is the larger value, and among equal values the lower index.  The top C of a workgroup's keys are C rounds of a block maximum (a
// shuffle tree per wave, four partial maxima through LDS, one barrier per round); the winner is cleared in whichever thread holds it.
// Every sum has a fixed order (per thread in index order, the shuffle tree, the waves and the slices in order): the same inputs give the
// same bits, eager or replayed.  Candidates enter a row's top C by their raw logit (ties: the lower index), and the prompt's top C by
// their accumulated value (ties: the lower flat index).
//
// dec_cache_gather: new row r of every layer's K and V (slots [0, *len)), of the key-valid mask and of the next positions = old row
// src[r].  Never in place (a swap would read what it has just overwritten): a layer is gathered into a scratch and copied back by the
// NEXT launch, which at the same time gathers the next layer into the scratch's other half - L + 1 launches for L layers, the mask and the
// positions riding on the first two.  Rows with src[r] == r leave at once, in both directions.  Every workgroup checks all of src first:
// one index outside [0, rows_in) and no launch writes anything but the error word (3).
//
// Beam search with processors (include/fvhd.h "LLM beam search with processors"): beam_norm_* turn the rows into log-probabilities in place
// with the statistics above, beam_group / beam_sample_group take such rows as they are (`prenorm`), and dec_hist_move carries the rows'
// processor histories and automaton states behind the cache reorder, by its rules.
#include <algorithm>

#include "fvhd_common.h"
#include "launchers.h"      // (with llm_decode.h: DecCacheGatherArgs, DecBeamSampleArgs)
#include "sample_rng.h"     // scaled, philox4x32_10, gumbel_of_word

namespace {

typedef unsigned long long u64;

constexpr int SLICE = 4096;                      // logits per beam_slice workgroup: 16 per thread
constexpr int SMAXB = 64;                        // slices per row at most (V <= SLICE * SMAXB)
constexpr int CMAX = 64;
constexpr int RMAX = 64;                         // rows = G * K

// order-preserving key of an fp32 value (llm_sample.hip's): a > b <=> key(a) > key(b); -0 and +0 share one key
FVHD_DEV unsigned okey(float s)
{
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FVHD_DEV float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// 0 = no candidate: below every real key (the key of -inf is 0x007fffff........)
FVHD_DEV u64 make_key(float v, unsigned idx) { return ((u64)okey(v) << 32) | (0xffffffffu - idx); }
FVHD_DEV float cand_value(u64 k) { return key_value((unsigned)(k >> 32)); }
FVHD_DEV unsigned cand_index(u64 k) { return 0xffffffffu - (unsigned)k; }

FVHD_DEV u64 wave_max(u64 v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), o), lo = (unsigned)__shfl_xor((int)(unsigned)v, o);
        const u64 w = ((u64)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

FVHD_DEV float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);      // a fixed tree: every lane ends with the same bits
    return v;
}

// the block maximum of one key per thread; `red`: 4 LDS words of the caller, free again after the next barrier
FVHD_DEV u64 block_max(u64 v, u64* red)
{
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const u64 a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}

// the C largest of the workgroup's keys (EPT per thread, real keys are distinct) -> out[0 .. C) in descending order (LDS or global;
// exhausted: 0).  `red`: 8 LDS words, used alternately, so that one barrier per round is enough.
template <int EPT>
FVHD_DEV void block_top(u64 (&key)[EPT], int C, u64* out, u64* red)
{
    for (int c = 0; c < C; ++c) {
        u64 best = 0;
#pragma unroll
        for (int j = 0; j < EPT; ++j) best = key[j] > best ? key[j] : best;
        best = block_max(best, red + 4 * (c & 1));
#pragma unroll
        for (int j = 0; j < EPT; ++j) key[j] = key[j] == best ? 0 : key[j];
        if (threadIdx.x == 0) out[c] = best;
    }
}

__global__ __launch_bounds__(256) void beam_slice_kernel(const float* __restrict__ logits, int V, int S, int C, u64* __restrict__ keys,
                                                         float* __restrict__ pmax, float* __restrict__ psum)
{
    __shared__ u64 red[8];
    __shared__ float fred[4];
    const int s = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    const float* x = logits + (size_t)row * V;
    u64 key[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = s * SLICE + (j * 256 + t) * 4;
        if (e < V) {                                             // V % 16 == 0: a float4 lies inside the row or outside it
            const f32x4 v = *(const f32x4*)(x + e);
            key[4 * j + 0] = make_key(v[0], e); key[4 * j + 1] = make_key(v[1], e + 1);
            key[4 * j + 2] = make_key(v[2], e + 2); key[4 * j + 3] = make_key(v[3], e + 3);
        } else {
            key[4 * j + 0] = key[4 * j + 1] = key[4 * j + 2] = key[4 * j + 3] = 0;
        }
    }
    u64 best = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) best = key[j] > best ? key[j] : best;
    const float m = cand_value(block_max(best, red));            // (every slice holds at least 16 logits)
    float acc = 0.f;
    if (m > -INFINITY) {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (key[j]) acc += expf(cand_value(key[j]) - m);
    }
    acc = wave_sum(acc);
    if ((t & 63) == 0) fred[t >> 6] = acc;
    __syncthreads();                                             // (also: `red` is free for block_top)
    if (t == 0) {
        pmax[row * S + s] = m;
        psum[row * S + s] = ((fred[0] + fred[1]) + fred[2]) + fred[3];
    }
    block_top<16>(key, C, keys + ((size_t)row * S + s) * C, red);
}

// a row's (max, log sum exp(x - max)) from its slices' partials, in slice order: ONE copy of the order, for beam_row and the normalisation
FVHD_DEV void row_stats(const float* __restrict__ pmax, const float* __restrict__ psum, int row, int S, float& M_out, float& L_out)
{
    float M = -INFINITY;
    for (int s = 0; s < S; ++s) M = fmaxf(M, pmax[row * S + s]);
    float sum = 0.f;
    for (int s = 0; s < S; ++s) {
        const float ms = pmax[row * S + s];
        if (ms > -INFINITY) sum += psum[row * S + s] * expf(ms - M);
    }
    M_out = M;
    L_out = logf(sum);
}

__global__ __launch_bounds__(256) void beam_row_kernel(const u64* __restrict__ keys, const float* __restrict__ pmax, const float* __restrict__ psum,
                                                       int S, int C, u64* __restrict__ rowtop, float* __restrict__ rowmax, float* __restrict__ rowlog)
{
    __shared__ u64 red[8];
    const int row = blockIdx.x, t = threadIdx.x, n = S * C;      // n <= 4096
    u64 key[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int i = j * 256 + t;
        key[j] = i < n ? keys[(size_t)row * n + i] : 0;
    }
    if (t == 0) row_stats(pmax, psum, row, S, rowmax[row], rowlog[row]);
    block_top<16>(key, C, rowtop + (size_t)row * C, red);
}

__global__ __launch_bounds__(256) void beam_group_kernel(const u64* __restrict__ rowtop, const float* __restrict__ rowmax, const float* __restrict__ rowlog,
                                                         const float* __restrict__ scores, int K, int C, int V, int prenorm,
                                                         float* __restrict__ out_v, int64_t* __restrict__ out_i)
{
    __shared__ u64 red[8];
    __shared__ u64 top[CMAX];
    const int g = blockIdx.x, t = threadIdx.x, n = K * C;        // n <= 1024
    u64 key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = j * 256 + t;
        key[j] = 0;
        if (i < n) {
            const int k = i / C, row = g * K + k;
            const u64 c = rowtop[(size_t)row * C + i % C];
            if (c && !(prenorm && cand_value(c) == -INFINITY)) {                // a pre-normalised row: its value as it is; a banned entry is no candidate
                const float acc = prenorm ? cand_value(c) + scores[row] : ((cand_value(c) - rowmax[row]) - rowlog[row]) + scores[row];
                key[j] = make_key(acc, (unsigned)k * (unsigned)V + cand_index(c));
            }
        }
    }
    block_top<4>(key, C, top, red);
    __syncthreads();
    if (t < C) {
        const u64 c = top[t];
        out_v[(size_t)g * C + t] = c ? cand_value(c) : -INFINITY;
        out_i[(size_t)g * C + t] = c ? (int64_t)cand_index(c) : 0;
    }
}

// ---- row normalisation: x[r][v] <- (x[r][v] - M_r) - L_r in place (include/fvhd.h "LLM beam search with processors") -------------------------
// Under beams transformers runs its processors on log_softmax(x).  M_r and L_r are beam_slice's / beam_row's: the same slices, the same
// per-thread element order, the same trees - so an entry that no processor edits holds, bit for bit, what the plain chain adds to the beam
// score.  Two launches of grid (S, rows): the slices' partials, then the apply (every workgroup merges its row's partials again, in slice
// order).  Any V: a row that is not 16-byte aligned (V % 4 != 0) and a row's last 1 .. 3 entries go element by element.
__global__ __launch_bounds__(256) void beam_norm_slice_kernel(const float* __restrict__ logits, int V, int S, float* __restrict__ pmax,
                                                              float* __restrict__ psum, const int* __restrict__ status)
{
    if (status && *status) return;
    __shared__ float fred[8];
    const int s = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    const float* x = logits + (size_t)row * V;
    const bool vec = ((uintptr_t)x & 15) == 0;
    float v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = s * SLICE + (j * 256 + t) * 4;
        if (vec && e + 3 < V) {
            const f32x4 q = *(const f32x4*)(x + e);
            v[4 * j + 0] = q[0]; v[4 * j + 1] = q[1]; v[4 * j + 2] = q[2]; v[4 * j + 3] = q[3];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * j + i] = e + i < V ? x[e + i] : -INFINITY;      // (outside the row: no part of the maximum, skipped by the sum)
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) m = fmaxf(m, v[j]);
#pragma unroll
    for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((t & 63) == 0) fred[4 + (t >> 6)] = m;
    __syncthreads();
    m = fmaxf(fmaxf(fred[4], fred[5]), fmaxf(fred[6], fred[7]));
    m = m == 0.f ? 0.f : m;                                      // (beam_slice's maximum comes out of a key: -0 is +0 there)
    float acc = 0.f;
    if (m > -INFINITY) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int e = s * SLICE + ((j >> 2) * 256 + t) * 4 + (j & 3);
            if (e < V) acc += expf(v[j] - m);
        }
    }
    acc = wave_sum(acc);
    if ((t & 63) == 0) fred[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        pmax[row * S + s] = m;
        psum[row * S + s] = ((fred[0] + fred[1]) + fred[2]) + fred[3];
    }
}

__global__ __launch_bounds__(256) void beam_norm_apply_kernel(float* __restrict__ logits, int V, int S, const float* __restrict__ pmax,
                                                              const float* __restrict__ psum, float* __restrict__ stats, const int* __restrict__ status)
{
    if (status && *status) return;
    __shared__ float ml[2];
    const int s = blockIdx.x, row = blockIdx.y, t = threadIdx.x;
    if (t == 0) {
        row_stats(pmax, psum, row, S, ml[0], ml[1]);
        if (stats && s == 0) { stats[2 * row] = ml[0]; stats[2 * row + 1] = ml[1]; }
    }
    __syncthreads();
    const float M = ml[0], L = ml[1];
    float* x = logits + (size_t)row * V;
    const bool vec = ((uintptr_t)x & 15) == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = s * SLICE + (j * 256 + t) * 4;
        if (vec && e + 3 < V) {
            f32x4 q = *(const f32x4*)(x + e);
            q[0] = (q[0] - M) - L; q[1] = (q[1] - M) - L; q[2] = (q[2] - M) - L; q[3] = (q[3] - M) - L;
            *(f32x4*)(x + e) = q;
        } else {
            for (int i = 0; i < 4; ++i)
                if (e + i < V) x[e + i] = (x[e + i] - M) - L;
        }
    }
}

// ---- beam-search sampling: per prompt the `keep` KEPT candidates with the largest a + g (include/fvhd.h "LLM beam-search sampling") --------------
// transformers' `_beam_search(do_sample=True)`: a = log_softmax(x) / T + score behind the top-k / top-p warpers with min_tokens_to_keep = m, then
// torch.multinomial without replacement over the prompt's K * V values = the top `keep` of a + Gumbel noise, returned in that order with the
// unperturbed a.  The noise is per candidate, so a row's candidates can no longer be pre-selected by their raw logits: the greedy chain runs over
// PERTURBED keys.  Launches (dec_beam_sample below):
//   beam_slice, beam_row (C = m)   the kernels above on the raw logits: M, L, and the m largest logits of every row (v_m = the m-th / T)
//   the sampler's max / level passes in blocks of 16 rows (fvhd_launch_dec_sample_theta; none when no filter is on): theta_s on s = x / T for
//                                  top_k' = max(top_k, m) and top_p.  The kept set is {s >= min(theta_s, v_m), x > -inf}: theta_s is the top-p
//                                  threshold when top-p is on (searched among the top-k' survivors, so it is >= theta_k'), else theta_k' <= v_m.
//   beam_sample_slice              the slice's kept tokens keyed by s + g -> its top C and its kept count
//   beam_row                       the kernel above over those keys -> the row's top C by s + g
//   beam_sample_group              the K * C survivors re-keyed by (((x - M) - L) / T + score) + g -> the C best, their unperturbed a, flat indices
// Within a row a differs from s by one constant, so the row's order under s + g is its order under a + g up to fp32 rounding (the bound is in
// DESIGN 4.3); with g = 0 and T = 1 the keys are the greedy chain's and so are the results, bit for bit.  g is Philox word v & 3 of the counter
// (row, n, v >> 2, 1) - one generator call per float4 - or noise_override[row][v].
struct BeamNoise {
    const float* over;
    unsigned n, k0, k1;
    FVHD_DEV BeamNoise(const DecBeamSampleArgs& a)
    {
        over = a.noise_override;
        n = (unsigned)((a.len ? *a.len : 0) + a.n_add);
        k0 = (unsigned)a.seed;
        k1 = (unsigned)(a.seed >> 32);
    }
    FVHD_DEV Philox4 words(int row, int v) const { return philox4x32_10((unsigned)row, n, (unsigned)v >> 2, 1u, k0, k1); }
};

// the kept set's threshold key of a row: min(the sampler's, the key of v_m)
FVHD_DEV unsigned beam_theta(const DecBeamSampleArgs& a, const u64* __restrict__ rawtop, const unsigned* __restrict__ theta_s, int row)
{
    const u64 c = rawtop[(size_t)row * a.min_keep + a.min_keep - 1];
    const unsigned vm = c ? okey(scaled(cand_value(c), a.temperature)) : 0u;
    const unsigned ts = theta_s ? theta_s[row] : 0u;
    return ts < vm ? ts : vm;
}

FVHD_DEV float beam_acc(float x, float M, float L, float T, float score) { return scaled((x - M) - L, T) + score; }
// a.prenorm: the rows hold log-probabilities already - a = x / T + score
FVHD_DEV float beam_acc(const DecBeamSampleArgs& a, float x, const float* __restrict__ rowmax, const float* __restrict__ rowlog, int row)
{
    return a.prenorm ? scaled(x, a.temperature) + a.scores[row] : beam_acc(x, rowmax[row], rowlog[row], a.temperature, a.scores[row]);
}

__global__ __launch_bounds__(256) void beam_sample_slice_kernel(const DecBeamSampleArgs a, int S, const u64* __restrict__ rawtop,
                                                                const unsigned* __restrict__ theta_s, u64* __restrict__ keys, int* __restrict__ pcnt)
{
    __shared__ u64 red[8];
    __shared__ int cred[4];
    const int s = blockIdx.x, row = blockIdx.y, t = threadIdx.x, V = a.V;
    const float* x = a.logits + (size_t)row * V;
    const unsigned theta = beam_theta(a, rawtop, theta_s, row);
    const BeamNoise noise(a);
    const float T = a.temperature;
    u64 key[16];
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = s * SLICE + (j * 256 + t) * 4;
        if (e < V) {                                             // V % 16 == 0: a float4 lies inside the row or outside it
            const f32x4 v = *(const f32x4*)(x + e);
            f32x4 g;
            if (noise.over) {
                g = *(const f32x4*)(noise.over + (size_t)row * V + e);
            } else {
                const Philox4 w = noise.words(row, e);
                g[0] = gumbel_of_word(w.w[0]); g[1] = gumbel_of_word(w.w[1]); g[2] = gumbel_of_word(w.w[2]); g[3] = gumbel_of_word(w.w[3]);
            }
            if (a.noise_out) *(f32x4*)(a.noise_out + (size_t)row * V + e) = g;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float sv = scaled(v[i], T);
                const bool kept = okey(sv) >= theta && v[i] > -INFINITY;      // a -inf logit is never kept
                key[4 * j + i] = kept ? make_key(sv + g[i], e + i) : 0;
                cnt += kept;
            }
        } else {
            key[4 * j + 0] = key[4 * j + 1] = key[4 * j + 2] = key[4 * j + 3] = 0;
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((t & 63) == 0) cred[t >> 6] = cnt;
    __syncthreads();
    if (t == 0) pcnt[row * S + s] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
    block_top<16>(key, a.keep, keys + ((size_t)row * S + s) * a.keep, red);
}

__global__ __launch_bounds__(256) void beam_sample_group_kernel(const DecBeamSampleArgs a, int S, const u64* __restrict__ rowtop, const float* __restrict__ rowmax,
                                                                const float* __restrict__ rowlog, const u64* __restrict__ rawtop,
                                                                const unsigned* __restrict__ theta_s, const int* __restrict__ pcnt)
{
    __shared__ u64 red[8];
    __shared__ u64 top[CMAX];
    const int g = blockIdx.x, t = threadIdx.x, K = a.K, C = a.keep, V = a.V, n = K * C;      // n <= 1024
    const BeamNoise noise(a);
    u64 key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = j * 256 + t;
        key[j] = 0;
        if (i < n) {
            const int k = i / C, row = g * K + k;
            const u64 c = rowtop[(size_t)row * C + i % C];
            if (c) {
                const int v = (int)cand_index(c);
                const float acc = beam_acc(a, a.logits[(size_t)row * V + v], rowmax, rowlog, row);
                const float gn = noise.over ? noise.over[(size_t)row * V + v] : gumbel_of_word(noise.words(row, v).w[v & 3]);
                key[j] = make_key(acc + gn, (unsigned)k * (unsigned)V + (unsigned)v);
            }
        }
    }
    block_top<4>(key, C, top, red);
    __syncthreads();
    if (t < C) {
        const u64 c = top[t];
        float acc = -INFINITY;
        if (c) {
            const int k = (int)(cand_index(c) / (unsigned)V), v = (int)(cand_index(c) % (unsigned)V), row = g * K + k;
            acc = beam_acc(a, a.logits[(size_t)row * V + v], rowmax, rowlog, row);       // the unperturbed value
        }
        a.out_v[(size_t)g * C + t] = acc;
        a.out_i[(size_t)g * C + t] = c ? (int64_t)cand_index(c) : 0;
    }
    if (a.info && t < K) {
        const int row = g * K + t;
        const unsigned theta = beam_theta(a, rawtop, theta_s, row);
        int kept = 0;
        for (int s = 0; s < S; ++s) kept += pcnt[row * S + s];
        float* o = a.info + (size_t)row * 4;
        o[0] = theta == 0u ? -INFINITY : key_value(theta);
        o[1] = (float)kept;
        o[2] = rowmax[row];
        o[3] = rowlog[row];
    }
}

struct TopkWs { u64* keys; float* pmax; float* psum; u64* rowtop; float* rowmax; float* rowlog; };

size_t al256b(size_t x) { return (x + 255) & ~(size_t)255; }

TopkWs carve_topk(void* base)
{
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = p + off; off += al256b(bytes); return q; };
    TopkWs w;
    w.keys = (u64*)take((size_t)8 * RMAX * SMAXB * CMAX);
    w.pmax = (float*)take(4 * RMAX * SMAXB);
    w.psum = (float*)take(4 * RMAX * SMAXB);
    w.rowtop = (u64*)take(8 * RMAX * CMAX);
    w.rowmax = (float*)take(4 * RMAX);
    w.rowlog = (float*)take(4 * RMAX);
    return w;
}

// one direction of the reorder: row r of `dst` = row (indirect ? src[r] : r) of `from`, for the rows with src[r] != r
struct CacheMove {
    const char* from_k = nullptr;      // K and V of one layer, rows of nkv * cap * hd bf16 (NULL: this launch moves no layer in this direction)
    const char* from_v = nullptr;
    char* to_k = nullptr;
    char* to_v = nullptr;
    const unsigned char* from_m = nullptr;     // the key-valid mask rows [cap] and the next positions (NULL: not in this launch)
    unsigned char* to_m = nullptr;
    const int64_t* from_p = nullptr;
    int64_t* to_p = nullptr;
    int indirect = 0;
};

struct CacheMoveArgs {
    CacheMove job[2];                  // blockIdx.z: 0 = gather a layer into the scratch, 1 = copy the previous layer back from it
    const int64_t* src;
    int rows_in, rows_out, nkv, hd, cap;
    const int* len;
    int* status;
    int* status_host;
};

__global__ __launch_bounds__(256) void dec_cache_move_kernel(CacheMoveArgs a)
{
    __shared__ int bad;
    const CacheMove& j = a.job[blockIdx.z];
    const int t = threadIdx.x;
    if (t == 0) bad = 0;
    __syncthreads();
    if (t < a.rows_out) {
        const int64_t s = a.src[t];
        if (s < 0 || s >= a.rows_in) bad = 1;
    }
    __syncthreads();
    const int st = *(volatile const int*)a.status;
    if (bad) {                                                   // every workgroup of every launch finds the same: nothing is written
        if (!st && t == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
            *a.status = 3;
            if (a.status_host) *a.status_host = 3;
        }
        return;
    }
    if (st) return;
    const int per_row = 2 * a.nkv + 1, r = blockIdx.y / per_row, w = blockIdx.y % per_row;
    const int64_t s = a.src[r];
    if (s == r) return;
    const int64_t from = j.indirect ? s : r;
    const int len = min(*a.len, a.cap);
    if (w < 2 * a.nkv) {
        if (!j.to_k) return;
        const size_t head = (size_t)a.cap * a.hd * 2, off = (size_t)(w >> 1) * head, rowb = (size_t)a.nkv * head;
        const u32x4* sp = (const u32x4*)(((w & 1) ? j.from_v : j.from_k) + from * rowb + off);
        u32x4* dp = (u32x4*)(((w & 1) ? j.to_v : j.to_k) + r * rowb + off);
        const int n16 = len * a.hd / 8;                          // hd % 8 == 0: whole 16-byte words
        for (int i = blockIdx.x * 256 + t; i < n16; i += gridDim.x * 256) dp[i] = sp[i];
    } else {
        if (!j.to_m) return;
        for (int i = blockIdx.x * 256 + t; i < len; i += gridDim.x * 256) j.to_m[(size_t)r * a.cap + i] = j.from_m[from * a.cap + i];
        if (blockIdx.x == 0 && t == 0) j.to_p[r] = j.from_p[from];
    }
}

// ---- the rows' processor histories and automaton states behind the KV reorder (DecHistGatherArgs) ---------------------------------------------
// New row r = old row src[r] of: the first count[src[r]] history entries (sign bits and all), the seen-bitmap's W words, the count, the
// constraint's state and flag words.  dec_cache_move's rules: through a scratch, never in place (launch 0 gathers into it, launch 1 copies back);
// rows with src[r] == r leave at once; every workgroup checks all of src first.  grid (x, rows_out): the x workgroups of a row stride over it.
static_assert(RMAX <= 256, "dec_cache_move / dec_hist_move check all of src with one thread per row of one 256-thread workgroup");
struct HistScratch { int* hist; unsigned* seen; int* count; int* state; int* flags; size_t bytes; };

HistScratch carve_hist(char* base, int batch, int cap, int W)
{
    HistScratch h;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = base + off; off += (bytes + 255) & ~(size_t)255; return q; };
    h.hist = (int*)take((size_t)batch * cap * 4);
    h.seen = (unsigned*)take((size_t)batch * W * 4);
    h.count = (int*)take((size_t)batch * 4);
    h.state = (int*)take(RMAX * 4);
    h.flags = (int*)take(RMAX * 4);
    h.bytes = off;
    return h;
}

__global__ __launch_bounds__(256) void dec_hist_move_kernel(DecHistGatherArgs a, HistScratch sc, int back)
{
    __shared__ int bad;
    const int t = threadIdx.x;
    if (t == 0) bad = 0;
    __syncthreads();
    if (t < a.rows_out) {
        const int64_t s = a.src[t];
        if (s < 0 || s >= a.rows_in) bad = 1;
    }
    __syncthreads();
    const int st = *(volatile const int*)a.status;
    if (bad) {                                                   // every workgroup of both launches finds the same: nothing is written
        if (!st && t == 0 && blockIdx.x == 0 && blockIdx.y == 0) {
            *a.status = 3;
            if (a.status_host) *a.status_host = 3;
        }
        return;
    }
    if (st) return;
    const int r = blockIdx.y, W = (a.V + 31) / 32;
    const int64_t s = a.src[r];
    if (s == r) return;
    const int64_t from = back ? r : s;
    const bool one = blockIdx.x == 0 && t == 0;
    if (a.hist) {
        const int* fc = back ? sc.count : a.count;
        const int* fh = back ? sc.hist : a.hist;
        const unsigned* fs = back ? sc.seen : a.seen;
        int* th = back ? a.hist : sc.hist;
        unsigned* ts = back ? a.seen : sc.seen;
        const int n = max(0, min(fc[from], a.cap));
        for (int i = blockIdx.x * 256 + t; i < n; i += gridDim.x * 256) th[(size_t)r * a.cap + i] = fh[from * a.cap + i];
        for (int i = blockIdx.x * 256 + t; i < W; i += gridDim.x * 256) ts[(size_t)r * W + i] = fs[from * W + i];
        if (one) (back ? a.count : sc.count)[r] = fc[from];
    }
    if (a.states && one) {
        (back ? a.states : sc.state)[r] = (back ? sc.state : a.states)[from];
        (back ? a.flags : sc.flags)[r] = (back ? sc.flags : a.flags)[from];
    }
}

}  // namespace

extern "C" size_t fvhd_dec_hist_gather_ws_bytes(int batch, int cap, int V)
{
    return al256b((size_t)batch * cap * 4) + al256b((size_t)batch * ((V + 31) / 32) * 4) + al256b((size_t)batch * 4) + 2 * al256b(RMAX * 4);
}

extern "C" int fvhd_launch_dec_hist_gather(hipStream_t st, const DecHistGatherArgs* a)
{
    if (!a->src || !a->status || !a->ws || a->rows_in < 1 || a->rows_out < 1 || a->rows_in > a->batch || a->rows_out > a->batch || a->batch > RMAX ||
        a->cap < 1 || a->V < 1 || (a->hist && (!a->seen || !a->count)) || (a->states && !a->flags) || ((uintptr_t)a->ws & 15))
        return (int)hipErrorInvalidValue;
    if (!a->hist && !a->states) return 0;
    const int W = (a->V + 31) / 32, gx = a->hist ? std::min(8, (std::max(a->cap, W) + 255) / 256) : 1;
    const HistScratch sc = carve_hist(a->ws, a->batch, a->cap, W);
    for (int back = 0; back < 2; ++back) hipLaunchKernelGGL(dec_hist_move_kernel, dim3(gx, a->rows_out), dim3(256), 0, st, *a, sc, back);
    return (int)hipGetLastError();
}

// the normalisation's scratch: the slices' partials of RMAX rows
extern "C" size_t fvhd_dec_beam_norm_ws_bytes(void) { return 2 * al256b(4 * RMAX * SMAXB); }

extern "C" int fvhd_dec_beam_norm_supported(int rows, int V) { return rows >= 1 && rows <= RMAX && V >= 1 && V <= SLICE * SMAXB; }

extern "C" int fvhd_launch_dec_beam_norm(hipStream_t st, float* logits, int rows, int V, void* ws, float* stats, const int* status)
{
    if (!fvhd_dec_beam_norm_supported(rows, V) || !logits || !ws || ((uintptr_t)logits & 3)) return (int)hipErrorInvalidValue;
    float* pmax = (float*)ws;
    float* psum = (float*)((char*)ws + al256b(4 * RMAX * SMAXB));
    const int S = (V + SLICE - 1) / SLICE;
    hipLaunchKernelGGL(beam_norm_slice_kernel, dim3(S, rows), dim3(256), 0, st, logits, V, S, pmax, psum, status);
    hipLaunchKernelGGL(beam_norm_apply_kernel, dim3(S, rows), dim3(256), 0, st, logits, V, S, pmax, psum, stats, status);
    return (int)hipGetLastError();
}

extern "C" size_t fvhd_dec_beam_topk_ws_bytes(void)
{
    return al256b((size_t)8 * RMAX * SMAXB * CMAX) + 2 * al256b(4 * RMAX * SMAXB) + al256b(8 * RMAX * CMAX) + 2 * al256b(4 * RMAX);
}

extern "C" int fvhd_dec_beam_topk_supported(int G, int K, int C, int V)
{
    return G >= 1 && K >= 2 && K <= 16 && C >= 1 && C <= CMAX && C <= V && G * K <= RMAX && V >= 16 && V % 16 == 0 && V <= SLICE * SMAXB;
}

extern "C" int fvhd_launch_dec_beam_topk(hipStream_t st, const float* logits, const float* scores, int G, int K, int C, int V, float* out_v, int64_t* out_i,
                                         void* ws)
{
    return fvhd_launch_dec_beam_topk_mode(st, logits, scores, G, K, C, V, 0, out_v, out_i, ws);
}

// prenorm: the rows hold processed log-probabilities - acc = x + score, and a -inf entry is no candidate; the same three launches
extern "C" int fvhd_launch_dec_beam_topk_mode(hipStream_t st, const float* logits, const float* scores, int G, int K, int C, int V, int prenorm,
                                              float* out_v, int64_t* out_i, void* ws)
{
    if (!fvhd_dec_beam_topk_supported(G, K, C, V) || ((uintptr_t)logits & 15)) return (int)hipErrorInvalidValue;
    const TopkWs w = carve_topk(ws);
    const int rows = G * K, S = (V + SLICE - 1) / SLICE;
    hipLaunchKernelGGL(beam_slice_kernel, dim3(S, rows), dim3(256), 0, st, logits, V, S, C, w.keys, w.pmax, w.psum);
    hipLaunchKernelGGL(beam_row_kernel, dim3(rows), dim3(256), 0, st, w.keys, w.pmax, w.psum, S, C, w.rowtop, w.rowmax, w.rowlog);
    hipLaunchKernelGGL(beam_group_kernel, dim3(G), dim3(256), 0, st, w.rowtop, w.rowmax, w.rowlog, scores, K, C, V, prenorm, out_v, out_i);
    return (int)hipGetLastError();
}

// two top-K workspaces (the raw pass, the perturbed pass), the rows' thresholds, the slices' kept counts, the sampler's workspace
extern "C" size_t fvhd_dec_beam_sample_ws_bytes(void)
{
    return 2 * al256b(fvhd_dec_beam_topk_ws_bytes()) + al256b(4 * RMAX) + al256b(4 * RMAX * SMAXB) + al256b(fvhd_dec_sample_ws_bytes());
}

extern "C" int fvhd_launch_dec_beam_sample(hipStream_t st, const DecBeamSampleArgs* a, void* ws)
{
    if (!fvhd_dec_beam_topk_supported(a->G, a->K, a->keep, a->V) || ((uintptr_t)a->logits & 15) || !a->scores || !a->out_v || !a->out_i || !ws ||
        !(a->temperature > 0.f) || a->top_k < 0 || !(a->top_p >= 0.f && a->top_p <= 1.f) || a->min_keep < 1 || a->min_keep > a->keep ||
        ((uintptr_t)a->noise_override & 15) || ((uintptr_t)a->noise_out & 15))
        return (int)hipErrorInvalidValue;
    char* p = (char*)ws;
    const TopkWs raw = carve_topk(p), sel = carve_topk(p + al256b(fvhd_dec_beam_topk_ws_bytes()));
    p += 2 * al256b(fvhd_dec_beam_topk_ws_bytes());
    unsigned* theta = (unsigned*)p;
    int* pcnt = (int*)(p + al256b(4 * RMAX));
    void* sws = p + al256b(4 * RMAX) + al256b(4 * RMAX * SMAXB);
    const int rows = a->G * a->K, V = a->V, m = a->min_keep, C = a->keep, S = (V + SLICE - 1) / SLICE;
    hipLaunchKernelGGL(beam_slice_kernel, dim3(S, rows), dim3(256), 0, st, a->logits, V, S, m, raw.keys, raw.pmax, raw.psum);
    hipLaunchKernelGGL(beam_row_kernel, dim3(rows), dim3(256), 0, st, raw.keys, raw.pmax, raw.psum, S, m, raw.rowtop, raw.rowmax, raw.rowlog);
    const int top_k = a->top_k > 0 ? std::max(a->top_k, m) : 0;  // TopKLogitsWarper: max(top_k, min_tokens_to_keep)
    const bool filtered = (top_k > 0 && top_k < V) || a->top_p < 1.f;
    if (filtered) {
        DecSampleArgs sa;
        sa.logits = a->logits; sa.B = rows; sa.V = V; sa.temperature = a->temperature; sa.top_k = top_k; sa.top_p = a->top_p;
        if (int e = fvhd_launch_dec_sample_theta(st, &sa, sws, theta)) return e;
    }
    const unsigned* th = filtered ? theta : nullptr;
    hipLaunchKernelGGL(beam_sample_slice_kernel, dim3(S, rows), dim3(256), 0, st, *a, S, raw.rowtop, th, sel.keys, pcnt);
    // (M and L again from the same partials: the same bits)
    hipLaunchKernelGGL(beam_row_kernel, dim3(rows), dim3(256), 0, st, sel.keys, raw.pmax, raw.psum, S, C, sel.rowtop, sel.rowmax, sel.rowlog);
    hipLaunchKernelGGL(beam_sample_group_kernel, dim3(a->G), dim3(256), 0, st, *a, S, sel.rowtop, sel.rowmax, sel.rowlog, raw.rowtop, th, pcnt);
    return (int)hipGetLastError();
}

// scratch: two halves of (K | V of `rows` rows), then `rows` mask rows, then `rows` positions
extern "C" size_t fvhd_dec_cache_gather_ws_bytes(int rows, int nkv, int hd, int cap)
{
    const size_t rowb = (size_t)nkv * cap * hd * 2;
    return 4 * al256b((size_t)rows * rowb) + al256b((size_t)rows * cap) + al256b((size_t)rows * 8);
}

extern "C" int fvhd_launch_dec_cache_gather(hipStream_t st, const DecCacheGatherArgs* g)
{
    if (g->layers < 1 || g->rows_in < 1 || g->rows_out < 1 || g->rows_in > g->batch || g->rows_out > g->batch || g->batch > RMAX || g->nkv < 1 ||
        g->hd < 8 || g->hd % 8 || g->cap < 1 || ((uintptr_t)g->kc & 15) || ((uintptr_t)g->vc & 15) || ((uintptr_t)g->ws & 15))
        return (int)hipErrorInvalidValue;
    const size_t rowb = (size_t)g->nkv * g->cap * g->hd * 2, layer = (size_t)g->batch * rowb, half = al256b((size_t)g->batch * rowb);
    char* sm = g->ws + 4 * half;
    char* sp = sm + al256b((size_t)g->batch * g->cap);
    CacheMoveArgs a;
    a.src = g->src; a.rows_in = g->rows_in; a.rows_out = g->rows_out; a.nkv = g->nkv; a.hd = g->hd; a.cap = g->cap; a.len = g->len;
    a.status = g->status; a.status_host = g->status_host;
    const int gx = (int)std::min<size_t>(8, ((size_t)g->cap * g->hd / 8 + 255) / 256);
    for (int i = 0; i <= g->layers; ++i) {
        a.job[0] = CacheMove();
        a.job[1] = CacheMove();
        if (i < g->layers) {
            CacheMove& m = a.job[0];
            char* h = g->ws + 2 * half * (i & 1);
            m.from_k = g->kc + i * layer; m.from_v = g->vc + i * layer; m.to_k = h; m.to_v = h + half; m.indirect = 1;
            if (i == 0) { m.from_m = g->mask; m.to_m = (unsigned char*)sm; m.from_p = g->posv; m.to_p = (int64_t*)sp; }
        }
        if (i > 0) {
            CacheMove& m = a.job[1];
            char* h = g->ws + 2 * half * ((i - 1) & 1);
            m.from_k = h; m.from_v = h + half; m.to_k = g->kc + (i - 1) * layer; m.to_v = g->vc + (i - 1) * layer;
            if (i == 1) { m.from_m = (const unsigned char*)sm; m.to_m = g->mask; m.from_p = (const int64_t*)sp; m.to_p = g->posv; }
        }
        hipLaunchKernelGGL(dec_cache_move_kernel, dim3(gx, g->rows_out * (2 * g->nkv + 1), 2), dim3(256), 0, st, a);
    }
    return (int)hipGetLastError();
}
