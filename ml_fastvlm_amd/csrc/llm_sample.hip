// Token sampling on the device: temperature / top-k / top-p over the fp32 logits [B][V] of the lm_head (include/fvhd.h "LLM sampling").
//
// transformers' multinomial sampling for num_beams = 1 (min_tokens_to_keep = 1), in the order of its logits processors:
//   s = logits / T (IEEE division), top-k keeps s >= the min(k, V)-th largest value (ties kept), top-p keeps a token when the
//   normalised mass of the tokens before it (descending s) is < top_p, then one draw from the softmax over the kept set.
// Both filters keep a prefix by value, so the kept set is {i : s_i >= theta} for one threshold per row; tokens tied at the top-p
// boundary are kept as a group (transformers' unstable sort may split them).  A -inf logit (a suppressed token) is never kept, never
// counted and never drawn, also when no filter is on or the top-k threshold itself is -inf.  A row needs one finite logit: a row of
// -inf only has s_max = -inf and NaN masses, its result is undefined (include/fvhd.h).
//
// Launches (grid = S slices x B rows, 256 threads; each pass reads the whole row, the slices meet in the last-arriving workgroup of the
// row as in the decode GEMM's split-K):
//   dec_sample_max      the row maximum -> s_max, and the row's search state
//   dec_sample_level    one 8-bit digit of the threshold's order-preserving 32-bit key per launch (MSB first): a 256-bin histogram of
//                       counts and exp(s - s_max) masses of the keys that match the digits found so far; 4 launches find the top-k
//                       threshold (by count), 4 more the top-p threshold among its kept set (by mass).  The histograms sum integers
//                       (counts, and masses in 2^-40 fixed point) so their totals do not depend on the order of the LDS adds; there
//                       are no floating-point atomics.
//   dec_sample_draw     Z = sum of exp(s - s_max) over the kept set (per-thread contiguous chunks in index order, chunk sums scanned in a
//                       fixed order), u from Philox4x32-10, and the inverse CDF in TOKEN-INDEX order: the smallest kept index whose
//                       prefix mass is > u * Z (the last kept token if rounding finds none).  Same distribution as a draw in sorted
//                       order, no sort.  Then the ids, the optional info row, and - behind every row - the advance of positions / length.
// The warpers behind top-p (fvhd_llm_set_sampling_warpers; off by default, and then the launches above are all there is), in
// transformers' order, each on the set K the earlier ones left; x = s - s_max, e = expf(x), Z = sum e over K, A = sum e x over K / Z:
//   min_p            keeps e >= min_p (p >= min_p p_max: Z cancels) - a term in the predicate of the passes behind it, no launch
//   typical_p        dec_sample_stats (Z, A), then dec_sample_tlevel x 4: the digit search over the bits of d = |x - A| (= |-log p - H|: log Z
//                    cancels) by mass, keeping the smallest keys; a group of equal d is kept iff the mass below it is < typical_p Z
//   epsilon_cutoff   dec_sample_stats, then e >= eps Z or s = the largest s of K (which typical_p may have moved below s_max)
//   eta_cutoff       dec_sample_stats, then the same with eta = min(eps, sqrt(eps) exp(-H)), H = log Z - A
// Behind them the kept set is KeepSet's predicate on (s, e, d) with the row's constants (WarpRow) instead of {s >= theta}; the draw and its
// re-walk use it (dec_sample_draw_warp).  The statistics are sums of 2^-40 fixed-point integers; their slice partials and the WarpRow lie in
// slabs that are idle at that point (hc / hm, pmax), so the workspace is what it was.
// DecSampleArgs.seq_rows: the rows are T <= 16 consecutive positions of ONE sequence (the verify step of llm_spec.hip).  Row r draws with the
// Philox counter (seq_row, n + r, 0, 0), the counter of the plain step at that position, and the launch writes the ids (and info) only.
// Everything is deterministic: the same logits, settings, seed and n give the same id, eager or replayed.
#include "fvhd_common.h"
#include "launchers.h"      // (with llm_decode.h: the argument structs)
#include "sample_rng.h"     // scaled, philox_x0
#include "split_handoff.h"  // arrive_last

namespace {

constexpr int SMAX = 32;                         // slices per row
constexpr int BMAX = 16;                         // rows per launch (a wider batch runs in blocks of BMAX rows, fvhd_launch_dec_sample)
enum { SM_TOPK = 1, SM_TOPP = 2, SM_DRAW = 3, SM_TYP = 4 };
enum { ST_MINP = 1, ST_TYP = 2, ST_EPS = 3, ST_ETA = 4 };                         // the warper stages behind top-p, in transformers' order

struct SampleRow {                               // per-row search state, written by the row's last-arriving workgroup
    float smax;
    unsigned prefix;                             // the threshold key's digits found so far
    int shift;                                   // bit position of the next digit (24 .. 0)
    int mode;
    unsigned cnt_above;                          // keys above the prefix (and >= lo_key)
    unsigned lo_key;                             // top-p after top-k: only keys >= the top-k threshold take part
    unsigned theta_key;                          // SM_DRAW: the kept set is {key >= theta_key}
    int target_set;
    unsigned long long mass_above;               // fixed-point mass of those keys
    unsigned long long target;                   // top-p: top_p * Z_k, fixed point
};

// per-row constants of the warpers behind top-p, written by the last-arriving workgroup of the statistics pass in front of each stage.
// It lives in the row's pmax slab, which is idle once dec_sample_max has run (SMAX floats = 128 bytes a row).
struct WarpRow {
    float A;                                     // typical_p: sum e (s - M) / Z over the set it acts on; its key is d = |(s - M) - A|
    unsigned dstar;                              // typical_p resolved: the kept tokens have bits(d) <= dstar
    float efl_eps, efl_eta;                      // epsilon_cutoff / eta_cutoff: the floor on e (cutoff * Z of the set the stage acts on)
    unsigned top_eps, top_eta;                   // the largest key of that set: tokens tied at it always stay
    unsigned c_minp, c_typ, c_eps;               // kept counts behind min_p, typical_p, epsilon_cutoff (each where a later stage ran)
};
static_assert(sizeof(WarpRow) <= 4 * SMAX, "WarpRow lives in a row's pmax slab");

struct SampleWs {
    SampleRow* rows;                             // [BMAX]
    float* pmax;                                 // [BMAX][SMAX]; behind dec_sample_max: the row's WarpRow
    unsigned* hc;                                // [BMAX][SMAX][256]
    unsigned long long* hm;                      // [BMAX][SMAX][256]
    float* dpre;                                 // [BMAX][SMAX][256] exclusive prefix of the chunk masses within the slice
    float* dchunk;                               // [BMAX][SMAX][256] chunk masses
    float* dsum;                                 // [BMAX][SMAX] slice mass
    int* dlast;                                  // [BMAX][SMAX] last kept index of the slice (-1: none)
    unsigned* dcnt;                              // [BMAX][SMAX] kept count of the slice
    int* cnt;                                    // [BMAX + 1] arrival counters (zero between launches)
};

size_t al256s(size_t x) { return (x + 255) & ~(size_t)255; }

SampleWs carve(void* base)
{
    char* p = (char*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* q = p + off; off += al256s(bytes); return q; };
    SampleWs w;
    w.rows = (SampleRow*)take(sizeof(SampleRow) * BMAX);
    w.pmax = (float*)take(4 * BMAX * SMAX);
    w.hc = (unsigned*)take(4 * BMAX * SMAX * 256);
    w.hm = (unsigned long long*)take(8 * BMAX * SMAX * 256);
    w.dpre = (float*)take(4 * BMAX * SMAX * 256);
    w.dchunk = (float*)take(4 * BMAX * SMAX * 256);
    w.dsum = (float*)take(4 * BMAX * SMAX);
    w.dlast = (int*)take(4 * BMAX * SMAX);
    w.dcnt = (unsigned*)take(4 * BMAX * SMAX);
    w.cnt = (int*)take(4 * (BMAX + 1));
    return w;
}

size_t ws_bytes()
{
    return al256s(sizeof(SampleRow) * BMAX) + 2 * al256s(4 * BMAX * SMAX) + al256s(4 * BMAX * SMAX * 256) + al256s(8 * BMAX * SMAX * 256) +
           2 * al256s(4 * BMAX * SMAX * 256) + 2 * al256s(4 * BMAX * SMAX) + al256s(4 * (BMAX + 1));
}

// order-preserving key of an fp32 value: a > b <=> key(a) > key(b); -0 and +0 share one key
FVHD_DEV unsigned okey(float s)
{
    unsigned u = __float_as_uint(s);
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

FVHD_DEV float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

FVHD_DEV unsigned long long fixed_mass(float e) { return (unsigned long long)(e * 0x1p40f); }

// slice s of S over a row of V: [i0, i1)
FVHD_DEV void slice_of(int V, int S, int s, int& i0, int& i1)
{
    const int L = (V + S - 1) / S;
    i0 = min(s * L, V);
    i1 = min(i0 + L, V);
}

// inclusive scan over 256 threads in LDS (Hillis-Steele; a fixed order of additions)
template <typename T>
FVHD_DEV T block_scan_incl(T v, T* buf)
{
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const T add = tid >= o ? buf[tid - o] : (T)0;
        __syncthreads();
        v += add;
        buf[tid] = v;
        __syncthreads();
    }
    return v;
}

FVHD_DEV WarpRow* warp_row(const SampleWs& w, int b) { return (WarpRow*)(w.pmax + b * SMAX); }

// which warpers behind top-p are on (DecSampleArgs: the off values are 0, 1, 0, 0)
__host__ __device__ inline bool minp_on(const DecSampleArgs& a) { return a.min_p > 0.f; }
__host__ __device__ inline bool typ_on(const DecSampleArgs& a) { return a.typical_p < 1.f; }
__host__ __device__ inline bool eps_on(const DecSampleArgs& a) { return a.epsilon_cutoff > 0.f; }
__host__ __device__ inline bool eta_on(const DecSampleArgs& a) { return a.eta_cutoff > 0.f; }

// typical_p's key: the fp32 bits of d = |(s - M) - A| (d >= 0, so its bits order it)
FVHD_DEV unsigned dkey(float v, float M, float A) { return __float_as_uint(fabsf((v - M) - A)); }

// The kept set behind the stages before `upto` (ST_MINP: top-k / top-p only ... ST_ETA + 1: everything).  v = s, e = expf(v - M).
struct KeepSet {
    unsigned theta;
    float M, min_p;
    bool minp, typ, eps, eta;
    WarpRow wr;
    FVHD_DEV KeepSet(const DecSampleArgs& a, const SampleRow& r, const WarpRow* p, int upto)
    {
        theta = r.theta_key;
        M = r.smax;
        min_p = a.min_p;
        minp = minp_on(a) && upto > ST_MINP;
        typ = typ_on(a) && upto > ST_TYP;
        eps = eps_on(a) && upto > ST_EPS;
        eta = eta_on(a) && upto > ST_ETA;
        wr = WarpRow{};
        if (typ || eps || eta) wr = *p;
    }
    FVHD_DEV bool operator()(float v, float e) const
    {
        const unsigned k = okey(v);
        if (!(k >= theta && v > -INFINITY)) return false;                      // a -inf logit is never kept
        if (minp && !(e >= min_p)) return false;
        if (typ && !(dkey(v, M, wr.A) <= wr.dstar)) return false;
        if (eps && !(e >= wr.efl_eps || k == wr.top_eps)) return false;
        if (eta && !(e >= wr.efl_eta || k == wr.top_eta)) return false;
        return true;
    }
};

// e (s - M) in signed 2^-40 fixed point (|e x| <= 1 / e: a row's sum stays far inside 63 bits)
FVHD_DEV long long fixed_signed(float y) { return (long long)(y * 0x1p40f); }

}  // namespace

// ---------------------------------------------------------------------------------------------------
// the row maximum (s_max = max(logits) / T: IEEE division is monotonic) and the initial search state
__global__ __launch_bounds__(256) void dec_sample_max_kernel(const DecSampleArgs a, const SampleWs w)
{
    if (a.status && *a.status) return;
    __shared__ float red[4];
    __shared__ int flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const float* x = a.logits + (size_t)(a.row0 + b) * a.V;
    int i0, i1;
    slice_of(a.V, S, s, i0, i1);
    float m = -INFINITY;
    for (int i = i0 + tid; i < i1; i += 256) m = fmaxf(m, x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) w.pmax[b * SMAX + s] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (!arrive_last(w.cnt + b, S, &flag)) return;
    if (tid == 0) {
        float M = -INFINITY;
        for (int t = 0; t < S; ++t) M = fmaxf(M, w.pmax[b * SMAX + t]);
        const bool topk = a.top_k > 0 && a.top_k < a.V, topp = a.top_p < 1.0f;
        SampleRow r;
        r.smax = scaled(M, a.temperature);
        r.prefix = 0;
        r.shift = 24;
        r.mode = topk ? SM_TOPK : topp ? SM_TOPP : SM_DRAW;
        r.cnt_above = 0;
        r.lo_key = 0;
        r.theta_key = 0;
        r.target_set = 0;
        r.mass_above = 0;
        r.target = 0;
        w.rows[b] = r;
    }
}

// one 8-bit digit of the threshold key (see the file comment)
__global__ __launch_bounds__(256) void dec_sample_level_kernel(const DecSampleArgs a, const SampleWs w)
{
    if (a.status && *a.status) return;
    __shared__ unsigned hc[256];
    __shared__ unsigned long long hm[256];
    __shared__ unsigned long long scan64[256];
    __shared__ unsigned scan32[256];
    __shared__ int flag, pick;
    const int tid = threadIdx.x, b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const SampleRow r = w.rows[b];
    if (r.mode != SM_TOPK && r.mode != SM_TOPP) return;                        // row resolved: every workgroup of it leaves
    hc[tid] = 0;
    hm[tid] = 0;
    __syncthreads();
    const float* x = a.logits + (size_t)(a.row0 + b) * a.V;
    int i0, i1;
    slice_of(a.V, S, s, i0, i1);
    const float T = a.temperature, M = r.smax;
    const int shift = r.shift;
    const unsigned pre = r.prefix, lo = r.lo_key;
    const bool top = shift == 24;
    for (int i = i0 + tid; i < i1; i += 256) {
        const float v = scaled(x[i], T);
        const unsigned k = okey(v);
        if (k >= lo && (top || (k >> (shift + 8)) == pre)) {
            const int d = (k >> shift) & 255;
            atomicAdd(&hc[d], 1u);
            atomicAdd(&hm[d], fixed_mass(expf(v - M)));
        }
    }
    __syncthreads();
    const size_t slab = ((size_t)b * SMAX + s) * 256 + tid;
    w.hc[slab] = hc[tid];
    w.hm[slab] = hm[tid];
    if (!arrive_last(w.cnt + b, S, &flag)) return;
    // the row's histogram: thread j = bin j; j' = 255 - j orders the bins by descending key, so an inclusive scan over j' gives the keys at
    // or above bin j
    const int j = 255 - tid;
    unsigned c = 0;
    unsigned long long m = 0;
    for (int t = 0; t < S; ++t) {
        c += w.hc[((size_t)b * SMAX + t) * 256 + j];
        m += w.hm[((size_t)b * SMAX + t) * 256 + j];
    }
    const unsigned c_incl = block_scan_incl<unsigned>(c, scan32);
    const unsigned long long m_incl = block_scan_incl<unsigned long long>(m, scan64);
    const unsigned above_c = r.cnt_above + c_incl - c;
    const unsigned long long above_m = r.mass_above + m_incl - m;
    unsigned long long target = r.target;
    if (r.mode == SM_TOPP && !r.target_set)                                     // top-p alone: Z over the whole row (the level-0 total)
        target = (unsigned long long)((double)a.top_p * (double)scan64[255]);
    if (tid == 0) pick = -1;
    __syncthreads();
    bool chosen;
    if (r.mode == SM_TOPK) {
        const unsigned need = (unsigned)a.top_k;
        chosen = c > 0 && above_c < need && above_c + c >= need;                // the bin holding the k-th largest key
    } else {
        // kept: nothing (or less than top_p of the mass) lies above; the top token always.  above_m grows with j', so the kept bins are
        // the j' up to the largest eligible one - the lowest kept key
        if (c > 0 && (above_m < target || above_m == 0)) atomicMax(&pick, tid);
        __syncthreads();
        chosen = tid == pick;
    }
    if (!chosen) return;
    SampleRow n = r;
    n.prefix = (top ? 0u : (pre << 8)) | (unsigned)j;
    n.cnt_above = above_c;
    n.mass_above = above_m;
    n.target = target;
    n.target_set = r.mode == SM_TOPP ? 1 : r.target_set;
    if (shift > 0) {
        n.shift = shift - 8;
    } else if (r.mode == SM_TOPK && a.top_p < 1.0f) {                           // top-k resolved: top-p over its kept set next
        n.mode = SM_TOPP;
        n.prefix = 0;
        n.shift = 24;
        n.lo_key = (pre << 8) | (unsigned)j;
        n.cnt_above = 0;
        n.mass_above = 0;
        n.target = (unsigned long long)((double)a.top_p * (double)(above_m + m));
        n.target_set = 1;
    } else {
        n.mode = SM_DRAW;
        n.theta_key = (pre << 8) | (unsigned)j;
    }
    w.rows[b] = n;
}

// The statistics of the set a warper stage acts on (the kept set behind the stages before `stage`): Z = sum e and sum e (s - M) in 2^-40
// fixed point, the count and the largest key - integers all, so no total depends on the order of the adds.  The slice partials lie in the
// first words of the slice's hc / hm slabs; the row's last workgroup turns the totals into the stage's constants (WarpRow).
__global__ __launch_bounds__(256) void dec_sample_stats_kernel(const DecSampleArgs a, const SampleWs w, const int stage)
{
    if (a.status && *a.status) return;
    __shared__ unsigned long long zsum, asum;
    __shared__ unsigned csum, tmax;
    __shared__ int flag;
    const int tid = threadIdx.x, b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const SampleRow r = w.rows[b];
    const KeepSet keep(a, r, warp_row(w, b), stage);
    if (tid == 0) { zsum = 0; asum = 0; csum = 0; tmax = 0; }
    __syncthreads();
    const float* x = a.logits + (size_t)(a.row0 + b) * a.V;
    int i0, i1;
    slice_of(a.V, S, s, i0, i1);
    const float T = a.temperature, M = r.smax;
    unsigned long long z = 0;
    long long as = 0;
    unsigned c = 0, km = 0;
    for (int i = i0 + tid; i < i1; i += 256) {
        const float v = scaled(x[i], T);
        const float e = expf(v - M);
        if (keep(v, e)) {                                                       // v is finite: e (v - M) is no NaN
            z += fixed_mass(e);
            as += fixed_signed(e * (v - M));
            ++c;
            km = max(km, okey(v));
        }
    }
    if (c) {
        atomicAdd(&zsum, z);
        atomicAdd(&asum, (unsigned long long)as);                               // two's complement: the sum is the signed sum
        atomicAdd(&csum, c);
        atomicMax(&tmax, km);
    }
    __syncthreads();
    if (tid == 0) {
        const size_t slab = ((size_t)b * SMAX + s) * 256;
        w.hm[slab] = zsum;
        w.hm[slab + 1] = asum;
        w.hc[slab] = csum;
        w.hc[slab + 1] = tmax;
    }
    if (!arrive_last(w.cnt + b, S, &flag)) return;
    if (tid != 0) return;
    unsigned long long Zf = 0, Au = 0;
    unsigned cnt = 0, top = 0;
    for (int t = 0; t < S; ++t) {
        const size_t slab = ((size_t)b * SMAX + t) * 256;
        Zf += w.hm[slab];
        Au += w.hm[slab + 1];
        cnt += w.hc[slab];
        top = max(top, w.hc[slab + 1]);
    }
    // Zf = 0: typical_p left only tokens of e < 2^-40 (the row maximum is not among them), which the fixed-point sums do not see.  The floors
    // are 0 then and a cutoff keeps that set whole, where transformers would cut against its tiny Z - masses below 2^-40 of the row's
    // largest are beyond what the sampler resolves anywhere (the top-p search has the same floor).
    const double Zd = (double)Zf * 0x1p-40, Ad = Zf ? (double)(long long)Au / (double)Zf : 0.0;
    WarpRow wr = *warp_row(w, b);
    if (stage == ST_TYP) {
        wr.c_minp = cnt;
        wr.A = (float)Ad;
        wr.dstar = 0;
        SampleRow n = r;                                                        // theta_key stays: the search is among the kept set
        n.mode = SM_TYP;
        n.prefix = 0;
        n.shift = 24;
        n.cnt_above = 0;
        n.mass_above = 0;
        n.target = (unsigned long long)((double)a.typical_p * (double)Zf);
        n.target_set = 1;
        w.rows[b] = n;
    } else if (stage == ST_EPS) {
        wr.c_typ = cnt;
        wr.efl_eps = (float)((double)a.epsilon_cutoff * Zd);
        wr.top_eps = top;
    } else {
        wr.c_eps = cnt;
        const double eps = (double)a.eta_cutoff, H = (Zf ? log(Zd) : 0.0) - Ad;
        wr.efl_eta = (float)(fmin(eps, sqrt(eps) * exp(-H)) * Zd);
        wr.top_eta = top;
    }
    *warp_row(w, b) = wr;
}

// one 8-bit digit of typical_p's threshold d*: dec_sample_level's search over the bits of d by mass, among the set behind min_p, keeping
// the SMALLEST keys - a group of equal d is kept iff the mass of the groups below it is < typical_p * Z (the first group always)
__global__ __launch_bounds__(256) void dec_sample_tlevel_kernel(const DecSampleArgs a, const SampleWs w)
{
    if (a.status && *a.status) return;
    __shared__ unsigned hc[256];
    __shared__ unsigned long long hm[256];
    __shared__ unsigned long long scan64[256];
    __shared__ int flag, pick;
    const int tid = threadIdx.x, b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const SampleRow r = w.rows[b];
    if (r.mode != SM_TYP) return;
    const KeepSet keep(a, r, warp_row(w, b), ST_TYP);
    const float A = warp_row(w, b)->A;
    hc[tid] = 0;
    hm[tid] = 0;
    __syncthreads();
    const float* x = a.logits + (size_t)(a.row0 + b) * a.V;
    int i0, i1;
    slice_of(a.V, S, s, i0, i1);
    const float T = a.temperature, M = r.smax;
    const int shift = r.shift;
    const unsigned pre = r.prefix;
    const bool top = shift == 24;
    for (int i = i0 + tid; i < i1; i += 256) {
        const float v = scaled(x[i], T);
        const float e = expf(v - M);
        if (!keep(v, e)) continue;
        const unsigned k = dkey(v, M, A);
        if (top || (k >> (shift + 8)) == pre) {
            const int d = (k >> shift) & 255;
            atomicAdd(&hc[d], 1u);
            atomicAdd(&hm[d], fixed_mass(e));
        }
    }
    __syncthreads();
    const size_t slab = ((size_t)b * SMAX + s) * 256 + tid;
    w.hc[slab] = hc[tid];
    w.hm[slab] = hm[tid];
    if (!arrive_last(w.cnt + b, S, &flag)) return;
    // thread j = bin j, ascending: an inclusive scan gives the mass at or below bin j
    unsigned c = 0;
    unsigned long long m = 0;
    for (int t = 0; t < S; ++t) {
        c += w.hc[((size_t)b * SMAX + t) * 256 + tid];
        m += w.hm[((size_t)b * SMAX + t) * 256 + tid];
    }
    const unsigned long long m_incl = block_scan_incl<unsigned long long>(m, scan64);
    const unsigned long long below_m = r.mass_above + m_incl - m;
    if (tid == 0) pick = -1;
    __syncthreads();
    if (c > 0 && (below_m < r.target || below_m == 0)) atomicMax(&pick, tid);   // below_m grows with j: the largest eligible bin holds d*
    __syncthreads();
    if (tid != pick) return;
    SampleRow n = r;
    n.prefix = (top ? 0u : (pre << 8)) | (unsigned)tid;
    n.mass_above = below_m;
    if (shift > 0) {
        n.shift = shift - 8;
    } else {
        n.mode = SM_DRAW;
        warp_row(w, b)->dstar = n.prefix;
    }
    w.rows[b] = n;
}

// Z, the draw in token-index order, the ids and the advance (see the file comment).  W: a warper behind top-p is on - the kept set is
// KeepSet's predicate on (s, e, d) instead of {s >= theta}, and the info8 row is written.
template <bool W>
FVHD_DEV void dec_sample_draw(const DecSampleArgs& a, const SampleWs& w)
{
    if (a.status && *a.status) return;
    __shared__ float scan[256];
    __shared__ float ssum[SMAX];
    __shared__ int slast[SMAX];
    __shared__ unsigned scnt[SMAX];
    __shared__ int flag, pick_t, pick_s, pick_id;
    __shared__ float base_s, target_s, z_s, u_s;
    __shared__ unsigned kept_s;
    __shared__ int ilast[4];
    __shared__ unsigned icnt[4];
    __shared__ unsigned ikmin[4], ikmax[4], kmin_s, kmax_s;                     // W only
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const int row = a.row0 + b;                                                 // the batch row: b indexes the workspace only
    const SampleRow r = w.rows[b];
    const float* x = a.logits + (size_t)(a.row0 + b) * a.V;
    const float T = a.temperature, M = r.smax;
    const unsigned theta = r.mode == SM_DRAW ? r.theta_key : 0u;
    const KeepSet keep(a, r, warp_row(w, b), W ? ST_ETA + 1 : 0);               // W only
    unsigned kmin = 0xffffffffu, kmax = 0;
    int i0, i1;
    slice_of(a.V, S, s, i0, i1);
    const int C = (i1 - i0 + 255) / 256;
    const int c0 = min(i0 + tid * C, i1), c1 = min(c0 + C, i1);
    float local = 0.f;
    int last = -1;
    unsigned cnt = 0;
    for (int i = c0; i < c1; ++i) {
        const float v = scaled(x[i], T);
        if constexpr (W) {
            const float e = expf(v - M);
            if (keep(v, e)) { local += e; last = i; ++cnt; kmin = min(kmin, okey(v)); kmax = max(kmax, okey(v)); }
        } else {
            if (okey(v) >= theta && v > -INFINITY) { local += expf(v - M); last = i; ++cnt; }  // a -inf logit is never kept
        }
    }
    const float incl = block_scan_incl<float>(local, scan);
    const size_t slab = ((size_t)b * SMAX + s) * 256 + tid;
    w.dpre[slab] = incl - local;
    w.dchunk[slab] = local;
    int lm = last;
    unsigned cs = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lm = max(lm, __shfl_xor(lm, o, 64)); cs += __shfl_xor(cs, o, 64); }
    if (lane == 0) { ilast[wave] = lm; icnt[wave] = cs; }
    if constexpr (W) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, o, 64)); kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64)); }
        if (lane == 0) { ikmin[wave] = kmin; ikmax[wave] = kmax; }
    }
    __syncthreads();
    if (tid == 0) {
        w.dlast[b * SMAX + s] = max(max(ilast[0], ilast[1]), max(ilast[2], ilast[3]));
        w.dcnt[b * SMAX + s] = icnt[0] + icnt[1] + icnt[2] + icnt[3];
        if constexpr (W) {                                                      // the slice's lowest / highest kept key: hc is idle here
            w.hc[((size_t)b * SMAX + s) * 256] = min(min(ikmin[0], ikmin[1]), min(ikmin[2], ikmin[3]));
            w.hc[((size_t)b * SMAX + s) * 256 + 1] = max(max(ikmax[0], ikmax[1]), max(ikmax[2], ikmax[3]));
        }
    }
    if (tid == 255) w.dsum[b * SMAX + s] = incl;                                // the slice total: the scan's last element
    if (!arrive_last(w.cnt + b, S, &flag)) return;
    if (tid < S) {
        ssum[tid] = w.dsum[b * SMAX + tid];
        slast[tid] = w.dlast[b * SMAX + tid];
        scnt[tid] = w.dcnt[b * SMAX + tid];
    }
    if (tid == 0) pick_t = 256;
    __syncthreads();
    if (tid == 0) {
        float Z = 0.f;
        unsigned kept = 0;
        int lastk = -1;
        for (int t = 0; t < S; ++t) { Z += ssum[t]; kept += scnt[t]; lastk = max(lastk, slast[t]); }
        if constexpr (W) {
            unsigned lo = 0xffffffffu, hi = 0;
            for (int t = 0; t < S; ++t) { lo = min(lo, w.hc[((size_t)b * SMAX + t) * 256]); hi = max(hi, w.hc[((size_t)b * SMAX + t) * 256 + 1]); }
            kmin_s = lo;
            kmax_s = hi;
        }
        float u;
        if (a.u_override) {
            u = a.u_override[row];
        } else {
            // the rows of one sequence: row r draws with the counter of the plain step at its position
            const int n = (a.len ? *a.len : 0) + a.n_add + (a.seq_rows ? row : 0);
            u = (float)(philox_x0((unsigned)(a.seq_rows ? a.seq_row : row), (unsigned)n, 0u, 0u, (unsigned)a.seed, (unsigned)(a.seed >> 32)) >> 8) * 0x1p-24f;
        }
        const float target = u * Z;
        float cum = 0.f;
        int ps = -1;
        for (int t = 0; t < S; ++t) {
            if (scnt[t] > 0 && cum + ssum[t] > target) { ps = t; break; }
            cum += ssum[t];
        }
        pick_s = ps;
        pick_id = ps < 0 ? lastk : -1;
        base_s = cum;
        target_s = target;
        z_s = Z;
        u_s = u;
        kept_s = kept;
    }
    __syncthreads();
    const int ps = pick_s;
    if (ps >= 0) {
        const size_t sl = ((size_t)b * SMAX + ps) * 256 + tid;
        const float base = base_s + w.dpre[sl], ch = w.dchunk[sl];
        if (ch > 0.f && base + ch > target_s) atomicMin(&pick_t, tid);
        __syncthreads();
        if (tid == pick_t) {                                                     // walk the chunk with the sum order of the first pass
            int p0, p1;
            slice_of(a.V, S, ps, p0, p1);
            const int Cp = (p1 - p0 + 255) / 256;
            const int q0 = min(p0 + tid * Cp, p1), q1 = min(q0 + Cp, p1);
            float acc = 0.f;
            int id = -1;
            for (int i = q0; i < q1; ++i) {
                const float v = scaled(x[i], T);
                bool in;
                if constexpr (W) in = keep(v, expf(v - M));
                else in = okey(v) >= theta && v > -INFINITY;
                if (in) {
                    acc += expf(v - M);
                    id = i;
                    if (base + acc > target_s) break;
                }
            }
            pick_id = id;
        }
        __syncthreads();
        if (tid == 0 && pick_id < 0) pick_id = slast[ps];                       // rounding: the slice's last kept token
    }
    __syncthreads();
    if (tid == 0) {
        const int64_t id = pick_id < 0 ? 0 : pick_id;
        if (a.last && !a.seq_rows) a.last[row] = id;
        if (a.ids_out) a.ids_out[row] = id;
        if (a.posv && !a.seq_rows) a.posv[row] += 1;
        if (a.info) {
            a.info[row * 4 + 0] = theta == 0u ? -INFINITY : key_value(theta);
            a.info[row * 4 + 1] = (float)kept_s;
            a.info[row * 4 + 2] = z_s;
            a.info[row * 4 + 3] = u_s;
        }
        if constexpr (W) {
            if (a.info8) {
                // a stage's count was taken by the statistics pass of the next stage that is on; behind the last one it is the final count
                const WarpRow wr = *warp_row(w, b);
                const unsigned c_eps = eta_on(a) ? wr.c_eps : kept_s, c_typ = eps_on(a) ? wr.c_typ : c_eps, c_minp = typ_on(a) ? wr.c_minp : c_typ;
                float* o = a.info8 + (size_t)row * 8;
                o[0] = kept_s ? key_value(kmin_s) : INFINITY;
                o[1] = (float)kept_s;
                o[2] = z_s;
                o[3] = u_s;
                o[4] = kept_s ? key_value(kmax_s) : -INFINITY;
                o[5] = (float)c_minp;
                o[6] = (float)c_typ;
                o[7] = (float)c_eps;
            }
        }
    }
    // every row has read n (the earlier blocks of a wide batch ran before this launch): the last row to get here advances the length
    if (a.len_advance && !a.seq_rows && arrive_last(w.cnt + BMAX, gridDim.y, &flag) && tid == 0) *a.len_advance += 1;
}

// two kernels, so that the one a launch without warpers takes keeps its name and its code
__global__ __launch_bounds__(256) void dec_sample_draw_kernel(const DecSampleArgs a, const SampleWs w) { dec_sample_draw<false>(a, w); }
__global__ __launch_bounds__(256) void dec_sample_draw_warp_kernel(const DecSampleArgs a, const SampleWs w) { dec_sample_draw<true>(a, w); }

// the search's result of a block of rows, for a caller that does not draw (fvhd_launch_dec_sample_theta)
__global__ __launch_bounds__(64) void dec_sample_theta_kernel(const SampleWs w, int B, unsigned* __restrict__ theta_key)
{
    const int b = threadIdx.x;
    if (b < B) theta_key[b] = w.rows[b].mode == SM_DRAW ? w.rows[b].theta_key : 0u;
}

// ---------------------------------------------------------------------------------------------------
static int slices_of(int V) { return V >= SMAX * 2048 ? SMAX : (V + 2047) / 2048; }
static int levels_of(const DecSampleArgs& a) { return 4 * ((a.top_k > 0 && a.top_k < a.V) + (a.top_p < 1.f)); }

extern "C" size_t fvhd_dec_sample_ws_bytes(void) { return ws_bytes(); }

extern "C" int fvhd_launch_dec_sample(hipStream_t st, const DecSampleArgs* a, void* ws)
{
    if (!a->logits || !ws || a->B < 1 || a->B > 4 * BMAX || a->V < 1 || !(a->temperature > 0.f) || a->top_k < 0 || !(a->top_p >= 0.f && a->top_p <= 1.f))
        return (int)hipErrorInvalidValue;
    if (a->seq_rows && (a->B > BMAX || !a->ids_out)) return (int)hipErrorInvalidValue;      // one block of the workspace; the ids are its output
    if (!(a->min_p >= 0.f && a->min_p <= 1.f) || !(a->typical_p > 0.f && a->typical_p <= 1.f) || !(a->epsilon_cutoff >= 0.f && a->epsilon_cutoff < 1.f) ||
        !(a->eta_cutoff >= 0.f && a->eta_cutoff < 1.f))
        return (int)hipErrorInvalidValue;
    const bool warp = minp_on(*a) || typ_on(*a) || eps_on(*a) || eta_on(*a) || a->info8;    // off: today's launches, today's kernels
    const SampleWs w = carve(ws);
    const int S = slices_of(a->V);
    const int levels = levels_of(*a);
    // blocks of BMAX rows, one after the other on the stream (they share the workspace): every block reads the same n, the last one
    // advances the length
    for (int row0 = 0; row0 < a->B; row0 += BMAX) {
        DecSampleArgs blk = *a;
        blk.row0 = row0;
        blk.B = a->B - row0 < BMAX ? a->B - row0 : BMAX;
        if (row0 + BMAX < a->B) blk.len_advance = nullptr;
        const dim3 grid((unsigned)S, (unsigned)blk.B), block(256);
        hipLaunchKernelGGL(dec_sample_max_kernel, grid, block, 0, st, blk, w);
        for (int l = 0; l < levels; ++l) hipLaunchKernelGGL(dec_sample_level_kernel, grid, block, 0, st, blk, w);
        if (typ_on(*a)) {
            hipLaunchKernelGGL(dec_sample_stats_kernel, grid, block, 0, st, blk, w, (int)ST_TYP);
            for (int l = 0; l < 4; ++l) hipLaunchKernelGGL(dec_sample_tlevel_kernel, grid, block, 0, st, blk, w);
        }
        if (eps_on(*a)) hipLaunchKernelGGL(dec_sample_stats_kernel, grid, block, 0, st, blk, w, (int)ST_EPS);
        if (eta_on(*a)) hipLaunchKernelGGL(dec_sample_stats_kernel, grid, block, 0, st, blk, w, (int)ST_ETA);
        if (warp) hipLaunchKernelGGL(dec_sample_draw_warp_kernel, grid, block, 0, st, blk, w);
        else hipLaunchKernelGGL(dec_sample_draw_kernel, grid, block, 0, st, blk, w);
    }
    return (int)hipGetLastError();
}

// The threshold search alone (beam-search sampling, llm_beam.hip): the max and level passes of the launch above on temperature / top_k / top_p,
// stopping in front of the draw - theta_key[row] = the order-preserving key of the row's threshold on s (0: no filter binds).  Nothing else
// of the arguments is read or written: no ids, no positions, no length.
extern "C" int fvhd_launch_dec_sample_theta(hipStream_t st, const DecSampleArgs* a, void* ws, unsigned* theta_key)
{
    if (!a->logits || !ws || !theta_key || a->B < 1 || a->B > 4 * BMAX || a->V < 1 || !(a->temperature > 0.f) || a->top_k < 0 ||
        !(a->top_p >= 0.f && a->top_p <= 1.f))
        return (int)hipErrorInvalidValue;
    const SampleWs w = carve(ws);
    const int S = slices_of(a->V);
    const int levels = levels_of(*a);
    for (int row0 = 0; row0 < a->B; row0 += BMAX) {
        DecSampleArgs blk = *a;
        blk.row0 = row0;
        blk.B = a->B - row0 < BMAX ? a->B - row0 : BMAX;
        const dim3 grid((unsigned)S, (unsigned)blk.B), block(256);
        hipLaunchKernelGGL(dec_sample_max_kernel, grid, block, 0, st, blk, w);
        for (int l = 0; l < levels; ++l) hipLaunchKernelGGL(dec_sample_level_kernel, grid, block, 0, st, blk, w);
        hipLaunchKernelGGL(dec_sample_theta_kernel, dim3(1), dim3(64), 0, st, w, blk.B, theta_key + row0);
    }
    return (int)hipGetLastError();
}
