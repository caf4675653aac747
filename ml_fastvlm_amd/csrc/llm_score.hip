// Scoring given tokens (include/fvhd.h "LLM scoring"): lm_head on EVERY row with the log-softmax and the pick of the target fused in.
//     z = xn[M][K] . W[V][K]^T      lse[m] = log sum_v exp(z[m][v])      logprob[m] = z[m][target[m]] - lse[m]
// The [M, V] logits never exist: at the benchmark's prefill shape (8 x 317 rows, V = 151 936) they would be 1.5 GB of fp32, written and
// read back to keep one number per row.
//
// Launch 1 (lm_score_kernel): a 256-thread workgroup owns 128 rows and walks ONE SEGMENT of the vocabulary in tiles of 128 columns - the
// register-prefetch 16x16x32 bf16 MFMA loop of gemm.hip v1 (same LDS image and swizzle, same "swapped" issue D = Wfrag x Afrag^T), waves
// 2 (rows) x 2 (columns).  After a tile, lane (lr, g) of wave (wm, wn) holds for each of its 4 rows m = 64 wm + 16 i + lr the 16 logits of
// columns n0 + 64 wn + 16 j + 4 g + c: it folds them into ITS OWN running (max, sum of exp(z - max), target logit) of that row - an online
// softmax per lane over the lane's fixed subset of the columns, no cross-lane traffic inside the walk.  At the end of the segment the 8
// partial states of a row (4 lane groups g x 2 waves wn) are combined in a fixed tree and one 16-byte vector store per row writes
// (max, sum, target logit) of the segment to scratch[segment][row].
// Launch 2 (lm_score_finish_kernel): one thread per row combines the S segment states in segment order and writes lse and logprob.
//
// Why a second launch and not the last-arriving workgroup (llm_decode.hip does that for its split-K GEMMs): the finish reads 16 S bytes per
// row, a launch of microseconds behind a walk of milliseconds, and a counter would be state in the scratch that has to be zero before
// every launch - a caller's scratch (fvhd_op_lm_score) would need a memset, and an arrival counter a replayed graph shares with an eager
// call is one more thing to get wrong.  The scratch here needs no initialisation: every word the finish reads was written by launch 1 of
// the same call.  Nothing is combined through atomics; all stores are ordinary vector stores ordered by the kernel boundary.
//
// Stable bits: which columns a lane sums, in which order, and the combine tree depend on (M, V, K) through the plan (S) only - not on the
// row's index inside its block, not on the other rows, not on any target (the target only selects which logit is copied out).
#include <math.h>

#include "fvhd_common.h"
#include "launchers.h"

namespace {

constexpr int SC_BM = 128, SC_BN = 128, SC_MAX_SEG = 64;
constexpr float kLog2e = 1.4426950408889634f;

template <int BK> FVHD_DEV int sc_lds_off(int row, int ks)      // gemm.hip lds_off: XOR swizzle of the 16-B slot, conflict-free fragment reads
{
    if constexpr (BK == 64) return row * 128 + ((ks ^ ((row >> 1) & 7)) << 4);
    else return row * 64 + ((ks ^ ((0 - (row >> 2)) & 3)) << 4);
}

// (m, s) <- (m, s) (+) (m2, s2): the sum of exp(z - max) of the union; an empty state is (-inf, 0)
FVHD_DEV void sc_combine(float& m, float& s, float m2, float s2)
{
    const float mx = fmaxf(m, m2);
    const float ms = mx == -INFINITY ? 0.f : mx;              // both empty: exp2(-inf) = 0 twice, never inf - inf
    s = s * __builtin_amdgcn_exp2f((m - ms) * kLog2e) + s2 * __builtin_amdgcn_exp2f((m2 - ms) * kLog2e);
    m = mx;
}

template <int BK>
__global__ __launch_bounds__(256, 2) void lm_score_kernel(const bf16* __restrict__ A, const bf16* __restrict__ Wt, const int64_t* __restrict__ target,
                                                          f32x4* __restrict__ scratch, int M, int V, int K, int S, int nrb, int ntile)
{
    constexpr int BM = SC_BM, BN = SC_BN, MF = 4, NF = 4;
    constexpr int ROWB = BK * 2, CPR = BK / 8, A_CH = BM * CPR / 256, W_CH = BN * CPR / 256;
    __shared__ __attribute__((aligned(16))) char lds[(BM + BN) * ROWB];
    __shared__ float comb[BM][3];
    char* ldsA = lds;
    char* ldsW = lds + BM * ROWB;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 15, g = lane >> 4;
    // the row blocks of one segment are neighbours in the logical order, and xcd_remap gives every XCD a contiguous run of it: the
    // workgroups that walk the same W tiles at the same time share one private L2
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int seg = L / nrb, rb = L - seg * nrb;
    const int m0 = rb * BM;
    const int t0 = (int)((long)seg * ntile / S), t1 = (int)((long)(seg + 1) * ntile / S);      // S <= ntile: never empty

    u32x4 ra[A_CH], rw[W_CH];
    const bf16* a_src[A_CH];
    const bf16* w_src[W_CH];
    int a_dst[A_CH], w_dst[W_CH], w_row[W_CH], w_ks[W_CH];
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
        const int idx = i * 256 + tid, row = idx / CPR, ks = idx % CPR;
        a_src[i] = A + (size_t)min(m0 + row, M - 1) * K + ks * 8;          // rows past M: a valid row, never written out
        a_dst[i] = sc_lds_off<BK>(row, ks);
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
        const int idx = i * 256 + tid;
        w_row[i] = idx / CPR; w_ks[i] = idx % CPR;
        w_dst[i] = sc_lds_off<BK>(w_row[i], w_ks[i]);
    }
    auto point_w = [&](int t) {                                            // columns past V: a valid W row, masked below
#pragma unroll
        for (int i = 0; i < W_CH; ++i) w_src[i] = Wt + (size_t)min(t * BN + w_row[i], V - 1) * K + w_ks[i] * 8;
    };

    // the targets of the lane's 4 rows: -1 never matches (ignored, or a row past M), INT_MAX never matches (>= V: NaN in the finish)
    int tg[MF];
    float rm[MF], rs[MF], rz[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int m = m0 + wm * 64 + i * 16 + lr;
        const int64_t t = m < M ? target[m] : -1;
        tg[i] = t < 0 ? -1 : t >= V ? 0x7fffffff : (int)t;
        rm[i] = -INFINITY; rs[i] = 0.f; rz[i] = 0.f;
    }

    const int nk = K / BK;
    point_w(t0);
#pragma unroll
    for (int i = 0; i < A_CH; ++i) ra[i] = *(const u32x4*)(a_src[i]);
#pragma unroll
    for (int i = 0; i < W_CH; ++i) rw[i] = *(const u32x4*)(w_src[i]);

    for (int t = t0; t < t1; ++t) {
        f32x4 acc[MF][NF];
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kt = 0; kt < nk; ++kt) {
            if (t > t0 || kt > 0) __syncthreads();       // the previous K tile's fragment reads are done
#pragma unroll
            for (int i = 0; i < A_CH; ++i) *(u32x4*)(ldsA + a_dst[i]) = ra[i];
#pragma unroll
            for (int i = 0; i < W_CH; ++i) *(u32x4*)(ldsW + w_dst[i]) = rw[i];
            __syncthreads();
            // the next K tile - of this vocabulary tile, or the first of the next one (in flight under the softmax update below)
            int ko = (kt + 1) * BK;
            bool more = true;
            if (kt + 1 == nk) {
                ko = 0;
                more = t + 1 < t1;
                if (more) point_w(t + 1);
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < A_CH; ++i) ra[i] = *(const u32x4*)(a_src[i] + ko);
#pragma unroll
                for (int i = 0; i < W_CH; ++i) rw[i] = *(const u32x4*)(w_src[i] + ko);
            }
#pragma unroll
            for (int kk = 0; kk < BK / 32; ++kk) {
                bf16x8 af[MF], wf[NF];
                const int ks = kk * 4 + g;
#pragma unroll
                for (int i = 0; i < MF; ++i) af[i] = *(const bf16x8*)(ldsA + sc_lds_off<BK>(wm * 64 + i * 16 + lr, ks));
#pragma unroll
                for (int j = 0; j < NF; ++j) wf[j] = *(const bf16x8*)(ldsW + sc_lds_off<BK>(wn * 64 + j * 16 + lr, ks));
#pragma unroll
                for (int i = 0; i < MF; ++i)
#pragma unroll
                    for (int j = 0; j < NF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
            }
        }
        // acc[i][j][c] = z[m0 + 64 wm + 16 i + lr][c0 + 16 j + c], c0 = the lane's first column of this tile
        const int c0 = t * BN + wn * 64 + g * 4;
        if (t * BN + BN > V) {                           // the ragged last tile: columns >= V enter neither the max nor the sum
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c0 + 16 * j + c >= V) {
#pragma unroll
                        for (int i = 0; i < MF; ++i) acc[i][j][c] = -INFINITY;
                    }
        }
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            float zmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float z = acc[i][j][c];
                    zmax = fmaxf(zmax, z);
                    if (c0 + 16 * j + c == tg[i]) rz[i] = z;             // the very value that enters the sum
                }
            const float mx = fmaxf(rm[i], zmax);
            const float ms = mx == -INFINITY ? 0.f : mx;                  // a lane with no valid column yet stays (-inf, 0)
            float add = 0.f;
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) add += __builtin_amdgcn_exp2f((acc[i][j][c] - ms) * kLog2e);
            rs[i] = rs[i] * __builtin_amdgcn_exp2f((rm[i] - ms) * kLog2e) + add;
            rm[i] = mx;
        }
    }

    // the 8 states of a row -> one: lane groups g (xor 16, then xor 32: both partners compute the same commutative combine), then the
    // column wave wn = 1 hands its result to wn = 0 through LDS
#pragma unroll
    for (int i = 0; i < MF; ++i) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float m2 = __shfl_xor(rm[i], o, 64), s2 = __shfl_xor(rs[i], o, 64), z2 = __shfl_xor(rz[i], o, 64);
            sc_combine(rm[i], rs[i], m2, s2);
            rz[i] += z2;                                 // at most one lane of a row holds a non-zero target logit
        }
    }
    if (wn == 1 && g == 0) {
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int r = wm * 64 + i * 16 + lr;
            comb[r][0] = rm[i]; comb[r][1] = rs[i]; comb[r][2] = rz[i];
        }
    }
    __syncthreads();
    if (wn == 0 && g == 0) {
#pragma unroll
        for (int i = 0; i < MF; ++i) {
            const int r = wm * 64 + i * 16 + lr, m = m0 + r;
            if (m >= M) continue;                        // rows past M are not written
            sc_combine(rm[i], rs[i], comb[r][0], comb[r][1]);
            scratch[(size_t)seg * M + m] = f32x4{rm[i], rs[i], rz[i] + comb[r][2], 0.f};
        }
    }
}

__global__ __launch_bounds__(256) void lm_score_finish_kernel(const f32x4* __restrict__ scratch, const int64_t* __restrict__ target, float* __restrict__ logprob,
                                                              float* __restrict__ lse_out, int M, int V, int S)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float rm = -INFINITY, rs = 0.f, rz = 0.f;
    for (int s = 0; s < S; ++s) {                        // segment order: fixed
        const f32x4 p = scratch[(size_t)s * M + m];
        sc_combine(rm, rs, p[0], p[1]);
        rz += p[2];
    }
    const float lse = rm + logf(rs);
    if (lse_out) lse_out[m] = lse;
    const int64_t t = target[m];
    logprob[m] = t < 0 ? 0.f : t >= V ? __builtin_nanf("") : rz - lse;
}

}  // namespace

extern "C" {

// segments S of the vocabulary walk.  512 = 256 compute units (MI355X) x the 2 workgroups of this kernel a CU holds (__launch_bounds__(256, 2),
// 34 KB of LDS): the grid (row blocks x S) is the largest that is resident AT ONCE - a workgroup beyond it would run alone in a second
// round behind the others.  A constant and not the device's CU count: the plan must be a pure function of (M, V, K), since a row's bits
// depend on it.  S <= 64 and <= tiles.
int fvhd_lm_score_plan(int M, int V, int K)
{
    if (M < 1 || V < 8 || V % 8 || K < 32 || K % 32) return 0;
    const long nrb = ((long)M + SC_BM - 1) / SC_BM, ntile = ((long)V + SC_BN - 1) / SC_BN;
    long S = 512 / nrb;
    if (S > SC_MAX_SEG) S = SC_MAX_SEG;
    if (S > ntile) S = ntile;
    return (int)(S < 1 ? 1 : S);
}

size_t fvhd_lm_score_scratch_bytes(int M, int V, int K)
{
    const int S = fvhd_lm_score_plan(M, V, K);
    return S ? (size_t)S * (size_t)M * sizeof(f32x4) : 0;
}

// the caller has checked the shape (fvhd_lm_score_plan(M, V, K) != 0) and the scratch size; scratch aligned to 16 bytes
int fvhd_launch_lm_score(hipStream_t st, const void* xn, const void* Wt, const int64_t* target, int M, int V, int K, float* logprob, float* lse, void* scratch)
{
    const int S = fvhd_lm_score_plan(M, V, K);
    if (!S) return (int)hipErrorInvalidValue;
    const int nrb = (M + SC_BM - 1) / SC_BM, ntile = (V + SC_BN - 1) / SC_BN;
    const dim3 grid((unsigned)(nrb * S));
    if (K % 64 == 0)
        hipLaunchKernelGGL(lm_score_kernel<64>, grid, dim3(256), 0, st, (const bf16*)xn, (const bf16*)Wt, target, (f32x4*)scratch, M, V, K, S, nrb, ntile);
    else
        hipLaunchKernelGGL(lm_score_kernel<32>, grid, dim3(256), 0, st, (const bf16*)xn, (const bf16*)Wt, target, (f32x4*)scratch, M, V, K, S, nrb, ntile);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lm_score_finish_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, (const f32x4*)scratch, target, logprob, lse, M, V, S);
    return (int)hipGetLastError();
}

}  // extern "C"
