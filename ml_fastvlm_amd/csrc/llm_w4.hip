// 4-bit weights for the Qwen2 decode (include/fvhd.h "LLM 4-bit weights"): the packed matrices as OCP MXFP4 - e2m1 codes, two per byte,
// with one e8m0 power-of-two scale per 32 consecutive k of a row (4.25 bits per weight).
//   quantize_mxfp4_kernel  bf16 [N][K] -> codes + block scales: per block se = ceil(log2(amax / 6)) from amax's own exponent and mantissa,
//                          kept in [-125, 125] (an all-zero block: 0), codes = w / 2^se rounded to the nearest grid value, ties to the
//                          even index, the sign bit of w kept; integer / float C++, no conversion instruction (its ties are not the recipe's
//                          to rely on)
//   dec_gemm_w4_kernel     dec_gemm_kernel / dec_gemm_wide_kernel (llm_decode.hip) on such a matrix.  What the decode GEMMs share - row
//                          statistics, weight-row mapping, split-K slabs, epilogues - is dec_gemm_parts.h; this kernel's own is its main
//                          loop (`trip`): the weight fragment of an MFMA step is four
//                          v_cvt_scalef32_pk_bf16_fp4 of one dword with the step's block scale, which is exactly bf16(code * scale) - the
//                          operand the bf16 kernel reads from the dequantised matrix - so the output has the bf16 kernel's bits.  Nothing
//                          scales the accumulator.
//   w4_unpack_kernel       packed -> bf16 [N][K] (the prefill's GEMMs stay bf16 and read each matrix from a scratch it is dequantised
//                          into right before); also the plain-order read-back / repack of the codes
//   dec_embed_w4_kernel    dec_embed_kernel on the lm_head codes of a tied model
// The K order of a packed row: w4_layout.h.
#include "fvhd_common.h"
#include "launchers.h"      // (with llm_decode.h: the argument structs)
#include "dec_gemm_parts.h"  // better, the row statistics, the split-K meeting, the epilogues (with rope.h, split_handoff.h)
#include "w4_layout.h"  // w4_pos, w4_scale, fp4x8_to_bf8

#include <type_traits>

// 128-deep chunks per loop trip of dec_gemm_w4_kernel at NB <= 2 (1 or 2; identical bits): the step is latency-bound, so what counts is
// the bytes a wave has in flight, and a chunk is only 16 bytes of codes per lane (DESIGN 4.3 "4-bit weights" has the A/B)
#ifndef FVHD_W4_CHUNKS
#define FVHD_W4_CHUNKS 1
#endif

namespace {

typedef unsigned char u8;

FVHD_DEV u32x4 ld_nt16(const u8* p) { return __builtin_nontemporal_load((const u32x4*)p); }

// |v| on the e2m1 grid {0, 0.5, 1, 1.5, 2, 3, 4, 6} -> its index: nearest, a tie (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5) to the even index,
// above 6 saturates
FVHD_DEV unsigned e2m1_index(float a)
{
    return (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.f);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// Workgroup = one row, thread = 8 consecutive k, four adjacent lanes = one block of 32.  Block amax over the bf16 bit patterns (exact);
// amax = m 2^e with m in [1, 2) -> ceil(log2(amax / 6)) = e - 2 + (m > 1.5), clamped to [-125, 125].
// codes: rows of `pitch` bytes (PACKED: the K order of w4_layout.h, else k order), scales: rows of `spitch` bytes.  K % 32 == 0.
template <bool PACKED>
__global__ __launch_bounds__(256) void quantize_mxfp4_kernel(const bf16* __restrict__ w, int K, u8* __restrict__ codes, long pitch, u8* __restrict__ scales,
                                                             long spitch)
{
    const int tid = threadIdx.x;
    const bf16* wr = w + (size_t)blockIdx.x * K;
    u8* cr = codes + (size_t)blockIdx.x * pitch;
    u8* sr = scales + (size_t)blockIdx.x * spitch;
    for (int base = 0; base < K; base += 2048) {                 // (uniform trip count: the shuffles below run with every lane present)
        const int k0 = base + tid * 8;
        const bool valid = k0 < K;                               // the same for the four lanes of a block
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (valid) v = *(const u32x4*)(wr + k0);
        unsigned am = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) am = max(am, max(v[i] & 0x7fffu, (v[i] >> 16) & 0x7fffu));
        am = max(am, (unsigned)__shfl_xor((int)am, 1, 64));
        am = max(am, (unsigned)__shfl_xor((int)am, 2, 64));
        int se = 0;
        if (am) se = min(max((int)(am >> 7) - 127 - 2 + ((am & 0x7fu) > 0x40u ? 1 : 0), -125), 125);
        const float inv = __builtin_bit_cast(float, (unsigned)(127 - se) << 23);
        unsigned q = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned bits = (i & 1) ? (v[i >> 1] >> 16) : (v[i >> 1] & 0xffffu);
            const float a = __builtin_bit_cast(float, (bits & 0x7fffu) << 16) * inv;
            q |= (((bits >> 15) << 3) | e2m1_index(a)) << (4 * i);
        }
        if (valid) {
            *(uint32_t*)(cr + (PACKED ? w4_pos(k0) : k0 / 2)) = q;
            if ((tid & 3) == 0) sr[k0 >> 5] = (u8)(127 + se);
        }
    }
}

// One thread = 8 codes (a dword) of a [N][K] matrix.  MODE 0: packed codes + block scales -> bf16 code * scale in k order; 1: packed ->
// plain codes; 2: plain -> packed codes.  (The scales are in k order either way.)
template <int MODE>
__global__ __launch_bounds__(256) void w4_unpack_kernel(const u8* __restrict__ src, const u8* __restrict__ scales, void* __restrict__ dst, long groups, int K)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= groups) return;
    const int gpr = K / 8;
    const long row = idx / gpr;
    const int k0 = (int)(idx % gpr) * 8;
    const uint32_t q = *(const uint32_t*)(src + row * (K / 2) + (MODE == 2 ? k0 / 2 : w4_pos(k0)));
    if constexpr (MODE == 0) {
        *(bf16x8*)((bf16*)dst + row * K + k0) = fp4x8_to_bf8(q, w4_scale(scales[row * (K / 32) + (k0 >> 5)]));
    } else {
        *(uint32_t*)((u8*)dst + row * (K / 2) + (MODE == 2 ? w4_pos(k0) : k0 / 2)) = q;
    }
}

// dec_embed_kernel (llm_decode.hip) on the lm_head codes of a tied model: h[b] = bf16(code * scale) of row id_b
__global__ __launch_bounds__(256) void dec_embed_w4_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ last, const u8* __restrict__ table,
                                                           const u8* __restrict__ scales, int V, int H, bf16* __restrict__ h,
                                                           unsigned char* __restrict__ key_valid, int cap, const int* len, int* status, int* status_host)
{
    if (*status) return;
    const int b = blockIdx.x;
    const int L = *len;
    if (L >= cap) {
        if (b == 0 && threadIdx.x == 0) { *status = 1; *status_host = 1; }
        return;
    }
    const int64_t id = tok ? tok[b] : last[b];
    if (id < 0 || id >= V) {
        if (threadIdx.x == 0) { *status = 2; *status_host = 2; }
        return;
    }
    const u8* src = table + (size_t)id * (H / 2);
    const u8* sr = scales + (size_t)id * (H / 32);
    for (int c = threadIdx.x * 8; c < H; c += 256 * 8)
        *(bf16x8*)(h + (size_t)b * H + c) = fp4x8_to_bf8(*(const uint32_t*)(src + w4_pos(c)), w4_scale(sr[c >> 5]));
    if (threadIdx.x == 0) key_valid[(size_t)b * cap + L] = 1;
}

// ---------------------------------------------------------------------------------------------------
// The decode GEMM on MXFP4 weights, NB = ceil(B / 16) batch tiles in 1 .. 4.  Lane (lr, g) of a wave owns weight row lr of its tile and
// loads, per 128-deep chunk, the 16 bytes at 16 g of the chunk's 64 (its dwords of MFMA steps 0 .. 3) and the chunk's four scale bytes
// (one dword, the same address for the four lane groups of a row).  Everything else - the activation fragments, the folded RMSNorm, the
// order of the MFMAs, the slabs [S][N / 16][NB][64][4] and their sum in slice order, the epilogues - is dec_gemm_kernel's (NB = 1) /
// dec_gemm_wide_kernel's (the loop by its text, the rest by dec_gemm_parts.h), and the weight fragment is exactly the one those kernels load from bf16(code * scale): identical bits.
template <int EPI, int NB>
__global__ __launch_bounds__(256) void dec_gemm_w4_kernel(const DecGemmArgs a)
{
    static_assert(NB >= 1 && NB <= 4, "batch tiles of the decode GEMM");
    if (a.status && *a.status) return;
    __shared__ float sh[16 * NB + 4 + 4 * 16 * NB * 2];
    float* rstd = sh;
    int* flag = (int*)(sh + 16 * NB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
    const int ntiles = a.N / 16, S = a.S;
    const int column = blockIdx.x / S, s = blockIdx.x % S;
    const int tile = column * 4 + wave;
    const bool active = tile < ntiles;                           // wave-uniform
    const int B = a.B, K = a.K;
    const bf16* x = (const bf16*)a.x;
    dec_row_stats<(NB > 1)>(a, rstd, tid, lane, wave, B, K, x);
    const int wrow = dec_weight_row<EPI>(a, tile, lr);
    int xb[NB];
    f32x4 acc[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) { xb[t] = min(t * 16 + lr, B - 1); acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (active) {
        const u8* wr = (const u8*)a.W + (size_t)min(wrow, a.N - 1) * (K / 2) + g * 16;
        const u8* sr = a.wblk + (size_t)min(wrow, a.N - 1) * (K / 32);
        const bf16* xr[NB];
        float rs[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            xr[t] = x + (size_t)xb[t] * a.ldx + g * 8;
            rs[t] = a.norm_w ? rstd[xb[t]] : 1.f;
        }
        const int KC = K / 128, c0 = s * a.cpw, c1 = min(c0 + a.cpw, KC);
        // UC consecutive chunks of one loop trip: every load of the trip is issued before the first conversion, then the chunks' MFMAs in
        // chunk order - per accumulator the order of the one-chunk loop, so the bits do not depend on UC
        auto trip = [&](int c, auto uc) {
            constexpr int UC = decltype(uc)::value;
            u32x4 wq[UC];
            uint32_t se[UC];
            bf16x8 xf[UC][NB][4];
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                wq[u] = ld_nt16(wr + (c + u) * 64);
                se[u] = *(const uint32_t*)(sr + (c + u) * 4);
            }
#pragma unroll
            for (int u = 0; u < UC; ++u)
#pragma unroll
                for (int t = 0; t < NB; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) xf[u][t][j] = *(const bf16x8*)(xr[t] + (c + u) * 128 + j * 32);
            if (a.norm_w) {
#pragma unroll
                for (int u = 0; u < UC; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float* w = a.norm_w + (c + u) * 128 + j * 32 + g * 8;
                        const f32x4 w0 = *(const f32x4*)w, w1 = *(const f32x4*)(w + 4);
#pragma unroll
                        for (int t = 0; t < NB; ++t) {
                            const f32x8 v = bf8_to_f32(xf[u][t][j]);
                            f32x8 o;
#pragma unroll
                            for (int k = 0; k < 4; ++k) { o[k] = v[k] * rs[t] * w0[k]; o[4 + k] = v[4 + k] * rs[t] * w1[k]; }
                            xf[u][t][j] = f32_to_bf8(o);
                        }
                    }
            }
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                bf16x8 wf[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) wf[j] = fp4x8_to_bf8(wq[u][j], w4_scale(se[u] >> (8 * j)));
#pragma unroll
                for (int t = 0; t < NB; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[u][t][j], acc[t], 0, 0, 0);
            }
        };
        constexpr int U = NB <= 2 ? FVHD_W4_CHUNKS : 1;           // (NB = 3, 4: the activation fragments of two chunks do not fit the register budget)
        int c = c0;
        if constexpr (U > 1)
            for (; c + U <= c1; c += U) trip(c, std::integral_constant<int, U>{});
        for (; c < c1; ++c) trip(c, std::integral_constant<int, 1>{});
    }
    if (S > 1) {
        dec_slab_store<NB>(a.part, acc, s, ntiles, tile, active, lane);
        if (!arrive_last(a.cnt + column, S, flag)) return;
        dec_slab_sum<NB>(a.part, acc, S, ntiles, tile, active, lane);
    }
    const int n0 = tile * 16 + g * 4;                            // this lane's 4 outputs of batch tile t: rows n0 .. n0 + 3 of batch row t * 16 + lr
    dec_gemm_epilogue<EPI, NB>(a, acc, sh, tid, lane, wave, lr, g, B, tile, active, n0);
}

// ---------------------------------------------------------------------------------------------------
template <int EPI>
static void launch_dec_gemm_w4(hipStream_t st, const dim3 grid, const DecGemmArgs& a)
{
    const dim3 block(256);
    switch ((a.B + 15) / 16) {
    case 1: hipLaunchKernelGGL((dec_gemm_w4_kernel<EPI, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((dec_gemm_w4_kernel<EPI, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((dec_gemm_w4_kernel<EPI, 3>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((dec_gemm_w4_kernel<EPI, 4>), grid, block, 0, st, a); break;
    }
}

// called by fvhd_launch_dec_gemm (llm_decode.hip) for arguments with block scales: it has checked them and launched dec_rstd_kernel
extern "C" int fvhd_launch_dec_gemm_w4(hipStream_t st, const DecGemmArgs* a)
{
    if (!a->wblk || a->wscale || a->B < 1 || a->B > 64 || a->N % 16 || a->K % 128 || ((uintptr_t)a->W & 15) || ((uintptr_t)a->wblk & 3))
        return (int)hipErrorInvalidValue;
    const int ncol = (a->N / 16 + 3) / 4;
    const dim3 grid((unsigned)((long)ncol * a->S));
    switch (a->epi) {
    case DEC_EPI_RESID: launch_dec_gemm_w4<DEC_EPI_RESID>(st, grid, *a); break;
    case DEC_EPI_SWIGLU: launch_dec_gemm_w4<DEC_EPI_SWIGLU>(st, grid, *a); break;
    case DEC_EPI_QKV: launch_dec_gemm_w4<DEC_EPI_QKV>(st, grid, *a); break;
    case DEC_EPI_ARGMAX: launch_dec_gemm_w4<DEC_EPI_ARGMAX>(st, grid, *a); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

// bf16 rows [rows][K] (contiguous, K % 32 == 0) -> codes rows of `pitch` bytes (packed != 0: the K order of the decode GEMM, needs
// K % 128 == 0) and scale rows of `spitch` bytes
extern "C" int fvhd_launch_quantize_mxfp4(hipStream_t st, const void* w, int rows, int K, void* codes, long pitch, void* scales, long spitch, int packed)
{
    if (rows < 1 || K < 32 || K % 32 || (packed && K % 128) || pitch < K / 2 || pitch % 4 || spitch < K / 32) return (int)hipErrorInvalidValue;
    if (packed) hipLaunchKernelGGL(quantize_mxfp4_kernel<true>, dim3(rows), dim3(256), 0, st, (const bf16*)w, K, (u8*)codes, pitch, (u8*)scales, spitch);
    else hipLaunchKernelGGL(quantize_mxfp4_kernel<false>, dim3(rows), dim3(256), 0, st, (const bf16*)w, K, (u8*)codes, pitch, (u8*)scales, spitch);
    return (int)hipGetLastError();
}

// mode 0: packed codes [N][K / 2] + scales [N][K / 32] -> bf16 code * scale; 1: packed -> plain codes; 2: plain -> packed codes.  K % 128 == 0.
extern "C" int fvhd_launch_w4_unpack(hipStream_t st, const void* src, const void* scales, void* dst, long N, int K, int mode)
{
    if (N < 1 || K < 128 || K % 128 || mode < 0 || mode > 2 || (mode == 0 && !scales)) return (int)hipErrorInvalidValue;
    const long groups = N * (K / 8);
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    if (mode == 0) hipLaunchKernelGGL(w4_unpack_kernel<0>, grid, block, 0, st, (const u8*)src, (const u8*)scales, dst, groups, K);
    else if (mode == 1) hipLaunchKernelGGL(w4_unpack_kernel<1>, grid, block, 0, st, (const u8*)src, (const u8*)scales, dst, groups, K);
    else hipLaunchKernelGGL(w4_unpack_kernel<2>, grid, block, 0, st, (const u8*)src, (const u8*)scales, dst, groups, K);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_embed_w4(hipStream_t st, const int64_t* tok, const int64_t* last, const void* table, const void* scales, int V, int H, void* h,
                                        unsigned char* key_valid, int B, int cap, const int* len, int* status, int* status_host)
{
    if (B < 1 || H % 128) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_embed_w4_kernel, dim3(B), dim3(256), 0, st, tok, last, (const u8*)table, (const u8*)scales, V, H, (bf16*)h, key_valid, cap, len, status,
                       status_host);
    return (int)hipGetLastError();
}
