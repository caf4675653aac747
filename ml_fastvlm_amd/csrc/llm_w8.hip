// 8-bit weights for the Qwen2 decode (include/fvhd.h "LLM 8-bit weights"): the packed matrices as OCP e4m3 codes (gfx950's e4m3fn) with
// one fp32 scale per output row, row n standing for code * scale[n].
//   quantize_e4m3_kernel   bf16 [N][K] -> codes + scales: scale = 2^ceil(log2(amax_row / 448)) (an all-zero row: 1), codes = w / scale
//                          rounded to nearest even by v_cvt_pk_fp8_f32; nothing saturates (amax / scale <= 448)
//   dec_gemm_w8_kernel     dec_gemm_kernel / dec_gemm_wide_kernel (llm_decode.hip) on such a matrix.  What the decode GEMMs share - row
//                          statistics, weight-row mapping, split-K slabs, epilogues - is dec_gemm_parts.h; this kernel's own is its main
//                          loop: the weight fragment is loaded as bytes, converted e4m3 -> fp32 -> bf16 (exact) in registers and
//                          multiplies the same activation fragments on the same 16 x 16 x 32 bf16 MFMA; the row scale multiplies the
//                          finished accumulator (after the split-K sum, before the epilogue; q|k|v: fused with the bias add).  A kernel
//                          of its own, not an instantiation of the bf16 kernels: kernels and loops stay separate.
//   w8_unpack_kernel       codes -> bf16 [N][K] (code * scale, exact for power-of-two scales): the prefill's GEMMs stay bf16 and read
//                          each matrix from a scratch it is dequantised into right before; also the plain-order read-back / repack
//   dec_embed_w8_kernel    dec_embed_kernel on the lm_head codes of a tied model
//
// K order of a packed row: inside every 128-deep chunk the 8 codes of MFMA step j (0..3) and lane group g (0..3) - k = 32 j + 8 g .. + 7
// - sit at byte 64 (j / 2) + 16 g + 8 (j % 2), so that lane (lr, g) reads its operands of two MFMA steps with ONE 16-byte load and a
// wave's load covers 64 contiguous bytes of 16 rows - the access shape of the bf16 kernel at half the bytes.
#include "fvhd_common.h"
#include "launchers.h"      // (with llm_decode.h: the argument structs)
#include "dec_gemm_parts.h"  // better, the row statistics, the split-K meeting, the epilogues (with rope.h, split_handoff.h)
#include "w8_layout.h"  // w8_pos, e4m3x8_to_f32

namespace {

typedef unsigned char u8;

// 8 codes -> the bf16 MFMA fragment: every e4m3 value is a bf16 value (4 significant bits, a narrower exponent range)
FVHD_DEV bf16x8 e4m3x8_to_bf8(uint32_t lo, uint32_t hi) { return f32_to_bf8(e4m3x8_to_f32(lo, hi)); }

FVHD_DEV u32x4 ld_nt16(const u8* p) { return __builtin_nontemporal_load((const u32x4*)p); }

}  // namespace

// ---------------------------------------------------------------------------------------------------
// Workgroup = one row.  amax over the bf16 bit patterns (exact), the scale's exponent from amax's own exponent and mantissa:
// amax = m 2^e with m in [1, 2) -> ceil(log2(amax / 448)) = e - 8 + (m > 1.75), kept >= -126 so that the scale is a normal fp32.
// codes: [rows] rows of `pitch` bytes (PACKED: the K order above, else k order), scales: one every `sstride` floats.
template <bool PACKED>
__global__ __launch_bounds__(256) void quantize_e4m3_kernel(const bf16* __restrict__ w, int K, u8* __restrict__ codes, long pitch, float* __restrict__ scale,
                                                            int sstride)
{
    __shared__ unsigned sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bf16* wr = w + (size_t)blockIdx.x * K;
    unsigned am = 0;
    for (int k0 = tid * 8; k0 < K; k0 += 2048) {
        const u32x4 v = *(const u32x4*)(wr + k0);
#pragma unroll
        for (int i = 0; i < 4; ++i) am = max(am, max(v[i] & 0x7fffu, (v[i] >> 16) & 0x7fffu));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = max(am, (unsigned)__shfl_xor((int)am, o, 64));
    if (lane == 0) sh[wave] = am;
    __syncthreads();
    am = max(max(sh[0], sh[1]), max(sh[2], sh[3])) << 16;       // amax as fp32 bits
    int se = 0;
    if (am) se = max((int)(am >> 23) - 127 - 8 + ((am & 0x7fffffu) > 0x600000u ? 1 : 0), -126);
    const float inv = __builtin_bit_cast(float, (unsigned)(127 - se) << 23);
    if (tid == 0) scale[(size_t)blockIdx.x * sstride] = __builtin_bit_cast(float, (unsigned)(127 + se) << 23);
    u8* cr = codes + (size_t)blockIdx.x * pitch;
    for (int k0 = tid * 8; k0 < K; k0 += 2048) {
        const f32x8 v = bf8_to_f32(*(const bf16x8*)(wr + k0));
        int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, 0, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, lo, true);
        int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, 0, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, hi, true);
        *(u32x2*)(cr + (PACKED ? w8_pos(k0) : k0)) = u32x2{(uint32_t)lo, (uint32_t)hi};
    }
}

// One thread = 8 codes of a [N][K] matrix.  MODE 0: packed codes -> bf16 code * scale[row] in k order; 1: packed -> plain codes;
// 2: plain -> packed codes.
template <int MODE>
__global__ __launch_bounds__(256) void w8_unpack_kernel(const u8* __restrict__ src, const float* __restrict__ scale, void* __restrict__ dst, long groups, int K)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= groups) return;
    const int gpr = K / 8;
    const long row = idx / gpr;
    const int k0 = (int)(idx % gpr) * 8;
    const u32x2 q = *(const u32x2*)(src + row * K + (MODE == 2 ? k0 : w8_pos(k0)));
    if constexpr (MODE == 0) {
        const float s = scale[row];
        f32x8 v = e4m3x8_to_f32(q[0], q[1]);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] *= s;
        *(bf16x8*)((bf16*)dst + row * K + k0) = f32_to_bf8(v);
    } else {
        *(u32x2*)((u8*)dst + row * K + (MODE == 2 ? w8_pos(k0) : k0)) = q;
    }
}

// dec_embed_kernel (llm_decode.hip) on the lm_head codes of a tied model: h[b] = bf16(code * scale) of row id_b
__global__ __launch_bounds__(256) void dec_embed_w8_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ last, const u8* __restrict__ table,
                                                           const float* __restrict__ scale, int V, int H, bf16* __restrict__ h,
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
    const u8* src = table + (size_t)id * H;
    const float s = scale[id];
    for (int c = threadIdx.x * 8; c < H; c += 256 * 8) {
        const u32x2 q = *(const u32x2*)(src + w8_pos(c));
        f32x8 v = e4m3x8_to_f32(q[0], q[1]);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] *= s;
        *(bf16x8*)(h + (size_t)b * H + c) = f32_to_bf8(v);
    }
    if (threadIdx.x == 0) key_valid[(size_t)b * cap + L] = 1;
}

// ---------------------------------------------------------------------------------------------------
// The decode GEMM on e4m3 weights, NB = ceil(B / 16) batch tiles in 1 .. 4.  Lane (lr, g) of a wave owns weight row lr of its tile and
// loads, per 128-deep chunk, the 16 bytes at 16 g of both 64-byte halves: MFMA steps (0, 1) and (2, 3).  Everything else - the activation
// fragments, the folded RMSNorm, the order of the MFMAs, the slabs [S][N / 16][NB][64][4] and their sum in slice order, the epilogues - is
// dec_gemm_kernel's (NB = 1) / dec_gemm_wide_kernel's (the loop by its text, the rest by dec_gemm_parts.h), so that with every scale = 1 the output has the bits of the bf16 kernel on
// bf16(codes).  The scales of a lane's four output rows multiply its accumulator once, after the split-K sum.
template <int EPI, int NB>
__global__ __launch_bounds__(256) void dec_gemm_w8_kernel(const DecGemmArgs a)
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
        const u8* wr = (const u8*)a.W + (size_t)min(wrow, a.N - 1) * K + g * 16;
        const bf16* xr[NB];
        float rs[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            xr[t] = x + (size_t)xb[t] * a.ldx + g * 8;
            rs[t] = a.norm_w ? rstd[xb[t]] : 1.f;
        }
        const int KC = K / 128, c0 = s * a.cpw, c1 = min(c0 + a.cpw, KC);
        for (int c = c0; c < c1; ++c) {
            u32x4 wq[2];
            bf16x8 xf[NB][4];
#pragma unroll
            for (int h = 0; h < 2; ++h) wq[h] = ld_nt16(wr + c * 128 + h * 64);
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) xf[t][j] = *(const bf16x8*)(xr[t] + c * 128 + j * 32);
            if (a.norm_w) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* w = a.norm_w + c * 128 + j * 32 + g * 8;
                    const f32x4 w0 = *(const f32x4*)w, w1 = *(const f32x4*)(w + 4);
#pragma unroll
                    for (int t = 0; t < NB; ++t) {
                        const f32x8 v = bf8_to_f32(xf[t][j]);
                        f32x8 o;
#pragma unroll
                        for (int k = 0; k < 4; ++k) { o[k] = v[k] * rs[t] * w0[k]; o[4 + k] = v[4 + k] * rs[t] * w1[k]; }
                        xf[t][j] = f32_to_bf8(o);
                    }
                }
            }
            bf16x8 wf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = e4m3x8_to_bf8(wq[j >> 1][(j & 1) * 2], wq[j >> 1][(j & 1) * 2 + 1]);
#pragma unroll
            for (int t = 0; t < NB; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[t][j], acc[t], 0, 0, 0);
        }
    }
    if (S > 1) {
        dec_slab_store<NB>(a.part, acc, s, ntiles, tile, active, lane);
        if (!arrive_last(a.cnt + column, S, flag)) return;
        dec_slab_sum<NB>(a.part, acc, S, ntiles, tile, active, lane);
    }
    const int n0 = tile * 16 + g * 4;                            // this lane's 4 outputs of batch tile t: rows n0 .. n0 + 3 of batch row t * 16 + lr
    f32x4 sc = {1.f, 1.f, 1.f, 1.f};
    if (active) {                                                // their scales: the weight rows the lane's accumulator rows came from
        int srow = n0;
        if constexpr (EPI == DEC_EPI_QKV) {
            const int hd = a.hd, tph = hd / 16, head = tile / tph, pb = tile % tph;
            srow = head * hd + (g < 2 ? 0 : hd / 2) + pb * 8 + (g & 1) * 4;
        }
        sc = *(const f32x4*)(a.wscale + srow);
        if constexpr (EPI != DEC_EPI_QKV) {
#pragma unroll
            for (int t = 0; t < NB; ++t) acc[t] *= sc;
        }
    }
    // q|k|v: the scale is left to the epilogue, which rounds acc * scale + bias once (a fused multiply-add)
    dec_gemm_epilogue<EPI, NB>(a, acc, sh, tid, lane, wave, lr, g, B, tile, active, n0, EPI == DEC_EPI_QKV ? &sc : nullptr);
}

// ---------------------------------------------------------------------------------------------------
template <int EPI>
static void launch_dec_gemm_w8(hipStream_t st, const dim3 grid, const DecGemmArgs& a)
{
    const dim3 block(256);
    switch ((a.B + 15) / 16) {
    case 1: hipLaunchKernelGGL((dec_gemm_w8_kernel<EPI, 1>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((dec_gemm_w8_kernel<EPI, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((dec_gemm_w8_kernel<EPI, 3>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((dec_gemm_w8_kernel<EPI, 4>), grid, block, 0, st, a); break;
    }
}

// called by fvhd_launch_dec_gemm (llm_decode.hip) for arguments with a scale vector: it has checked them and launched dec_rstd_kernel
extern "C" int fvhd_launch_dec_gemm_w8(hipStream_t st, const DecGemmArgs* a)
{
    if (!a->wscale || a->B < 1 || a->B > 64 || a->N % 16 || a->K % 128) return (int)hipErrorInvalidValue;
    const int ncol = (a->N / 16 + 3) / 4;
    const dim3 grid((unsigned)((long)ncol * a->S));
    switch (a->epi) {
    case DEC_EPI_RESID: launch_dec_gemm_w8<DEC_EPI_RESID>(st, grid, *a); break;
    case DEC_EPI_SWIGLU: launch_dec_gemm_w8<DEC_EPI_SWIGLU>(st, grid, *a); break;
    case DEC_EPI_QKV: launch_dec_gemm_w8<DEC_EPI_QKV>(st, grid, *a); break;
    case DEC_EPI_ARGMAX: launch_dec_gemm_w8<DEC_EPI_ARGMAX>(st, grid, *a); break;
    default: return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

// bf16 rows [rows][K] (contiguous) -> codes rows of `pitch` bytes (packed != 0: the K order of the decode GEMM, needs K % 128 == 0) and
// one scale every `sstride` floats
extern "C" int fvhd_launch_quantize_e4m3(hipStream_t st, const void* w, int rows, int K, void* codes, long pitch, float* scale, int sstride, int packed)
{
    if (rows < 1 || K < 8 || K % 8 || (packed && K % 128) || pitch < K || pitch % 8 || sstride < 1) return (int)hipErrorInvalidValue;
    if (packed) hipLaunchKernelGGL(quantize_e4m3_kernel<true>, dim3(rows), dim3(256), 0, st, (const bf16*)w, K, (u8*)codes, pitch, scale, sstride);
    else hipLaunchKernelGGL(quantize_e4m3_kernel<false>, dim3(rows), dim3(256), 0, st, (const bf16*)w, K, (u8*)codes, pitch, scale, sstride);
    return (int)hipGetLastError();
}

// mode 0: packed codes [N][K] -> bf16 code * scale; 1: packed -> plain codes; 2: plain -> packed codes.  K % 128 == 0.
extern "C" int fvhd_launch_w8_unpack(hipStream_t st, const void* src, const float* scale, void* dst, long N, int K, int mode)
{
    if (N < 1 || K < 128 || K % 128 || mode < 0 || mode > 2 || (mode == 0 && !scale)) return (int)hipErrorInvalidValue;
    const long groups = N * (K / 8);
    const dim3 grid((unsigned)((groups + 255) / 256)), block(256);
    if (mode == 0) hipLaunchKernelGGL(w8_unpack_kernel<0>, grid, block, 0, st, (const u8*)src, scale, dst, groups, K);
    else if (mode == 1) hipLaunchKernelGGL(w8_unpack_kernel<1>, grid, block, 0, st, (const u8*)src, scale, dst, groups, K);
    else hipLaunchKernelGGL(w8_unpack_kernel<2>, grid, block, 0, st, (const u8*)src, scale, dst, groups, K);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_embed_w8(hipStream_t st, const int64_t* tok, const int64_t* last, const void* table, const float* scale, int V, int H, void* h,
                                        unsigned char* key_valid, int B, int cap, const int* len, int* status, int* status_host)
{
    if (B < 1 || H % 128) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_embed_w8_kernel, dim3(B), dim3(256), 0, st, tok, last, (const u8*)table, scale, V, H, (bf16*)h, key_valid, cap, len, status, status_host);
    return (int)hipGetLastError();
}
