// First and last ops of the FastViTHD tower.
//
//   stem[0]   MobileOneBlock dense 3x3 s2 p1, 3 -> 96, + bias, GELU          mci.py:563-574, 194-198
//             reads the caller's NCHW image (f32 / f16 / bf16) and writes NHWC bf16 - this is the only
//             layout change on the whole path; the tower's output [B, HW, 3072] *is* NHWC.
//   conv_exp  SEBlock (avg-pool -> 1x1 reduce -> ReLU -> 1x1 expand -> sigmoid -> scale) and the final
//             GELU, applied to y = dw3x3(x)+b computed by the generic depthwise kernel  mci.py:72-81, 198
//             written straight in the tower's output dtype/layout (feature_select is free:
//             mobileclip_encoder.py:60-68).
#include "fvhd_common.h"
#include "launchers.h"

template <typename T> FVHD_DEV float ld_as_f32(const T* p, size_t i);
template <> FVHD_DEV float ld_as_f32<float>(const float* p, size_t i) { return p[i]; }
template <> FVHD_DEV float ld_as_f32<_Float16>(const _Float16* p, size_t i) { return (float)p[i]; }
template <> FVHD_DEV float ld_as_f32<bf16>(const bf16* p, size_t i) { return (float)p[i]; }

typedef float f32x16 __attribute__((ext_vector_type(16)));

// stem[0] as an MFMA GEMM:  out[px][96] = gelu(W[96 x 27] . patch[27 x px] + b),  K padded to 32.
//   * a wave owns tiles of 32 consecutive output pixels of one output row; the im2col patch is the B operand of
//     v_mfma_f32_32x32x16_bf16 (lane = (pixel, k-half)), gathered straight from the caller's NCHW image (any of
//     f32 / f16 / bf16; rounded to bf16, the tower's compute dtype - mobileclip_encoder.py:85 casts images likewise);
//     the k axis is ordered so that a lane's 16 slots are whole (ci, ky) rows of 3 taps: half 0 = rows 0-4, half 1 = rows 5-8;
//   * the weights are the A operand (3 blocks of 32 output channels x 2 k-steps): each workgroup builds the bf16 fragment
//     image once in LDS from the fp32 [27][96] taps and every lane keeps its 6 fragments in registers;
//   * bias + exact-erf GELU in fp32 on the accumulators, then the [32 px][96 ch] bf16 tile goes through LDS so that the
//     NHWC store is 16 B per lane, fully coalesced (a tile is 6 KiB contiguous in HBM).
// (The VALU version of this kernel spent 648 FMA + 162 LDS weight reads per thread and ran at 1.1 TB/s.)
#define STEM_TPW 4      // tiles per wave
template <typename T>
__global__ __launch_bounds__(256) void stem_conv_kernel(const T* __restrict__ img, bf16* __restrict__ out,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        int B, int R, long ntiles)
{
    constexpr int CO = 96;
    __shared__ __attribute__((aligned(16))) char smem[6 * 64 * 16 + 4 * 32 * CO * 2];
    bf16x8* wimg = (bf16x8*)smem;                       // [cb][s][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int px = lane & 31, half = lane >> 5;
    // tap index of k-slot q (0..15) of k-half h: rows (ci*3+ky) 0-4 -> half 0, 5-8 -> half 1; -1 = zero padding
    auto tap_of = [](int h, int q) { const int row = (h ? 5 : 0) + q / 3; return (q < (h ? 12 : 15)) ? row * 3 + q % 3 : -1; };
    for (int i = tid; i < 6 * 64; i += 256) {
        const int l = i & 63, s = (i >> 6) & 1, cb = i >> 7;
        const int ch = cb * 32 + (l & 31), h = l >> 5;
        bf16x8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = tap_of(h, s * 8 + j);
            f[j] = (bf16)(t >= 0 ? w[t * CO + ch] : 0.0f);
        }
        wimg[i] = f;
    }
    __syncthreads();
    bf16x8 wa[3][2];
#pragma unroll
    for (int cb = 0; cb < 3; ++cb)
#pragma unroll
        for (int s = 0; s < 2; ++s) wa[cb][s] = wimg[(cb * 2 + s) * 64 + lane];
    f32x4 bv[3][4];                                     // bias of this lane's 48 channels: ch = 32cb + 8q + 4half + j
#pragma unroll
    for (int cb = 0; cb < 3; ++cb)
#pragma unroll
        for (int q = 0; q < 4; ++q) bv[cb][q] = *(const f32x4*)(bias + cb * 32 + q * 8 + half * 4);

    const int OH = R / 2, OW = R / 2, TX = OW / 32;
    char* otile = smem + 6 * 64 * 16 + wave * (32 * CO * 2);
    for (int it = 0; it < STEM_TPW; ++it) {
        const long tile = ((long)blockIdx.x * 4 + wave) * STEM_TPW + it;
        if (tile >= ntiles) break;
        const int tx = (int)(tile % TX), oy = (int)((tile / TX) % OH), b = (int)(tile / ((long)TX * OH));
        const int ox = tx * 32 + px;
        // ---- im2col gather: this lane's 5 (half 0) or 4 (half 1) rows of 3 taps
        bf16x8 xb[2];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int t = tap_of(half, q);               // half is a runtime value: both variants are evaluated below
            float v = 0.0f;
            const int row = (half ? 5 : 0) + q / 3, kx = q % 3;
            const int ci = row / 3, ky = row % 3;
            const int iy = oy * 2 + ky - 1, ix = ox * 2 + kx - 1;
            if (t >= 0 && iy >= 0 && iy < R && ix >= 0)
                v = ld_as_f32<T>(img, (((size_t)b * 3 + ci) * R + iy) * R + ix);
            xb[q >> 3][q & 7] = (bf16)v;
        }
        f32x16 acc[3];
#pragma unroll
        for (int cb = 0; cb < 3; ++cb) {
            f32x16 z;
#pragma unroll
            for (int r = 0; r < 16; ++r) z[r] = 0.0f;
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[cb][0], xb[0], z, 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[cb][1], xb[1], acc[cb], 0, 0, 0);
        }
        // ---- bias + GELU, [px][96] bf16 tile into LDS (lane: pixel px, channels 32cb + 8q + 4half .. +3)
#pragma unroll
        for (int cb = 0; cb < 3; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 g;
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = gelu_erf(acc[cb][4 * q + j] + bv[cb][q][j]);
                *(bf16x4*)(otile + px * (CO * 2) + (cb * 32 + q * 8 + half * 4) * 2) = f32_to_bf4(g);
            }
        // a wave's tile is private to it: the LDS round trip needs no workgroup barrier, only the wave's own ordering
        __builtin_amdgcn_s_waitcnt(0xc07f);               // lgkmcnt(0)
        bf16* dst = out + (((size_t)b * OH + oy) * OW + tx * 32) * CO;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const u32x4 v = *(const u32x4*)(otile + (i * 64 + lane) * 16);
            *(u32x4*)((char*)dst + (i * 64 + lane) * 16) = v;
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);               // reads done before the next tile overwrites the buffer
    }
}

// img [B,3,R,R] (dtype) -> out [B,R/2,R/2,96] bf16;  R % 64 == 0 (so R/2 is a multiple of the 32-pixel tile)
extern "C" int fvhd_launch_stem_conv(hipStream_t st, const void* img, int dtype, void* out, const float* w,
                                     const float* bias, int B, int R)
{
    if (R % 64) return (int)hipErrorInvalidValue;
    const long ntiles = (long)B * (R / 2) * (R / 64);
    dim3 grid((unsigned)((ntiles + 4 * STEM_TPW - 1) / (4 * STEM_TPW))), block(256);
    if (dtype == FVHD_F32) hipLaunchKernelGGL(stem_conv_kernel<float>, grid, block, 0, st, (const float*)img, (bf16*)out, w, bias, B, R, ntiles);
    else if (dtype == FVHD_F16) hipLaunchKernelGGL(stem_conv_kernel<_Float16>, grid, block, 0, st, (const _Float16*)img, (bf16*)out, w, bias, B, R, ntiles);
    else if (dtype == FVHD_BF16) hipLaunchKernelGGL(stem_conv_kernel<bf16>, grid, block, 0, st, (const bf16*)img, (bf16*)out, w, bias, B, R, ntiles);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// ---- stem[0] + stem[1] (+ stem[2]) fused: dense 3x3 s2 (3 -> 96) + GELU, depthwise 3x3 s2 + GELU, 1x1 conv + GELU ---------
// mci.py:563-598.  Unfused, stem[0] writes and stem[1] re-reads a [B, R/2, R/2, 96] bf16 tensor (1.6 GB at B = 32, R = 1024:
// the two launches were write- / read-bound on it, 0.75 + 0.48 ms); here it only ever exists as LDS tiles.
//   * a tile is 8 x 8 stem[1] outputs = a 17 x 17 region of stem[0] outputs (recomputed halo: x1.13), computed exactly as
//     stem_conv_kernel does (same MFMA shapes, k order, bias, GELU, bf16 rounding - the fused result is bit-identical to the
//     two-kernel path) in 10 MFMA tiles of 32 positions and stored position-major [289][96] bf16 in LDS; positions outside
//     the stem[0] map are stored as zeros (stem[1]'s zero padding);
//   * (pixel, 8-channel) units of the depthwise conv are computed from that region (taps fp32 in LDS, same accumulation
//     order as dwconv_tiled_kernel);
//   * w2 != NULL (FULL): stem[2] - the 1x1 conv 96 -> 96 + bias + GELU - on the [64 px][96] bf16 tile while it is in LDS: 18
//     v_mfma_f32_16x16x32_bf16 per wave (W2 fragments as the A operand so that a lane ends with 4 consecutive output channels of
//     one pixel; three K = 32 MFMAs from zero, then + bias, GELU, one rounding, as gemm_kernel<3, 32> does: bit-identical to the
//     GEMM route), stored as whole 192-B pixels.  The unfused path wrote and re-read a [B, R/4, R/4, 96] tensor and cost a launch.
//
// A 512-thread workgroup (one per CU, two waves per SIMD) walks its tiles as a two-stage pipeline, one s_barrier per tile:
//   waves 0-3  PRODUCERS: the stem[0] region of tile k + 1 (im2col gather from an LDS image tile, 6 MFMAs + 48 GELUs per lane and
//              32 positions) into region buffer (k + 1) & 1.  Weight fragments and bias live in registers.
//   waves 4-7  CONSUMERS: stem[1] and stem[2] of tile k from region buffer k & 1.  Wave 4 + c owns pixels 16 c .. 16 c + 15 of the
//              tile from the depthwise units to the store, so the hand-over between the two needs only the wave's own LDS order.
//              Taps of stem[2] and all biases live in registers: the only global loads inside the tile loop are the image's.
//              The consumers also carry the image: the 3 x 35 x 35 pixels under the region of tile k + 3 are loaded into registers
//              during tile k and written, as bf16, into image tile k & 1 one iteration later (the producers gather tile k + 1
//              from the other one meanwhile) - the loads stay in flight for a whole tile.
// (Four 256-thread phases between four barriers, two workgroups per CU, spent 45 % of the wave-cycles waiting: every wave of a
// workgroup was in the same phase, LDS-bound or VALU-bound, at the same time.)
#define STEMF_T 8                         // stem[1] outputs per tile side
#define STEMF_R (2 * STEMF_T + 1)         // stem[0] region side (17)
#define STEMF_NP (STEMF_R * STEMF_R)      // 289 positions
#define STEMF_IR (2 * STEMF_R + 1)        // image rows / columns under the region (35)
#define STEMF_IS 40                       // image tile row stride in LDS (elements): 4-B aligned 3-pixel runs
#define STEMF_IB (3 * STEMF_IR * STEMF_IS * 2)   // image tile bytes (8400)
#define STEMF_PS 208                      // bytes per region position in LDS: 96 bf16 + 16 B pad (a 192-B stride put the 16
                                          // lanes of a ds_write_b64 group on 4 banks: 8-way conflicts; 208 leaves 2-way, the
                                          // least a 16-B aligned pitch allows: pitch / 4 mod 32 is a multiple of 4)
#define STEMF_RB (STEMF_NP * STEMF_PS)    // region buffer bytes (60112)
#define STEMF_YB (64 * STEMF_PS)          // stem[1] tile [64 px][STEMF_PS] (13312)
// LDS: taps of stem[1] | stem[1] tile (the weight fragment image of the prologue aliases it) | 2 image tiles | 2 region buffers
#define STEMF_OFF_Y (9 * 96 * 4)
#define STEMF_OFF_I (STEMF_OFF_Y + STEMF_YB)
#define STEMF_OFF_R (STEMF_OFF_I + 2 * STEMF_IB)
#define STEMF_LDS (STEMF_OFF_R + 2 * STEMF_RB)
static_assert(STEMF_LDS <= 160 * 1024, "the stem pipeline fits the LDS of a CU");
static_assert(6 * 64 * 16 <= STEMF_YB, "the weight fragment image fits into the stem[1] tile it aliases");
static_assert(STEMF_OFF_Y % 16 == 0 && STEMF_IB % 16 == 0 && STEMF_RB % 16 == 0 && STEMF_PS % 16 == 0, "16-B aligned LDS images");

// gelu_erf on a pair: the same clamp, Horner chain and final product, every step one v_pk_*_f32 (a packed fma rounds exactly as
// two v_fma_f32) - 8 packed + 2 v_med3 per pair instead of 11 per value.  Written out because the SLP vectoriser leaves the scalar
// form alone here (the coefficients become literals of v_fmaak_f32).
#define STEM_PK(c) (f32x2{c, c})
FVHD_DEV f32x2 gelu_erf2(f32x2 x)
{
    const f32x2 xc = {__builtin_amdgcn_fmed3f(x[0], -FVHD_GELU_CLAMP, FVHD_GELU_CLAMP), __builtin_amdgcn_fmed3f(x[1], -FVHD_GELU_CLAMP, FVHD_GELU_CLAMP)};
    const f32x2 u = xc * xc;
    f32x2 q = __builtin_elementwise_fma(STEM_PK(FVHD_GELU_C7), u, STEM_PK(FVHD_GELU_C6));
    q = __builtin_elementwise_fma(q, u, STEM_PK(FVHD_GELU_C5));
    q = __builtin_elementwise_fma(q, u, STEM_PK(FVHD_GELU_C4));
    q = __builtin_elementwise_fma(q, u, STEM_PK(FVHD_GELU_C3));
    q = __builtin_elementwise_fma(q, u, STEM_PK(FVHD_GELU_C2));
    q = __builtin_elementwise_fma(q, u, STEM_PK(FVHD_GELU_C1));
    q = __builtin_elementwise_fma(q, u, STEM_PK(FVHD_GELU_C0));
    return x * __builtin_elementwise_fma(xc, q, STEM_PK(0.5f));
}

// The pipeline's barrier: LDS writes of this wave visible, then every wave of the workgroup.  Producers and consumers sit in loops of
// their own and must pass it the same number of times.  (Workgroup scope: no wait for the image loads in flight.)
FVHD_DEV void stemf_barrier()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// LDS hand-over between lanes of ONE wave (its DS operations execute in order): only the compiler must keep the order
FVHD_DEV void stemf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, bool FULL>
__global__ __launch_bounds__(512) void stem_fused_kernel(const T* __restrict__ img, bf16* __restrict__ out,
                                                         const float* __restrict__ w0, const float* __restrict__ b0,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const bf16* __restrict__ w2, const float* __restrict__ b2,
                                                         int B, int R, int ntiles)
{
    constexpr int CO = 96;
    extern __shared__ __attribute__((aligned(16))) char smem_f[];
    float* lw1 = (float*)smem_f;                                 // [9][96] fp32 taps of stem[1]
    char* y1 = smem_f + STEMF_OFF_Y;                             // stem[1] output tile [64 px][STEMF_PS]
    bf16x8* wimg = (bf16x8*)y1;                                  // [cb][s][lane]: 6 KiB, read once before the tile loop
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    auto tap_of = [](int h, int q) { const int row = (h ? 5 : 0) + q / 3; return (q < (h ? 12 : 15)) ? row * 3 + q % 3 : -1; };
    for (int i = tid; i < 6 * 64; i += 512) {
        const int l = i & 63, s = (i >> 6) & 1, cb = i >> 7;
        const int ch = cb * 32 + (l & 31), h = l >> 5;
        bf16x8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = tap_of(h, s * 8 + j);
            f[j] = (bf16)(t >= 0 ? w0[t * CO + ch] : 0.0f);
        }
        wimg[i] = f;
    }
    for (int i = tid; i < 9 * CO / 4; i += 512) *(f32x4*)&lw1[i * 4] = *(const f32x4*)&w1[i * 4];

    const int H1 = R / 2, H2 = R / 4, TXY = H2 / STEMF_T;        // stem[0] map side, stem[1] map side, tiles per side
    // this workgroup's tiles: tile0, tile0 + G, ... (neighbouring workgroups work on neighbouring tiles at the same time: halo pixels hit L2)
    const int G = gridDim.x, tile0 = blockIdx.x;
    const int n = (ntiles - tile0 + G - 1) / G;                  // >= 1: the grid never exceeds the tile count

    if (wave < 4) {
        // ================================================ PRODUCERS: iteration k = the stem[0] region of this workgroup's k-th tile
        const int px = lane & 31, half = lane >> 5;
        stemf_barrier();                                          // weight image visible
        bf16x8 wa[3][2];
#pragma unroll
        for (int cb = 0; cb < 3; ++cb)
#pragma unroll
            for (int s = 0; s < 2; ++s) wa[cb][s] = wimg[(cb * 2 + s) * 64 + lane];
        f32x4 bv[3][4];                                           // bias of this lane's 48 channels: ch = 32cb + 8q + 4half + j
#pragma unroll
        for (int cb = 0; cb < 3; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) bv[cb][q] = *(const f32x4*)(b0 + cb * 32 + q * 8 + half * 4);
        // (the consumers first write the stem[1] tile that aliases the weight image behind the barrier that ends iteration 0)
#pragma unroll 1
        for (int k = 0; k < n; ++k) {
            const int tile = tile0 + k * G;
            const int tx = tile % TXY, ty = (tile / TXY) % TXY;
            const int cy0 = 2 * ty * STEMF_T - 1, cx0 = 2 * tx * STEMF_T - 1;      // stem[0] coordinates of region position (0, 0)
            const bf16* itile = (const bf16*)(smem_f + STEMF_OFF_I + (k & 1) * STEMF_IB);    // [3][35][STEMF_IS] bf16, zero outside the image
            char* reg = smem_f + STEMF_OFF_R + (k & 1) * STEMF_RB;                 // [289][96] bf16
#pragma unroll 1
            for (int t = wave; t * 32 < STEMF_NP; t += 4) {
                const int p = t * 32 + px;
                const int ry = p / STEMF_R, rx = p - ry * STEMF_R;
                const int gy = cy0 + ry, gx = cx0 + rx;               // this lane's stem[0] output pixel
                const bool inside = p < STEMF_NP && gy >= 0 && gy < H1 && gx >= 0 && gx < H1;
                // k-slot q = 3 i + kx of this lane's k-half <-> tap row (ci, ky) = 5 half + i, pixel 2 rx + kx of image-tile row
                // ci * 35 + 2 ry + ky: per tap row two words wa = (px0, px1), wb = (px2, -).  (half 1 has 4 rows: its fifth read
                // and, for lanes past position 288, rows past the tile land in the LDS that follows - never used.)
                unsigned ra[5], rb2[5];
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int rr = half * 5 + i;                      // 0..8 (9 = unused)
                    const int ci = rr / 3, ky = rr - ci * 3;
                    const unsigned* src = (const unsigned*)(itile + (ci * STEMF_IR + 2 * ry + ky) * STEMF_IS + 2 * rx);
                    ra[i] = src[0];
                    rb2[i] = src[1];
                }
                u32x4 x0, x1;
                x0[0] = ra[0];
                x0[1] = (rb2[0] & 0xffffu) | (ra[1] << 16);
                x0[2] = (ra[1] >> 16) | (rb2[1] << 16);
                x0[3] = ra[2];
                x1[0] = (rb2[2] & 0xffffu) | (ra[3] << 16);
                x1[1] = (ra[3] >> 16) | (rb2[3] << 16);
                x1[2] = half ? 0u : ra[4];
                x1[3] = half ? 0u : (rb2[4] & 0xffffu);
                bf16x8 xb[2] = {__builtin_bit_cast(bf16x8, x0), __builtin_bit_cast(bf16x8, x1)};
                f32x16 acc[3];
#pragma unroll
                for (int cb = 0; cb < 3; ++cb) {
                    f32x16 z;
#pragma unroll
                    for (int r = 0; r < 16; ++r) z[r] = 0.0f;
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[cb][0], xb[0], z, 0, 0, 0);
                    acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[cb][1], xb[1], acc[cb], 0, 0, 0);
                }
                if (p < STEMF_NP) {
#pragma unroll
                    for (int cb = 0; cb < 3; ++cb)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const f32x2 g0 = gelu_erf2(f32x2{acc[cb][4 * q], acc[cb][4 * q + 1]} + f32x2{bv[cb][q][0], bv[cb][q][1]});
                            const f32x2 g1 = gelu_erf2(f32x2{acc[cb][4 * q + 2], acc[cb][4 * q + 3]} + f32x2{bv[cb][q][2], bv[cb][q][3]});
                            const u32x2 o = __builtin_bit_cast(u32x2, f32_to_bf4(f32x4{g0[0], g0[1], g1[0], g1[1]}));
                            *(u32x2*)(reg + p * STEMF_PS + (cb * 32 + q * 8 + half * 4) * 2) = inside ? o : u32x2{0u, 0u};   // zero padding of stem[1]
                        }
                }
            }
            stemf_barrier();      // region k complete; the consumers are done with region k - 1 and have written image tile k + 1
        }
        stemf_barrier();          // the consumers' last tile
    } else {
        // ================================================ CONSUMERS: iteration k = stem[1] (+ stem[2]) of the k-th tile; k = -1 only moves the image
        const int cw = wave - 4, rt = tid & 255;
        // The consumers are the longer role (27 ds_read_b128 per depthwise unit): they win the SIMD's issue arbitration against the producer
        // they share it with.  Measured alone at B = 32, R = 1024: 0.633 -> 0.598 ms; the producers preferred instead: 0.690 ms.
        __builtin_amdgcn_s_setprio(1);
        // 3 x 35 x 35 = 3675 image elements under a region.  A thread's elements are (row 8 i + rt / 32, column rt % 32) for
        // i = 0 .. 13 (the 105 x 32 block) and two more for the three remaining columns - rows, channel index and the LDS address are
        // compile-time offsets from one per-thread base.
        constexpr int NROW = 3 * STEMF_IR, NIT = 16;
        auto elem = [&](int i, int ln, int& row, int& col) {         // element i of thread ln: (row of the [105][35] region image, column)
            if (i < 14) { row = 8 * i + ((ln >> 5) & 7); col = ln & 31; }      // (& 7: ln is opaque, the compiler needs the range to fold row / 35)
            else { const int t3 = ln / 3; row = (i == 14 ? 0 : 85) + t3; col = 32 + (ln - 3 * t3); if (i == 15 && ln >= 60) row = NROW; }
        };
        // Buffer loads through a per-image descriptor: an element outside the image gets an out-of-range offset and comes back as
        // zero bits - no validity mask to carry, no 64-bit address arithmetic, no exec-masked branches.  The raw bits ride in registers
        // for a whole tile: NO dependent operation until they are written to LDS.
        // The loads are inline assembly, so the compiler keeps no score of them: it puts no wait behind them (as builtins, the 16-bit
        // mask of a bf16 / f16 element, or the packing of two of them into one register, followed the load at once, and with it the
        // wait for a memory latency per tile; so did address arithmetic that borrowed a load's destination as a don't-care operand
        // half).  image_arrived() is the wait; nothing reads or copies vimg between the two (checked in the assembly: the loop-carried
        // registers are the "+v" operands themselves).
        auto load_image = [&](int tile, unsigned (&v)[NIT]) {
            int ln = rt;
            asm volatile("" : "+v"(ln));                              // opaque: keeps the per-thread address chains out of the tile loop's live set
            const int tx_ = tile % TXY, ty_ = (tile / TXY) % TXY, b_ = tile / (TXY * TXY);
            const int iy0 = 2 * (2 * ty_ * STEMF_T - 1) - 1, ix0 = 2 * (2 * tx_ * STEMF_T - 1) - 1;
            // buffer descriptor of image b_: base, stride 0, 3 R R elements in bytes (offsets beyond return zero), raw 32-bit data format
            const uint64_t base = (uint64_t)(img + (size_t)b_ * 3 * R * R);
            u32x4 rimg = {(uint32_t)base, (uint32_t)(base >> 32) & 0xffffu, (uint32_t)(3 * R * R * sizeof(T)), 0x00020000u};
#pragma unroll
            for (int j = 0; j < 4; ++j) rimg[j] = __builtin_amdgcn_readfirstlane(rimg[j]);
            unsigned off[NIT];
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                int row, col;
                elem(i, ln, row, col);
                const int ci = (row >= STEMF_IR) + (row >= 2 * STEMF_IR), r = row - ci * STEMF_IR;      // compile-time for all but two values of i
                const int iy = iy0 + r, ix = ix0 + col;
                const bool ok = (i < 13 || row < NROW) & ((unsigned)iy < (unsigned)R) & ((unsigned)ix < (unsigned)R);     // '&': selects, not branches
                off[i] = ok ? (unsigned)(((ci * R + iy) * R + ix) * (int)sizeof(T)) : 0xffffffffu;
            }
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                if constexpr (sizeof(T) == 4) asm volatile("buffer_load_dword %0, %1, %2, 0 offen" : "+v"(v[i]) : "v"(off[i]), "s"(rimg) : "memory");
                else asm volatile("buffer_load_ushort %0, %1, %2, 0 offen" : "+v"(v[i]) : "v"(off[i]), "s"(rimg) : "memory");   // zero-extends
            }
        };
        auto image_arrived = [&](unsigned (&v)[NIT]) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < NIT; ++i) asm volatile("" : "+v"(v[i]));      // every use of the values comes after the wait
        };
        auto bits_as_f32 = [](unsigned bits) -> float {               // raw element bits -> its value (zero bits = 0.0 in every dtype)
            if constexpr (sizeof(T) == 4) return __uint_as_float(bits);
            else { const unsigned short h = (unsigned short)bits; return ld_as_f32<T>((const T*)&h, 0); }
        };
        auto store_image = [&](bf16* itile, const unsigned (&v)[NIT]) {     // rounded to bf16, the tower's compute dtype
            int ln = rt;
            asm volatile("" : "+v"(ln));
#pragma unroll
            for (int i = 0; i < NIT; ++i) {
                int row, col;
                elem(i, ln, row, col);
                if (i < 13 || row < NROW) itile[row * STEMF_IS + col] = (bf16)bits_as_f32(v[i]);
            }
        };
        unsigned vimg[NIT] = {};
        load_image(tile0, vimg);
        image_arrived(vimg);
        store_image((bf16*)(smem_f + STEMF_OFF_I), vimg);
        if (1 < n) load_image(tile0 + G, vimg);
        stemf_barrier();                                          // image tile 0 complete (and the weight image, for the producers)

        // this lane's three depthwise units: pixel 16 cw + u / 12, channels 8 (u % 12) .. + 7, u = 64 i + lane
        f32x4 b1v[3][2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int cg = (i * 64 + lane) % 12;
            b1v[i][0] = *(const f32x4*)(b1 + cg * 8);
            b1v[i][1] = *(const f32x4*)(b1 + cg * 8 + 4);
        }
        // stem[2]: B operand: lane (pixel lr, k-group g) holds y1[px][32 ks + 8 g .. + 7]; A operand: W2 rows 16 ob + lr (output channels),
        // the same k range, from the [96][96] bf16 weights; D: lane holds output channels 16 ob + 4 g .. + 3 of pixel lr.
        const int lr = lane & 15, g = lane >> 4;
        char* yrow = y1 + (cw * 16 + lr) * STEMF_PS;
        bf16x8 wb[FULL ? 6 : 1][3];
        f32x4 bq[FULL ? 6 : 1];
        if constexpr (FULL) {
#pragma unroll
            for (int ob = 0; ob < 6; ++ob) {
#pragma unroll
                for (int ks = 0; ks < 3; ++ks) wb[ob][ks] = *(const bf16x8*)(w2 + (ob * 16 + lr) * CO + g * 8 + ks * 32);
                bq[ob] = *(const f32x4*)(b2 + ob * 16 + g * 4);
            }
        }
        // weights and biases arrive HERE (an empty asm is a use): inside the loop the compiler's wait for them would also wait for the
        // previous tile's stores
#pragma unroll
        for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(b1v[i][0]), "+v"(b1v[i][1]));
        if constexpr (FULL) {
#pragma unroll
            for (int ob = 0; ob < 6; ++ob) asm volatile("" : "+v"(wb[ob][0]), "+v"(wb[ob][1]), "+v"(wb[ob][2]), "+v"(bq[ob]));
        }
#pragma unroll 1
        for (int k = -1; k < n; ++k) {
            const int tile = tile0 + k * G;
            const int tx = tile % TXY, ty = (tile / TXY) % TXY, b = tile / (TXY * TXY);
            const char* reg = smem_f + STEMF_OFF_R + (k & 1) * STEMF_RB;
            if (k >= 0) {
                // ---- stem[1] on the LDS region
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int u = i * 64 + lane;
                    const int cg = u % 12, pxl = cw * 16 + u / 12;
                    const int oy = pxl / STEMF_T, ox = pxl - oy * STEMF_T;
                    f32x2 acc[4] = {f32x2{b1v[i][0][0], b1v[i][0][1]}, f32x2{b1v[i][0][2], b1v[i][0][3]},
                                    f32x2{b1v[i][1][0], b1v[i][1][1]}, f32x2{b1v[i][1][2], b1v[i][1][3]}};
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const f32x8 v = bf8_to_f32(*(const bf16x8*)(reg + ((2 * oy + ky) * STEMF_R + 2 * ox + kx) * STEMF_PS + cg * 16));
                            const f32x4 t0 = *(const f32x4*)&lw1[(ky * 3 + kx) * CO + cg * 8], t1 = *(const f32x4*)&lw1[(ky * 3 + kx) * CO + cg * 8 + 4];
                            acc[0] = __builtin_elementwise_fma(f32x2{t0[0], t0[1]}, f32x2{v[0], v[1]}, acc[0]);
                            acc[1] = __builtin_elementwise_fma(f32x2{t0[2], t0[3]}, f32x2{v[2], v[3]}, acc[1]);
                            acc[2] = __builtin_elementwise_fma(f32x2{t1[0], t1[1]}, f32x2{v[4], v[5]}, acc[2]);
                            acc[3] = __builtin_elementwise_fma(f32x2{t1[2], t1[3]}, f32x2{v[6], v[7]}, acc[3]);
                        }
                    f32x8 r;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const f32x2 gl = gelu_erf2(acc[c]);
                        r[2 * c] = gl[0];
                        r[2 * c + 1] = gl[1];
                    }
                    if constexpr (FULL) *(bf16x8*)(y1 + pxl * STEMF_PS + cg * 16) = f32_to_bf8(r);
                    else *(bf16x8*)(out + (((size_t)b * H2 + ty * STEMF_T + oy) * H2 + tx * STEMF_T + ox) * CO + cg * 8) = f32_to_bf8(r);
                }
            }
            // ---- the image: tile k + 2 (loaded during iteration k - 1) into image tile k & 1, which the producers gathered tile k from
            //      one iteration ago; then tile k + 3 into the registers.  Between the two phases: the stores of tile k - 1 that precede
            //      the loads in the memory queue are long done, and stem[2] below needs nothing from memory.
            if (k + 2 < n) {
                image_arrived(vimg);
                store_image((bf16*)(smem_f + STEMF_OFF_I + (k & 1) * STEMF_IB), vimg);
                if (k + 3 < n) load_image(tile + 3 * G, vimg);
            }
            if constexpr (FULL) {
                if (k >= 0) {
                    // ---- stem[2] on this wave's 16 pixels
                    stemf_wave_sync();
                    bf16x8 yb[3];
#pragma unroll
                    for (int ks = 0; ks < 3; ++ks) yb[ks] = *(const bf16x8*)(yrow + ks * 64 + g * 16);
#pragma unroll
                    for (int ob = 0; ob < 6; ++ob) {
                        f32x4 a2 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int ks = 0; ks < 3; ++ks) a2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[ob][ks], yb[ks], a2, 0, 0, 0);
                        const f32x2 g0 = gelu_erf2(f32x2{a2[0], a2[1]} + f32x2{bq[ob][0], bq[ob][1]});
                        const f32x2 g1 = gelu_erf2(f32x2{a2[2], a2[3]} + f32x2{bq[ob][2], bq[ob][3]});
                        *(bf16x4*)(yrow + (ob * 16 + g * 4) * 2) = f32_to_bf4(f32x4{g0[0], g0[1], g1[0], g1[1]});   // in place: the row is in yb
                    }
                    stemf_wave_sync();
                    // whole pixels out: chunk c = 16-B piece (c % 12) of pixel 16 cw + c / 12; a tile row of 8 pixels is 1536 B contiguous
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const int c = i * 64 + lane, pxl = cw * 16 + c / 12, part = c % 12;
                        const int oy = pxl / STEMF_T, ox = pxl - oy * STEMF_T;
                        const u32x4 v = *(const u32x4*)(y1 + pxl * STEMF_PS + part * 16);
                        *(u32x4*)(out + (((size_t)b * H2 + ty * STEMF_T + oy) * H2 + tx * STEMF_T + ox) * CO + part * 8) = v;
                    }
                    stemf_wave_sync();                            // the next tile's units rewrite the rows
                }
            }
            stemf_barrier();      // done with region k (the producers rewrite it in two iterations' time); image tile k & 1 complete
        }
    }
}

// img [B,3,R,R] (dtype) -> out [B,R/4,R/4,96] bf16 = gelu(dw3x3s2(gelu(conv3x3s2(img) + b0)) + b1);  R % 64 == 0
// w2 (bf16 [96][96], as the GEMM packs 1x1 weights) / b2 (fp32 [96]) != NULL: stem[2] too - out = gelu(conv1x1(.) + b2)
extern "C" int fvhd_launch_stem_fused(hipStream_t st, const void* img, int dtype, void* out, const float* w0, const float* b0,
                                      const float* w1, const float* b1, const void* w2, const float* b2, int B, int R)
{
    if ((w2 == nullptr) != (b2 == nullptr)) return (int)hipErrorInvalidValue;
    const bool full = w2 != nullptr;
    if (R % 64 || R <= 0 || B <= 0) return (int)hipErrorInvalidValue;
    const int txy = R / 4 / STEMF_T;
    const size_t shmem = STEMF_LDS;
    const long ntiles = (long)B * txy * txy;
    if (ntiles > 0x7fffffffl / 4) return (int)hipErrorInvalidValue;      // tile indices up to ntiles + 3 G stay ints
    // STEMF_TPW tiles per workgroup, strided by the grid (tile, tile + G, ...): neighbouring workgroups work on neighbouring tiles at
    // the same time (halo pixels hit L2), the tail is at most one tile per workgroup.  The pipeline fills and drains once per workgroup
    // (one tile's time of each role): 8 / 16 / 32 / 64 tiles measured 0.674 / 0.644 / 0.629 / 0.624 ms at B = 32, R = 1024; 32 still gives
    // 256 workgroups, one per CU, at the 8192 tiles where this grid begins.  Smaller problems keep one tile per workgroup to fill the machine.
    constexpr int STEMF_TPW = 32;
    const long G = ntiles >= 8192 ? (ntiles + STEMF_TPW - 1) / STEMF_TPW : ntiles;
    dim3 grid((unsigned)G), block(512);
    static bool attr_set[64][6];
    int dev = 0;
    (void)hipGetDevice(&dev);
#define STEMF_LAUNCH_(TT, FF, IDX)                                                                                             \
    do {                                                                                                                       \
        if (!attr_set[dev & 63][IDX]) {                                                                                        \
            hipError_t e = hipFuncSetAttribute((const void*)stem_fused_kernel<TT, FF>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                               (int)shmem);                                                                    \
            if (e != hipSuccess) return (int)e;                                                                                \
            attr_set[dev & 63][IDX] = true;                                                                                    \
        }                                                                                                                      \
        hipLaunchKernelGGL((stem_fused_kernel<TT, FF>), grid, block, shmem, st, (const TT*)img, (bf16*)out, w0, b0, w1, b1,    \
                           (const bf16*)w2, b2, B, R, (int)ntiles);                                                            \
    } while (0)
#define STEMF_LAUNCH(TT, IDX) do { if (full) STEMF_LAUNCH_(TT, true, 2 * IDX + 1); else STEMF_LAUNCH_(TT, false, 2 * IDX); } while (0)
    if (dtype == FVHD_F32) STEMF_LAUNCH(float, 0);
    else if (dtype == FVHD_F16) STEMF_LAUNCH(_Float16, 1);
    else if (dtype == FVHD_BF16) STEMF_LAUNCH(bf16, 2);
    else return (int)hipErrorInvalidValue;
#undef STEMF_LAUNCH
#undef STEMF_LAUNCH_
    return (int)hipGetLastError();
}

// ---- SE: global average pool over the T tokens of each image -------------------------------------
// y [B, T, C] bf16 -> pooled [B, C] fp32.  grid (C/128, B); a workgroup = 16 channel groups of 8 (one 16-B load each) x 16 token slices: every
// thread sums T/16 tokens (independent loads in flight instead of one dependent 2-B load per token: 75 -> ~8 us at B = 32), the slices
// are added in order through LDS.
__global__ __launch_bounds__(256) void se_pool_kernel(const bf16* __restrict__ y, float* __restrict__ pooled, int T, int C)
{
    __shared__ float red[16][128 + 4];
    const int cg = threadIdx.x & 15, ts = threadIdx.x >> 4, b = blockIdx.y;
    const int c = blockIdx.x * 128 + cg * 8;
    f32x8 s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < C) {
        const bf16* p = y + (size_t)b * T * C + c;
#pragma unroll 4
        for (int t = ts; t < T; t += 16) s += bf8_to_f32(*(const bf16x8*)(p + (size_t)t * C));
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) red[ts][cg * 8 + k] = s[k];
    __syncthreads();
    if (threadIdx.x < 128 && blockIdx.x * 128 + (int)threadIdx.x < C) {
        float a = red[0][threadIdx.x];
#pragma unroll
        for (int i = 1; i < 16; ++i) a += red[i][threadIdx.x];
        pooled[(size_t)b * C + blockIdx.x * 128 + threadIdx.x] = a / (float)T;
    }
}

// ---- SE MLP: scale[b] = sigmoid(We . relu(Wr . pooled[b] + br) + be) -----------------------------
// Wr fp32 [RD][C], We fp32 [C][RD].  Two small launches so that B*RD/4 resp. B*C/256 workgroups
// (1536 / 384 at B = 32) share the 2 x 2.4 MB of weights through L2 instead of 32 workgroups
// streaming them serially.
// hidden[b][r] = relu(Wr[r] . pooled[b] + br[r]);  grid (RD/4, B), one wave per hidden unit.
__global__ __launch_bounds__(256) void se_reduce_kernel(const float* __restrict__ pooled, const float* __restrict__ wr,
                                                        const float* __restrict__ br, float* __restrict__ hidden,
                                                        int C, int RD)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= RD) return;
    const float* wrow = wr + (size_t)r * C;
    const float* p = pooled + (size_t)b * C;
    float s = 0.f;
    for (int i = lane * 4; i < C; i += 256) {
        const f32x4 a = *(const f32x4*)(wrow + i), v = *(const f32x4*)(p + i);
        s += a[0] * v[0] + a[1] * v[1] + a[2] * v[2] + a[3] * v[3];
    }
    s = wave_sum(s);
    if (lane == 0) hidden[(size_t)b * RD + r] = fmaxf(s + br[r], 0.0f);
}

// scale[b][c] = sigmoid(We[c] . hidden[b] + be[c]);  grid (C/256, B), one thread per channel.
__global__ __launch_bounds__(256) void se_expand_kernel(const float* __restrict__ hidden, const float* __restrict__ we,
                                                        const float* __restrict__ be, float* __restrict__ scale,
                                                        int C, int RD)
{
    extern __shared__ float sh[];       // hidden row [RD]
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < RD; i += 256) sh[i] = hidden[(size_t)b * RD + i];
    __syncthreads();
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float* wrow = we + (size_t)c * RD;
    float s = be[c];
    for (int r = 0; r < RD; r += 4) {
        const f32x4 a = *(const f32x4*)(wrow + r);
        s += a[0] * sh[r] + a[1] * sh[r + 1] + a[2] * sh[r + 2] + a[3] * sh[r + 3];
    }
    scale[(size_t)b * C + c] = sigmoidf_fast(s);
}

// ---- out[b,t,c] = gelu(y[b,t,c] * scale[b,c]) in the caller's dtype -------------------------------
template <typename T>
__global__ __launch_bounds__(256) void se_scale_gelu_kernel(const bf16* __restrict__ y, const float* __restrict__ scale,
                                                            T* __restrict__ out, int TT, int C, long total8)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total8) return;
    const long e = i * 8;
    const int c = (int)(e % C);
    const int b = (int)(e / ((long)TT * C));
    const f32x8 v = bf8_to_f32(*(const bf16x8*)(y + e));
    const float* sc = scale + (size_t)b * C + c;
#pragma unroll
    for (int k = 0; k < 8; ++k) out[e + k] = (T)gelu_erf(v[k] * sc[k]);
}

extern "C" int fvhd_launch_se_head(hipStream_t st, const void* y, float* pooled, float* scale, const float* wr,
                                   const float* br, const float* we, const float* be, void* out, int out_dtype,
                                   int B, int T, int C, int RD)
{
    if (C % 8 || RD % 4 || RD > 1024) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(se_pool_kernel, dim3((C + 127) / 128, B), dim3(256), 0, st, (const bf16*)y, pooled, T, C);
    // `pooled` is [B, C + RD]: the pooled row followed by the SE hidden row
    float* hidden = pooled + (size_t)B * C;
    hipLaunchKernelGGL(se_reduce_kernel, dim3((RD + 3) / 4, B), dim3(256), 0, st, pooled, wr, br, hidden, C, RD);
    hipLaunchKernelGGL(se_expand_kernel, dim3((C + 255) / 256, B), dim3(256), (size_t)RD * sizeof(float), st,
                       hidden, we, be, scale, C, RD);
    const long total8 = (long)B * T * C / 8;
    dim3 grid((unsigned)((total8 + 255) / 256));
    if (out_dtype == FVHD_F32) hipLaunchKernelGGL(se_scale_gelu_kernel<float>, grid, dim3(256), 0, st, (const bf16*)y, scale, (float*)out, T, C, total8);
    else if (out_dtype == FVHD_F16) hipLaunchKernelGGL(se_scale_gelu_kernel<_Float16>, grid, dim3(256), 0, st, (const bf16*)y, scale, (_Float16*)out, T, C, total8);
    else if (out_dtype == FVHD_BF16) hipLaunchKernelGGL(se_scale_gelu_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)y, scale, (bf16*)out, T, C, total8);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// ---- dtype conversion of token rows (projector input when the caller's tokens are not bf16) -------
template <typename T>
__global__ __launch_bounds__(256) void cast_to_bf16_kernel(const T* __restrict__ x, bf16* __restrict__ y, long n)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (bf16)(float)x[i];
}

extern "C" int fvhd_launch_cast_to_bf16(hipStream_t st, const void* x, int dtype, void* y, long n)
{
    dim3 grid((unsigned)((n + 255) / 256));
    if (dtype == FVHD_F32) hipLaunchKernelGGL(cast_to_bf16_kernel<float>, grid, dim3(256), 0, st, (const float*)x, (bf16*)y, n);
    else if (dtype == FVHD_F16) hipLaunchKernelGGL(cast_to_bf16_kernel<_Float16>, grid, dim3(256), 0, st, (const _Float16*)x, (bf16*)y, n);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}
