// The parts of the decode GEMM that do not depend on the weight format: what dec_gemm_kernel / dec_gemm_wide_kernel (llm_decode.hip),
// dec_gemm_w8_kernel (llm_w8.hip) and dec_gemm_w4_kernel (llm_w4.hip) do around their main loops.  The four kernels and their loops stay
// separate texts - they differ in how a weight fragment reaches the MFMA, and the 16-row kernel's schedule is a measured one
// - and each keeps its signature, its __shared__ array, its index preamble and its operand pointers.
//
// How the parts are spelt, so that a kernel compiles to what it was with the text in place (profiles/dec_gemm_parts_isa.md):
//   - force-inlined, and handed the kernel's own indices (tid, lane, wave, lr, g, tile, ..) instead of recomputing them;
//   - DecGemmArgs BY VALUE, never by reference.  A helper is optimised on its own before it is inlined; through a reference every
//     a.field is a load that the stores of the epilogue's batch-tile loop may alias, so nothing computed from a field leaves that loop -
//     the q|k|v epilogue then evaluated rope_rotate's powf once per batch tile instead of once (+20 .. +37 % instructions at NB >= 2).
//     The copy exists for the optimiser only: the fields stay the kernel-argument loads they were, nothing goes to scratch;
//   - no helper holds the `return` of a kernel (the split-K meeting): see dec_slab_store.
//
// NB = batch tiles of 16 rows (1 .. 4); `acc` points to the lane's NB accumulators, accumulator t holding out[row = g * 4 + r][batch =
// t * 16 + lr].  The workgroup's LDS is float sh[16 NB + 4 + 4 * 16 NB * 2]: the row statistics [16 NB], the hand-off's flag (4 words),
// then the argmax pairs.
#pragma once
#include "fvhd_common.h"
#include "llm_decode.h"
#include "rope.h"
#include "split_handoff.h"

// (value, index) order of torch.argmax: larger value first, the lower index on a tie
FVHD_DEV bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// RMSNorm row statistics of the B operand rows into rstd[0 .. B), when the launch folds a norm (a.norm_w): either the copy of what
// dec_rstd_kernel wrote once for the launch (FROM_LAUNCH kernels with a.rstd given), or rmsnorm_kernel's statistics, in its order
// (identical bits), recomputed by every workgroup.  The 16-row bf16 kernel never reads a.rstd: FROM_LAUNCH = false.
template <bool FROM_LAUNCH>
FVHD_DEV void dec_row_stats(const DecGemmArgs a, float* rstd, int tid, int lane, int wave, int B, int K, const bf16* x)
{
    if (a.norm_w) {
        if (FROM_LAUNCH && a.rstd) {                             // dec_rstd_kernel wrote them once for the launch
            if (tid < B) rstd[tid] = a.rstd[tid];
        } else {                                                 // rmsnorm_kernel's statistics, in its order (identical bits)
            for (int b = wave; b < B; b += 4) {
                const bf16* xr = x + (size_t)b * a.ldx;
                float ss = 0.f;
                for (int c = lane * 8; c < K; c += 512) {
                    const f32x8 v = bf8_to_f32(*(const bf16x8*)(xr + c));
#pragma unroll
                    for (int k = 0; k < 8; ++k) ss = __builtin_fmaf(v[k], v[k], ss);
                }
                ss = wave_sum(ss);
                if (lane == 0) rstd[b] = 1.0f / sqrtf(ss / (float)K + a.eps);
            }
        }
        __syncthreads();
    }
}

// The weight row lane lr of a wave loads for its tile.  QKV tiles pair every rotate_half partner in one tile: local rows 0-7 = i .. i + 7
// of a head, rows 8-15 = i + hd/2 .., so the rotation of a lane's 4 values needs only the lane 32 apart.
template <int EPI>
FVHD_DEV int dec_weight_row(const DecGemmArgs a, int tile, int lr)
{
    int wrow = tile * 16 + lr;
    if constexpr (EPI == DEC_EPI_QKV) {
        const int tph = a.hd / 16, head = tile / tph, pb = tile % tph;
        wrow = head * a.hd + (lr < 8 ? pb * 8 + lr : a.hd / 2 + pb * 8 + lr - 8);
    }
    return wrow;
}

// The split-K meeting of the S workgroups of a column (a.S > 1), in the kernel:
//     dec_slab_store<NB>(..);  if (!arrive_last(a.cnt + column, S, flag)) return;  dec_slab_sum<NB>(..);
// slice s stores its accumulators to the slab [S][N / 16][NB][64][4]; every workgroup but the last to arrive (split_handoff.h) leaves; in
// the last one the accumulators become the sum of the S slabs in slice order (deterministic, no float atomics).  The `return` stays in
// the kernel: a helper that returns "leave" costs a merged flag and accumulator copies behind it.
template <int NB>
FVHD_DEV void dec_slab_store(float* part, const f32x4* acc, int s, int ntiles, int tile, bool active, int lane)
{
    if (active) {
#pragma unroll
        for (int t = 0; t < NB; ++t) *(f32x4*)(part + ((((size_t)s * ntiles + tile) * NB + t) * 64 + lane) * 4) = acc[t];
    }
}

template <int NB>
FVHD_DEV void dec_slab_sum(const float* part, f32x4* acc, int S, int ntiles, int tile, bool active, int lane)
{
    if (active) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int u = 0; u < S; ++u) acc[t] += *(const f32x4*)(part + ((((size_t)u * ntiles + tile) * NB + t) * 64 + lane) * 4);
        }
    }
}

// The epilogue: this lane's 4 outputs of batch tile t are rows n0 .. n0 + 3 (n0 = tile * 16 + g * 4) of batch row t * 16 + lr.
// rowscale (q|k|v of the e4m3 kernel only, else NULL): the scales of the lane's four rows, which that kernel leaves to this epilogue -
// its projection is fma(acc, scale, bias), ONE rounding.  (It always was: while the kernel's multiply and this sum were one text the
// compiler contracted them, because they met in one basic block; across a helper they did so at NB = 1 only.  Now the code says it.)
template <int EPI, int NB>
FVHD_DEV void dec_gemm_epilogue(const DecGemmArgs a, const f32x4* acc, float* sh, int tid, int lane, int wave, int lr, int g, int B, int tile, bool active,
                                int n0, const f32x4* rowscale = nullptr)
{
    if constexpr (EPI == DEC_EPI_RESID) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int b = t * 16 + lr;
            if (active && b < B) {
                const f32x4 r = bf4_to_f32(*(const bf16x4*)((const bf16*)a.resid + (size_t)b * a.ldo + n0));
                *(bf16x4*)((bf16*)a.out + (size_t)b * a.ldo + n0) = f32_to_bf4(r + acc[t]);
            }
        }
    } else if constexpr (EPI == DEC_EPI_SWIGLU) {
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int b = t * 16 + lr;
            if (active && b < B) {
                bf16x2 o;
                o[0] = (bf16)(acc[t][0] * sigmoidf_fast(acc[t][0]) * acc[t][1]);
                o[1] = (bf16)(acc[t][2] * sigmoidf_fast(acc[t][2]) * acc[t][3]);
                *(bf16x2*)((bf16*)a.out + (size_t)b * a.ldo + n0 / 2) = o;
            }
        }
    } else if constexpr (EPI == DEC_EPI_QKV) {
        if (active) {
            const int hd = a.hd, tph = hd / 16, head = tile / tph, pb = tile % tph;
            const bool first = g < 2;
            const int i4 = pb * 8 + (g & 1) * 4, d = first ? i4 : hd / 2 + i4;
            const f32x4 bias = *(const f32x4*)(a.bias + head * hd + d);
#pragma unroll
            for (int t = 0; t < NB; ++t) {
                const int b = t * 16 + lr;
                // the projection's output as the reference holds it (bf16)
                const f32x4 v = bf4_to_f32(f32_to_bf4(rowscale ? __builtin_elementwise_fma(acc[t], *rowscale, bias) : acc[t] + bias));
                f32x4 other;
#pragma unroll
                for (int r = 0; r < 4; ++r) other[r] = __shfl_xor(v[r], 32, 64);
                bf16x4 res = f32_to_bf4(v);
                if (b < B) {
                    if (head < a.nh + a.nkv) {
                        bf16x4 ra, rb;
                        rope_rotate(first ? v : other, first ? other : v, (long)a.pos[b], i4, a.rope, hd, a.P, a.theta, ra, rb);
                        res = first ? ra : rb;
                    }
                    if (head < a.nh) {
                        *(bf16x4*)((bf16*)a.out + (size_t)b * a.ldo + head * hd + d) = res;
                    } else {
                        const int kvh = head < a.nh + a.nkv ? head - a.nh : head - a.nh - a.nkv;
                        bf16* cache = (bf16*)(head < a.nh + a.nkv ? a.kc : a.vc);
                        const int slot = *a.len;
                        if (slot >= 0 && slot < a.cap)
                            *(bf16x4*)(cache + (((size_t)b * a.nkv + kvh) * a.cap + slot) * hd + d) = res;
                    }
                }
            }
        }
    } else if constexpr (EPI == DEC_EPI_ARGMAX) {
        float* rv = sh + 16 * NB + 4;                            // [wave][batch tile][16] best value / index of the wave's 16 weight rows
        int* ri = (int*)(rv + 64 * NB);
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            const int b = t * 16 + lr;
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            if (active && b < B) {
                if (a.logits) *(f32x4*)(a.logits + (size_t)b * a.N + n0) = acc[t];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (better(acc[t][r], n0 + r, bv, bi)) { bv = acc[t][r]; bi = n0 + r; }
            }
#pragma unroll
            for (int o = 16; o <= 32; o <<= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane < 16) { rv[(wave * NB + t) * 16 + lane] = bv; ri[(wave * NB + t) * 16 + lane] = bi; }
        }
        __syncthreads();
        if (tid < 16 * NB && tid < B) {
            const int t = tid >> 4, r = tid & 15;
            float v = rv[t * 16 + r];
            int i = ri[t * 16 + r];
            for (int w = 1; w < 4; ++w)
                if (better(rv[(w * NB + t) * 16 + r], ri[(w * NB + t) * 16 + r], v, i)) { v = rv[(w * NB + t) * 16 + r]; i = ri[(w * NB + t) * 16 + r]; }
            a.amax_v[(size_t)blockIdx.x * (16 * NB) + tid] = v;
            a.amax_i[(size_t)blockIdx.x * (16 * NB) + tid] = i;
        }
    }
}
