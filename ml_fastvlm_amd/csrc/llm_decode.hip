// Qwen2 decode step kernels: one new token per sequence against the library's own KV cache (include/fvhd.h "LLM decode").
//
// A decode step is a weight stream: B <= 64 rows against every weight of the model.  The prefill's GEMMs (gemm.hip) pad M to 128 / 256
// rows and launch a handful of workgroups at N = 896, so the step has kernels of its own:
//   dec_gemm_kernel     M = B in [1, 16]: every wave owns 16 weight rows (one 16 x 16 x 32 MFMA tile: A = weights, B = the activation
//                       rows), streams them once from HBM straight to VGPRs (non-temporal), and K is split over workgroups where N alone
//                       does not fill the chip; the slices meet in the last-arriving workgroup (fp32 slabs, agent-scope release / acquire,
//                       summed in slice order: deterministic, no float atomics).  RMSNorm is folded into the operand load (every workgroup
//                       recomputes the B row statistics), the epilogue is one of: residual add, silu(gate) * up, bias + rotary embedding +
//                       KV-cache append, or fp32 logits + per-workgroup argmax.  Everything around the main loop - statistics, weight-row
//                       mapping, slabs, epilogues - is dec_gemm_parts.h, shared with the e4m3 and MXFP4 kernels (llm_w8.hip, llm_w4.hip);
//                       the hand-off is split_handoff.h.
//   dec_gemm_wide_kernel   the same for B in [17, 64]: ceil(B / 16) batch tiles of 16 rows per weight fragment, the arithmetic of
//                       dec_gemm_kernel per tile; the row statistics come from dec_rstd_kernel, once per launch.
//   dec_attention       single-query grouped-query attention over the cache, split over the key axis (flash-decoding) with the same
//                       in-launch combine.
//   dec_embed / dec_argmax_finish (+ dec_argmax_blocks / dec_start_state at fvhd_llm_start)     the step's first and last launches: token embedding + the capacity check, the
//                       argmax reduce and the advance of the device-side length / positions.
// Everything that changes from token to token (the cache slot, the positions, the mask column) is read from device memory, so one
// captured graph replays the step for a whole generation.
#include "fvhd_common.h"
#include "launchers.h"      // (with llm_decode.h: the argument structs)
#include "dec_gemm_parts.h"  // better, the row statistics, the split-K meeting, the epilogues (with rope.h, split_handoff.h)

namespace {

FVHD_DEV bf16x8 ld_nt(const bf16* p) { return __builtin_bit_cast(bf16x8, __builtin_nontemporal_load((const u32x4*)p)); }

}  // namespace

// ---------------------------------------------------------------------------------------------------
// Workgroup = 4 waves = 4 tiles of 16 weight rows (a "column" of the grid), K range = slice s of S.  Lane (lr, g) of a wave loads weight
// row lr and activation row min(lr, B - 1), 8 consecutive k at g * 8 of every 32-deep MFMA step; its accumulator holds
// out[row = g * 4 + r][batch = lr].  QKV tiles pair every rotate_half partner in one tile: local rows 0-7 = i .. i + 7 of a head,
// rows 8-15 = i + hd/2 .., so the rotation of a lane's 4 values needs only the lane 32 apart.
template <int EPI>
__global__ __launch_bounds__(256) void dec_gemm_kernel(const DecGemmArgs a)
{
    if (a.status && *a.status) return;
    __shared__ float sh[16 + 4 + 4 * 16 * 2];
    float* rstd = sh;
    int* flag = (int*)(sh + 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
    const int ntiles = a.N / 16, S = a.S;
    const int column = blockIdx.x / S, s = blockIdx.x % S;
    const int tile = column * 4 + wave;
    const bool active = tile < ntiles;                           // wave-uniform
    const int B = a.B, K = a.K;
    const bf16* x = (const bf16*)a.x;
    dec_row_stats<false>(a, rstd, tid, lane, wave, B, K, x);
    const int wrow = dec_weight_row<EPI>(a, tile, lr);
    const int xb = min(lr, B - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const bf16* wr = (const bf16*)a.W + (size_t)min(wrow, a.N - 1) * K + g * 8;
        const bf16* xr = x + (size_t)xb * a.ldx + g * 8;
        const float rs = a.norm_w ? rstd[xb] : 1.f;
        const int KC = K / 128, c0 = s * a.cpw, c1 = min(c0 + a.cpw, KC);
        for (int c = c0; c < c1; ++c) {
            bf16x8 wf[4], xf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = ld_nt(wr + c * 128 + j * 32);
#pragma unroll
            for (int j = 0; j < 4; ++j) xf[j] = *(const bf16x8*)(xr + c * 128 + j * 32);
            if (a.norm_w) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float* w = a.norm_w + c * 128 + j * 32 + g * 8;
                    const f32x4 w0 = *(const f32x4*)w, w1 = *(const f32x4*)(w + 4);
                    const f32x8 v = bf8_to_f32(xf[j]);
                    f32x8 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) { o[k] = v[k] * rs * w0[k]; o[4 + k] = v[4 + k] * rs * w1[k]; }
                    xf[j] = f32_to_bf8(o);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[j], acc, 0, 0, 0);
        }
    }
    if (S > 1) {
        dec_slab_store<1>(a.part, &acc, s, ntiles, tile, active, lane);
        if (!arrive_last(a.cnt + column, S, flag)) return;
        dec_slab_sum<1>(a.part, &acc, S, ntiles, tile, active, lane);
    }
    const int n0 = tile * 16 + g * 4;                            // this lane's 4 outputs: rows n0 .. n0 + 3 of batch row lr
    dec_gemm_epilogue<EPI, 1>(a, &acc, sh, tid, lane, wave, lr, g, B, tile, active, n0);
}

// The same GEMM for 17 .. 64 rows: NB = ceil(B / 16) batch tiles of 16 rows in 2 .. 4.  A weight fragment is still read once (ld_nt) and
// multiplies the NB activation fragments into NB accumulators; lane (lr, g) loads activation row min(t * 16 + lr, B - 1) for tile t and
// accumulator t holds out[row = g * 4 + r][batch = t * 16 + lr].  Batch tile t does the arithmetic of dec_gemm_kernel on rows
// [16 t, 16 t + 16) in its order, so a row's bits do not depend on the batch it is decoded in; the split-K slab is [S][N / 16][NB][64][4],
// the (max, index) pairs [gridDim][16 * NB].  dec_gemm_kernel stays a kernel and a loop of its own: written as the NB = 1 case of this
// template the compiler scheduled its prologue differently, which cost 0.2-0.5 % of the 0.5B step at B = 1 / 8.  The parts
// around the loops are shared (dec_gemm_parts.h): they leave both kernels' prologues and loops as they were.
template <int EPI, int NB>
__global__ __launch_bounds__(256) void dec_gemm_wide_kernel(const DecGemmArgs a)
{
    static_assert(NB >= 2 && NB <= 4, "batch tiles of the wide decode GEMM");
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
    dec_row_stats<true>(a, rstd, tid, lane, wave, B, K, x);
    const int wrow = dec_weight_row<EPI>(a, tile, lr);
    int xb[NB];
    f32x4 acc[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) { xb[t] = min(t * 16 + lr, B - 1); acc[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (active) {
        const bf16* wr = (const bf16*)a.W + (size_t)min(wrow, a.N - 1) * K + g * 8;
        const bf16* xr[NB];
        float rs[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
            xr[t] = x + (size_t)xb[t] * a.ldx + g * 8;
            rs[t] = a.norm_w ? rstd[xb[t]] : 1.f;
        }
        const int KC = K / 128, c0 = s * a.cpw, c1 = min(c0 + a.cpw, KC);
        for (int c = c0; c < c1; ++c) {
            bf16x8 wf[4], xf[NB][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = ld_nt(wr + c * 128 + j * 32);
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
    dec_gemm_epilogue<EPI, NB>(a, acc, sh, tid, lane, wave, lr, g, B, tile, active, n0);
}

// The RMSNorm row statistics of a wide launch (B > 16), once per launch site instead of once per workgroup of dec_gemm_kernel: wave = row,
// the same loop, the same bits.
__global__ __launch_bounds__(256) void dec_rstd_kernel(const bf16* __restrict__ x, int ldx, int K, int B, float eps, float* __restrict__ rstd,
                                                       const int* status)
{
    if (status && *status) return;
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const bf16* xr = x + (size_t)b * ldx;
    float ss = 0.f;
    for (int c = lane * 8; c < K; c += 512) {
        const f32x8 v = bf8_to_f32(*(const bf16x8*)(xr + c));
#pragma unroll
        for (int k = 0; k < 8; ++k) ss = __builtin_fmaf(v[k], v[k], ss);
    }
    ss = wave_sum(ss);
    if (lane == 0) rstd[b] = 1.0f / sqrtf(ss / (float)K + eps);
}

// ---------------------------------------------------------------------------------------------------
// Single-query attention of q [B][nh * HD] over the cache keys [0, *len + len_add) of sequence b (kv head h / (nh / nkv)), key_valid
// [cache_batch][cap]: out = softmax(q . k * HD^-0.5 over valid keys) . v, fp32 softmax.  Workgroup = (b, h, key slice of `chunk` keys);
// the 4 waves take 64-key blocks of the slice in turn (lane = key for the scores, lane = HD / 64 output dims for P.V) with an online
// softmax, meet in LDS, and the S slices of (b, h) meet in the last-arriving workgroup, in slice order.
template <int HD>
__global__ __launch_bounds__(256) void dec_attention_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kc, const bf16* __restrict__ vc,
                                                            const unsigned char* __restrict__ key_valid, bf16* __restrict__ out, int nh, int nkv,
                                                            int cap, const int* len, int len_add, int S, int chunk, float* part, int* cnt,
                                                            const int* status, float scale)
{
    constexpr int DPL = HD / 64;
    if (status && *status) return;
    __shared__ float sh[HD + 4 * (HD + 2) + 4];
    float* qs = sh;
    float* ws = sh + HD;                                         // per wave: m, l, o[HD]
    int* flag = (int*)(sh + HD + 4 * (HD + 2));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bh = blockIdx.x / S, s = blockIdx.x % S, b = bh / nh, h = bh % nh, kvh = h / (nh / nkv);
    const int Lk = min(*len + len_add, cap);
    const int k0 = s * chunk, k1 = min(k0 + chunk, Lk);
    if (tid < HD) qs[tid] = (float)q[(size_t)b * nh * HD + h * HD + tid];
    __syncthreads();
    const bf16* kb_ = kc + ((size_t)b * nkv + kvh) * cap * HD;
    const bf16* vb_ = vc + ((size_t)b * nkv + kvh) * cap * HD;
    const unsigned char* mk = key_valid + (size_t)b * cap;
    float m = -INFINITY, l = 0.f, o[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) o[i] = 0.f;
    for (int kb = k0 + wave * 64; kb < k1; kb += 256) {
        const int key = kb + lane;
        const bool valid = key < k1 && mk[min(key, cap - 1)] != 0;
        float sc = -INFINITY;
        if (valid) {
            const bf16* kr = kb_ + (size_t)key * HD;
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < HD; c += 8) {
                const f32x8 kv = bf8_to_f32(*(const bf16x8*)(kr + c));
#pragma unroll
                for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(kv[e], qs[c + e], acc);
            }
            sc = acc * scale;
        }
        float mb = sc;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mb = fmaxf(mb, __shfl_xor(mb, off, 64));
        if (mb == -INFINITY) continue;                           // no valid key in this block (wave-uniform)
        const float mn = fmaxf(m, mb);
        const float alpha = m == -INFINITY ? 0.f : expf(m - mn);
        const float p = valid ? expf(sc - mn) : 0.f;
        l = l * alpha + wave_sum(p);
#pragma unroll
        for (int i = 0; i < DPL; ++i) o[i] *= alpha;
        m = mn;
        for (int j = 0; j < 64; ++j) {
            const float pj = __shfl(p, j, 64);
            if (pj == 0.f) continue;                             // masked or beyond the slice (wave-uniform): its row is never read
            const bf16* vr = vb_ + (size_t)(kb + j) * HD + lane * DPL;
            if constexpr (DPL == 1) o[0] = __builtin_fmaf(pj, (float)vr[0], o[0]);
            else {
                const bf16x2 vv = *(const bf16x2*)vr;
                o[0] = __builtin_fmaf(pj, (float)vv[0], o[0]);
                o[1] = __builtin_fmaf(pj, (float)vv[1], o[1]);
            }
        }
    }
    float* mine = ws + wave * (HD + 2);
    if (lane == 0) { mine[0] = m; mine[1] = l; }
#pragma unroll
    for (int i = 0; i < DPL; ++i) mine[2 + lane * DPL + i] = o[i];
    __syncthreads();
    // waves -> one (m, l, o) of this slice, in wave order (wave 0)
    float M = -INFINITY, L = 0.f, O[DPL];
#pragma unroll
    for (int i = 0; i < DPL; ++i) O[i] = 0.f;
    if (wave == 0) {
        for (int w = 0; w < 4; ++w) M = fmaxf(M, ws[w * (HD + 2)]);
        if (M != -INFINITY)
            for (int w = 0; w < 4; ++w) {
                const float wm = ws[w * (HD + 2)];
                if (wm == -INFINITY) continue;
                const float f = expf(wm - M);
                L += ws[w * (HD + 2) + 1] * f;
#pragma unroll
                for (int i = 0; i < DPL; ++i) O[i] += ws[w * (HD + 2) + 2 + lane * DPL + i] * f;
            }
    }
    if (S > 1) {
        if (wave == 0) {
            float* slab = part + ((size_t)bh * S + s) * (HD + 2);
            if (lane == 0) { slab[0] = M; slab[1] = L; }
#pragma unroll
            for (int i = 0; i < DPL; ++i) slab[2 + lane * DPL + i] = O[i];
        }
        if (!arrive_last(cnt + bh, S, flag)) return;             // every wave joins the hand-off's barriers (split_handoff.h)
        if (wave != 0) return;
        M = -INFINITY;
        for (int t = 0; t < S; ++t) M = fmaxf(M, part[((size_t)bh * S + t) * (HD + 2)]);
        L = 0.f;
#pragma unroll
        for (int i = 0; i < DPL; ++i) O[i] = 0.f;
        if (M != -INFINITY)
            for (int t = 0; t < S; ++t) {
                const float* sl = part + ((size_t)bh * S + t) * (HD + 2);
                if (sl[0] == -INFINITY) continue;
                const float f = expf(sl[0] - M);
                L += sl[1] * f;
#pragma unroll
                for (int i = 0; i < DPL; ++i) O[i] += sl[2 + lane * DPL + i] * f;
            }
    } else if (wave != 0) {
        return;
    }
    const float inv = L > 0.f ? 1.0f / L : 0.f;                  // a sequence with no valid key at all: zeros (finite)
#pragma unroll
    for (int i = 0; i < DPL; ++i) out[(size_t)b * nh * HD + h * HD + lane * DPL + i] = (bf16)(O[i] * inv);
}

// ---------------------------------------------------------------------------------------------------
// The step's first launch: the capacity check, then h[b] = table[id_b] (the packed lm_head of a tied model, else the embedding table)
// and key_valid[b][*len] = 1.  ids: token_ids, or the ids the previous step chose.
__global__ __launch_bounds__(256) void dec_embed_kernel(const int64_t* __restrict__ tok, const int64_t* __restrict__ last, const bf16* __restrict__ table,
                                                        int V, int H, bf16* __restrict__ h, unsigned char* __restrict__ key_valid, int cap,
                                                        const int* len, int* status, int* status_host)
{
    if (*status) return;
    const int b = blockIdx.x;
    const int L = *len;
    if (L >= cap) {                                              // past the capacity: nothing is written, the error is sticky
        if (b == 0 && threadIdx.x == 0) { *status = 1; *status_host = 1; }
        return;
    }
    const int64_t id = tok ? tok[b] : last[b];
    if (id < 0 || id >= V) {
        if (threadIdx.x == 0) { *status = 2; *status_host = 2; }
        return;
    }
    const bf16* src = table + (size_t)id * H;
    for (int c = threadIdx.x * 8; c < H; c += 256 * 8) *(u32x4*)(h + (size_t)b * H + c) = *(const u32x4*)(src + c);
    if (threadIdx.x == 0) key_valid[(size_t)b * cap + L] = 1;
}

// The lm_head's per-workgroup (max, index) pairs [nblk][16 * ceil(B / 16)] -> ids of the B rows (ties: lowest index), then - when `len` is
// given - the advance of the step: positions + 1, length + 1.  Workgroup t takes the 16 rows of batch tile t.
__global__ __launch_bounds__(256) void dec_argmax_finish_kernel(const float* __restrict__ av, const int* __restrict__ ai, int nblk, int B, int64_t* last,
                                                                int64_t* ids_out, int64_t* posv, int* len, const int* status)
{
    if (status && *status) return;
    __shared__ float sv[256];
    __shared__ int si[256];
    const int tid = threadIdx.x, ld = 16 * gridDim.x;
    for (int b = blockIdx.x * 16; b < min(B, blockIdx.x * 16 + 16); ++b) {
        float v = -INFINITY;
        int i = 0x7fffffff;
        for (int k = tid; k < nblk; k += 256)
            if (better(av[(size_t)k * ld + b], ai[(size_t)k * ld + b], v, i)) { v = av[(size_t)k * ld + b]; i = ai[(size_t)k * ld + b]; }
        sv[tid] = v;
        si[tid] = i;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o && better(sv[tid + o], si[tid + o], sv[tid], si[tid])) { sv[tid] = sv[tid + o]; si[tid] = si[tid + o]; }
            __syncthreads();
        }
        if (tid == 0) {
            const int64_t id = si[0] == 0x7fffffff ? 0 : si[0];
            if (last) last[b] = id;
            if (ids_out) ids_out[b] = id;
            if (posv) posv[b] += 1;
        }
        __syncthreads();
    }
    if (tid == 0 && blockIdx.x == 0 && len) *len += 1;          // nothing in this launch reads it
}

// fvhd_llm_start's first-token argmax over the prefill's fp32 logits [B][V], in the lm_head's shape: workgroup k takes columns
// [64 k, 64 k + 64) of every row (wave w: rows w, w + 4, ..; lane = column) and leaves its (max, index) pairs in av / ai [k][16] for
// dec_argmax_finish_kernel
__global__ __launch_bounds__(256) void dec_argmax_blocks_kernel(const float* __restrict__ logits, int V, int B, float* __restrict__ av, int* __restrict__ ai)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane, ld = (B + 15) / 16 * 16;
    for (int b = wave; b < B; b += 4) {
        float v = -INFINITY;
        int i = 0x7fffffff;
        if (col < V) { v = logits[(size_t)b * V + col]; i = col; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(i, o, 64);
            if (better(ov, oi, v, i)) { v = ov; i = oi; }
        }
        if (lane == 0) { av[(size_t)blockIdx.x * ld + b] = v; ai[(size_t)blockIdx.x * ld + b] = i; }
    }
}

// fvhd_llm_start's state: the first decode position (position_ids[b][T - 1] + 1, or T), the cache length T, the error word cleared
__global__ __launch_bounds__(64) void dec_start_state_kernel(int64_t* posv, const int64_t* position_ids, int B, int T, int* len, int* status)
{
    const int b = threadIdx.x;
    if (b < B) posv[b] = position_ids ? position_ids[(size_t)b * T + T - 1] + 1 : (int64_t)T;
    if (b == 0) { *len = T; *status = 0; }
}

// ---------------------------------------------------------------------------------------------------
template <int EPI>
static void launch_dec_gemm(hipStream_t st, const dim3 grid, const DecGemmArgs& a)
{
    const dim3 block(256);
    switch ((a.B + 15) / 16) {
    case 1: hipLaunchKernelGGL(dec_gemm_kernel<EPI>, grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((dec_gemm_wide_kernel<EPI, 2>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((dec_gemm_wide_kernel<EPI, 3>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((dec_gemm_wide_kernel<EPI, 4>), grid, block, 0, st, a); break;
    }
}

extern "C" int fvhd_launch_dec_gemm(hipStream_t st, const DecGemmArgs* a)
{
    if (a->B < 1 || a->B > 64 || a->N % 16 || a->K % 128 || a->S < 1 || a->cpw < 1 || (long)a->S * a->cpw < a->K / 128 ||
        (long)(a->S - 1) * a->cpw >= a->K / 128 || (a->S > 1 && (!a->part || !a->cnt)))
        return (int)hipErrorInvalidValue;
    if (a->epi < DEC_EPI_RESID || a->epi > DEC_EPI_ARGMAX) return (int)hipErrorInvalidValue;
    if (a->epi == DEC_EPI_QKV && (a->hd % 16 || a->N != (a->nh + 2 * a->nkv) * a->hd)) return (int)hipErrorInvalidValue;
    if (a->epi == DEC_EPI_ARGMAX && a->S != 1) return (int)hipErrorInvalidValue;
    if (a->norm_w && a->rstd && a->B > 16)
        hipLaunchKernelGGL(dec_rstd_kernel, dim3((a->B + 3) / 4), dim3(256), 0, st, (const bf16*)a->x, a->ldx, a->K, a->B, a->eps, a->rstd, a->status);
    if (a->wscale) return fvhd_launch_dec_gemm_w8(st, a);         // e4m3 weights: the sibling kernels
    if (a->wblk) return fvhd_launch_dec_gemm_w4(st, a);           // MXFP4 weights: theirs
    const int ncol = (a->N / 16 + 3) / 4;
    const dim3 grid((unsigned)((long)ncol * a->S));
    switch (a->epi) {
    case DEC_EPI_RESID: launch_dec_gemm<DEC_EPI_RESID>(st, grid, *a); break;
    case DEC_EPI_SWIGLU: launch_dec_gemm<DEC_EPI_SWIGLU>(st, grid, *a); break;
    case DEC_EPI_QKV: launch_dec_gemm<DEC_EPI_QKV>(st, grid, *a); break;
    default: launch_dec_gemm<DEC_EPI_ARGMAX>(st, grid, *a); break;
    }
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_attention(hipStream_t st, const void* q, const void* kc, const void* vc, const unsigned char* key_valid, void* out, int B,
                                         int nh, int nkv, int hd, int cap, const int* len, int len_add, int S, int chunk, float* part, int* cnt,
                                         const int* status)
{
    if (B < 1 || nh < 1 || nkv < 1 || nh % nkv || cap < 1 || S < 1 || chunk < 1 || (long)S * chunk < cap || (S > 1 && (!part || !cnt)))
        return (int)hipErrorInvalidValue;
    const float scale = 1.0f / sqrtf((float)hd);
    const dim3 grid((unsigned)((long)B * nh * S)), block(256);
    if (hd == 64)
        hipLaunchKernelGGL(dec_attention_kernel<64>, grid, block, 0, st, (const bf16*)q, (const bf16*)kc, (const bf16*)vc, key_valid, (bf16*)out, nh, nkv, cap,
                           len, len_add, S, chunk, part, cnt, status, scale);
    else if (hd == 128)
        hipLaunchKernelGGL(dec_attention_kernel<128>, grid, block, 0, st, (const bf16*)q, (const bf16*)kc, (const bf16*)vc, key_valid, (bf16*)out, nh, nkv, cap,
                           len, len_add, S, chunk, part, cnt, status, scale);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_embed(hipStream_t st, const int64_t* tok, const int64_t* last, const void* table, int V, int H, void* h, unsigned char* key_valid,
                                     int B, int cap, const int* len, int* status, int* status_host)
{
    if (B < 1 || H % 8) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_embed_kernel, dim3(B), dim3(256), 0, st, tok, last, (const bf16*)table, V, H, (bf16*)h, key_valid, cap, len, status, status_host);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_argmax_finish(hipStream_t st, const float* av, const int* ai, int nblk, int B, int64_t* last, int64_t* ids_out, int64_t* posv,
                                             int* len, const int* status)
{
    if (B < 1 || B > 64 || nblk < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_argmax_finish_kernel, dim3((B + 15) / 16), dim3(256), 0, st, av, ai, nblk, B, last, ids_out, posv, len, status);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_argmax_blocks(hipStream_t st, const float* logits, int V, int B, float* av, int* ai)
{
    if (B < 1 || B > 64 || V < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_argmax_blocks_kernel, dim3((V + 63) / 64), dim3(256), 0, st, logits, V, B, av, ai);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_start_state(hipStream_t st, int64_t* posv, const int64_t* position_ids, int B, int T, int* len, int* status)
{
    if (B < 1 || B > 64 || T < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_start_state_kernel, dim3(1), dim3(64), 0, st, posv, position_ids, B, T, len, status);
    return (int)hipGetLastError();
}
