// Extending a started KV cache by a chunk of T tokens per row (include/fvhd.h "LLM extend", fvhd_llm_extend / fvhd_llm_cache_rewind):
//     llm_attention_past_kernel<HD>     causal grouped-query attention of the chunk's T queries over cache slots [0, P + T), P = *past_len
//     llm_cache_append_kernel           the chunk's rotated k heads and v heads -> slots P + t of one layer's strided caches (+ the mask column)
//     llm_extend_positions_kernel       the positions of a chunk given without position ids
//     llm_extend_state_kernel           length += T, next positions
//     llm_cache_rewind_kernel           drop the slots >= keep[b] of every row
// P is a DEVICE word in all of them: the host arguments do not depend on the length, so the call composes with replayed decode graphs
// without a synchronisation.  The sticky error word of the decode (llm_decode.hip: dec_embed_kernel) gates every launch.
#include "fvhd_common.h"
#include "launchers.h"

// ---------------------------------------------------------------------------------------------------
// The sibling of llm_attention_kernel (llm.hip) whose keys sit in the cache: the same flash structure (S^T = K . Q^T on the 16x16x32 bf16
// MFMA, P in registers as the B operand of O^T = V^T . P^T, the denominator from a ones fragment, 64-key tiles double-buffered in LDS,
// 128 queries per workgroup = 2 x 16 per wave, the XCD remap, the all-masked-row rule).  Key tiles are aligned to slot 0; key j is visible to
// chunk query t iff j <= P + t and key_valid[b][j].  A tile takes the masking branch when it holds an invalid key or reaches past P + the
// wave's first query; tiles beyond P + the workgroup's last query are never loaded.  With P = 0 every operation of llm_attention_kernel
// happens in the same order on the same values: the outputs are bit-identical (tests/test_gpu_extend_ops.py).
template <int HD>
struct PastAttCfg {
    static constexpr int KT = 64, QW = 2, QB = 64 * QW;
    static constexpr int KBYTES = KT * HD * 2;                  // K tile: HD / 64 panels of [64 keys][64 d], 128-B rows, XOR-swizzled slots
    static constexpr int VSTRIDE = 136;                         // bytes per V^T row (64 keys * 2 B + 8 B pad)
    static constexpr int VBYTES = HD * VSTRIDE;
    static constexpr int LDS = 2 * (KBYTES + VBYTES);
};

template <int HD>
__global__ __launch_bounds__(256) void llm_attention_past_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ kcache, const bf16* __restrict__ vcache,
                                                                 bf16* __restrict__ out, const unsigned char* __restrict__ key_valid, int T, int nh, int nkv,
                                                                 int cap, const int* __restrict__ past_len, const int* __restrict__ status, float scale_log2e)
{
    using K = PastAttCfg<HD>;
    constexpr int KS = HD / 32, DF = HD / 16, CH = HD / 8;      // score k-steps, output fragments, 16-B chunks per key row
    constexpr int NST = K::KT * CH / 256;                       // staging chunks per thread per matrix (2 / 4)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    if (status && *status != 0) return;
    const int P = *past_len;
    if (P < 0 || (long)P + T > cap) return;                     // the append's launch has set the error word: nothing is written
    const int N = P + T;                                        // keys of the sequence: slots [0, N)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, g = lane >> 4;
    const int nqb = (T + K::QB - 1) / K::QB;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int qb = L % nqb, h = (L / nqb) % nh, b = L / (nqb * nh);
    const int hk = h / (nh / nkv);
    const int width = (nh + 2 * nkv) * HD;
    const bf16* qbase = qkv + (size_t)b * T * width + h * HD;
    const bf16* kbase = kcache + ((size_t)b * nkv + hk) * cap * HD;
    const bf16* vbase = vcache + ((size_t)b * nkv + hk) * cap * HD;
    const unsigned char* kv = key_valid ? key_valid + (size_t)b * cap : nullptr;

    int q_idx[K::QW];
    bf16x8 qf[K::QW][KS];
#pragma unroll
    for (int w = 0; w < K::QW; ++w) {
        q_idx[w] = qb * K::QB + (wave * K::QW + w) * 16 + lr;
        const bf16* qr = qbase + (size_t)min(q_idx[w], T - 1) * width;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) qf[w][kk] = *(const bf16x8*)(qr + kk * 32 + g * 8);
    }
    // staging: chunk id c = i * 256 + tid -> key c / CH, 16-B chunk c % CH of the key's HD values
    int skey[NST], sch[NST], kdst[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const int c = i * 256 + tid;
        skey[i] = c / CH;
        sch[i] = c % CH;
        kdst[i] = (sch[i] >> 3) * (K::KT * 128) + skey[i] * 128 + (((sch[i] & 7) ^ ((skey[i] >> 1) & 7)) << 4);
    }

    f32x4 o_acc[K::QW][DF];
    f32x4 l_acc[K::QW];                 // softmax denominators on the matrix cores (a ones fragment as one more V^T fragment)
    float m_run[K::QW];
    bf16x8 ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (bf16)1.0f;
#pragma unroll
    for (int w = 0; w < K::QW; ++w) {
#pragma unroll
        for (int df = 0; df < DF; ++df) o_acc[w][df] = f32x4{0.f, 0.f, 0.f, 0.f};
        l_acc[w] = f32x4{0.f, 0.f, 0.f, 0.f};
        m_run[w] = -1e30f;
    }

    const int kmax = min(N, P + (qb + 1) * K::QB);              // causal: no key beyond this workgroup's last query (at slot P + its index)
    const int ntiles = (kmax + K::KT - 1) / K::KT;
    u32x4 rk[NST], rv[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const size_t ro = (size_t)min(skey[i], N - 1) * HD + sch[i] * 8;
        rk[i] = *(const u32x4*)(kbase + ro);
        rv[i] = *(const u32x4*)(vbase + ro);
    }
    for (int t = 0; t < ntiles; ++t) {
        char* kbuf = lds + (t & 1) * (K::KBYTES + K::VBYTES);
        char* vbuf = kbuf + K::KBYTES;
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            *(u32x4*)(kbuf + kdst[i]) = rk[i];
            const bf16x8 vv = __builtin_bit_cast(bf16x8, rv[i]);
#pragma unroll
            for (int e = 0; e < 8; ++e) *(bf16*)(vbuf + (sch[i] * 8 + e) * K::VSTRIDE + skey[i] * 2) = vv[e];
        }
        __syncthreads();
        if (t + 1 < ntiles) {
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const size_t ro = (size_t)min((t + 1) * K::KT + skey[i], N - 1) * HD + sch[i] * 8;
                rk[i] = *(const u32x4*)(kbase + ro);
                rv[i] = *(const u32x4*)(vbase + ro);
            }
        }
        // validity of the tile's 64 keys as one wave-uniform 64-bit mask (bit = key inside the tile)
        const int kl = t * K::KT + lane;
        const unsigned long long vmask = __ballot(kl < N && (!kv || kv[min(kl, N - 1)] != 0));

        f32x4 s[K::QW][4];
#pragma unroll
        for (int kf = 0; kf < 4; ++kf) {
            const int krow = kf * 16 + lr;
#pragma unroll
            for (int w = 0; w < K::QW; ++w) s[w][kf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int ks = kk * 4 + g;
                const bf16x8 kfr = *(const bf16x8*)(kbuf + (ks >> 3) * (K::KT * 128) + krow * 128 + (((ks & 7) ^ ((krow >> 1) & 7)) << 4));
#pragma unroll
                for (int w = 0; w < K::QW; ++w) s[w][kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[w][kk], s[w][kf], 0, 0, 0);
            }
        }
        // masking only where a tile needs it - an invalid key in it, or keys beyond slot P + the wave's FIRST query (the causal diagonal):
        // a real wave-uniform branch (llm.hip: the asm statement keeps the block from being if-converted)
        const int q_first = P + qb * K::QB + wave * K::QW * 16;
        if (vmask != ~0ull || t * K::KT + K::KT - 1 > q_first) {
            asm volatile("; masked key tile");
#pragma unroll
            for (int w = 0; w < K::QW; ++w)
#pragma unroll
                for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int kin = kf * 16 + g * 4 + r;                    // key inside the tile
                        const bool ok = ((vmask >> kin) & 1ull) && (t * K::KT + kin <= P + q_idx[w]);
                        if (!ok) s[w][kf][r] = -1e30f;
                    }
        }
        bf16x8 pf[K::QW][2];
#pragma unroll
        for (int w = 0; w < K::QW; ++w) {
            float mx = -1e30f;
#pragma unroll
            for (int kf = 0; kf < 4; ++kf)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[w][kf][r]);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m_run[w], mx);
            // a row that has seen no visible key yet keeps m = -1e30; its exponent is taken against 0 instead, so every masked score gives
            // exp2(-huge) = 0 exactly (llm.hip explains the NaN this avoids)
            const float m_ref = m_new <= -1e29f ? 0.f : m_new;
            const float alpha = __builtin_amdgcn_exp2f((m_run[w] <= -1e29f ? -1e30f : m_run[w] - m_ref) * scale_log2e);
            m_run[w] = m_new;
            const float mb = m_ref * scale_log2e;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                f32x8 p;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[w][2 * c][r], scale_log2e, -mb));
                    p[4 + r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[w][2 * c + 1][r], scale_log2e, -mb));
                }
                pf[w][c] = f32_to_bf8(p);
            }
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0) {      // alpha == 1 exactly once the running maximum stops moving
                l_acc[w] *= alpha;
#pragma unroll
                for (int df = 0; df < DF; ++df) o_acc[w][df] *= alpha;
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) l_acc[w] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, pf[w][c], l_acc[w], 0, 0, 0);
        }
#pragma unroll
        for (int df = 0; df < DF; ++df)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const char* vr = vbuf + (df * 16 + lr) * K::VSTRIDE + (c * 32 + g * 4) * 2;
                const bf16x4 lo = *(const bf16x4*)(vr);
                const bf16x4 hi = *(const bf16x4*)(vr + 32);
                const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int w = 0; w < K::QW; ++w) o_acc[w][df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[w][c], o_acc[w][df], 0, 0, 0);
            }
    }

#pragma unroll
    for (int w = 0; w < K::QW; ++w)
        if (q_idx[w] < T) {
            // a query row whose keys are ALL masked has l = 0: it is written as zeros
            const float inv = l_acc[w][0] > 0.f ? 1.0f / l_acc[w][0] : 0.f;
            bf16* orow = out + ((size_t)b * T + q_idx[w]) * ((size_t)nh * HD) + h * HD;
#pragma unroll
            for (int df = 0; df < DF; ++df) *(bf16x4*)(orow + df * 16 + g * 4) = f32_to_bf4(o_acc[w][df] * inv);
        }
}

template <int HD>
static hipError_t launch_attention_past(hipStream_t st, const bf16* qkv, const bf16* kc, const bf16* vc, bf16* out, const unsigned char* key_valid, int B, int T,
                                        int nh, int nkv, int cap, const int* past_len, const int* status)
{
    using K = PastAttCfg<HD>;
    static bool attr_set[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!attr_set[dev & 63]) {
        hipError_t e = hipFuncSetAttribute((const void*)llm_attention_past_kernel<HD>, hipFuncAttributeMaxDynamicSharedMemorySize, K::LDS);
        if (e != hipSuccess) return e;
        attr_set[dev & 63] = true;
    }
    const float scale_log2e = (1.0f / sqrtf((float)HD)) * 1.4426950408889634f;
    const long grid = (long)((T + K::QB - 1) / K::QB) * nh * B;
    if (grid <= 0 || grid > 0x7fffffffl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(llm_attention_past_kernel<HD>, dim3((unsigned)grid), dim3(256), K::LDS, st, qkv, kc, vc, out, key_valid, T, nh, nkv, cap, past_len, status,
                       scale_log2e);
    return hipGetLastError();
}

// qkv [B*T, (nh + 2 nkv) * HD] bf16 (the chunk's packed rows, rope applied; only the q heads are read), kc / vc [>= B][nkv][cap][HD] bf16 with the
// chunk already in slots [*past_len, *past_len + T), key_valid uint8 [>= B][cap] or null -> out [B*T, nh * HD] bf16; status: null or the error word
extern "C" int fvhd_launch_llm_attention_past(hipStream_t st, const void* qkv, const void* kc, const void* vc, const unsigned char* key_valid, void* out, int B,
                                              int T, int nh, int nkv, int HD, int cap, const int* past_len, const int* status)
{
    if (B <= 0 || T <= 0 || nh <= 0 || nkv <= 0 || nh % nkv || cap <= 0 || T > cap || !past_len) return (int)hipErrorInvalidValue;
    if (HD == 64) return (int)launch_attention_past<64>(st, (const bf16*)qkv, (const bf16*)kc, (const bf16*)vc, (bf16*)out, key_valid, B, T, nh, nkv, cap, past_len, status);
    if (HD == 128) return (int)launch_attention_past<128>(st, (const bf16*)qkv, (const bf16*)kc, (const bf16*)vc, (bf16*)out, key_valid, B, T, nh, nkv, cap, past_len, status);
    return (int)hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------------------------
// The chunk's rotated k heads and its v heads -> slots P + t of one layer's caches, one thread per 16-byte piece of a head.  With
// key_valid (the first layer's launch) the mask bytes [P, P + T) of every row are written too: chunk_valid[b][t] != 0, or 1 without one.
// P + T > cap: nothing is written and the sticky error word becomes 1 (and its host-mapped copy, as dec_embed_kernel does).
__global__ __launch_bounds__(256) void llm_cache_append_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ kcache, bf16* __restrict__ vcache,
                                                               unsigned char* __restrict__ key_valid, const unsigned char* __restrict__ chunk_valid, int B, int T,
                                                               int nh, int nkv, int HD, int cap, const int* __restrict__ past_len, int* status, int* status_host)
{
    if (status && *status != 0) return;
    const int P = *past_len;
    if (P < 0 || (long)P + T > cap) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && status) {
            *status = 1;
            if (status_host) *status_host = 1;
        }
        return;
    }
    const int CH = HD / 8;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)B * T * 2 * nkv * CH;
    if (key_valid && idx < (long)B * T) {
        const int b = (int)(idx / T), t = (int)(idx % T);
        key_valid[(size_t)b * cap + P + t] = chunk_valid ? (unsigned char)(chunk_valid[idx] != 0) : (unsigned char)1;
    }
    if (idx >= total) return;
    const int c = (int)(idx % CH);
    const int j = (int)((idx / CH) % (2 * nkv));                 // k heads, then v heads: the order of the packed row behind the q heads
    const long row = idx / ((long)CH * 2 * nkv);
    const int b = (int)(row / T), t = (int)(row % T);
    const bf16* src = qkv + (size_t)row * ((nh + 2 * nkv) * HD) + (size_t)(nh + j) * HD + c * 8;
    bf16* dst = (j < nkv ? kcache : vcache) + (((size_t)b * nkv + (j < nkv ? j : j - nkv)) * cap + P + t) * HD + c * 8;
    *(u32x4*)dst = *(const u32x4*)src;
}

extern "C" int fvhd_launch_llm_cache_append(hipStream_t st, const void* qkv, void* kc, void* vc, unsigned char* key_valid, const unsigned char* chunk_valid, int B,
                                            int T, int nh, int nkv, int HD, int cap, const int* past_len, int* status, int* status_host)
{
    if (B <= 0 || T <= 0 || nh <= 0 || nkv <= 0 || HD <= 0 || HD % 8 || cap <= 0 || T > cap || !past_len) return (int)hipErrorInvalidValue;
    const long total = (long)B * T * 2 * nkv * (HD / 8);         // >= B * T: the mask bytes have their threads
    hipLaunchKernelGGL(llm_cache_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const bf16*)qkv, (bf16*)kc, (bf16*)vc, key_valid,
                       chunk_valid, B, T, nh, nkv, HD, cap, past_len, status, status_host);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// pos[b][t] = next[b] + (valid chunk tokens of row b before t): transformers' cumsum(mask) - 1, continued from the row's next position.
// One thread per row walks its T mask bytes (T is a chunk: tens to hundreds of tokens).
__global__ __launch_bounds__(64) void llm_extend_positions_kernel(const int64_t* __restrict__ next, const unsigned char* __restrict__ chunk_valid,
                                                                  int64_t* __restrict__ pos, int B, int T, const int* status)
{
    if (status && *status != 0) return;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int64_t p = next[b];
    for (int t = 0; t < T; ++t) {
        pos[(size_t)b * T + t] = p;
        if (!chunk_valid || chunk_valid[(size_t)b * T + t]) ++p;
    }
}

extern "C" int fvhd_launch_llm_extend_positions(hipStream_t st, const int64_t* next, const unsigned char* chunk_valid, int64_t* pos, int B, int T, const int* status)
{
    if (B <= 0 || T <= 0 || !next || !pos) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(llm_extend_positions_kernel, dim3((B + 63) / 64), dim3(64), 0, st, next, chunk_valid, pos, B, T, status);
    return (int)hipGetLastError();
}

// after the token is chosen: *len += T, next[b] = pos[b][T - 1] + 1; nothing while the error word is set.  B <= 64: one wave.
__global__ __launch_bounds__(64) void llm_extend_state_kernel(int64_t* __restrict__ next, const int64_t* __restrict__ pos, int B, int T, int* len, const int* status)
{
    if (*status != 0) return;
    const int b = threadIdx.x;
    if (b < B) next[b] = pos[(size_t)b * T + T - 1] + 1;
    if (b == 0) *len += T;
}

extern "C" int fvhd_launch_llm_extend_state(hipStream_t st, int64_t* next, const int64_t* pos, int B, int T, int* len, const int* status)
{
    if (B <= 0 || B > 64 || T <= 0 || !next || !pos || !len || !status) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(llm_extend_state_kernel, dim3(1), dim3(64), 0, st, next, pos, B, T, len, status);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Rewind: for every row the slots [keep[b], *len) leave the sequence - next[b] drops by the VALID ones among them and their mask bytes are
// cleared - then *len = max_b keep[b].  K / V bytes stay: later appends overwrite them.  A keep[b] outside [0, *len] changes nothing and
// sets the error word to 4.  One workgroup: every thread reads *len before thread 0 replaces it (the barrier in between).
__global__ __launch_bounds__(256) void llm_cache_rewind_kernel(const int* __restrict__ keep, int rows, unsigned char* __restrict__ key_valid, int64_t* __restrict__ next,
                                                               int cap, int* len, int* status, int* status_host)
{
    __shared__ int bad, kmax, dropped;
    if (*status != 0) return;
    const int L = *len;
    if (threadIdx.x == 0) { bad = 0; kmax = 0; }
    __syncthreads();
    for (int b = threadIdx.x; b < rows; b += 256) {
        const int k = keep[b];
        if (k < 0 || k > L) atomicOr(&bad, 1);
        else atomicMax(&kmax, k);
    }
    __syncthreads();
    if (bad || L > cap) {
        if (threadIdx.x == 0) {
            *status = 4;
            if (status_host) *status_host = 4;
        }
        return;
    }
    for (int b = 0; b < rows; ++b) {
        if (threadIdx.x == 0) dropped = 0;
        __syncthreads();
        unsigned char* m = key_valid + (size_t)b * cap;
        int n = 0;
        for (int j = keep[b] + threadIdx.x; j < L; j += 256) {
            n += m[j] != 0;
            m[j] = 0;
        }
        if (n) atomicAdd(&dropped, n);
        __syncthreads();
        if (threadIdx.x == 0) next[b] -= dropped;
        __syncthreads();
    }
    if (threadIdx.x == 0) *len = kmax;
}

extern "C" int fvhd_launch_llm_cache_rewind(hipStream_t st, const int* keep, int rows, unsigned char* key_valid, int64_t* next, int cap, int* len, int* status,
                                            int* status_host)
{
    if (rows <= 0 || cap <= 0 || !keep || !key_valid || !next || !len || !status) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(llm_cache_rewind_kernel, dim3(1), dim3(256), 0, st, keep, rows, key_valid, next, cap, len, status, status_host);
    return (int)hipGetLastError();
}
