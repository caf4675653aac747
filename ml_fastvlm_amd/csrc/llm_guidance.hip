// Classifier-free guidance over the fp32 logits [2 G][V] of the lm_head (include/fvhd.h "LLM classifier-free guidance"): row g is the
// conditional sequence of prompt g, row G + g its unconditional one (transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor):
//
//     lc = log_softmax(x[g])    lu = log_softmax(x[G + g])    guided[v] = s * (lc[v] - lu[v]) + lu[v]     -> written over row g
//
// The logits are FINITE: guidance is the first edit of the step, in front of every launch that writes -inf (processors, constraint).  Rows
// G .. 2 G - 1 are read only and keep their bits.
//
// TWO launches (the second needs every slice of the first, so they cannot be one):
//   1  row statistics, grid = S slices x 2 G rows, 256 threads - the scheme of llm_logprobs.hip: S = min(64, ceil(V / 2048)), slice s owns
//      the indices [s L, s L + L), L = ceil(V / S), thread t of it the indices s L + t + 256 j (4-byte loads: rows of a V that is no
//      multiple of 4 are not 16-byte aligned).  m = the slice maximum (exact); sum exp(x - m): a thread adds its elements in index order,
//      the 256 thread sums meet in a butterfly over the wave and (r0 + r1) + (r2 + r3) over the four waves.  (m, sum) go to the scratch and
//      the row's last-arriving workgroup (a counter per row, which it leaves at zero) merges them in one wave: M = max m_s,
//      Z = sum_s sum_s * exp(m_s - M) in a butterfly over the slices, and stores (M, log Z).  No floating-point atomics, a fixed order of
//      additions: the same inputs give the same bits, eager or replayed.
//   2  apply, grid = ceil(V / 2048) slices x G pairs, 256 threads.  In this order, every operation rounded once to fp32 and none contracted:
//          lc = (xc - Mc) - log Zc      lu = (xu - Mu) - log Zu      d = lc - lu      p = s * d      guided = p + lu
//      (identical rows: d = 0, p = +-0, guided = lu = lc bit for bit).  A pair whose two rows are both 16-byte aligned (every pair when
//      V % 4 == 0) moves 16 bytes per load and store over the multiple-of-4 part of a slice, with a scalar tail of at most 3 elements in the
//      row's last slice; a pair with a misaligned row (V % 4 != 0) takes the scalar path for the whole slice.
// Behind the choice ONE small launch (`dec_guidance_mirror_kernel`) copies the chosen id of row g to row G + g - both rows are fed the
// same token - and, in a decode step, advances the positions of rows G .. 2 G - 1, which the choice's launch (run on G rows) left alone.
#include "fvhd_common.h"
#include "launchers.h"
#include "split_handoff.h"  // publish, arrive_last_published

namespace {

constexpr int GD_SMAX = 64;                      // slices per row (one wave merges them)
constexpr int GD_RMAX = 64;                      // rows per launch = 2 * 32 pairs: their arrival counters are the head of the scratch
constexpr int GD_CNT_STRIDE = 64;                // ints between two rows' counters: a 256-byte line each (llm_logprobs.hip)
constexpr int GD_SLICE = 2048;                   // a row shorter than GD_SMAX slices of this many elements gets fewer slices; the apply's slice

struct GdWs {
    int* cnt;                                    // [GD_RMAX] arrival counters, one per GD_CNT_STRIDE ints (zero between launches)
    float* pm;                                   // [2 G][S] slice maximum
    float* ps;                                   // [2 G][S] sum of exp(x - slice maximum)
    float* stat;                                 // [2 G][2] the row's (M, log Z)
};

size_t al256g(size_t x) { return (x + 255) & ~(size_t)255; }

int slices_of(int V) { return V >= GD_SMAX * GD_SLICE ? GD_SMAX : (V + GD_SLICE - 1) / GD_SLICE; }

GdWs carve(void* base, int rows, int S)
{
    char* p = (char*)base;
    GdWs w;
    w.cnt = (int*)p;
    p += al256g(4 * GD_RMAX * GD_CNT_STRIDE);
    w.pm = (float*)p;
    p += al256g((size_t)4 * rows * S);
    w.ps = (float*)p;
    p += al256g((size_t)4 * rows * S);
    w.stat = (float*)p;
    return w;
}

// the apply's arithmetic: five subtractions / one product / one addition, each rounded once (no fused multiply-add)
FVHD_DEV float guide(float c, float u, float Mc, float Lc, float Mu, float Lu, float s)
{
    const float lc = __fsub_rn(__fsub_rn(c, Mc), Lc);
    const float lu = __fsub_rn(__fsub_rn(u, Mu), Lu);
    const float d = __fsub_rn(lc, lu);
    return __fadd_rn(__fmul_rn(s, d), lu);
}

}  // namespace

__global__ __launch_bounds__(256) void dec_guidance_stats_kernel(const float* __restrict__ logits, int V, const GdWs w, const int* status)
{
    if (status && *status) return;
    __shared__ float redm[4], reds[4];
    __shared__ int flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const float* x = logits + (size_t)b * V;
    const int L = (V + S - 1) / S;
    const int i0 = min(s * L, V), i1 = min(i0 + L, V);
    float m = -INFINITY;
    for (int i = i0 + tid; i < i1; i += 256) m = fmaxf(m, x[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) redm[wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
    float acc = 0.f;
    if (m > -INFINITY)                                            // (an empty slice: 0, never exp(-inf - -inf))
        for (int i = i0 + tid; i < i1; i += 256) acc += expf(x[i] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) reds[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        publish(w.pm + b * S + s, m);
        publish(w.ps + b * S + s, (reds[0] + reds[1]) + (reds[2] + reds[3]));
    }
    if (!arrive_last_published(w.cnt + b * GD_CNT_STRIDE, S, &flag)) return;
    // ---- the row's last workgroup: merge the slices in one wave ----
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
            w.stat[2 * b] = M;
            w.stat[2 * b + 1] = logf(z);
        }
    }
}

__global__ __launch_bounds__(256) void dec_guidance_apply_kernel(float* logits, int G, int V, float scale, const float* __restrict__ stat,
                                                                 const int* status)
{
    if (status && *status) return;
    const int tid = threadIdx.x, g = blockIdx.y;
    float* xc = logits + (size_t)g * V;
    const float* xu = logits + (size_t)(G + g) * V;
    const float Mc = stat[2 * g], Lc = stat[2 * g + 1], Mu = stat[2 * (G + g)], Lu = stat[2 * (G + g) + 1];
    const int i0 = blockIdx.x * GD_SLICE, i1 = min(i0 + GD_SLICE, V);      // i0 is a multiple of 4: the slice is aligned as its row is
    int i = i0 + tid;
    if ((((uintptr_t)xc | (uintptr_t)xu) & 15) == 0) {
        const int n4 = (i1 - i0) / 4;
        const float4* c4 = (const float4*)(xc + i0);
        const float4* u4 = (const float4*)(xu + i0);
        for (int q = tid; q < n4; q += 256) {
            const float4 c = c4[q], u = u4[q];
            float4 r;
            r.x = guide(c.x, u.x, Mc, Lc, Mu, Lu, scale);
            r.y = guide(c.y, u.y, Mc, Lc, Mu, Lu, scale);
            r.z = guide(c.z, u.z, Mc, Lc, Mu, Lu, scale);
            r.w = guide(c.w, u.w, Mc, Lc, Mu, Lu, scale);
            ((float4*)(xc + i0))[q] = r;
        }
        i = i0 + 4 * n4 + tid;                                    // the tail: at most 3 elements, in the row's last slice
    }
    for (; i < i1; i += 256) xc[i] = guide(xc[i], xu[i], Mc, Lc, Mu, Lu, scale);
}

// behind the choice: row G + g takes the id row g chose; decode steps (posv given) advance the positions of the unconditional rows
__global__ __launch_bounds__(64) void dec_guidance_mirror_kernel(int G, int64_t* last, int64_t* ids_out, int64_t* posv, const int* status)
{
    if (status && *status) return;
    const int g = threadIdx.x;
    if (g >= G) return;
    if (last) last[G + g] = last[g];
    if (ids_out) ids_out[G + g] = ids_out[g];
    if (posv) posv[G + g] += 1;
}

// ---------------------------------------------------------------------------------------------------
extern "C" size_t fvhd_dec_guidance_scratch_bytes(int G, int V)
{
    if (G < 1 || 2 * G > GD_RMAX || V < 1) return 0;
    const int S = slices_of(V);
    return al256g(4 * GD_RMAX * GD_CNT_STRIDE) + 2 * al256g((size_t)4 * 2 * G * S) + al256g((size_t)4 * 2 * 2 * G);
}

extern "C" int fvhd_launch_dec_guidance(hipStream_t st, float* logits, int G, int V, float scale, void* scratch, const int* status)
{
    if (!logits || !scratch || G < 1 || 2 * G > GD_RMAX || V < 1 || ((uintptr_t)logits & 3)) return (int)hipErrorInvalidValue;
    const int S = slices_of(V);
    const GdWs w = carve(scratch, 2 * G, S);
    hipLaunchKernelGGL(dec_guidance_stats_kernel, dim3((unsigned)S, (unsigned)(2 * G)), dim3(256), 0, st, logits, V, w, status);
    hipLaunchKernelGGL(dec_guidance_apply_kernel, dim3((unsigned)((V + GD_SLICE - 1) / GD_SLICE), (unsigned)G), dim3(256), 0, st, logits, G, V, scale,
                       w.stat, status);
    return (int)hipGetLastError();
}

extern "C" int fvhd_launch_dec_guidance_mirror(hipStream_t st, int G, int64_t* last, int64_t* ids_out, int64_t* posv, const int* status)
{
    if (G < 1 || 2 * G > GD_RMAX) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(dec_guidance_mirror_kernel, dim3(1), dim3(64), 0, st, G, last, ids_out, posv, status);
    return (int)hipGetLastError();
}
