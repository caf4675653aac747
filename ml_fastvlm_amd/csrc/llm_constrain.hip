// Constrained decoding inside the decode step: a token-level automaton bans, per row, every id its state does not allow, in place on
// the fp32 logits [B][V] between the lm_head and the choice (include/fvhd.h "LLM constrained decoding").
//
// The automaton is CSR data on the device: state s owns the edges offsets[s] .. offsets[s + 1], tokens[e] (ascending inside a state) is
// an allowed id, targets[e] the next state or -1 = FREE (unconstrained from then on).  Per row the step keeps one int32 state and one
// flag word.  This is transformers' PrefixConstrainedLogitsProcessor with the callback replaced by the tables.  Its place in
// `_get_logits_processor` is behind repetition penalty, n-gram and min-new-tokens and in front of suppress; every one of those but the
// penalty is a ban, bans commute, and -inf survives the penalty (-inf * p = -inf / p = -inf for p > 0), so ONE launch behind the
// processors' launch (llm_logits.hip) gives the same values.
//
// Two launches, so that no workgroup can read a state another has replaced:
//   advance  one workgroup, thread b = row b: the fed token (tok[b], else last[b]: the ids dec_embed embeds) is looked up in the sorted
//            edges of the row's state by binary search.  Found: the edge's target.  Not found: FREE and flag bit 0 (only ids the caller
//            fed itself can do that).  FREE stays FREE.  With `reset` the row takes its start state instead and the flags are cleared.
//   mask     grid = slices x rows, 256 threads; a slice is DEC_CON_SLICE consecutive ids.  The states are read-only here.  A workgroup
//            finds its slice's edge range with one wave-uniform binary search per border, its lanes set the allowed ids' bits in an LDS
//            bitmap (integer LDS atomics), and after the barrier every lane stores -inf over the banned ids: 16 bytes per lane where all
//            four ids of a 16-byte-aligned group are banned (1 KiB per wave instruction), single floats at group, row and slice edges
//            (a row of an odd V is not 16-byte aligned: the groups are aligned in MEMORY, not in id space).
// Allowed entries are neither read nor written: they keep the lm_head's (or the processors') bits, -0.0 included.  Every banned logit is
// written by exactly one lane and the value is a constant; the new state depends on the old state and the fed id only: eager and
// replayed runs give the same bits.  A FREE row is not touched.  The launch writes at most 4 V bytes per constrained row and reads only
// the edges of the rows' current states; the logits are not read at all.
#include "fvhd_common.h"
#include "launchers.h"      // (with llm_decode.h: DecConstrainArgs)

namespace {

constexpr int CON_WORDS = DEC_CON_SLICE / 32;

// the first edge in [lo, hi) whose token is >= id (hi: none)
FVHD_DEV int lower_edge(const int* __restrict__ tokens, int lo, int hi, int id)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tokens[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(64) void dec_constrain_advance_kernel(const DecConstrainArgs a)
{
    if (a.status && *a.status) return;
    const int b = threadIdx.x;
    if (b >= a.B) return;
    if (a.reset) {
        const int s = a.start[a.n_start == 1 ? 0 : b];
        a.states[b] = s >= 0 && s < a.n_states ? s : -1;
        a.flags[b] = 0;
        return;
    }
    const int s = a.states[b];
    if (s < 0 || s >= a.n_states) return;                        // FREE stays FREE
    const long id = a.tok ? a.tok[b] : a.last[b];
    const int e0 = a.offsets[s], e1 = a.offsets[s + 1];
    if (id >= 0 && id < a.V) {
        const int e = lower_edge(a.tokens, e0, e1, (int)id);
        if (e < e1 && a.tokens[e] == (int)id) {
            const int next = a.targets[e];
            a.states[b] = next >= 0 && next < a.n_states ? next : -1;
            return;
        }
    }
    a.states[b] = -1;                                            // an id the state does not list: unconstrained from here, and say so
    a.flags[b] |= 1;
}

__global__ __launch_bounds__(256) void dec_constrain_mask_kernel(const DecConstrainArgs a)
{
    if (a.status && *a.status) return;
    __shared__ unsigned bits[CON_WORDS + 1];                     // (+1: the nibble of a group may be fetched across the last word)
    const int tid = threadIdx.x, b = blockIdx.y, V = a.V;
    const int s = a.states[b];
    if (s < 0 || s >= a.n_states) return;                        // FREE: the row is not touched
    const int lo = blockIdx.x * DEC_CON_SLICE, hi = min(lo + DEC_CON_SLICE, V);
    if (tid <= CON_WORDS) bits[tid] = 0;
    // the slice's edges: tokens in [lo, hi) - every lane runs the same search on the same addresses
    const int e0 = a.offsets[s], e1 = a.offsets[s + 1];
    const int f0 = lower_edge(a.tokens, e0, e1, lo), f1 = lower_edge(a.tokens, f0, e1, hi);
    __syncthreads();
    for (int e = f0 + tid; e < f1; e += 256) {
        const unsigned i = (unsigned)(a.tokens[e] - lo);
        if (i < (unsigned)DEC_CON_SLICE) atomicOr(&bits[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
    float* x = a.logits + (size_t)b * V;                         // ids lo .. hi - 1 of the row are x[lo .. hi)
    const float ninf = -INFINITY;
    // the first id of the slice whose address is 16-byte aligned
    const int head = min((int)((4u - (unsigned)(((uintptr_t)(x + lo) >> 2) & 3)) & 3u), hi - lo);
    const int groups = (hi - lo - head) >> 2, tail = lo + head + 4 * groups;
    if (tid < head && !((bits[tid >> 5] >> (tid & 31)) & 1u)) x[lo + tid] = ninf;
    for (int g = tid; g < groups; g += 256) {
        const int i = head + 4 * g;                              // slice-relative id of the group's first element
        const unsigned long long w = (unsigned long long)bits[i >> 5] | ((unsigned long long)bits[(i >> 5) + 1] << 32);
        const unsigned nib = (unsigned)(w >> (i & 31)) & 15u;
        float* p = x + lo + i;
        if (nib == 0) {
            *reinterpret_cast<float4*>(p) = make_float4(ninf, ninf, ninf, ninf);
        } else if (nib != 15u) {
            // a group at the border of a run: rare.  Not unrolled - unrolled, the compiler merges the fourth store with the 16-byte one's
            // last component and splits that store into 12 + 4 bytes
#pragma unroll 1
            for (int j = 0; j < 4; ++j)
                if (!((nib >> j) & 1u)) p[j] = ninf;
        }
    }
    const int t = tail + tid;
    if (tid < 3 && t < hi) {
        const int i = t - lo;
        if (!((bits[i >> 5] >> (i & 31)) & 1u)) x[t] = ninf;
    }
}

// ---------------------------------------------------------------------------------------------------
extern "C" int fvhd_dec_constrain_slice(void) { return DEC_CON_SLICE; }

extern "C" int fvhd_launch_dec_constrain(hipStream_t st, const DecConstrainArgs* a)
{
    if (!a->logits || !a->offsets || !a->tokens || !a->targets || !a->states || !a->flags || a->B < 1 || a->B > 64 || a->V < 1 || a->n_states < 1 ||
        ((uintptr_t)a->logits & 3) || (a->reset && a->n_start != 1 && a->n_start < a->B))
        return (int)hipErrorInvalidValue;
    if (a->reset || a->tok || a->last) {
        hipLaunchKernelGGL(dec_constrain_advance_kernel, dim3(1), dim3(64), 0, st, *a);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    const int S = (a->V + DEC_CON_SLICE - 1) / DEC_CON_SLICE;
    hipLaunchKernelGGL(dec_constrain_mask_kernel, dim3((unsigned)S, (unsigned)a->B), dim3(256), 0, st, *a);
    return (int)hipGetLastError();
}
