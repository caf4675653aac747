// The in-launch hand-off of a split reduction (cdna_hip_programming.md §5, "In-launch split-K reduction"): the workgroups that share a
// reduction each leave a partial result in global memory and add to one counter; the workgroup that arrives last reads every partial and
// finishes the reduction in the same launch - deterministic (it sums in slice order), no float atomics, no second launch.  Two protocols,
// which differ in the producer side only; each kernel uses one of them and states nothing of it again.
//
// Common to both: `c` is the reduction's arrival counter, zero before the launch; `n` the number of workgroups that share it; `flag` one
// int of the workgroup's LDS.  EVERY wave of the workgroup must reach the call (it holds __syncthreads()), with the same `c` and `n`.
// The result is the same in every thread: true in exactly one of the n workgroups, the one whose add found n - 1.  That workgroup has
// put the counter back to zero (nobody else touches it any more), so a launch always finds it zero, and it stands behind an agent-scope
// acquire: it may read what every other workgroup stored before its own call, with plain loads.
#pragma once
#include "fvhd_common.h"

// arrive_last: for partials written with PLAIN stores by any thread of the workgroup (the slabs of the decode GEMMs and of the attention
// kernels, the sampler's histograms).  Before the call: every thread has issued its stores.  The call waits for them (vmcnt), meets in a
// barrier, and thread 0 releases them at agent scope - an L2 write-back, which is what makes plain stores of one XCD visible to
// another - before it adds to the counter.
static __device__ bool arrive_last(int* c, int n, int* flag)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == n - 1;
        if (last) {
            __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}

// publish + arrive_last_published: the lighter producer side, for a partial of a few words that THREAD 0 ALONE writes (llm_logprobs.hip,
// llm_guidance.hip).  Thread 0 stores each word with publish() - a write-through, agent-scope relaxed atomic store - and the call waits
// until they have left (vmcnt) before it adds to the counter: no release fence.  That fence is an L2 write-back per workgroup; those
// serialise within an XCD, and at 64 rows x 64 slices they were most of the launch (87 us against 25).  What any other thread
// stored, or thread 0 stored plainly, is NOT handed over.  There is no barrier in front of the add, only behind it.
template <typename T>
FVHD_DEV void publish(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

static __device__ bool arrive_last_published(int* c, int n, int* flag)
{
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int t = __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = t == n - 1;
        if (last) {
            __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *flag = last;
    }
    __syncthreads();
    return *flag != 0;
}
