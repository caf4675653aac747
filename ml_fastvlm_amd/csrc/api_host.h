// Host-side helpers shared by the C-ABI sources (fvhd_api.hip and the llm_*.hip files).  Hidden visibility: none of them is an exported symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#pragma GCC visibility push(hidden)

inline uint16_t f32_to_bf16_rne(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// Every entry point that takes a context runs with the CONTEXT's device current and restores the caller's on exit: a tower on
// cuda:1 must neither allocate its arena on cuda:0 nor leave cuda:1 current for the caller's next torch allocation.
struct DeviceGuard {
    int prev = -1; bool switched = false; hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) { err = hipGetDevice(&prev); if (err == hipSuccess && prev != dev) { err = hipSetDevice(dev); switched = err == hipSuccess; } }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// bump allocation of 256-byte aligned pieces: take() returns the piece's offset, `off` ends as the arena's size
struct Arena {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off += align256(bytes); return o; }
};

// is `st` being captured into a graph?  `if_unknown` is the answer when the query itself fails: the callers that would only lose an
// optimisation by assuming a capture pass true, the ones that would refuse the call pass false - each site keeps the meaning it had
inline bool is_capturing(hipStream_t st, bool if_unknown = false)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess ? cs != hipStreamCaptureStatusNone : if_unknown;
}

#pragma GCC visibility pop
