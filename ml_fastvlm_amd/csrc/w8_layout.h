// The packed e4m3 row layout of the decode's 8-bit weights (llm_w8.hip, include/fvhd.h "LLM 8-bit weights"), for every kernel that reads a
// packed row: inside every 128-deep chunk the 8 codes of MFMA step j (0..3) and lane group g (0..3) - k = 32 j + 8 g .. + 7 - sit at
// byte 64 (j / 2) + 16 g + 8 (j % 2).
#pragma once
#include "fvhd_common.h"

// byte offset, in a packed row, of the 8 codes k0 .. k0 + 7 (k0 % 8 == 0)
FVHD_DEV int w8_pos(int k0)
{
    const int j = (k0 >> 5) & 3, g = (k0 >> 3) & 3;
    return (k0 & ~127) + ((j >> 1) << 6) + (g << 4) + ((j & 1) << 3);
}

FVHD_DEV f32x8 e4m3x8_to_f32(uint32_t lo, uint32_t hi)
{
    const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(lo, true);
    const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8(hi, true);
    return f32x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
