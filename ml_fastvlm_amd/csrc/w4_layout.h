// The packed MXFP4 row layout of the decode's 4-bit weights (llm_w4.hip, include/fvhd.h "LLM 4-bit weights"), for every kernel that reads a
// packed row.  A row of K elements is K / 2 code bytes; inside every 128-deep chunk (64 bytes) the 8 codes of MFMA step j (0..3) and lane
// group g (0..3) - k = 32 j + 8 g .. + 7 - are the dword at byte 16 g + 4 j, element i of them in nibble i (even elements low), so that lane
// (lr, g) reads its operands of all four MFMA steps with ONE 16-byte load and a wave's load covers 64 contiguous bytes of 16 rows.  The
// block scales are not reordered: u8 [K / 32] per row, byte k / 32 = E standing for 2^(E - 127); a chunk's four scales are one dword.
#pragma once
#include "fvhd_common.h"

// byte offset, in a packed row, of the dword holding the 8 codes k0 .. k0 + 7 (k0 % 8 == 0)
FVHD_DEV int w4_pos(int k0)
{
    const int j = (k0 >> 5) & 3, g = (k0 >> 3) & 3;
    return ((k0 >> 7) << 6) + (g << 4) + (j << 2);
}

// the fp32 whose bits are E << 23: 2^(E - 127), the scale operand of v_cvt_scalef32_pk_bf16_fp4
FVHD_DEV float w4_scale(unsigned E) { return __builtin_bit_cast(float, (E & 0xffu) << 23); }

// 8 e2m1 codes (one dword, element i in nibble i) times a power-of-two scale -> the bf16 MFMA fragment; every product is exactly a bf16
// value (a code has 2 significant bits), so nothing is rounded
FVHD_DEV bf16x8 fp4x8_to_bf8(uint32_t q, float scale)
{
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3);
    return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
