// What the sampler (llm_sample.hip) and beam-search sampling (llm_beam.hip) share on the device: the temperature division, the Philox4x32-10
// generator and the Gumbel variate of one of its words.
#pragma once
#include "fvhd_common.h"

FVHD_DEV float scaled(float x, float T) { return __fdiv_rn(x, T); }     // TemperatureLogitsWarper: scores / temperature, IEEE

struct Philox4 { unsigned w[4]; };

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> the four output words
FVHD_DEV Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// ... -> the first output word (the sampler's u)
FVHD_DEV unsigned philox_x0(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
    return philox4x32_10(c0, c1, c2, c3, k0, k1).w[0];
}

// Gumbel(0, 1) from one Philox word: u = (2 (w >> 9) + 1) 2^-24, an exact fp32 value in (0, 1), g = -log(-log u).  t = -log u is taken through
// log1p above 1/2 (u - 1 is exact there): log(u) itself loses relative accuracy as u -> 1, where t -> 2^-24 and g is largest.
FVHD_DEV float gumbel_of_word(unsigned w)
{
    const float u = (float)(2u * (w >> 9) + 1u) * 0x1p-24f;
    const float t = u > 0.5f ? -log1pf(u - 1.0f) : -logf(u);
    return -logf(t);
}
