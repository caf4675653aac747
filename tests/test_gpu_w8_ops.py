"""The single ops of the 8-bit weight path (csrc/llm_w8.hip, include/fvhd.h version 504) on the GPU.

  quantise      codes and scales equal `ml_fastvlm_amd.quantize_rows_e4m3` (plain torch on the CPU) bit for bit
  bit equality  with every scale = 1 fvhd_op_dec_gemm_w8 has the bits of fvhd_op_dec_gemm on codes.to(bfloat16): the conversion is exact and
                the arithmetic is the bf16 kernel's; with power-of-two scales and a zero residual the output is that output times the scale
  tolerance     the three ops against tests/decode_reference.py on W = codes.double() * scale: the weights are exact and the arithmetic is
                the bf16 ops', so the bounds are theirs (tests/test_gpu_decode.py: rel-L2 1e-2)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as R  # noqa: E402
from llm_testlib import (GEMM_SHAPES, rel,  # noqa: E402
                         dec_gemm as _gemm_bf16, gemm_scratch as _scratch, lowest_argmax as _lowest_argmax, nb as _nb, ptr as _p, stream as _st)

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 8, 16, 17, 33, 64)


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import _lib
    return _lib.w8_lib()


# ---- 1. the quantiser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 128), (13, 896), (33, 4864), (5, 18944), (16, 8), (7, 2056), (300, 3584)])
def test_quantize_op_equals_the_torch_recipe(lib, N, K):
    from ml_fastvlm_amd import _lib, quantize_rows_e4m3
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    w[0] *= torch.exp2(torch.randint(-24, 12, (K,), generator=g).float())        # a row spanning many binades
    if N > 4:
        w[1] = 0                                                                  # a zero row
        w[2] = w[2].clamp(-1, 1)
        w[2, K // 2] = 1.75                                                       # amax / scale = 448 exactly
        w[3] = w[3].clamp(-1, 1)
        w[3, 0] = -1.7578125                                                      # one bf16 ulp above: the scale doubles
        w[4] *= 1e-30
    w = w.to(torch.bfloat16)
    want_codes, want_scale = quantize_rows_e4m3(w)
    wd = w.cuda()
    codes = torch.full((N * K + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    scale = torch.full((N + 8,), -3.0, device="cuda")
    _lib.check(lib.fvhd_op_quantize_e4m3(_st(), _p(wd), N, K, _p(codes), _p(scale)), "quantize")
    torch.cuda.synchronize()
    assert bool((codes[N * K:] == 0x5A).all()) and bool((scale[N:] == -3.0).all()), "guard written"
    assert torch.equal(scale[:N].cpu(), want_scale)
    assert torch.equal(codes[:N * K].view(N, K).cpu(), want_codes.view(torch.uint8))


# ---- 2. bit equality with the bf16 op ------------------------------------------------------------------------------------------------------
def _random_codes(N, K, g):
    """e4m3 codes of N(0, 1) values: every binade of the format, both signs, denormals and zeros"""
    return torch.randn(N, K, device="cuda", generator=g).to(torch.float8_e4m3fn)


def _gemm_w8(lib, epi, x, nw, codes, scale, resid, splits):
    """-> (out, counters left zero)"""
    from ml_fastvlm_amd import _lib
    B, K = x.shape
    N = codes.shape[0]
    out = torch.empty(B, N // 2 if epi == "swiglu" else N, device="cuda", dtype=torch.bfloat16)
    part, cnt = _scratch(N, B, splits)
    _lib.check(lib.fvhd_op_dec_gemm_w8(_st(), _lib.EPI_SWIGLU if epi == "swiglu" else _lib.EPI_RESID, _p(x), B, _p(nw), 1e-6, _p(codes), _p(scale), N, K,
                                       _p(resid), _p(out), _p(part), _p(cnt), splits), "dec_gemm_w8")
    torch.cuda.synchronize()
    return out, cnt is None or int(cnt.abs().sum()) == 0


@pytest.mark.parametrize("N,K", GEMM_SHAPES)
def test_dec_gemm_w8_has_the_bits_of_the_bf16_op(lib, N, K):
    g = torch.Generator(device="cuda").manual_seed(N + K)
    codes = _random_codes(N, K, g)
    W = codes.to(torch.bfloat16)
    assert torch.equal(W.float(), codes.float())                  # every e4m3 value is a bf16 value
    ones = torch.ones(N, device="cuda")
    scale = torch.exp2(torch.randint(-12, -1, (N,), device="cuda", generator=g).float())
    nw = (1 + 0.3 * torch.randn(K, device="cuda", generator=g)).float()
    for B in BATCHES:
        x = (torch.randn(B, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        resid = torch.randn(B, N, device="cuda", generator=g).to(torch.bfloat16)
        zero = torch.zeros_like(resid)
        for norm in (nw, None):
            for splits in (1, 16):
                what = f"N={N} K={K} B={B} norm={norm is not None} splits={splits}"
                for epi in ("resid", "swiglu"):
                    want = _gemm_bf16(lib, epi, x, norm, W, resid, splits)
                    got, zeroed = _gemm_w8(lib, epi, x, norm, codes, ones, resid, splits)
                    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (epi, what, int((got != want).sum()))
                    assert zeroed, "counters not back at zero: " + what
                # power-of-two scales, zero residual: the bf16 op's output times the scale, exactly
                base = _gemm_bf16(lib, "resid", x, norm, W, zero, splits)
                got, _ = _gemm_w8(lib, "resid", x, norm, codes, scale, zero, splits)
                want = (base.float() * scale[None, :]).to(torch.bfloat16)
                assert torch.equal(want.float(), base.float() * scale[None, :])           # (no bf16 underflow in this test's range)
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), ("scaled", what, int((got != want).sum()))


# ---- 3. the three ops against the fp64 reference on W = codes * scale ---------------------------------------------------------------------
def _quantised(N, K, g):
    """a weight matrix as the library would hold it -> (codes e4m3 [N, K], power-of-two scales [N], W = codes * scale in fp64)"""
    from ml_fastvlm_amd import quantize_rows_e4m3
    w = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5 * torch.exp2(torch.randint(-3, 4, (N, 1), device="cuda", generator=g).float())).to(torch.bfloat16)
    codes, scale = quantize_rows_e4m3(w)
    return codes, scale, codes.double() * scale.double()[:, None]


@pytest.mark.parametrize("N,K,swiglu", [(896, 4864, False), (9728, 896, True), (1536, 8960, False), (3584, 18944, False), (37888, 3584, True), (896, 896, False)])
def test_dec_gemm_w8_against_the_reference(lib, N, K, swiglu):
    g = torch.Generator(device="cuda").manual_seed(N + K + 1)
    codes, scale, Wd = _quantised(N, K, g)
    epi = "swiglu" if swiglu else "resid"
    nw = (1 + 0.1 * torch.randn(K, device="cuda", generator=g)).float() if swiglu else None
    worst = 0.0
    for B in BATCHES:
        x = torch.randn(B, K, device="cuda", generator=g).to(torch.bfloat16)
        resid = torch.randn(B, N, device="cuda", generator=g).to(torch.bfloat16)
        want = R.dec_gemm_ref(x, nw, 1e-6, Wd, resid, epi)
        for splits in (1, 16):
            got, zeroed = _gemm_w8(lib, epi, x, nw, codes, scale, resid, splits)
            again, _ = _gemm_w8(lib, epi, x, nw, codes, scale, resid, splits)
            err = rel(got, want)
            worst = max(worst, err)
            assert err <= 1e-2, (B, splits, err)
            assert torch.equal(got.view(torch.int16), again.view(torch.int16)) and zeroed, (B, splits)
    print(f"dec_gemm_w8 N={N} K={K} {epi}: worst rel-L2 {worst:.2e}")


@pytest.mark.parametrize("nh,nkv,hd,H", [(14, 2, 64, 896), (12, 2, 128, 1536), (28, 4, 128, 3584)])
@pytest.mark.parametrize("B", [1, 3, 16, 40])
def test_dec_qkv_w8_against_the_reference(lib, nh, nkv, hd, H, B):
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    g = torch.Generator(device="cuda").manual_seed(hd + B + H)
    N, cap, slot, P = (nh + 2 * nkv) * hd, 40, 17, 8192
    codes, scale, Wd = _quantised(N, H, g)
    x = torch.randn(B, H, device="cuda", generator=g).to(torch.bfloat16)
    bias = 0.1 * torch.randn(N, device="cuda", generator=g)
    nw = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).float()
    pos = torch.arange(B, device="cuda", dtype=torch.long) * 421 + 5
    pos[-1] = 9000 if B > 1 else 5                                  # 9000: beyond the table
    table = rope_table(P, hd, 1e6, "cuda")
    qw, kw, vw = R.dec_qkv_ref(x, nw, 1e-6, Wd, bias, pos, nh, nkv, hd, 1e6)
    length = torch.tensor([slot], device="cuda", dtype=torch.int32)
    runs = []
    for splits in (1, 4, 4):
        kc = torch.zeros(B, nkv, cap, hd, device="cuda", dtype=torch.bfloat16)
        vc = torch.zeros_like(kc)
        q = torch.empty(B, nh * hd, device="cuda", dtype=torch.bfloat16)
        part, cnt = _scratch(N, B, splits)
        _lib.check(lib.fvhd_op_dec_qkv_w8(_st(), _p(x), B, H, _p(nw), 1e-6, _p(codes), _p(scale), _p(bias), _p(q), _p(pos), _p(table), P, 1e6, _p(kc), _p(vc),
                                          cap, _p(length), nh, nkv, hd, _p(part), _p(cnt), splits), "dec_qkv_w8")
        torch.cuda.synchronize()
        assert rel(q.view(B, nh, hd), qw) <= 1e-2 and rel(kc[:, :, slot], kw) <= 1e-2 and rel(vc[:, :, slot], vw) <= 1e-2, splits
        others = torch.ones(cap, dtype=torch.bool)
        others[slot] = False
        assert kc[:, :, others].abs().sum() == 0 and vc[:, :, others].abs().sum() == 0
        assert cnt is None or int(cnt.abs().sum()) == 0
        runs.append((q, kc, vc))
    assert all(torch.equal(a, b) for a, b in zip(runs[1], runs[2]))               # two launches: identical bits


def _lm_w8(lib, x, nw, codes, scale, logits=True):
    from ml_fastvlm_amd import _lib
    B, H = x.shape
    V = codes.shape[0]
    nb = _nb(B)
    lg = torch.empty(B, V, device="cuda") if logits else None
    ids = torch.full((B,), -7, device="cuda", dtype=torch.long)
    nblk = (V // 16 + 3) // 4
    sv = torch.empty(nblk * 16 * nb, device="cuda")
    si = torch.empty(nblk * 16 * nb, device="cuda", dtype=torch.int32)
    _lib.check(lib.fvhd_op_dec_lm_argmax_w8(_st(), _p(x), B, _p(nw), 1e-6, _p(codes), _p(scale), V, H, _p(lg), _p(ids), _p(sv), _p(si)), "lm_argmax_w8")
    torch.cuda.synchronize()
    return lg, ids


@pytest.mark.parametrize("V,H", [(151936, 896), (152064, 3584), (4112, 896)])
@pytest.mark.parametrize("B", [1, 5, 16, 33])
def test_dec_lm_argmax_w8_against_the_reference_and_ties(lib, V, H, B):
    g = torch.Generator(device="cuda").manual_seed(V + H + B)
    codes, scale, Wd = _quantised(V, H, g)
    x = torch.randn(B, H, device="cuda", generator=g).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).float()
    xa = R.normed_operand(x, nw, 1e-6)
    want = torch.cat([xa @ Wd[i:i + 32768].t() for i in range(0, V, 32768)], 1)
    lg, ids = _lm_w8(lib, x, nw, codes, scale)
    assert rel(lg, want) <= 1e-2, rel(lg, want)
    assert torch.equal(ids, _lowest_argmax(lg))
    lg2, ids2 = _lm_w8(lib, x, nw, codes, scale)
    assert torch.equal(lg, lg2) and torch.equal(ids, ids2)
    _, ids3 = _lm_w8(lib, x, nw, codes, scale, logits=False)
    assert torch.equal(ids, ids3)
    # planted ties: row 0's winning weight row (codes AND scale) copied to a higher and a lower index - the lowest copy must win
    best = int(ids[0])
    codes8 = codes.view(torch.uint8)
    for lo, hi in ((7, V - 3), (1029, 1030)):
        c2, s2 = codes8.clone(), scale.clone()
        for j in (lo, hi):
            c2[j] = codes8[best]
            s2[j] = scale[best]
        lg, ids = _lm_w8(lib, x, nw, c2.view(torch.float8_e4m3fn), s2)
        assert float(lg[0, lo]) == float(lg[0, hi]) == float(lg[0].max()), (lo, hi)
        assert int(ids[0]) == min(lo, best) and torch.equal(ids, _lowest_argmax(lg))
