"""The single ops of the 4-bit weight path (csrc/llm_w4.hip, include/fvhd.h "LLM 4-bit weights") on the GPU.

  quantise      codes and scale bytes equal `ml_fastvlm_amd.quantize_blocks_mxfp4` (plain torch on the CPU) byte for byte, the planted tie,
                zero and clamp rows of tests/w4_testlib.py included
  bit equality  fvhd_op_dec_gemm_w4 / _qkv_w4 / _lm_argmax_w4 have the BITS of the bf16 ops on `dequantize_blocks_mxfp4(codes, scales)`:
                code * 2^k is exactly a bf16 value and the block scale is applied before the MFMA, so the kernels feed the MFMAs the operands
                the bf16 kernels read, in the same order.  The bf16 ops are tested element by element against fp64 elsewhere
                (tests/test_gpu_decode_ops.py); no tolerance appears here.
  layout        plain -> packed -> plain is the identity; packed -> bf16 equals the torch dequantisation"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
import w4_testlib as W  # noqa: E402

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 16, 17, 33, 64)


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import _lib
    return _lib.w4_lib()


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. the quantiser ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(64, 128), (13, 896), (5, 18944), (7, 384)])
def test_quantize_op_equals_the_torch_recipe(lib, N, K):
    from ml_fastvlm_amd import quantize_blocks_mxfp4
    g = torch.Generator().manual_seed(N + K)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    w[0] *= torch.exp2(torch.randint(-24, 12, (K,), generator=g).float())        # a row spanning many binades
    planted = W.planted_rows(K)
    n = min(N - 1, planted.shape[0])
    w[1:1 + n] = planted[[2, 5, 6, 3, 4, 0, 1, 7][:n]]                            # (5 and 7 rows: the tie and clamp rows first)
    w = w.to(torch.bfloat16)
    want_codes, want_scales = quantize_blocks_mxfp4(w)                            # on the CPU
    wd = w.cuda()
    codes = torch.full((N * K // 2 + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    scales = torch.full((N * K // 32 + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    L.check(lib.fvhd_op_quantize_mxfp4(L.stream(), L.ptr(wd), N, K, L.ptr(codes), L.ptr(scales)), "quantize")
    torch.cuda.synchronize()
    assert bool((codes[N * K // 2:] == 0x5A).all()) and bool((scales[N * K // 32:] == 0x5A).all()), "guard written"
    assert torch.equal(scales[:N * K // 32].view(N, K // 32).cpu(), want_scales)
    assert torch.equal(codes[:N * K // 2].view(N, K // 2).cpu(), want_codes)
    # the torch recipe gives the same bytes on the device
    dc, ds = quantize_blocks_mxfp4(wd)
    assert torch.equal(dc.cpu(), want_codes) and torch.equal(ds.cpu(), want_scales)


# ---- 2. the layout kernel -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(16, 128), (13, 384), (80, 896), (5, 18944)])
def test_pack_unpack_round_trip_and_dequantise(lib, N, K):
    from ml_fastvlm_amd import dequantize_blocks_mxfp4
    g = torch.Generator(device="cuda").manual_seed(N * K)
    codes, scales = W.random_plain(N, K, g, e_lo=2, e_hi=252)
    packed = torch.full((N * K // 2 + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    plain = torch.full((N * K // 2 + 64,), 0x5A, device="cuda", dtype=torch.uint8)
    buf, deq = L.guarded(N, K, "cuda")
    L.check(lib.fvhd_op_w4_unpack(L.stream(), L.ptr(codes), None, L.ptr(packed), N, K, 2), "pack")
    L.check(lib.fvhd_op_w4_unpack(L.stream(), L.ptr(packed), None, L.ptr(plain), N, K, 1), "unpack")
    L.check(lib.fvhd_op_w4_unpack(L.stream(), L.ptr(packed), L.ptr(scales), L.ptr(deq), N, K, 0), "dequantise")
    torch.cuda.synchronize()
    assert bool((packed[N * K // 2:] == 0x5A).all()) and bool((plain[N * K // 2:] == 0x5A).all()) and L.guard_intact(buf, N)
    assert torch.equal(plain[:N * K // 2].view(N, K // 2), codes)
    assert torch.equal(packed[:N * K // 2].sort().values, codes.flatten().sort().values)      # a permutation of dwords
    if K > 128:
        assert not torch.equal(packed[:N * K // 2].view(N, K // 2), codes)
    assert torch.equal(_bits(deq), _bits(dequantize_blocks_mxfp4(codes, scales)))              # signed zeros included


# ---- 3. the decode GEMM: the bits of the bf16 op ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", L.GEMM_SHAPES + [(64, 128), (80, 384), (912, 384)])
def test_dec_gemm_w4_has_the_bits_of_the_bf16_op(lib, N, K):
    from ml_fastvlm_amd import dequantize_blocks_mxfp4
    g = torch.Generator(device="cuda").manual_seed(N + K)
    codes, scales = W.random_plain(N, K, g)
    assert int(scales.max()) - int(scales.min()) >= 40 or scales.numel() < 256
    Wd = dequantize_blocks_mxfp4(codes, scales)
    assert bool(torch.isfinite(Wd).all())
    nw = (1 + 0.3 * torch.randn(K, device="cuda", generator=g)).float()
    plan = L.plan_splits(N, K)
    for B in BATCHES:
        x = (torch.randn(B, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        resid = torch.randn(B, N, device="cuda", generator=g).to(torch.bfloat16)
        for norm in (nw, None):
            for splits in sorted({1, 3, plan}):
                for epi in ("resid", "swiglu"):
                    want = L.dec_gemm(lib, epi, x, norm, Wd, resid, splits)
                    got = W.dec_gemm_w4(lib, epi, x, norm, codes, scales, resid, splits)
                    assert bool(torch.isfinite(want.float()).all())
                    assert torch.equal(_bits(got), _bits(want)), (epi, f"N={N} K={K} B={B} norm={norm is not None} splits={splits}",
                                                                  int((_bits(got) != _bits(want)).sum()))


# ---- 4. q|k|v: q, the cache slot and the bytes around it --------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,hd,H", [(14, 2, 64, 896), (28, 4, 128, 3584)])
@pytest.mark.parametrize("B", [1, 17])
def test_dec_qkv_w4_has_the_bits_of_the_bf16_op(lib, nh, nkv, hd, H, B):
    from ml_fastvlm_amd import dequantize_blocks_mxfp4
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    g = torch.Generator(device="cuda").manual_seed(hd + B + H)
    N, cap, slot, P = (nh + 2 * nkv) * hd, 24, 17, 8192
    codes, scales = W.random_plain(N, H, g, e_lo=96, e_hi=140)
    Wd = dequantize_blocks_mxfp4(codes, scales)
    x = torch.randn(B, H, device="cuda", generator=g).to(torch.bfloat16)
    bias = 0.1 * torch.randn(N, device="cuda", generator=g)
    nw = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).float()
    pos = torch.arange(B, device="cuda", dtype=torch.long) * 421 + 5
    pos[-1] = 9000 if B > 1 else 5                                  # 9000: beyond the table
    table = rope_table(P, hd, 1e6, "cuda")
    length = torch.tensor([slot], device="cuda", dtype=torch.int32)
    for splits in (1, 4):
        outs = []
        for w4 in (False, True):
            kc = torch.full((B + 1, nkv, cap, hd), L.SENT, device="cuda", dtype=torch.int16)
            vc = kc.clone()
            qbuf, q = L.guarded_rows(nh * hd, B)
            part, cnt = L.gemm_scratch(N, B, splits)
            tail = (L.ptr(bias), L.ptr(q), L.ptr(pos), L.ptr(table), P, 1e6, L.ptr(kc), L.ptr(vc), cap, L.ptr(length), nh, nkv, hd, L.ptr(part), L.ptr(cnt), splits)
            if w4:
                L.check(lib.fvhd_op_dec_qkv_w4(L.stream(), L.ptr(x), B, H, L.ptr(nw), 1e-6, L.ptr(codes), L.ptr(scales), *tail), "dec_qkv_w4")
            else:
                L.check(lib.fvhd_op_dec_qkv(L.stream(), L.ptr(x), B, H, L.ptr(nw), 1e-6, L.ptr(Wd), *tail), "dec_qkv")
            torch.cuda.synchronize()
            assert L.guard_intact(qbuf, B * nh * hd) and (cnt is None or int(cnt.abs().sum()) == 0)
            others = torch.ones(cap, dtype=torch.bool)
            others[slot] = False
            assert bool((kc[:, :, others] == L.SENT).all()) and bool((vc[:, :, others] == L.SENT).all()) and bool((kc[B] == L.SENT).all())
            assert not bool((kc[:B, :, slot] == L.SENT).all())
            outs.append((q.clone(), kc, vc))
        for a, b in zip(*outs):
            assert torch.equal(_bits(a), _bits(b)), splits


# ---- 5. lm_head + argmax ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def heads():
    """per (V, H): (codes, scales, the dequantised bf16 matrix), made once and left unchanged"""
    from ml_fastvlm_amd import dequantize_blocks_mxfp4
    out = {}
    for V, H in ((4112, 896), (151936, 896)):
        g = torch.Generator(device="cuda").manual_seed(V + H)
        codes, scales = W.random_plain(V, H, g, e_lo=110, e_hi=125)
        out[V, H] = (codes, scales, dequantize_blocks_mxfp4(codes, scales))
    return out


@pytest.mark.parametrize("V,H", [(4112, 896), (151936, 896)])
@pytest.mark.parametrize("B", [1, 33])
def test_dec_lm_argmax_w4_has_the_bits_of_the_bf16_op_and_ties(lib, heads, V, H, B):
    from ml_fastvlm_amd import dequantize_blocks_mxfp4
    codes, scales, Wd = heads[V, H]
    g = torch.Generator(device="cuda").manual_seed(V + H + B)
    x = torch.randn(B, H, device="cuda", generator=g).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).float()
    want_lg, want_ids = L.dec_lm_argmax(lib, x, nw, Wd)
    lg, ids = W.dec_lm_argmax_w4(lib, x, nw, codes, scales)
    assert bool(torch.isfinite(want_lg).all())
    assert torch.equal(lg.view(torch.int32), want_lg.view(torch.int32)) and torch.equal(ids, want_ids)
    assert torch.equal(ids, L.lowest_argmax(lg))
    _, ids3 = W.dec_lm_argmax_w4(lib, x, nw, codes, scales, logits=False)
    assert torch.equal(ids, ids3)
    # planted duplicates: row 0's winning weight row (codes AND scales) copied to a lower and a higher index - the lowest copy wins
    best = int(ids[0])
    for lo, hi in ((7, V - 3), (1029, 1030)):
        c2, s2 = codes.clone(), scales.clone()
        for j in (lo, hi):
            c2[j] = codes[best]
            s2[j] = scales[best]
        lg, ids = W.dec_lm_argmax_w4(lib, x, nw, c2, s2)
        want_lg, want_ids = L.dec_lm_argmax(lib, x, nw, dequantize_blocks_mxfp4(c2, s2))
        assert float(lg[0, lo]) == float(lg[0, hi]) == float(lg[0].max()), (lo, hi)
        assert int(ids[0]) == min(lo, best) and torch.equal(ids, L.lowest_argmax(lg))
        assert torch.equal(lg.view(torch.int32), want_lg.view(torch.int32)) and torch.equal(ids, want_ids)
