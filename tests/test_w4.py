"""4-bit LLM weights (include/fvhd.h "LLM 4-bit weights"), the parts that need no GPU: the MXFP4 recipe restated in torch
(`ml_fastvlm_amd.quantize_blocks_mxfp4`), the format tables, the refusals of the new entry points and the builder's per-format contexts.
The properties are checked against plain float arithmetic on the values, not against the restatement's own integer code."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
import w4_testlib as W  # noqa: E402

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def _unpack(codes):
    c = codes.to(torch.int32)
    return torch.stack([c & 0xf, c >> 4], -1).view(codes.shape[0], -1)


def _matrix():
    """rows spanning 36 binades, zero rows and zero blocks, and the planted corner rows"""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(40, 256, generator=g) * torch.exp2(torch.linspace(-18, 18, 40))[:, None]
    w[7] = 0
    w[9, 64:96] = 0
    w[11] *= torch.exp2(torch.randint(-18, 18, (256,), generator=g).float())
    return torch.cat([w.to(torch.bfloat16).float(), W.planted_rows(256)], 0)


def test_recipe_properties():
    from ml_fastvlm_amd import dequantize_blocks_mxfp4, quantize_blocks_mxfp4
    w = _matrix()
    N, K = w.shape
    codes, scales = quantize_blocks_mxfp4(w)
    assert codes.dtype == torch.uint8 and codes.shape == (N, K // 2) and scales.dtype == torch.uint8 and scales.shape == (N, K // 32)
    assert int(scales.min()) >= 2 and int(scales.max()) <= 252
    se = scales.to(torch.int32) - 127
    scale = torch.exp2(se.double())                               # fp64 holds 2^-125 .. 2^125
    code = _unpack(codes)
    val = torch.where((code & 8) != 0, -GRID[code & 7], GRID[code & 7]).view(N, K // 32, 32) * scale[..., None]
    deq = dequantize_blocks_mxfp4(codes, scales)
    assert deq.dtype == torch.bfloat16 and torch.equal(deq.double().view(N, K // 32, 32), val), "code * scale is exact in bf16"
    # value-idempotent (codes may differ: a block whose amax rounded down to 3 gets the next lower scale and doubled codes)
    deq2 = dequantize_blocks_mxfp4(*quantize_blocks_mxfp4(deq))
    assert torch.equal(deq2.view(torch.int16), deq.view(torch.int16))
    # amax / scale in (3, 6] wherever se is not clamped; an all-zero block: se = 0, every code a zero
    wb = w.double().view(N, K // 32, 32)
    amax = wb.abs().amax(-1)
    free = (amax > 0) & (se > -125) & (se < 125)
    ratio = amax[free] / scale[free]
    assert bool(((ratio > 3) & (ratio <= 6)).all()), (ratio.min(), ratio.max())
    assert bool((se[amax == 0] == 0).all()) and bool(((code.view(N, K // 32, 32)[amax == 0] & 7) == 0).all())
    # se = ceil(log2(amax / 6)) exactly (fp64 log2 of a bf16 value over 6 is never within an ulp of an integer except at m = 1.5, planted below)
    want_se = torch.ceil(torch.log2(amax[free] / 6)).to(torch.int32)
    near = (torch.log2(amax[free] / 6) - torch.log2(amax[free] / 6).round()).abs() < 1e-9
    assert torch.equal(se[free][~near], want_se[~near])
    # nearest grid value: |w / scale - code| is the minimum over the grid (ties checked separately)
    a = (wb.abs() / scale[..., None])[free]
    got = GRID[(code.view(N, K // 32, 32)[free] & 7)]
    best = (a[..., None] - GRID).abs().amin(-1)
    assert bool(((a - got).abs() == best).all())
    # the sign bit is w's own
    sign = (w.to(torch.bfloat16).view(torch.int16).to(torch.int32) >> 15) & 1
    assert torch.equal((code >> 3), sign)


def test_recipe_planted_corners():
    from ml_fastvlm_amd import quantize_blocks_mxfp4
    base = 40
    w = _matrix()
    codes, scales = quantize_blocks_mxfp4(w)
    code, se = _unpack(codes)[base:], scales[base:].to(torch.int32) - 127
    # row 2: ties at 0.25 .. 5 land on the even index, both signs, at scale 1 and at scale 2^-9
    for b, s in ((0, 0), (1, -9)):
        assert int(se[2, b]) == s
        blk = code[2, 32 * b:32 * b + 32]
        assert blk[0] == 7 and blk[15] == 15 and blk[16] == 6
        assert blk[1:8].tolist() == list(W.TIE_INDEX) and blk[8:15].tolist() == [8 + i for i in W.TIE_INDEX]
    # row 3: m just below 1.5, exactly 1.5, just above (amax = m 2^(i - 3)): se = e - 2 + (m > 1.5)
    assert se[3, :3].tolist() == [-5, -4, -2]
    assert code[3, 5] == 15 and code[3, 32 + 5] == 15 and code[3, 64 + 5] == 8 + 5      # 1.49 * 4 -> 6; 1.5 * 4 = 6; 1.5078 * 2 -> 3
    # row 4: signed zeros - -0.0 and a small negative both become -0 (code 8), a small positive +0
    assert code[4, :5].tolist() == [7, 8, 8, 0, 8 + 3] and int(se[4, 0]) == -1          # 3 / 0.5 = 6; -0.7 / 0.5 -> -1.5
    # row 5: the lower clamp (se would be -128 / -126): bf16 denormals -> 0 with their sign, 2^-126 -> 0.5, 1.5 * 2^-126 -> 0.75 ties to 1
    assert se[5, :2].tolist() == [-125, -125]
    assert code[5, :4].tolist() == [0, 8, 1, 8 + 2] and code[5, 32:36].tolist() == [4, 8 + 1, 3, 0]
    # row 6: the upper clamp (se would be 126): values above 6 * 2^125 saturate; the block below it is not clamped in effect (amax / scale = 6)
    assert se[6, :2].tolist() == [125, 125]
    assert code[6, :4].tolist() == [7, 15, 6, 0] and code[6, 32:36].tolist() == [7, 8 + 2, 4, 0]           # 2.5 ties to 2
    # row 0: zeros
    assert int(code[0].sum()) == 0 and bool((se[0] == 0).all())


def test_recipe_error_is_coarse_and_stated():
    """one Gaussian matrix: rel-L2 about 0.12 (include/fvhd.h says so); e4m3 with row scales is about 0.036"""
    from ml_fastvlm_amd import dequantize_blocks_mxfp4, quantize_blocks_mxfp4
    g = torch.Generator().manual_seed(1)
    w = torch.randn(128, 1024, generator=g).to(torch.bfloat16)
    err = L.rel(dequantize_blocks_mxfp4(*quantize_blocks_mxfp4(w)).float(), w.float())
    print("mxfp4 rel-L2 of a Gaussian matrix", err)
    assert 0.09 < err < 0.14


def test_quantize_blocks_takes_matrices_of_whole_blocks():
    from ml_fastvlm_amd import quantize_blocks_mxfp4
    with pytest.raises(ValueError, match="K % 32"):
        quantize_blocks_mxfp4(torch.zeros(64))
    with pytest.raises(ValueError, match="K % 32"):
        quantize_blocks_mxfp4(torch.zeros(4, 48))


def test_format_tables():
    import ml_fastvlm_amd
    from ml_fastvlm_amd import _lib
    assert _lib.weight_format_code("mxfp4") == 2 == _lib.W_MXFP4 and _lib.MX_WEIGHT_FORMATS == {"mxfp4": 2}
    assert _lib.WEIGHT_FORMATS == {"bf16": 0, "fp8_e4m3": 1}
    with pytest.raises(ValueError, match="weights must be one of") as e:
        _lib.weight_format_code("int3")
    assert all(n in str(e.value) for n in ("bf16", "fp8_e4m3", "mxfp4"))
    assert _lib.w4_lib() is _lib.load() and _lib.load().fvhd_version() == 510
    assert "quantize_blocks_mxfp4" in ml_fastvlm_amd.__all__ and "dequantize_blocks_mxfp4" in ml_fastvlm_amd.__all__


def test_new_entry_points_refuse_null_and_bad_arguments_with_a_message():
    """host pointers and a NULL stream: a launch would fault, the refusal comes first"""
    from ml_fastvlm_amd import _lib
    lib = _lib.w4_lib()
    host = torch.zeros(256)
    idb = torch.zeros(65, dtype=torch.long)
    p, q = C.c_void_p(host.data_ptr()), C.c_void_p(idb.data_ptr())

    def refused(code, *words):
        assert code != 0
        msg = lib.fvhd_last_error()
        for w in words:
            assert w in msg, (w, msg)

    refused(lib.fvhd_llm_set_weight_format(None, _lib.W_MXFP4), b"fvhd_llm_set_weight_format", b"NULL")
    refused(lib.fvhd_llm_debug_packed_mxfp4(None, 0, _lib.MAT_QKV, p, p, None), b"fvhd_llm_debug_packed_mxfp4", b"NULL")
    refused(lib.fvhd_op_quantize_mxfp4(None, None, 16, 128, p, p), b"fvhd_op_quantize_mxfp4", b"NULL")
    refused(lib.fvhd_op_quantize_mxfp4(None, p, 16, 128, p, None), b"fvhd_op_quantize_mxfp4", b"NULL")
    refused(lib.fvhd_op_quantize_mxfp4(None, p, 16, 48, p, p), b"K % 32")
    refused(lib.fvhd_op_w4_unpack(None, None, p, p, 16, 128, 0), b"fvhd_op_w4_unpack", b"NULL")
    refused(lib.fvhd_op_w4_unpack(None, p, p, p, 16, 64, 0), b"K % 128")
    refused(lib.fvhd_op_w4_unpack(None, p, p, p, 16, 128, 3), b"mode")
    for epi in (_lib.EPI_RESID, _lib.EPI_SWIGLU):
        refused(lib.fvhd_op_dec_gemm_w4(None, epi, p, 1, None, 1e-6, p, None, 16, 128, p, p, None, None, 1), b"fvhd_op_dec_gemm_w4", b"NULL")
        refused(lib.fvhd_op_dec_gemm_w4(None, epi, p, 1, None, 1e-6, None, p, 16, 128, p, p, None, None, 1), b"fvhd_op_dec_gemm_w4", b"NULL")
        refused(lib.fvhd_op_dec_gemm_w4(None, epi, p, 65, None, 1e-6, p, p, 16, 128, p, p, None, None, 1), b"B <= 64")
        refused(lib.fvhd_op_dec_gemm_w4(None, epi, p, 1, None, 1e-6, p, p, 16, 64, p, p, None, None, 1), b"K % 128")
        refused(lib.fvhd_op_dec_gemm_w4(None, epi, p, 1, None, 1e-6, p, p, 16, 128, p, p, None, None, 2), b"scratch")
    refused(lib.fvhd_op_dec_gemm_w4(None, _lib.EPI_BIAS, p, 1, None, 1e-6, p, p, 16, 128, p, p, None, None, 1), b"fvhd_op_dec_gemm_w4", b"epi")
    refused(lib.fvhd_op_dec_qkv_w4(None, p, 1, 128, None, 1e-6, p, None, p, p, q, p, 16, 1e6, p, p, 8, p, 1, 1, 64, None, None, 1),
            b"fvhd_op_dec_qkv_w4", b"NULL")
    refused(lib.fvhd_op_dec_qkv_w4(None, p, 65, 128, None, 1e-6, p, p, p, p, q, p, 16, 1e6, p, p, 8, p, 1, 1, 64, None, None, 1), b"B <= 64")
    refused(lib.fvhd_op_dec_qkv_w4(None, p, 1, 192, None, 1e-6, p, p, p, p, q, p, 16, 1e6, p, p, 8, p, 1, 1, 64, None, None, 1), b"K % 128")
    refused(lib.fvhd_op_dec_lm_argmax_w4(None, p, 1, None, 1e-6, p, None, 16, 128, None, q, p, p), b"fvhd_op_dec_lm_argmax_w4", b"NULL")
    refused(lib.fvhd_op_dec_lm_argmax_w4(None, p, 65, None, 1e-6, p, p, 16, 128, None, q, p, p), b"B <= 64")
    refused(lib.fvhd_op_dec_lm_argmax_w4(None, p, 1, None, 1e-6, p, p, 16, 64, None, q, p, p), b"K % 128")


def test_python_arguments_take_the_new_format():
    """before the device is looked at: "mxfp4" passes the format check (the CPU model is then refused for its device), a wrong prefill
    context is an error, never a repack"""
    from types import SimpleNamespace
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m = L.tiny_qwen2()
    with pytest.raises(RuntimeError, match="HIP device"):
        Qwen2Prefill.from_hf(m, weights="mxfp4")
    for have, want in (("bf16", "mxfp4"), ("mxfp4", "fp8_e4m3"), ("mxfp4", "bf16")):
        with pytest.raises(ValueError, match=have):
            Qwen2Generator.from_hf(m, 1, 8, prefill=SimpleNamespace(weight_format=have), weights=want)


def test_the_builder_caches_contexts_per_format(monkeypatch):
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd import qwen2_prefill as qp
    built = []

    class Pre:
        def __init__(self, weights):
            self.weight_format = weights

    monkeypatch.setattr(qp.Qwen2Prefill, "from_hf", classmethod(lambda cls, model, device=None, weights="bf16": built.append(weights) or Pre(weights)))
    m = L.tiny_qwen2()
    a = builder.prefill_context(m, weights="mxfp4")
    assert built == ["mxfp4"] and m._fvhd_llm_weights == "mxfp4" and a.weight_format == "mxfp4"
    assert builder.prefill_context(m) is a and built == ["mxfp4"]                  # None = the recorded format
    b = builder.prefill_context(m, weights="fp8_e4m3")
    assert built == ["mxfp4", "fp8_e4m3"] and b is not a
    c = builder.prefill_context(m, weights="mxfp4")
    assert built == ["mxfp4", "fp8_e4m3", "mxfp4"] and c.weight_format == "mxfp4"
    with pytest.raises(ValueError, match="mxfp4"):                                 # the refusal lists the new name
        builder.prefill_context(m, weights="int4")


def test_tools_take_the_new_format():
    import importlib
    tool = importlib.import_module("tools.decode_bench")
    old = sys.argv
    try:
        sys.argv = ["decode_bench.py", "--weights", "int3"]
        with pytest.raises(SystemExit):
            tool.main()
    finally:
        sys.argv = old
    from types import SimpleNamespace
    cfg = SimpleNamespace(hidden_size=896, num_hidden_layers=2, num_attention_heads=14, num_key_value_heads=2, intermediate_size=4864, vocab_size=4096)
    b4, b8, b16 = (tool.step_weight_bytes(cfg, w) for w in ("mxfp4", "fp8_e4m3", "bf16"))
    assert b4 < 0.54 * b8 < 0.54 * 0.52 * b16 and math.isfinite(b4)
