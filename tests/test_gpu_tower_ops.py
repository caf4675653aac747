"""Element-wise tests of the vision tower's kernels (csrc/gemm.hip, ffn_fused.hip, attention.hip, stem_head.hip, dwconv*.hip) through
the C ABI, against the fp64 references of tests/tower_reference.py (pinned on the CPU by tests/test_tower_reference.py) under that
module's per-element bounds.  Every launch writes into a sentinel-guarded output (tests/tower_testlib.py); afterwards the guard is
intact, every input has the bits it had before, and a second launch gives the same bits.  Every GEMM test asserts the kernel class it
means with fvhd_gemm_kernel_plan BEFORE the launch (the classes' thresholds are rounds of tiles on the 256 CUs of an MI355X), and where
rows of one shape reach two classes the two must give the same bits.  References of the larger GEMMs are computed in fp64 by torch on
the device: an independent implementation.  Each test prints its worst err / bound.

MEASURED: see profiles/tower_ops_pytest.log (the run this table was filled from) - worst err / bound per family as printed, beside the
CPU model's ratio of tests/test_tower_reference.py:
  family                                                        measured   CPU model
  GEMM rc, every class (v1 NF 4 / 3 x BK 64 / 32, v1s, 256 x 128, 256 x 256, ping-pong), EPI_NONE / BIAS / BIAS_LS_RESID
      bf16 out                                                    0.498      0.498
      f16 out (v1)                                                0.499      0.496
      f32 out (v1: the accumulation alone)                        0.254      0.263
  GEMM rc, EPI_BIAS_GELU, every class + 128 x 192                 0.882 .. 0.952   0.935 (polynomial) / 0.492 (exact GELU)
      the same outputs against the documented polynomial          0.498      0.497
  GEMM exact, every class, EPI_NONE / BIAS / BIAS_LS_RESID        68 cases, all the bits of bf16 / f16 / f32 (fp64 result)
  split-K rc (4 / 8 / 16 slices, v1s and v1 partials)             0.497      (the GEMM's)
  fused FFN, FFN_HALF / FFN_BF16, C = 96 / 192 / 384              0.269 / 0.254    0.259 / 0.193
  attention: plain / qscale / ascending / descending              0.383 / 0.411 / 0.395 / 0.373    0.285 / 0.409 / 0.306 / 0.290
      planted first / last / ragged tile, flat, dominant          0.335 / 0.259 / 0.342 / 0.130 / 0.001    0.228 / 0.315 / 0.243 / 0.124 / 0.000
  attention fp8, rel-L2 vs the e4m3 restatement / the exact       2.4e-3 / 9.1e-2 (contracts 1e-2 / 1e-1)
  layernorm plain / bigmean / const / wscale                      0.498 / 0.467 / 0.498 / 0.498    0.498 / 0.466 / 0.497 / 0.498
  SE head bf16 / f16 / f32 out                                    0.459 / 0.334 / 0.116    <= 0.5
  depthwise without GELU (VALU, dw7 mfma, dw3 + dw7 y and a)      0.497      0.497
  depthwise with GELU (stem[1], dw7 / stride 2 mfma)              0.924 / 0.818    0.836 / 0.902 (polynomial), 0.484 (exact GELU)
      the same outputs against the documented polynomial          0.497 / 0.494
Every ratio above 0.5 belongs to an output that went through the degree-7 GELU: GELU7_ABS is the error of that polynomial, which the
kernels evaluate as documented - the CPU model that evaluates it reaches the same ratios, and against the polynomial of the fp64
pre-activation (tower_reference.poly_contract, without any GELU allowance) the same outputs sit at half a rounding, 0.498.  Nothing
was found wrong in a kernel.  142 tests, 5.5 s.
"""
import os
import sys

import pytest
import torch

from ml_fastvlm_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_reference as R  # noqa: E402
import tower_testlib as T  # noqa: E402
from llm_testlib import lib  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu

DEV = T.DEV
BF16 = torch.bfloat16
NONE, BIAS, GELU, LSR = R.EPI_NONE, R.EPI_BIAS, R.EPI_BIAS_GELU, R.EPI_BIAS_LS_RESID
P = _lib
V1 = (P.GEMM_PLAN_V1_NF4_BK64, P.GEMM_PLAN_V1_NF4_BK32, P.GEMM_PLAN_V1_NF3_BK64, P.GEMM_PLAN_V1_NF3_BK32)


_bits = T.bits


def _plan(lib, M, N, K, epi, dtype=BF16):
    return T.plan(M, N, K, epi, dtype)


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------------
def _gemm_case(lib, plan, M, N, K, epi, family, dtype=BF16, seed=0, other_rows=()):
    """tower_testlib.gemm_case (shared with tests/test_gpu_prefill_gemm_ops.py) -> out"""
    return T.gemm_case(lib, plan, M, N, K, epi, family, dtype, seed, other_rows)[0]


V1_SHAPES = T.V1_SHAPES


@pytest.mark.parametrize("plan,M,N,K", V1_SHAPES)
def test_gemm_v1(lib, plan, M, N, K):
    for epi in (NONE, BIAS, LSR):
        _gemm_case(lib, plan, M, N, K, epi, "exact")
    for epi in (NONE, BIAS, GELU, LSR):
        _gemm_case(lib, plan, M, N, K, epi, "rc")


@pytest.mark.parametrize("M,N,K", [(1, 16, 32), (129, 144, 32), (257, 272, 96), (127, 48, 64)])
def test_gemm_v1_f16_f32_outputs(lib, M, N, K):
    plan = _plan(lib, M, N, K, BIAS, torch.float32)
    assert plan in V1
    for epi, dtype in ((BIAS, torch.float16), (BIAS, torch.float32), (NONE, torch.float32)):
        _gemm_case(lib, plan, M, N, K, epi, "exact", dtype)
        _gemm_case(lib, plan, M, N, K, epi, "rc", dtype)
    assert _plan(lib, M, N, K, LSR, torch.float32) < 0 and _plan(lib, M, N, K, NONE, torch.float16) < 0


@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (384, 256, 192), (640, 384, 320)])      # 2, 3 and 5 K tiles of 64: prologue only, ring not full, ring wraps
def test_gemm_v1s(lib, M, N, K):
    for epi in (NONE, BIAS, LSR):
        _gemm_case(lib, P.GEMM_PLAN_V1S, M, N, K, epi, "exact")
    for epi in (NONE, BIAS, GELU, LSR):
        _gemm_case(lib, P.GEMM_PLAN_V1S, M, N, K, epi, "rc", other_rows=(M - 1,))           # M - 1 rows: v1


def _streaming(lib, plan, M, N, K, full, other_rows=(256, 200)):
    """a class with 256-row tiles: the first 256 rows alone take v1s and the first 200 v1 - both must give the bits of the large launch"""
    T.streaming(lib, plan, M, N, K, [(NONE, "exact"), (BIAS, "exact"), (LSR, "exact"), (NONE, "rc"), (BIAS, "rc"), (GELU, "rc"), (LSR, "rc")] if full else
                [(LSR, "exact"), (GELU, "rc"), (LSR, "rc")], other_rows)


@pytest.mark.parametrize("M,N,K,full", [(8192, 2048, 128, True), (8192, 2048, 192, False), (11008, 384, 3072, False)])     # 512 tiles; the long-K rule with N % 256 != 0
def test_gemm_256x128(lib, M, N, K, full):
    _streaming(lib, P.GEMM_PLAN_256X128, M, N, K, full)


@pytest.mark.parametrize("M,N,K,full", [(12800, 2304, 128, False), (12800, 2304, 192, True), (12800, 2304, 320, False)])    # 450 tiles = 1.76 rounds
def test_gemm_256x256(lib, M, N, K, full):
    _streaming(lib, P.GEMM_PLAN_256X256, M, N, K, full)


@pytest.mark.parametrize("M,N,K,full", [(8192, 1024, 3072, True), (8192, 1024, 3136, False)])     # 48 and 49 K tiles of 64
def test_gemm_pingpong(lib, M, N, K, full):
    _streaming(lib, P.GEMM_PLAN_PINGPONG, M, N, K, full)


def test_gemm_128x192(lib):
    M, N, K = 131072 + 40, 192, 192
    _gemm_case(lib, P.GEMM_PLAN_128X192, M, N, K, GELU, "rc", other_rows=(300,))
    assert _plan(lib, M, N, K, BIAS) == P.GEMM_PLAN_V1_NF3_BK64           # the wide tile is the GELU epilogue's only


def test_gemm_plan_thresholds(lib):
    """the dispatch rules on this device's CU count: one tile (or one K tile) short of a rule takes another class"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert ncu == 256, "the shapes of this file were chosen for the 256 CUs of an MI355X"
    assert _plan(lib, 12800 - 256, 2304, 128, NONE) != P.GEMM_PLAN_256X256       # 441 tiles < 1.75 rounds
    assert _plan(lib, 8192, 1024, 3072 - 64, NONE) != P.GEMM_PLAN_PINGPONG
    assert _plan(lib, 8192 - 256, 2048, 128, NONE) in V1                          # 496 tiles < two rounds
    assert _plan(lib, 256 * 128, 128, 128, NONE) == P.GEMM_PLAN_V1S and _plan(lib, 257 * 128, 128, 128, NONE) in V1
    assert _plan(lib, 8, 8, 40, NONE) < 0 and _plan(lib, 0, 16, 32, NONE) < 0 and _plan(lib, 8, 16, 32, 9) < 0


@pytest.mark.parametrize("M,N,K,sp", [(128, 128, 2048, 4), (77, 128, 2560, 4), (1, 128, 6144, 16), (256, 256, 3072, 8)])
def test_gemm_split_k(lib, M, N, K, sp):
    """the existing split-K shapes reduced to their smallest plan: partials on v1s (M % 128 == 0) and on v1, 4 / 8 / 16 slices"""
    assert lib.fvhd_gemm_splitk_plan(M, N, K) == sp
    for family in ("exact", "rc"):
        A, W, b, ls, r = R.gemm_family(family, M, N, K, LSR, 5, device=DEV)
        out = T.gemm_splitk_ls(lib, A, W, b, ls, r, sp)
        assert _bits(out, T.gemm_splitk_ls(lib, A, W, b, ls, r, sp))
        want, S = R.gemm_ref(A, W, b, ls, r, LSR)
        plain = T.gemm(lib, A, W, b, ls, r, LSR)
        if family == "exact":
            assert torch.equal(out, want.to(BF16)) and _bits(out, plain)
        else:
            print(f"split-K {M}x{N}x{K}/{sp}: worst err / bound {R.inside(out, want, R.gemm_bound(want, S, LSR, BF16, ls), 'split-K'):.3f}")


# ---- fused ConvFFN --------------------------------------------------------------------------------------------------------------------
FFN_M = [1, 31, 32, 33, 127, 128, 129, 257]      # the 32-row blocks and the 128-row tile (every instantiation: 4 waves x 32 rows per workgroup)


@pytest.mark.parametrize("precision", [_lib.FFN_HALF, _lib.FFN_BF16])
@pytest.mark.parametrize("C", [96, 192, 384])
def test_ffn_fused(lib, C, precision):
    A, W1, b1, W2, b2, ls, X = R.ffn_family(257, C, seed=C + precision, device=DEV)
    w1img, w2img = T.pack_ffn(lib, W1, W2, precision)
    want, pre, hid = R.ffn_ref(A, W1, b1, W2, b2, ls, X, precision)
    bound = R.ffn_bound(want, pre, hid, A, W1, W2, ls, precision)
    worst, full = 0.0, None
    for M in reversed(FFN_M):
        a, x = A[:M].contiguous(), X[:M].contiguous()
        out = T.ffn(lib, a, w1img, b1, w2img, b2, ls, x, precision)
        assert _bits(out, T.ffn(lib, a, w1img, b1, w2img, b2, ls, x, precision)), "a second launch gave other bits"
        worst = max(worst, R.inside(out, want[:M], bound[:M], f"ffn C{C} M{M} precision {precision}"))
        if M == 257:
            full = out
        else:
            assert _bits(out, full[:M]), f"rows 0 .. {M - 1} alone differ from their bits inside the larger launch"
    # a block of rows that is NOT the head of the larger launch
    tail = T.ffn(lib, A[128:].contiguous(), w1img, b1, w2img, b2, ls, X[128:].contiguous(), precision)
    assert _bits(tail, full[128:])
    print(f"ffn C{C} precision {precision}: worst err / bound {worst:.3f}")


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
ATT_N = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 576, 1025]


@pytest.mark.parametrize("B,C", [(1, 64), (3, 96)])          # C = 96: three heads, a grid the XCD remap cannot divide by 8
@pytest.mark.parametrize("N", ATT_N)
def test_attention(lib, N, B, C):
    worst = {}
    for name in R.ATT_FAMILIES:
        qkv = R.attention_family(name, B, N, C, seed=N + B, device=DEV)
        out = T.attention(lib, qkv, B, N, C)
        assert _bits(out, T.attention(lib, qkv, B, N, C)), "a second launch gave other bits"
        bad, ratio = R.attention_violations(out, R.attention_ref(qkv, B, N, C), B, N, C)
        assert bad == 0, f"attention {name} B{B} N{N} C{C}: {bad} elements outside the budget, worst err / bound {ratio:.3g}"
        worst[name] = ratio
        if B > 1:                                            # one image alone: its bits inside the batch
            assert _bits(T.attention(lib, qkv[N:2 * N].contiguous(), 1, N, C), out[N:2 * N])
    print(f"attention B{B} N{N} C{C}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("B,C", [(1, 64), (3, 96)])
@pytest.mark.parametrize("N", ATT_N)
def test_attention_fp8(lib, N, B, C):
    """the fp8 form keeps its two rel-L2 contracts (<= 1e-2 against the e4m3 restatement, <= 1e-1 against the exact attention) and gains
    the lengths and the guards"""
    qkv = R.attention_family("plain", B, N, C, seed=N + B, device=DEV)
    out = T.attention(lib, qkv, B, N, C, fp8=True)
    assert _bits(out, T.attention(lib, qkv, B, N, C, fp8=True))
    got = out.double().cpu()
    emu, exact = R.attention_fp8_model(qkv, B, N, C).double(), R.attention_ref(qkv, B, N, C).cpu()
    rel_emu, rel_exact = float((got - emu).norm() / emu.norm()), float((got - exact).norm() / exact.norm())
    print(f"attention fp8 B{B} N{N} C{C}: rel-L2 vs the e4m3 restatement {rel_emu:.3e}, vs the exact attention {rel_exact:.3e}")
    assert rel_emu <= 1e-2 and rel_exact <= 1e-1, (rel_emu, rel_exact)
    if B > 1:
        assert _bits(T.attention(lib, qkv[N:2 * N].contiguous(), 1, N, C, fp8=True), out[N:2 * N])


# ---- layernorm ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 96, 252, 256, 260, 768, 1024, 1280, 1536, 1792, 2048])      # every VPL 1 .. 8, the partly filled last vector
def test_layernorm(lib, C):
    worst = {}
    for name in R.LN_FAMILIES:
        for M in (1, 3, 4, 5, 37):
            x, w, b = R.layernorm_family(name, M, C, seed=C + M, device=DEV)
            y = T.layernorm(lib, x, w, b)
            assert _bits(y, T.layernorm(lib, x, w, b))
            want, mean, rstd = R.layernorm_ref(x, w, b)
            bound = R.layernorm_bound(want, x, w, mean, rstd)
            worst[name] = max(worst.get(name, 0.0), R.inside(y, want, bound, f"layernorm {name} {M}x{C}"))
            if name == "const":
                R.inside(y, b.double().expand_as(want), bound, f"layernorm of constant rows {M}x{C}: not the bias")
    print(f"layernorm C{C}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_layernorm_rejects_widths_it_does_not_take(lib):
    x = torch.zeros(4, 2052, dtype=BF16, device=DEV)
    w = torch.zeros(2052, device=DEV)
    assert lib.fvhd_op_layernorm(T.st(), T.ptr(x), T.ptr(x), T.ptr(w), T.ptr(w), 4, 2052, 1e-5) != 0      # more than 8 vectors per lane
    assert lib.fvhd_op_layernorm(T.st(), T.ptr(x), T.ptr(x), T.ptr(w), T.ptr(w), 4, 6, 1e-5) != 0         # C % 4


# ---- SE head ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T_", [1, 16, 256])
def test_se_head(lib, T_, B):
    C, RD = 3072, 192
    y, wr, br, we, be = R.se_head_family(B, T_, C, RD, seed=T_ + B, device=DEV)
    want, S_arg = R.se_head_ref(y, wr, br, we, be)
    for dtype in (BF16, torch.float16, torch.float32):
        out = T.se_head(lib, y, wr, br, we, be, dtype)
        assert _bits(out, T.se_head(lib, y, wr, br, we, be, dtype))
        print(f"se head B{B} T{T_} {str(dtype)[6:]}: worst err / bound {R.inside(out, want, R.se_head_bound(want, y, S_arg, dtype, RD), 'se head'):.3f}")


# ---- depthwise convolutions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,K,S,mult,gelu,Cin,H,W", [
    ("dwconv", 7, 1, 1, 0, 192, 9, 20), ("dwconv", 3, 1, 1, 0, 96, 13, 17),            # the VALU kernels: ragged tiles
    ("dwconv", 3, 2, 1, 1, 96, 14, 18), ("dwconv", 3, 1, 2, 0, 64, 6, 6),              # stem[1], conv_exp
    ("dw7_mfma", 7, 1, 1, 0, 64, 9, 70), ("dw7_mfma", 7, 1, 1, 0, 96, 11, 32),         # a ragged second strip; 96-channel workgroups, half a strip
    ("dw7s2_mfma", 7, 2, 2, 1, 32, 10, 130), ("dw7s2_mfma", 7, 2, 2, 1, 96, 9, 20),    # a last strip one pixel wide; 1.5 channel blocks
])
def test_depthwise_colscale(lib, entry, K, S, mult, gelu, Cin, H, W, B=2):
    """channels spanning 1e-2 .. 10 in taps and input, the bound per element (hence per (image, channel) plane)"""
    x, w, b = R.dwconv_family(B, Cin, H, W, K, mult, seed=K + Cin, device=DEV)
    bf16_taps = entry != "dwconv"                     # the matrix-core kernels round their taps to bf16
    y = T.dwconv(lib, entry, x, w, b, S, mult, gelu)
    assert _bits(y, T.dwconv(lib, entry, x, w, b, S, mult, gelu))
    want, Sc = R.dwconv_ref(x.cpu(), w.cpu(), b.cpu(), S, bool(gelu), bf16_taps)
    line = f"{entry} K{K} S{S} m{mult} C{Cin} {H}x{W}: worst err / bound {R.inside(y.cpu(), want, R.dwconv_bound(want, Sc, K, bool(gelu)), entry):.3f}"
    if gelu:
        pre = R.dwconv_ref(x.cpu(), w.cpu(), b.cpu(), S, False, bf16_taps)[0]
        line += f", against the documented polynomial {R.inside(y.cpu(), *R.poly_contract(pre, (K * K + 1) * 2.0 ** -24 * Sc), entry + ' (polynomial)'):.3f}"
    print(line)


@pytest.mark.parametrize("C,H,W", [(64, 9, 68), (96, 9, 64)])      # a third strip 4 px wide; C % 64 == 32: the last channel block half masked
def test_dw3_dw7_colscale(lib, C, H, W, B=2):
    x, w3, b3 = R.dwconv_family(B, C, H, W, 3, 1, seed=C, device=DEV)
    w3[:, 0, 1, 1] += 1.0                             # a re-parameterised RepMixer: identity + branches
    _, w7, b7 = R.dwconv_family(B, C, H, W, 7, 1, seed=C + 1, device=DEV)
    y, a = T.dw3_dw7(lib, x, w3, b3, w7, b7)
    y2, a2 = T.dw3_dw7(lib, x, w3, b3, w7, b7)
    assert _bits(y, y2) and _bits(a, a2)
    want_y, S3 = R.dwconv_ref(x.cpu(), w3.cpu(), b3.cpu())
    ry = R.inside(y.cpu(), want_y, R.dwconv_bound(want_y, S3, 3, taps_rel=2.0 ** -17), "dw3_dw7: y")      # hi + lo bf16 taps: 16 mantissa bits
    want_a, S7 = R.dwconv_ref(y.cpu(), w7.cpu(), b7.cpu(), bf16_taps=True)                               # of the kernel's own y
    print(f"dw3_dw7 C{C} {H}x{W}: worst err / bound y {ry:.3f}, a {R.inside(a.cpu(), want_a, R.dwconv_bound(want_a, S7, 7), 'dw3_dw7: a'):.3f}")
