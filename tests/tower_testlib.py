"""TEST INFRASTRUCTURE ONLY - the launch wrappers of tests/test_gpu_tower_ops.py and tests/test_gpu_prefill_gemm_ops.py: one launch of a
tower op (or of a GEMM of the Qwen2 prefill, the same kernel family) through the C ABI into a sentinel-guarded output
(tests/llm_testlib.py: guarded / guard_intact), with the checks every launch gets - the guard behind the output keeps the sentinel and
every input keeps its bits - and the case runner the GEMM tests of both files share (gemm_case / streaming).  Importing it needs no GPU."""
import torch

from ml_fastvlm_amd import _lib

import tower_reference as R
from llm_testlib import check, guard_intact, guarded, ptr, stream

DEV = "cuda:0"


def st():
    return stream(DEV)


def guarded_out(rows, width, dtype=torch.bfloat16, guard_rows=64):
    """[rows, width] of `dtype` in front of `guard_rows` guard rows -> (the whole buffer as int16, the view)"""
    buf, _ = guarded(rows, width * (dtype.itemsize // 2), DEV, guard_rows)
    return buf, buf[:rows].view(dtype)


class unchanged:
    """with unchanged(a, b, ...): launch - every tensor (None allowed) has the bits it had before"""

    def __init__(self, *tensors):
        self.tensors = [t for t in tensors if t is not None]

    def __enter__(self):
        self.before = [t.clone() for t in self.tensors]

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            for i, (t, b) in enumerate(zip(self.tensors, self.before)):
                assert torch.equal(t.view(torch.int16 if t.dtype.itemsize == 2 else torch.int32), b.view(torch.int16 if b.dtype.itemsize == 2 else torch.int32)), f"input {i} was written"


def gemm(lib, A, W, bias, ls, resid, epi, dtype=torch.bfloat16, inplace=False):
    """one fvhd_op_gemm launch -> out [M, N] (a copy); inplace: the tower's and the prefill's form, resid IS out.  EPI_SWIGLU: out is
    [M, N / 2], rows back to back - the bytes behind column N / 2 of the last row are the first guard row - in front of max(64, M) guard
    rows, so that a kernel which walked the activation with the row stride N of every other epilogue would land in the guard"""
    (M, K), N = A.shape, W.shape[0]
    swiglu = epi == _lib.EPI_SWIGLU
    buf, out = guarded_out(M, N // 2 if swiglu else N, dtype, max(64, M) if swiglu else 64)
    if inplace:
        out.copy_(resid)
    with unchanged(A, W, bias, ls, None if inplace else resid):
        check(lib.fvhd_op_gemm(st(), ptr(A), ptr(W), ptr(bias), ptr(ls), ptr(out if inplace else resid), ptr(out), M, N, K, epi, _lib.dtype_code(dtype)),
              f"fvhd_op_gemm {M}x{N}x{K} epi {epi}")
    assert guard_intact(buf, M), "rows >= M were written"
    return out.clone()


def bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16 if a.dtype.itemsize == 2 else torch.int32),
                                                                     b.view(torch.int16 if b.dtype.itemsize == 2 else torch.int32))


def plan(M, N, K, epi, dtype=torch.bfloat16):
    return _lib.gemm_plan_lib().fvhd_gemm_kernel_plan(M, N, K, epi, _lib.dtype_code(dtype))


def gemm_case(lib, want_plan, M, N, K, epi, family, dtype=torch.bfloat16, seed=0, other_rows=()):
    """one (shape, epilogue, family) of one kernel class: plan asserted, guarded launch, inputs unchanged, second launch (in place for
    the residual epilogues, as the tower and the prefill call them) bit-identical, then the family's contract.  other_rows: row counts M'
    whose launch on the first M' rows takes ANOTHER class and must give the same bits.  -> (out, worst err / bound or None)"""
    assert plan(M, N, K, epi, dtype) == want_plan, (M, N, K, epi, plan(M, N, K, epi, dtype), want_plan)
    A, W, b, ls, r = R.gemm_family(family, M, N, K, epi, seed + 1000 * epi, device=DEV)
    out = gemm(lib, A, W, b, ls, r, epi, dtype)
    assert bits(out, gemm(lib, A, W, b, ls, r, epi, dtype, inplace=epi in (R.EPI_BIAS_LS_RESID, R.EPI_RESID))), "a second launch gave other bits"
    want, S = R.gemm_ref(A, W, b, ls, r, epi)
    pre = R.gemm_ref(A, W)[0] if epi == R.EPI_SWIGLU else None
    what = f"gemm plan {want_plan} {M}x{N}x{K} epi {epi} {str(dtype)[6:]} {family}"
    worst = None
    if family == "exact" and epi == R.EPI_SWIGLU:         # the integer pairing family: one bf16 ulp, element by element
        assert float(pre[:, 0::2].abs().max()) <= R.GATE_MAX, "the pairing family's gate sums"
        bad = R.one_ulp(out, want.to(dtype))
        assert bad == 0, f"{what}: {bad} of {want.numel()} elements further than one bf16 ulp from bf16(silu(g) u)"
        print(f"{what}: every element within one ulp")
    elif family == "exact":
        assert torch.equal(out, want.to(dtype)), f"{what}: not the bits of the exact result"
        print(f"{what}: exact")
    else:
        worst = R.inside(out, want, R.gemm_bound(want, S, epi, dtype, ls, pre=pre), what)
        line = f"{what}: worst err / bound {worst:.3f}"
        if epi == R.EPI_BIAS_GELU:      # GELU7_ABS is the polynomial's own error: against the polynomial of the fp64 pre-activation nothing of it is needed
            line += f", against the documented polynomial {R.inside(out, *R.poly_contract(R.gemm_ref(A, W, b, epi=R.EPI_BIAS)[0], R.C_ACC * S, dtype), what + ' (polynomial)'):.3f}"
        print(line)
    for Mp in other_rows:
        p2 = plan(Mp, N, K, epi, dtype)
        assert p2 >= 0 and p2 != want_plan, (Mp, p2)
        sub = gemm(lib, A[:Mp].contiguous(), W, b, ls, r[:Mp].contiguous() if r is not None else None, epi, dtype)
        assert bits(sub, out[:Mp]), f"{what}: class {p2} on the first {Mp} rows gives other bits"
    return out, worst


V1_SHAPES = [   # (plan, M, N, K): ragged N at 16-column granularity, one K tile (32: BK 32, 64: BK 64), three (96), M around the 128-row tile
    (_lib.GEMM_PLAN_V1_NF4_BK32, 1, 16, 32), (_lib.GEMM_PLAN_V1_NF4_BK64, 127, 48, 64), (_lib.GEMM_PLAN_V1_NF4_BK32, 128, 80, 96), (_lib.GEMM_PLAN_V1_NF4_BK32, 129, 144, 32),
    (_lib.GEMM_PLAN_V1_NF4_BK64, 257, 208, 64), (_lib.GEMM_PLAN_V1_NF4_BK32, 257, 272, 96),
    (_lib.GEMM_PLAN_V1_NF4_BK64, 257, 1152, 64),      # tiles_n = 9: the last super-tile group is narrower
    (_lib.GEMM_PLAN_V1_NF3_BK32, 129, 96, 96), (_lib.GEMM_PLAN_V1_NF3_BK64, 257, 288, 64), (_lib.GEMM_PLAN_V1_NF3_BK32, 1, 96, 32), (_lib.GEMM_PLAN_V1_NF3_BK64, 128, 192, 128),
]


def streaming(lib, want_plan, M, N, K, cases, other_rows=(256, 200)):
    """a class with 256-row tiles: the first 256 rows alone take v1s and the first 200 v1 - both must give the bits of the large launch.
    cases: (epilogue, family) pairs -> the worst err / bound of the rc cases"""
    worst = [gemm_case(lib, want_plan, M, N, K, epi, family, other_rows=other_rows if family == "rc" else ())[1] for epi, family in cases]
    return max([w for w in worst if w is not None], default=None)


def gemm_splitk_ls(lib, A, W, bias, ls, resid, splits):
    """one fvhd_op_gemm_splitk_ls launch, in place on a copy of resid (as the tower calls it) -> out [M, N] (a copy)"""
    (M, K), N = A.shape, W.shape[0]
    buf, out = guarded_out(M, N)
    out.copy_(resid)
    pbuf = torch.full((splits * M * N + 4096,), float("nan"), device=DEV)
    with unchanged(A, W, bias, ls):
        check(lib.fvhd_op_gemm_splitk_ls(st(), ptr(A), ptr(W), ptr(bias), ptr(ls), ptr(out), ptr(out), ptr(pbuf), M, N, K, splits), "fvhd_op_gemm_splitk_ls")
    assert guard_intact(buf, M), "rows >= M were written"
    assert bool(torch.isnan(pbuf[splits * M * N:]).all()), "the partial sums' guard tail was written"
    return out.clone()


def gemm_splitk(lib, A, W, resid, splits, inplace=False, norm_w=None, eps=1e-6):
    """one fvhd_op_gemm_splitk launch (norm_w given: fvhd_op_gemm_splitk_norm) into guarded outputs, the fp32 partials [splits][M][N] in
    front of a NaN tail; resid may be None (the entry points accept NULL); inplace: the prefill's form, resid IS out
    -> out [M, N] (a copy), or (out, norm_out)"""
    (M, K), N = A.shape, W.shape[0]
    buf, out = guarded_out(M, N)
    nbuf, nout = guarded_out(M, N)
    if inplace:
        out.copy_(resid)
    pbuf = torch.full((splits * M * N + 4096,), float("nan"), device=DEV)
    with unchanged(A, W, norm_w, None if inplace else resid):
        if norm_w is None:
            check(lib.fvhd_op_gemm_splitk(st(), ptr(A), ptr(W), ptr(out if inplace else resid), ptr(out), ptr(pbuf), M, N, K, splits), f"fvhd_op_gemm_splitk {M}x{N}x{K}/{splits}")
        else:
            check(lib.fvhd_op_gemm_splitk_norm(st(), ptr(A), ptr(W), ptr(out if inplace else resid), ptr(out), ptr(pbuf), M, N, K, splits, ptr(norm_w), ptr(nout), eps),
                  f"fvhd_op_gemm_splitk_norm {M}x{N}x{K}/{splits}")
    assert guard_intact(buf, M) and guard_intact(nbuf, M if norm_w is not None else 0), "rows >= M (or an output that is not this call's) were written"
    assert bool(torch.isnan(pbuf[splits * M * N:]).all()), "the partial sums' guard tail was written"
    assert not bool(torch.isnan(pbuf[:splits * M * N]).any()), "partial sums were left unwritten"
    return out.clone() if norm_w is None else (out.clone(), nout.clone())


def rmsnorm(lib, x, w, eps=1e-6):
    M, H = x.shape
    buf, y = guarded_out(M, H)
    with unchanged(x, w):
        check(lib.fvhd_op_rmsnorm(st(), ptr(x), ptr(y), ptr(w), M, H, eps), f"rmsnorm {M}x{H}")
    assert guard_intact(buf, M), "rows >= M were written"
    return y.clone()


def pack_ffn(lib, W1, W2, precision):
    """fc1 [4C, C], fc2 [C, 4C] (bf16 values) -> the device chunk images of fvhd_ffn_pack"""
    HID, C = W1.shape
    nch, che = HID // 32, 32 * C
    i1 = torch.empty((nch + 1) * che, dtype=torch.bfloat16)
    i2 = torch.empty(nch * che, dtype=torch.bfloat16)
    w1, w2 = W1.float().cpu().contiguous(), W2.float().cpu().contiguous()
    check(lib.fvhd_ffn_pack(C, ptr(w1), ptr(w2), ptr(i1), ptr(i2), precision), "fvhd_ffn_pack")
    return i1.to(DEV), i2.to(DEV)


def ffn(lib, A, w1img, b1, w2img, b2, ls, X, precision):
    """one fvhd_op_ffn_fused launch in place on a guarded copy of X -> X' [M, C] (a copy)"""
    M, C = A.shape
    buf, x = guarded_out(M, C)
    x.copy_(X)
    with unchanged(A, w1img, b1, w2img, b2, ls):
        check(lib.fvhd_op_ffn_fused(st(), ptr(A), ptr(w1img), ptr(b1), ptr(w2img), ptr(b2), ptr(ls), ptr(x), M, C, precision), f"fvhd_op_ffn_fused M{M} C{C}")
    assert guard_intact(buf, M), "rows >= M were written"
    return x.clone()


def attention(lib, qkv, B, N, C, fp8=False):
    buf, out = guarded_out(B * N, C)
    with unchanged(qkv):
        check((lib.fvhd_op_attention_fp8 if fp8 else lib.fvhd_op_attention)(st(), ptr(qkv), ptr(out), B, N, C), f"attention B{B} N{N} C{C}")
    assert guard_intact(buf, B * N), "rows >= B * N were written"
    return out.clone()


def layernorm(lib, x, w, b, eps=1e-5):
    M, C = x.shape
    buf, y = guarded_out(M, C)
    with unchanged(x, w, b):
        check(lib.fvhd_op_layernorm(st(), ptr(x), ptr(y), ptr(w), ptr(b), M, C, eps), f"layernorm {M}x{C}")
    assert guard_intact(buf, M), "rows >= M were written"
    return y.clone()


def se_head(lib, y, wr, br, we, be, dtype):
    B, T, C = y.shape
    RD = wr.shape[0]
    buf, out = guarded_out(B * T, C, dtype)
    pooled = torch.full((B * (C + RD) + 64,), float("nan"), device=DEV)
    scale = torch.full((B * C + 64,), float("nan"), device=DEV)
    with unchanged(y, wr, br, we, be):
        check(lib.fvhd_op_se_head(st(), ptr(y), ptr(pooled), ptr(scale), ptr(wr), ptr(br), ptr(we), ptr(be), ptr(out), _lib.dtype_code(dtype), B, T, C, RD), "se_head")
    assert guard_intact(buf, B * T), "rows >= B * T were written"
    assert bool(torch.isnan(pooled[B * (C + RD):]).all()) and bool(torch.isnan(scale[B * C:]).all()), "a scratch buffer's guard tail was written"
    return out.view(B, T, C).clone()


def pack_dw(w):
    """[Cout, 1, K, K] -> fp32 [K * K][Cout], the tap-major layout of the depthwise entry points"""
    co, _, k, _ = w.shape
    return w.reshape(co, k * k).t().contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def dw_out(B, OH, OW, C):
    buf, y = guarded_out(B * OH * OW, C)
    return buf, y.view(B, OH, OW, C)


def dwconv(lib, entry, x, w, b, stride=1, mult=1, gelu=0):
    """entry: "dwconv" (fvhd_op_dwconv), "dw7_mfma", "dw7s2_mfma"; x NCHW bf16, w [Cout, 1, K, K] fp32 -> y NCHW (a copy)"""
    B, Cin, H, W = x.shape
    K = w.shape[-1]
    OH, OW = (H + 2 * (K // 2) - K) // stride + 1, (W + 2 * (K // 2) - K) // stride + 1
    xn, wd = nhwc(x), pack_dw(w)
    buf, y = dw_out(B, OH, OW, Cin * mult)
    with unchanged(xn, wd, b):
        if entry == "dwconv":
            check(lib.fvhd_op_dwconv(st(), ptr(xn), ptr(y), ptr(wd), ptr(b), B, H, W, Cin, K, stride, mult, gelu), "fvhd_op_dwconv")
        elif entry == "dw7_mfma":
            check(lib.fvhd_op_dw7_mfma(st(), ptr(xn), ptr(y), ptr(wd), ptr(b), B, H, W, Cin), "fvhd_op_dw7_mfma")
        else:
            check(lib.fvhd_op_dw7s2_mfma(st(), ptr(xn), ptr(y), ptr(wd), ptr(b), B, H, W, Cin), "fvhd_op_dw7s2_mfma")
    assert guard_intact(buf, B * OH * OW), "rows behind the output were written"
    return y.permute(0, 3, 1, 2).clone()


def dw3_dw7(lib, x, w3, b3, w7, b7):
    """fvhd_op_dw3_dw7 -> (y, a) NCHW (copies)"""
    B, C, H, W = x.shape
    xn, w3d, w7d = nhwc(x), pack_dw(w3), pack_dw(w7)
    by, y = dw_out(B, H, W, C)
    ba, a = dw_out(B, H, W, C)
    with unchanged(xn, w3d, b3, w7d, b7):
        check(lib.fvhd_op_dw3_dw7(st(), ptr(xn), ptr(y), ptr(a), ptr(w3d), ptr(b3), ptr(w7d), ptr(b7), B, H, W, C, None), "fvhd_op_dw3_dw7")
    assert guard_intact(by, B * H * W) and guard_intact(ba, B * H * W), "rows behind an output were written"
    return y.permute(0, 3, 1, 2).clone(), a.permute(0, 3, 1, 2).clone()
