"""TEST INFRASTRUCTURE ONLY - the launch wrappers of tests/test_gpu_tower_ops.py: one launch of a tower op through the C ABI into a
sentinel-guarded output (tests/llm_testlib.py: guarded / guard_intact), with the checks every launch gets - the guard behind the output
keeps the sentinel and every input keeps its bits.  Importing it needs no GPU."""
import torch

from ml_fastvlm_amd import _lib

from llm_testlib import check, guard_intact, guarded, ptr, stream

DEV = "cuda:0"


def st():
    return stream(DEV)


def guarded_out(rows, width, dtype=torch.bfloat16):
    """[rows, width] of `dtype` in front of 64 guard rows -> (the whole buffer as int16, the view)"""
    buf, _ = guarded(rows, width * (dtype.itemsize // 2), DEV)
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
    """one fvhd_op_gemm launch -> out [M, N] (a copy); inplace: the tower's form, resid IS out"""
    (M, K), N = A.shape, W.shape[0]
    buf, out = guarded_out(M, N, dtype)
    if inplace:
        out.copy_(resid)
    with unchanged(A, W, bias, ls, None if inplace else resid):
        check(lib.fvhd_op_gemm(st(), ptr(A), ptr(W), ptr(bias), ptr(ls), ptr(out if inplace else resid), ptr(out), M, N, K, epi, _lib.dtype_code(dtype)),
              f"fvhd_op_gemm {M}x{N}x{K} epi {epi}")
    assert guard_intact(buf, M), "rows >= M were written"
    return out.clone()


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
