"""The weight ring of the fused ConvFFN (csrc/ffn_fused.hip): every chunk must meet its own ring slot.

The chunk loop streams the W1 / W2 chunk images (32 hidden units each) through LDS rings and pairs W1[t] with W2[t-2] two
iterations apart; a ring bug shows as a chunk read from a stale or foreign slot.  The cases here make SINGLE chunks visible:

  * one W2 chunk alive (every other hidden column of fc2 is zero): only chunk j of fc2 may reach the output;
  * one W1 chunk alive (every other row of fc1 and b1 is zero, so every other hidden unit is exactly gelu(0) = 0);
  * tile hand-over: several tiles per launch, every chunk of fc1 at its own scale, run twice - the two outputs must be bit-equal
    (a race between a late image and a fragment read shows as run-to-run differences).

j covers every ring slot (period 3) and S / P parity (period 2), the prologue iterations (0, 1) and the tail (NCH-3 .. NCH-1).

Reference and tolerance are those of tests/test_gpu_ops.py::test_ffn_fused: fp32 on the CPU from the bf16-rounded operands, the hidden
activation rounded as the kernel keeps it, |got - want| <= 1e-2 |want| + 1e-2 rms(want).  The ONE live chunk has 32 hidden units, so its
fc2 columns (one-chunk cases) / the whole fc2 (mirror cases) are drawn at the scale 32^-0.5 of that fan-in, not HID^-0.5: the live chunk
then contributes O(1) to every output element, 50 times the tolerance, and a chunk that met the wrong slot cannot hide in it.
"""
import ctypes
import functools

import pytest
import torch

from ml_fastvlm_amd import _lib
from oracle import fastvithd_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PRECISIONS = [_lib.FFN_HALF, _lib.FFN_BF16]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _bf(x):
    return x.to(torch.bfloat16)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _close(got, want, what):
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    rms = want.pow(2).mean().sqrt().item()
    err = (got - want).abs()
    bad = (err > 1e-2 * want.abs() + 1e-2 * rms).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} elements out of tolerance, max err {err.max():.4g}, rms {rms:.4g}"


def _pack(W1, W2, precision):
    """fc1 [4C, C], fc2 [C, 4C] (fp32 values, bf16-representable) -> device chunk images (fvhd_ffn_pack)"""
    lib = _lib.load()
    HID, C = W1.shape
    nch, che = HID // 32, 32 * C
    i1 = torch.empty((nch + 1) * che, dtype=torch.bfloat16)
    i2 = torch.empty(nch * che, dtype=torch.bfloat16)
    w1, w2 = W1.float().contiguous(), W2.float().contiguous()
    _lib.check(lib.fvhd_ffn_pack(C, _p(w1), _p(w2), _p(i1), _p(i2), precision), "fvhd_ffn_pack")
    return i1.to(DEV), i2.to(DEV)


def _round_hidden(h, precision):
    """what the kernel keeps of the hidden activation: f16 of gelu / 4 (FFN_HALF) or bf16 of gelu (FFN_BF16)"""
    return (h / 4.0).half().float() * 4.0 if precision == _lib.FFN_HALF else _bf(h).float()


def _run(A, X, W1, b1, W2, b2, ls, precision):
    """one launch, in place on a device copy of X -> the copy"""
    lib = _lib.load()
    M, C = A.shape
    w1d, w2d = _pack(W1, W2, precision)
    ad, xd = A.to(DEV), X.clone().to(DEV)
    b1d, b2d, lsd = b1.to(DEV), b2.to(DEV), ls.to(DEV)
    _lib.check(lib.fvhd_op_ffn_fused(_lib.stream_ptr(DEV), _p(ad), _p(w1d), _p(b1d), _p(w2d), _p(b2d), _p(lsd), _p(xd), M, C, precision),
               "fvhd_op_ffn_fused")
    torch.cuda.synchronize()
    return xd


def _want(A, X, W1, b1, W2, b2, ls, precision):
    hid = _round_hidden(O.gelu(A.float() @ W1.float().t() + b1), precision)
    return X.float() + ls * (hid @ W2.float().t() + b2)


@functools.lru_cache(maxsize=None)
def _inputs(C, M):
    """the operands of test_ffn_fused (same seeds and scales), drawn once per shape and never modified; W2 twice: at the
    scale of the whole hidden width and at the scale of one live chunk"""
    HID = 4 * C
    A, X = _bf(_rand(M, C, seed=1)), _bf(_rand(M, C, seed=2))
    W1 = _bf(_rand(HID, C, seed=3, scale=C ** -0.5))
    W2 = _bf(_rand(C, HID, seed=4, scale=HID ** -0.5))
    W2c = _bf(_rand(C, HID, seed=4, scale=32 ** -0.5))
    b1, b2 = _rand(HID, seed=5, scale=0.2), _rand(C, seed=6, scale=0.2)
    ls = torch.rand(C, generator=torch.Generator().manual_seed(7))
    return A, X, W1, b1, W2, W2c, b2, ls


def _chunks(C):
    nch = C // 8
    return [0, 1, 2, 3, 5, 6, nch - 3, nch - 2, nch - 1]


CASES = [(C, j) for C in (96, 192, 384) for j in _chunks(C)]
M_ONE = 160        # one full 128-row tile + a ragged 32-row block


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,j", CASES)
def test_one_w2_chunk_alive(C, j, precision):
    A, X, W1, b1, _, W2c, b2, ls = _inputs(C, M_ONE)
    W2 = torch.zeros_like(W2c)
    W2[:, 32 * j:32 * j + 32] = W2c[:, 32 * j:32 * j + 32]
    got = _run(A, X, W1, b1, W2, b2, ls, precision)
    _close(got, _want(A, X, W1, b1, W2, b2, ls, precision), f"one W2 chunk: C{C} chunk {j} precision {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,j", CASES)
def test_one_w1_chunk_alive(C, j, precision):
    A, X, W1r, b1r, _, W2c, b2, ls = _inputs(C, M_ONE)
    W1, b1 = torch.zeros_like(W1r), torch.zeros_like(b1r)
    W1[32 * j:32 * j + 32] = W1r[32 * j:32 * j + 32]
    b1[32 * j:32 * j + 32] = b1r[32 * j:32 * j + 32]
    got = _run(A, X, W1, b1, W2c, b2, ls, precision)
    _close(got, _want(A, X, W1, b1, W2c, b2, ls, precision), f"one W1 chunk: C{C} chunk {j} precision {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("C,M", [(384, 128 * 5 + 1), (96, 128 * 9 + 33)])
def test_tile_hand_over_is_deterministic(C, M, precision):
    A, X, W1r, b1, W2, _, b2, ls = _inputs(C, M)
    nch = C // 8
    # chunk k at the scale 2^((k % 5) - 2): neighbours in the ring never share a scale (exact in bf16)
    scale = torch.tensor([2.0 ** ((k % 5) - 2) for k in range(nch)]).repeat_interleave(32)[:, None]
    W1 = _bf(W1r.float() * scale)
    first = _run(A, X, W1, b1, W2, b2, ls, precision)
    second = _run(A, X, W1, b1, W2, b2, ls, precision)
    assert torch.equal(first, second), f"C{C} M{M} precision {precision}: two runs on the same inputs differ"
    _close(first, _want(A, X, W1, b1, W2, b2, ls, precision), f"tile hand-over: C{C} M{M} precision {precision}")
