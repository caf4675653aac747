"""The fused stem (one launch: stem[0] 3x3 s2 + GELU, stem[1] depthwise 3x3 s2 + GELU, optionally stem[2] 1x1 + GELU) against the
routes it replaces, BIT FOR BIT: fvhd_op_stem_conv -> fvhd_op_dwconv (two launches) and, with stem[2], -> fvhd_op_gemm.  The fused
kernel is a producer / consumer pipeline over double-buffered LDS regions, so beside the values the tests pin what a pipeline can
get wrong: tiles at every image border, a tile count that is not a multiple of the tiles per workgroup, the strided multi-tile grid
(taken from 8192 tiles on), an unwritten output pixel (sentinel fill) and a race between the two buffers (a second launch into the
same output must give the same bytes).

No tolerance anywhere: the fused kernel promises the same MFMA shapes, k order, tap order, fp32 accumulation, GELU chain and
rounding points as the routes it is compared with, so every comparison is on the raw 16-bit patterns."""
import functools
import os
import sys

import pytest
import torch

from ml_fastvlm_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import ptr as _p, stream  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -1          # 0xffff in every 16-bit word: a bf16 NaN no kernel result equals


def _rand(*shape, seed, scale):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=2)
def _case(dtype, B, R, gain):
    """inputs on the device and the results of the unfused routes, computed once per case: (args, two, three).
    gain scales the weights: 1 = the magnitudes of the parity tests (pre-activations of a few tenths), 12 = pre-activations far
    beyond +-4 in all three convolutions, so that both clamped tails of the GELU are evaluated."""
    lib = _lib.load()
    st = stream(DEV)
    img = torch.rand(B, 3, R, R, generator=torch.Generator().manual_seed(0)).to(dtype).to(DEV)          # [0, 1)
    w0, b0 = _rand(96, 3, 3, 3, seed=1, scale=0.5 * gain), _rand(96, seed=2, scale=0.1 * gain)
    w1, b1 = _rand(96, 1, 3, 3, seed=3, scale=0.4 * gain), _rand(96, seed=4, scale=0.1 * gain)
    w2, b2 = _rand(96, 96, seed=5, scale=96 ** -0.5 * gain).to(torch.bfloat16), _rand(96, seed=6, scale=0.1 * gain)
    w0d = w0.reshape(96, 27).t().contiguous().to(DEV)
    w1d = w1.reshape(96, 9).t().contiguous().to(DEV)
    b0d, b1d, w2d, b2d = b0.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV)
    code = _lib.dtype_code(dtype)
    mid = torch.empty(B, R // 2, R // 2, 96, dtype=torch.bfloat16, device=DEV)
    two = torch.empty(B, R // 4, R // 4, 96, dtype=torch.bfloat16, device=DEV)
    three = torch.empty_like(two)
    _lib.check(lib.fvhd_op_stem_conv(st, _p(img), code, _p(mid), _p(w0d), _p(b0d), B, R), "stem conv")
    _lib.check(lib.fvhd_op_dwconv(st, _p(mid), _p(two), _p(w1d), _p(b1d), B, R // 2, R // 2, 96, 3, 2, 1, 1), "stem dw")
    _lib.check(lib.fvhd_op_gemm(st, _p(two), _p(w2d), _p(b2d), None, None, _p(three), B * (R // 4) ** 2, 96, 96,
                                _lib.EPI_BIAS_GELU, _lib.BF16), "stem[2] gemm")
    torch.cuda.synchronize()
    del mid
    assert torch.isfinite(two.float()).all() and torch.isfinite(three.float()).all()
    if gain > 1:        # the case exists for the tails: the unfused stem[0] output must hold exact zeros (x <= -4) and values >= 4
        assert (two.float().abs().max() > 4) and (three.float().abs().max() > 4)
    return (img, code, w0d, b0d, w1d, b1d, w2d, b2d), two, three


def _bits(t):
    return t.view(torch.int16)


def _run(dtype, B, R, gain=1):
    lib = _lib.load()
    st = stream(DEV)
    (img, code, w0d, b0d, w1d, b1d, w2d, b2d), two, three = _case(dtype, B, R, gain)
    for what, w2a, b2a, want in (("stem[0..1]", None, None, two), ("stem[0..2]", w2d, b2d, three)):
        out = torch.empty_like(want)
        _bits(out).fill_(SENTINEL)
        _lib.check(lib.fvhd_op_stem_fused(st, _p(img), code, _p(out), _p(w0d), _p(b0d), _p(w1d), _p(b1d), _p(w2a), _p(b2a), B, R), what)
        torch.cuda.synchronize()
        first = out.clone()
        _lib.check(lib.fvhd_op_stem_fused(st, _p(img), code, _p(out), _p(w0d), _p(b0d), _p(w1d), _p(b1d), _p(w2a), _p(b2a), B, R), what)
        torch.cuda.synchronize()
        unwritten = (_bits(first) == SENTINEL).all(dim=-1)            # a whole pixel of sentinels
        assert not unwritten.any(), f"{what}: {int(unwritten.sum())} output pixels never written, first at {unwritten.nonzero()[0].tolist()}"
        diff = _bits(first) != _bits(want)
        assert not diff.any(), (f"{what}: {int(diff.sum())} of {diff.numel()} values differ from the unfused route, first at "
                                f"{diff.nonzero()[0].tolist()}, max |diff| {(first.float() - want.float()).abs().max().item()}")
        again = _bits(out) != _bits(first)
        assert not again.any(), f"{what}: a second launch changed {int(again.sum())} values, first at {again.nonzero()[0].tolist()}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("B,R", [(1, 64), (3, 64), (5, 128)], ids=["B1R64", "B3R64", "B5R128"])
def test_fused_stem_bits(dtype, B, R):
    """R = 64: 2 x 2 tiles per image, every one a border tile (zero padding of both convolutions on every side).
    R = 128, B = 5: 80 tiles - below the strided grid, one tile per workgroup: the pipeline only fills and drains."""
    _run(dtype, B, R)


@pytest.mark.parametrize("B,R", [(32, 512), (26, 576)], ids=["B32R512", "B26R576"])
def test_fused_stem_bits_strided_grid(B, R):
    """B = 32 at R = 512: 8192 tiles, the smallest count that takes the strided multi-tile grid (a workgroup walks 32 tiles, the
    pipeline in steady state: both region buffers and both image tiles in use).  B = 26 at R = 576: 8424 tiles = 32 x 263 + 8, the
    last tile of most workgroups is missing."""
    _run(torch.bfloat16, B, R)


def test_fused_stem_bits_gelu_tails():
    """Weights and biases x 12: pre-activations beyond +-4 in all three convolutions - gelu(x) = x and gelu(x) = 0 exactly there."""
    _run(torch.bfloat16, 3, 64, gain=12)
