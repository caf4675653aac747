"""fvhd_op_dec_guidance (csrc/llm_guidance.hip) on plain device pointers against tests/guidance_reference.py: the fp64 reference of

    guided[g] = s * (log_softmax(x[g]) - log_softmax(x[G + g])) + log_softmax(x[G + g])

under the bound derived there from the kernel's own order of operations, element-wise: |err| <= bound.  Logits and scratch sit between
sentinel guards; the unconditional rows must keep their bits and every launch must leave the arrival counters at zero.  Every test prints its
largest |err| / bound (profiles/guidance_bound.log keeps a run's)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_reference as GR  # noqa: E402
from llm_testlib import SENT, check as _check, guard_intact, guarded, ptr as _p, row_scales, stream as _st  # noqa: E402
from ml_fastvlm_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
FRONT = 64                     # guard rows in front of every buffer (llm_testlib.guarded puts 64 behind it)
SCALES = [0.5, 1.5, 3.0, -1.0]
GS = [1, 2, 16, 17, 32]
# 2047 / 2048 / 2049: one slice | two; 4096 / 4097: two | three; 4099: odd, three slices.  With an odd V the rows g V are 16-byte aligned only
# for g % 4 == 0: G = 16 has pairs with both rows aligned (16-byte path + a 3-element tail) beside pairs on the scalar path
SMALL_V = [1, 5, 2047, 2048, 2049, 4096, 4097, 4099]
# 129 024 = 63 * 2048: 63 slices | 64; the two vocabularies of the models
LARGE = [(129024, 1), (129025, 2), (151936, 3), (152064, 32)]


@pytest.fixture(scope="module")
def lib():
    return _lib.guidance_lib()


def _between_guards(rows, width16, dtype):
    buf, _ = guarded(FRONT + rows, width16, DEV)
    return buf, buf.view(dtype)[FRONT:FRONT + rows]


def _intact(buf, rows):
    return bool((buf[:FRONT] == SENT).all()) and guard_intact(buf, FRONT + rows)


def _scratch(lib, G, V):
    """a sentinel-filled scratch of exactly the documented size between guards, its 16 384 counter bytes zeroed -> (buffer, view, rows, bytes)"""
    nbytes = lib.fvhd_dec_guidance_scratch_bytes(G, V)
    assert nbytes >= 16384 and nbytes % 256 == 0
    rows = nbytes // 256
    buf, view = _between_guards(rows, 128, torch.int16)
    view[:64].zero_()
    return buf, view, rows, nbytes


def _launch(lib, x, s, scratch=None):
    """one launch on a guarded copy of x [2 G, V] -> guided fp32 [G, V] (a copy); asserts the guards, the counters and the unconditional rows"""
    B, V = x.shape
    G = B // 2
    sbuf, sview, srows, nbytes = scratch if scratch is not None else _scratch(lib, G, V)
    lbuf, lg = _between_guards(B, 2 * V, torch.float32)
    assert lg.shape == (B, V) and lg.is_contiguous()
    lg.copy_(x)
    _check(lib.fvhd_op_dec_guidance(_st(), _p(lg), G, V, float(s), _p(sview), nbytes), "fvhd_op_dec_guidance")
    torch.cuda.synchronize()
    assert _intact(lbuf, B), "the launch wrote outside the 2 G rows"
    assert _intact(sbuf, srows), "the scratch was written outside fvhd_dec_guidance_scratch_bytes"
    assert int(sview[:64].view(torch.int32).abs().sum()) == 0, "arrival counters not back at zero"
    assert torch.equal(lg[G:].view(torch.int32), x[G:].view(torch.int32)), "an unconditional row changed"
    return lg[:G].clone()


def _random(G, V, seed, dominant=True):
    """2 G rows of very different scale (factors 0.05 .. 20 side by side); pair 0: a single dominant logit in each row, at different ids"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(2 * G, V, device=DEV, generator=g) * row_scales(2 * G, g, DEV)[:, None]
    if dominant and V >= 5:
        x[0, V // 3] = 60.0
        x[G, V - 2] = 45.0
    return x.contiguous()


def _check_scales(lib, x, what):
    worst, ref = 0.0, GR.Reference(x)
    for s in SCALES:
        worst = max(worst, ref.check(s, _launch(lib, x, s), f"{what} s={s}"))
    print(f"guidance bound: {what} V={x.shape[1]} G={x.shape[0] // 2} s={SCALES}: max |err| / bound = {worst:.4f}")
    return worst


@pytest.mark.parametrize("V", SMALL_V)
@pytest.mark.parametrize("G", GS)
def test_rows_of_very_different_scale(lib, V, G):
    assert _check_scales(lib, _random(G, V, seed=100 * V + G), "row_scales") <= 1.0


@pytest.mark.parametrize("V,G", LARGE)
def test_slice_count_edge_and_model_vocabularies(lib, V, G):
    assert _check_scales(lib, _random(G, V, seed=V + G), "large") <= 1.0


@pytest.mark.parametrize("V,G", [(4099, 17), (152064, 3)])
def test_two_launches_give_equal_bits(lib, V, G):
    x = _random(G, V, seed=31)
    a, b = _launch(lib, x, 1.5), _launch(lib, x, 1.5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("V,G", [(5, 2), (2049, 17), (4099, 16), (151936, 2)])
def test_identical_rows_give_the_log_softmax_whatever_the_scale(lib, V, G):
    """x[G + g] = x[g]: d = 0, so guided = lc bit for bit - the op's own lc, equal under every scale - and that lc is the log-softmax"""
    x = _random(G, V, seed=37, dominant=False)
    x[G:] = x[:G]
    got = [_launch(lib, x, s) for s in SCALES]
    for other in got[1:]:
        assert torch.equal(got[0], other)
    assert GR.check(x, 3.0, got[0], "identical rows") <= 1.0


def test_launches_of_different_shape_on_one_scratch(lib):
    """G = 17 then 3 then 32 on the scratch sized for the largest: a counter left non-zero would end the next launch's row early (or never)"""
    V = 4099
    scratch = _scratch(lib, 32, V)
    for G in (17, 3, 32):
        x = _random(G, V, seed=41 + G)
        assert GR.check(x, 1.5, _launch(lib, x, 1.5, scratch=scratch), f"shared scratch G={G}") <= 1.0


def test_refusals_name_their_reason(lib):
    x = _random(2, 64, seed=43)
    sbuf, sview, srows, nbytes = _scratch(lib, 2, 64)

    def refused(*args):
        assert lib.fvhd_op_dec_guidance(_st(), *args) != 0
        return lib.fvhd_last_error().decode()

    assert "NULL" in refused(None, 2, 64, 1.5, _p(sview), nbytes)
    assert "G <= 32" in refused(_p(x), 33, 64, 1.5, _p(sview), nbytes)
    assert "finite" in refused(_p(x), 2, 64, float("inf"), _p(sview), nbytes)
    assert "scratch_bytes" in refused(_p(x), 2, 64, 1.5, _p(sview), nbytes - 256)
    assert lib.fvhd_dec_guidance_scratch_bytes(33, 64) == 0 and lib.fvhd_dec_guidance_scratch_bytes(0, 64) == 0
    torch.cuda.synchronize()
    assert _intact(sbuf, srows)
