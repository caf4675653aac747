"""tests/llm_testlib.py pinned on the CPU: the per-row bound catches what a pooled rms hides, both guard forms notice one written
element, and the decode ops' input helpers give the rows they state."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402


def _two_rows(err_in_rms):
    """rows of scale 0.05 and 20; ONE element of the small row (its smallest, so the bound there is ~ 1e-2 rms(row)) off by err_in_rms * rms(row)"""
    g = torch.Generator().manual_seed(0)
    want = (torch.randn(2, 64, generator=g) * torch.tensor([0.05, 20.0])[:, None]).double()
    got = want.clone()
    got[0, want[0].abs().argmin()] += err_in_rms * want[0].pow(2).mean().sqrt()
    return got, want


def test_close_is_per_row_where_a_pooled_rms_would_pass():
    got, want = _two_rows(3e-2)
    with pytest.raises(AssertionError, match="1 of 128 elements out of tolerance"):
        L.close(got, want, "planted")
    with pytest.raises(AssertionError, match="1 of 128 elements out of tolerance"):
        L.close_by_batch_row(got.view(2, 4, 16), want.view(2, 4, 16), "planted")
    assert L.violations(got, want, 1e-2, 1e-2, rows=torch.tensor([False, True])) == (0, 0.0)
    L.close_pooled(got, want, "planted")                          # the pooled rms (~ 14) hides it: why close() exists
    got, want = _two_rows(0.5e-2)
    worst = L.close(got, want, "within the bound")
    assert 0.25 < worst <= 0.5


def test_guard_intact_notices_one_element_behind_the_used_part():
    buf, out = L.guarded(3, 8, "cpu", guard_rows=2)
    out.fill_(1.0)
    assert L.guard_intact(buf, 3)
    buf[3, 0] = 0
    assert not L.guard_intact(buf, 3)
    buf, out = L.guarded_rows(8, 3, device="cpu")
    assert buf.numel() == 16 * 8 + 64 and L.guarded_rows(8, 40, device="cpu")[0].numel() == 42 * 8 + 64
    out.fill_(1.0)
    assert L.guard_intact(buf, 3 * 8)
    buf[3 * 8] = 0
    assert not L.guard_intact(buf, 3 * 8)


def test_row_scales_and_padded_mask():
    g = torch.Generator().manual_seed(1)
    assert L.row_scales(1, g, device="cpu").tolist() == [20.0]
    s = L.row_scales(40, g, device="cpu")
    base = torch.logspace(math.log10(0.05), math.log10(20.0), 16, dtype=torch.float32)
    assert s.shape == (40,) and torch.equal(s[:16].sort().values, base) and torch.equal(s[16:32].sort().values, base)
    kw = dict(cap=64, length=60, side="left", device="cpu")
    assert torch.equal(L.padded_mask(13, **kw), L.padded_mask(13, wrap=13, **kw))
    a, b = L.padded_mask(14, **kw), L.padded_mask(14, wrap=13, **kw)
    assert torch.equal(a[:13], b[:13]) and not torch.equal(a[13], b[13])
    assert int(b[13].sum()) == int(b[0].sum()) == 60 - 12         # row 13 wraps to row 0's padding
