"""The sampler on the T rows of ONE sequence (fvhd_op_dec_sample_rows, csrc/llm_sample.hip `seq_rows`): row r at n0 is the existing
single op on that row alone at B = 1 and n = n0 + r - the id and the four info words under torch.equal - and the launch leaves the
buffers alone that a decode step passes as last ids, positions and length."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import SENT, check, guard_intact, ptr, sample as _sample, stream  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = [(1.0, 0, 1.0), (0.2, 50, 1.0), (0.9, 40, 0.95)]      # no filter; predict.py's; top-k with top-p
N0, SEED = 285, 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import _lib
    return _lib.lookup_sample_lib()


def _sentinels(n, dtype):
    """n words of `dtype` (8 or 4 bytes) filled with the sentinel pattern -> (the int16 view the guard helper reads, the tensor)"""
    buf = torch.full((n * torch.empty((), dtype=dtype).element_size() // 2,), SENT, device="cuda", dtype=torch.int16)
    return buf, buf.view(dtype)


def _rows(lib, logits, T_, k, p, seed, n0, u=None, seq_row=0):
    T, V = logits.shape
    ids = torch.full((T + 4,), -1, device="cuda", dtype=torch.long)
    info = torch.full((T + 1, 4), -3.0, device="cuda")
    g_last, last = _sentinels(16, torch.long)
    g_pos, pos = _sentinels(16, torch.long)
    g_len, ln = _sentinels(4, torch.int32)
    check(lib.fvhd_op_dec_sample_rows(stream(), ptr(logits), T, V, float(T_), int(k), float(p), int(seed), int(seq_row), int(n0), ptr(u), ptr(ids),
                                      ptr(info), ptr(last), ptr(pos), ptr(ln)), "fvhd_op_dec_sample_rows")
    torch.cuda.synchronize()
    assert guard_intact(g_last, 0) and guard_intact(g_pos, 0) and guard_intact(g_len, 0), "last ids / positions / length were written"
    assert bool((ids[T:] == -1).all()) and bool((info[T:] == -3.0).all()), "rows >= T were written"
    return ids[:T].clone(), info[:T].clone()


@pytest.mark.parametrize("V", [1000, 4099, 65537])
@pytest.mark.parametrize("T", [2, 5, 16])
def test_row_r_is_the_single_op_at_n0_plus_r(lib, T, V):
    g = torch.Generator(device="cuda").manual_seed(1000 * T + V)
    logits = 3.0 * torch.randn(T, V, device="cuda", generator=g)
    logits[T - 1, torch.randperm(V, device="cuda", generator=g)[:V // 3]] = float("-inf")      # a row with suppressed tokens
    for T_, k, p in SETTINGS:
        ids, info = _rows(lib, logits, T_, k, p, SEED, N0)
        drawn = set()
        for r in range(T):
            want_id, want_info = _sample(lib, logits[r:r + 1].contiguous(), T_, k, p, seed=SEED, n=N0 + r)
            assert torch.equal(ids[r:r + 1], want_id) and torch.equal(info[r:r + 1], want_info), (T, V, (T_, k, p), r, ids[r], want_id, info[r], want_info)
            assert float(logits[r, ids[r]]) > float("-inf")
            drawn.add(float(info[r, 3]))
        assert len(drawn) == T                                   # one u per position: the counters differ


def test_u_override_is_indexed_by_the_row_and_seq_row_enters_the_counter(lib):
    from ml_fastvlm_amd.qwen2_decode import philox_uniform
    T, V = 5, 4099
    logits = torch.randn(T, V, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    u = torch.tensor([0.0, 0.25, 0.5, 0.75, 0.999], device="cuda")
    ids, info = _rows(lib, logits, 0.9, 40, 0.95, SEED, N0, u=u)
    assert torch.equal(info[:, 3], u)
    for r in range(T):
        want_id, want_info = _sample(lib, logits[r:r + 1].contiguous(), 0.9, 40, 0.95, u=u[r:r + 1].contiguous())
        assert torch.equal(ids[r:r + 1], want_id) and torch.equal(info[r:r + 1], want_info)
    _, info3 = _rows(lib, logits, 1.0, 0, 1.0, SEED, N0, seq_row=3)
    assert info3[:, 3].tolist() == [philox_uniform(SEED, 3, N0 + r) for r in range(T)]
