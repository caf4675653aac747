"""fvhd_op_dec_logprobs (csrc/llm_logprobs.hip) on plain device pointers against tests/logprobs_reference.py: the fp64 reference with the
op's ordering rules.  top_ids are compared EXACTLY, always; every log-probability within the per-row bound derived from the kernel's own
order of operations (`logprobs_reference.logprob_bound`):

    |err| <= (1 + 2^-10) ( d U + W U + 2 E + C U + E |log Z| + U |d + log Z| ),   U = 2^-24, E = 2^-23 (expf / logf: 1 ulp)
    d = M - value (one rounding of x - max), W = sum_v t_v (M - x_v) / Z (the roundings of the exponents, weighted by the terms' shares),
    C = ceil(ceil(V / S) / 256) + 14 (the longest chain of roundings thread -> slice -> merge), |log Z| (the log), the last subtraction.

Outputs and scratch sit between sentinel guards; every launch must leave the arrival counters at zero.  Every test prints its largest
|err| / bound (profiles/r17_logprobs_bound.log keeps a run's)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprobs_reference as LR  # noqa: E402
from llm_testlib import SENT, check as _check, guard_intact, guarded, lib, ptr as _p, row_scales, stream as _st  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
NINF = float("-inf")
SMALL_V, LARGE_V = [1, 17, 255, 256, 257, 1001, 4096], [151936, 152064]
SHAPES = [(V, B) for V in SMALL_V for B in (1, 3, 16, 17, 64)] + [(V, B) for V in LARGE_V for B in (1, 3, 64)]
NS = [0, 1, 5, 16]
FRONT = 64                     # guard rows in front of every buffer (llm_testlib.guarded puts 64 behind it)


def _between_guards(rows, width16, dtype):
    """`rows` rows of `width16` int16 elements viewed as `dtype`, with FRONT sentinel rows before and 64 behind -> (buffer, view [rows, ...])"""
    buf, _ = guarded(FRONT + rows, width16, DEV)
    return buf, buf.view(dtype)[FRONT:FRONT + rows]


def _intact(buf, rows):
    return bool((buf[:FRONT] == SENT).all()) and guard_intact(buf, FRONT + rows)


def _scratch(lib, B, V, n):
    """a sentinel-filled scratch of exactly the documented size between guards, its 16 384 counter bytes (64 rows of 256) zeroed ->
    (buffer, view, rows, bytes)"""
    nbytes = lib.fvhd_dec_logprobs_scratch_bytes(B, V, n)
    assert nbytes >= 16384 and nbytes % 256 == 0
    rows = nbytes // 256
    buf, view = _between_guards(rows, 128, torch.int16)
    view[:64].zero_()
    return buf, view, rows, nbytes


def _launch(lib, x, ids, n, scratch=None):
    """one launch -> (token_logprob fp32 [B], top_ids int64 [B, n], top_logprobs fp32 [B, n]), copies; asserts that every guard kept the
    sentinel, that the counters are back at zero and that no input changed"""
    B, V = x.shape
    sbuf, sview, srows, nbytes = scratch if scratch is not None else _scratch(lib, B, V, n)
    assert nbytes >= lib.fvhd_dec_logprobs_scratch_bytes(B, V, n)
    tb, tok = _between_guards(B, 2, torch.float32)
    ib, top = _between_guards(B, 4 * n, torch.int64) if n else (None, None)
    lb, top_lp = _between_guards(B, 2 * n, torch.float32) if n else (None, None)
    before = (x.clone(), ids.clone())
    _check(lib.fvhd_op_dec_logprobs(_st(), _p(x), _p(ids), B, V, n, _p(tok), _p(top), _p(top_lp), _p(sview), nbytes), "fvhd_op_dec_logprobs")
    torch.cuda.synchronize()
    assert _intact(tb, B) and (not n or (_intact(ib, B) and _intact(lb, B))), "an output wrote outside its rows"
    assert _intact(sbuf, srows), "the scratch was written outside fvhd_dec_logprobs_scratch_bytes"
    assert int(sview[:64].view(torch.int32).abs().sum()) == 0, "arrival counters not back at zero"
    assert torch.equal(x.view(torch.int32), before[0].view(torch.int32)) and torch.equal(ids, before[1]), "an input changed"
    if not n:
        return tok[:, 0].clone(), torch.zeros((B, 0), device=DEV, dtype=torch.long), torch.zeros((B, 0), device=DEV)
    return tok[:, 0].clone(), top.clone(), top_lp.clone()


def _check_all_n(lib, x, ids, what, ns=NS):
    """every n of `ns` that fits V against ONE reference -> the largest |err| / bound"""
    V = x.shape[1]
    ns = [n for n in ns if n <= V]
    ref = LR.Reference(x, ids, max(ns))
    worst = 0.0
    for n in ns:
        worst = max(worst, ref.check(n, *_launch(lib, x, ids, n), what=f"{what} n={n}"))
    print(f"logprobs bound: {what} V={V} B={x.shape[0]} n={ns}: max |err| / bound = {worst:.4f}")
    return worst


def _random(B, V, seed, scales=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, V, device=DEV, generator=g)
    if scales:
        x = x * row_scales(B, g, DEV)[:, None]
    ids = torch.randint(0, V, (B,), device=DEV, generator=g)
    return x.contiguous(), ids


def _slice_len(V):
    S = LR.slices(V)
    return S, (V + S - 1) // S


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,B", SHAPES)
def test_rows_of_very_different_scale(lib, V, B):
    """random rows with factors 0.05 .. 20 side by side (`row_scales`); chosen ids random, the first and last row's 0 and V - 1"""
    x, ids = _random(B, V, seed=V * 100 + B)
    ids[0] = 0
    ids[-1] = V - 1 if B > 1 else ids[-1]
    assert _check_all_n(lib, x, ids, "row_scales") <= 1.0


@pytest.mark.parametrize("V,B", [(17, 3), (4096, 17), (152064, 3)])
def test_chosen_id_at_both_ends(lib, V, B):
    x, _ = _random(B, V, seed=7)
    for end in (0, V - 1):
        ids = torch.full((B,), end, device=DEV, dtype=torch.long)
        assert _check_all_n(lib, x, ids, f"id={end}", ns=[0, 5]) <= 1.0


# ---- input families --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,B", [(257, 3), (4096, 17), (151936, 3)])
def test_a_dominant_token(lib, V, B):
    """one logit 60 above the rest: its log-probability is ~ -1e-26 (0 in fp32), every other one ~ -60"""
    x, ids = _random(B, V, seed=11, scales=False)
    dom = torch.arange(B, device=DEV) * (V // B) + (V // B) // 2
    x[torch.arange(B, device=DEV), dom] = 60.0
    ids[::2] = dom[::2]                                          # every other row chose the dominant token
    ref = LR.Reference(x, ids, 5)
    tok, top, top_lp = _launch(lib, x, ids, 5)
    worst = ref.check(5, tok, top, top_lp, "dominant")
    assert torch.equal(top[:, 0], dom) and bool((top_lp[:, 0].abs() < 1e-6).all()) and bool((top_lp[:, 1] < -50).all())
    assert bool((tok[::2].abs() < 1e-6).all())
    print(f"logprobs bound: dominant V={V} B={B} n=[5]: max |err| / bound = {worst:.4f}")


def _plant(x, rows_idx, base=30.0):
    """x[b][idx[k]] = base - k / 8 for the index lists of `rows_idx`: idx[0] is the largest"""
    for b, idx in enumerate(rows_idx):
        for k, i in enumerate(idx):
            x[b, i] = base - k / 8.0
    return x


@pytest.mark.parametrize("V", [4096, 152064, 300000])
def test_top_16_inside_one_threads_chunk_and_in_consecutive_ids(lib, V):
    """thread t of a slice owns the ids i0 + t + 256 j.  Row 0: the 16 largest values in as few threads' chunks as the slice allows (ONE
    thread at V = 300 000, where a chunk has 19 elements; 8 per thread at V = 4096), in an order that is not the index order; row 1: 16
    consecutive ids across a slice boundary; row 2: 16 consecutive ids at the end of the row"""
    S, L = _slice_len(V)
    per = (L + 255) // 256
    x, ids = _random(3, V, seed=13, scales=False)
    s0, t0 = S // 2, 37
    mine = [s0 * L + t0 + 256 * j for j in range(per) if t0 + 256 * j < L]
    chunk = (mine + [s0 * L + t0 + 1 + 256 * j for j in range(per)])[:16]
    assert len(chunk) == 16 and max(chunk) < V and (len(mine) >= 16) == (V == 300000)
    order = [chunk[(5 * k + 3) % 16] for k in range(16)]        # descending value in a scrambled index order
    across = list(range(L - 8, L + 8)) if S > 1 else list(range(100, 116))
    x = _plant(x, [order, across[::-1], list(range(V - 16, V))])
    ref = LR.Reference(x, ids, 16)
    assert ref.top[0].tolist() == order and ref.top[1].tolist() == across[::-1] and ref.top[2].tolist() == list(range(V - 16, V))
    assert _check_all_n(lib, x, ids, "one chunk / consecutive") <= 1.0


@pytest.mark.parametrize("V", [4096, 152064])
def test_top_16_one_per_slice(lib, V):
    """the 16 largest values in 16 different slices (2 slices at V = 4096: 8 each, interleaved), at a different offset in each"""
    S, L = _slice_len(V)
    x, ids = _random(2, V, seed=17, scales=False)
    step = max(S // 16, 1)
    idx = [((k * step) % S) * L + (k * 131 + 5 * (k // S)) % (L - 1) for k in range(16)]
    assert len(set(idx)) == 16 and max(idx) < V
    x = _plant(x, [idx, idx[::-1]])
    ref = LR.Reference(x, ids, 16)
    assert ref.top[0].tolist() == idx and ref.top[1].tolist() == idx[::-1]
    assert _check_all_n(lib, x, ids, "one per slice") <= 1.0


@pytest.mark.parametrize("V", [257, 4096, 152064])
def test_equal_values_across_slice_boundaries_lowest_ids_win(lib, V):
    """row 0: ONE value at 40 ids on both sides of every slice boundary (the maximum, tied): the 16 lowest ids; row 1: the whole row one
    value; row 2: -0 and +0 tied at the top across a boundary"""
    S, L = _slice_len(V)
    x, ids = _random(3, V, seed=19, scales=False)
    x = x - 10.0
    edges = sorted({min(max(s * L + o, 0), V - 1) for s in range(1, max(S, 2)) for o in (-2, -1, 0, 1)} | {V - 1, V - 2})[-40:]
    x[0, edges] = 3.5
    x[1] = -2.25
    zeros = sorted({(min(L, V - 8)) + o for o in range(-4, 4)})
    x[2].clamp_(max=-1.0)
    x[2, zeros] = torch.tensor([0.0, -0.0] * 4, device=DEV)
    n = min(16, V)
    ref = LR.Reference(x, ids, n)
    k = min(n, len(edges))                                       # (2 tied ids at V = 257, 6 at V = 4096, 40 at the model's vocabulary)
    assert ref.top[0, :k].tolist() == edges[:k] and ref.top[1].tolist() == list(range(n)) and ref.top[2, :8].tolist() == zeros
    assert _check_all_n(lib, x, ids, "ties") <= 1.0


@pytest.mark.parametrize("V,B", [(305, 3), (1001, 3), (4096, 17), (151936, 3)])
def test_300_suppressed_tokens(lib, V, B):
    """300 logits at -inf (at V = 305 that leaves 5 finite ones, fewer than n = 16): they add nothing, have log-probability -inf, rank
    behind every finite logit by ascending id, and there is no NaN; row 0 chose a suppressed token"""
    x, ids = _random(B, V, seed=23)
    g = torch.Generator().manual_seed(V)
    finite_of_row0 = None
    for b in range(B):
        sup = torch.randperm(V, generator=g)[:300].to(DEV)
        x[b, sup] = NINF
        if b == 0:
            ids[0] = sup[0]
            finite_of_row0 = V - 300
        elif bool(torch.isinf(x[b, ids[b]])):
            ids[b] = int(torch.isfinite(x[b]).nonzero()[0, 0])
    ref = LR.Reference(x, ids, 16)
    tok, top, top_lp = _launch(lib, x, ids, 16)
    worst = ref.check(16, tok, top, top_lp, "suppressed")
    assert tok[0].item() == NINF and not bool(torch.isnan(tok).any()) and not bool(torch.isnan(top_lp).any())
    k = min(16, finite_of_row0)
    assert bool(torch.isfinite(top_lp[0, :k]).all()) and bool((top_lp[0, k:] == NINF).all())
    if k < 16:
        want = torch.isinf(x[0]).nonzero()[:16 - k, 0]
        assert torch.equal(top[0, k:], want), "the -inf entries behind the finite ones are not in ascending id order"
    assert bool(torch.isfinite(x.gather(1, top[:, :k])).all()), "a suppressed token ranks above a finite one"
    worst = max(worst, _check_all_n(lib, x, ids, "suppressed", ns=[0, 1, 5]))
    print(f"logprobs bound: suppressed V={V} B={B} n=[16]: max |err| / bound = {worst:.4f}")


# ---- repeatability and the counters -----------------------------------------------------------------------------------------------------
def test_two_launches_of_different_batch_on_one_scratch(lib):
    """B = 17 then B = 3 then B = 64 on the scratch sized for the largest: a counter left non-zero by one launch would end the next one's
    row early (or never)"""
    V, n = 4096, 5
    scratch = _scratch(lib, 64, V, 16)
    for B in (17, 3, 64):
        x, ids = _random(B, V, seed=29 + B)
        got = _launch(lib, x, ids, n, scratch=scratch)
        assert LR.Reference(x, ids, n).check(n, *got, what=f"shared scratch B={B}") <= 1.0


@pytest.mark.parametrize("V,B", [(4096, 17), (152064, 64)])
def test_the_same_launch_twice_gives_equal_bits(lib, V, B):
    x, ids = _random(B, V, seed=31)
    a = _launch(lib, x, ids, 16)
    b = _launch(lib, x, ids, 16)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    # and n does not change the numbers: the first 5 of 16 are the 5
    c = _launch(lib, x, ids, 5)
    assert torch.equal(c[0].view(torch.int32), a[0].view(torch.int32)) and torch.equal(c[1], a[1][:, :5])
    assert torch.equal(c[2].view(torch.int32), a[2][:, :5].contiguous().view(torch.int32))


def test_refusals_name_their_reason(lib):
    x, ids = _random(2, 64, seed=37)
    sbuf, sview, srows, nbytes = _scratch(lib, 2, 64, 16)
    out = torch.zeros(2, device=DEV)
    ti, tl = torch.zeros((2, 16), device=DEV, dtype=torch.long), torch.zeros((2, 16), device=DEV)

    def refused(*args):
        assert lib.fvhd_op_dec_logprobs(_st(), *args) != 0
        return lib.fvhd_last_error().decode()

    assert "top_n" in refused(_p(x), _p(ids), 2, 64, 17, _p(out), _p(ti), _p(tl), _p(sview), nbytes)
    assert "exceeds" in refused(_p(x), _p(ids), 2, 8, 9, _p(out), _p(ti), _p(tl), _p(sview), nbytes)
    assert "scratch_bytes" in refused(_p(x), _p(ids), 2, 64, 16, _p(out), _p(ti), _p(tl), _p(sview), nbytes - 256)
    assert "NULL" in refused(_p(x), None, 2, 64, 16, _p(out), _p(ti), _p(tl), _p(sview), nbytes)
    torch.cuda.synchronize()
    assert _intact(sbuf, srows)
