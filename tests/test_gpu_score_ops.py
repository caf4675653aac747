"""fvhd_op_lm_score (csrc/llm_score.hip) on plain device pointers against tests/score_reference.py: the fp64 reference on the bf16-rounded
operands under the DERIVED per-row bound (K u A on a logit, + V u + 8 u (1 + |lse|) on lse), planted peaks at every column where a dropped
or doubled logit could hide, the exact cases, bit stability and the refusals.  Outputs go into sentinel-guarded buffers.

MEASURED (MI355X, worst err / bound as the tests print it): random rows 0.035 (M = 300, V = 512, K = 64), planted peaks 0.007, the exact
cases 0.017, logits of magnitude 1e4 0.021; the multi-tile shapes (MULTI): random 0.015, planted 0.004, 1e4 logits 0.021."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as SR  # noqa: E402
from llm_testlib import check as _check, guard_intact, guarded, lib, ptr as _p, row_scales, stream as _st  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
MS, VS, KS = [1, 17, 129, 300], [512, 520, 4104], [64, 128, 896]
SHAPES = [(M, V, K) for M in MS for V in VS for K in KS]
# Shapes whose plan gives FEWER segments than tiles, as every production call does (8 x 317 rows of a 151 936-id vocabulary: 47 - 48 tiles per
# segment): 20 / 40 / 79 row blocks -> S = 25 / 12 / 6 over the 33 tiles of V = 4104, segments of 1 - 2, 2 - 3 and 5 - 6 tiles.  Only there
# does a workgroup overwrite its LDS image for a next tile, prefetch across the tile edge, rescale its running sum and carry a target
# logit past later tiles.  K = 96 runs the K tiles of 32.
MULTI = [(2536, 4104, 64), (2536, 4104, 96), (5000, 4104, 64), (10001, 4104, 96)]


def test_the_multi_tile_shapes_walk_several_tiles_per_segment():
    for (M, V, K), (lo, hi) in zip(MULTI, [(1, 2), (1, 2), (2, 3), (5, 6)]):
        per = SR.tiles_per_segment(M, V, K)
        assert min(per) == lo and max(per) == hi and SR.plan(M, V, K) < 33, (M, V, K, per)
    for M, V, K in SHAPES:
        assert max(SR.tiles_per_segment(M, V, K)) == 1            # the small shapes: one tile per workgroup


def _f32_guarded(M):
    """fp32 [M] inside a sentinel-filled buffer (llm_testlib.guarded: int16 [M + 64, 2] = one fp32 per row) -> (buffer, fp32 view [M])"""
    buf, _ = guarded(M, 2, DEV)
    return buf, buf.view(torch.float32)[:M, 0]


def _score(lib, x, W, tg, want_lse=True, scratch_fill=None):
    """one launch -> (logprob fp32 [M], lse fp32 [M] or None), copies; asserts that nothing behind row M was written, that no input
    changed and that the plan the library reports is the reference's"""
    M, K = x.shape
    V = W.shape[0]
    S = lib.fvhd_lm_score_plan(M, V, K)
    assert S == SR.plan(M, V, K) and 1 <= S <= 64
    nbytes = lib.fvhd_lm_score_scratch_bytes(M, V, K)
    assert nbytes == 16 * S * M
    scratch = torch.empty(nbytes // 4 + 64, device=DEV)
    scratch.fill_(float("nan") if scratch_fill is None else scratch_fill)          # the scratch needs no initialisation
    lb, lp = _f32_guarded(M)
    sb, lse = _f32_guarded(M)
    before = (x.clone(), W.clone(), tg.clone())
    _check(lib.fvhd_op_lm_score(_st(), _p(x), _p(W), _p(tg), M, V, K, _p(lp), _p(lse) if want_lse else None, _p(scratch), nbytes), "fvhd_op_lm_score")
    torch.cuda.synchronize()
    assert guard_intact(lb, M) and guard_intact(sb, M), "rows behind M were written"
    assert bool(torch.isnan(scratch[nbytes // 4:]).all()) or scratch_fill is not None, "the scratch's tail was written"
    assert torch.equal(x.view(torch.int16), before[0].view(torch.int16)) and torch.equal(W.view(torch.int16), before[1].view(torch.int16))
    assert torch.equal(tg, before[2])
    if not want_lse:
        assert guard_intact(sb, 0), "lse_out = NULL but something was written"
    return lp.clone(), (lse.clone() if want_lse else None)


def _random(M, V, K, seed, scales=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g)
    if scales:
        x = x * row_scales(M, g, DEV)[:, None]
    W = torch.randn(V, K, device=DEV, generator=g) / math.sqrt(K)
    tg = torch.randint(0, V, (M,), device=DEV, generator=g)
    return x.to(torch.bfloat16), W.to(torch.bfloat16), tg


def _within(lp, lse, x, W, tg, what):
    wl, wp, _ = SR.reference(x, W, tg)
    _, bl, bp = SR.bounds(x, W, wl)
    r_lse, r_lp = SR.worst_ratio(lse, wl, bl), SR.worst_ratio(lp, wp, bp)
    print(f"{what}: worst err / bound lse {r_lse:.3f} logprob {r_lp:.3f}")
    assert r_lse <= 1 and r_lp <= 1, (what, r_lse, r_lp)
    ok = (tg >= 0) & (tg < W.shape[0])
    assert bool((lp.double()[ok] <= bp[ok]).all()), f"{what}: a log-probability above its bound"
    return wl, wp


@pytest.mark.parametrize("M,V,K", SHAPES + MULTI)
def test_random_rows_of_scales_side_by_side(lib, M, V, K):
    """rows of scales 0.05 .. 20 (logit spreads of 0.05 .. 20 nats) in one launch: every row within its own bound"""
    x, W, tg = _random(M, V, K, seed=M * 7 + V + K)
    lp, lse = _score(lib, x, W, tg)
    _within(lp, lse, x, W, tg, f"random M={M} V={V} K={K} S={SR.plan(M, V, K)}")


@pytest.mark.parametrize("M,V,K", [(M, V, K) for M in (17, 300) for V in VS for K in KS] + [(129, 4104, 96)] + MULTI)
def test_planted_peaks_at_every_edge(lib, M, V, K):
    """One column per row dominates by > 20 nats.  V u is as large as one dropped column of a FLAT row, so random data cannot show a
    dropped column; here dropping the peak moves lse by > 20, doubling it by log 2.  Peaks at column 0, V - 1, each side of every tile
    (and so segment) edge of the plan in force, inside the ragged last tile, at the wave and lane-group edges.  Once the peak is the
    target (logprob ~ 0), once another column is (logprob ~ -(gap))."""
    cols = SR.edge_columns(M, V, K)
    if (M, V, K) in MULTI:                          # peaks in the first, a middle and the last tile of one and the same segment
        walk = SR.walk_columns(M, V, K)
        assert len(walk) >= 4 and set(walk).issubset(cols)
    g = torch.Generator(device=DEV).manual_seed(V + K + M)
    per = min(K - 16, max(1, M))                    # peaks per launch: one peak dimension each, every peak on at least one row
    worst = 0.0
    for c0 in range(0, len(cols), per):
        x, W, peak = SR.planted(M, V, K, cols[c0:c0 + per], g, DEV)
        other = (peak + 1 + torch.randint(0, V - 1, (M,), device=DEV, generator=g)) % V
        for name, tg in (("peak", peak), ("other", other)):
            lp, lse = _score(lib, x, W, tg)
            wl, wp, z = SR.reference(x, W, tg)
            assert bool((z.gather(1, peak[:, None])[:, 0] == SR.PEAK).all())
            top2 = z.topk(2, -1).values
            assert float((top2[:, 0] - top2[:, 1]).min()) > 20, "the planted gap"
            _, bl, bp = SR.bounds(x, W, wl)
            worst = max(worst, SR.worst_ratio(lse, wl, bl), SR.worst_ratio(lp, wp, bp))
            if name == "peak":
                assert float(lp.abs().max()) < 1e-3
            else:
                assert float((lp.double() - (z.gather(1, tg[:, None])[:, 0] - SR.PEAK)).abs().max()) < 1e-2 and float(lp.max()) < -20
    print(f"planted M={M} V={V} K={K}: {len(cols)} columns, worst err / bound {worst:.3f}")
    assert worst <= 1


@pytest.mark.parametrize("M,V,K", [(17, 520, 64), (300, 4104, 128)])
def test_exact_cases(lib, M, V, K):
    x, W, tg = _random(M, V, K, seed=11)
    x[M // 2] = 0                                   # an all-zero row: every logit 0
    tg[0] = -100                                    # transformers' ignore label
    tg[M - 1] = -1
    if M > 4:
        tg[3] = V                                   # out of range: NaN, documented
        tg[4] = V + 12345
    lp, lse = _score(lib, x, W, tg)
    wl, wp = _within(lp, lse, x, W, tg, f"exact cases M={M} V={V} K={K}")
    assert lp[0].view(torch.int32).item() == 0 and lp[M - 1].view(torch.int32).item() == 0, "an ignored target is 0.0 bit for bit"
    if M > 4:
        assert bool(torch.isnan(lp[3])) and bool(torch.isnan(lp[4])) and bool(torch.isfinite(lse[3:5]).all())
    assert abs(lse[M // 2].item() - math.log(V)) <= V * SR.U + 8 * SR.U * (1 + math.log(V))
    if 0 <= int(tg[M // 2]) < V:
        assert abs(lp[M // 2].item() + math.log(V)) <= V * SR.U + 8 * SR.U * (1 + math.log(V))
    lp2, none = _score(lib, x, W, tg, want_lse=False)
    assert none is None and torch.equal(lp2.view(torch.int32), lp.view(torch.int32))


@pytest.mark.parametrize("M,V,K", [(17, 520, 64), (129, 4104, 128), (2536, 4104, 64), (10001, 4104, 96)])
def test_logits_of_magnitude_1e4_are_finite(lib, M, V, K):
    g = torch.Generator(device=DEV).manual_seed(5)
    s = 1e4 / math.sqrt(K)
    x = (torch.randn(M, K, device=DEV, generator=g) * math.sqrt(s)).to(torch.bfloat16)
    W = (torch.randn(V, K, device=DEV, generator=g) * math.sqrt(s)).to(torch.bfloat16)
    tg = torch.randint(0, V, (M,), device=DEV, generator=g)
    lp, lse = _score(lib, x, W, tg)
    wl, _, z = SR.reference(x, W, tg)
    assert float(z.abs().max()) > 1e4
    assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(lse).all())
    _within(lp, lse, x, W, tg, f"1e4 logits M={M} V={V} K={K}")
    per = SR.tiles_per_segment(M, V, K)
    if max(per) >= 2:
        # the online maximum INSIDE a walk: in the segment with the most tiles there are rows whose largest logit of the segment sits in
        # its first tile (every later tile adds terms that underflow against it) and rows where it sits in the last (the running sum,
        # thousands of nats below, is rescaled to nothing when it arrives), and the row's target logit comes from either
        s = per.index(max(per))
        t0 = SR.segment_tiles(V, SR.plan(M, V, K))[0][s]
        seg = z[:, t0 * SR.TILE:min((t0 + per[s]) * SR.TILE, V)]
        where = seg.argmax(-1) // SR.TILE
        assert bool((where == 0).any()) and bool((where == per[s] - 1).any())
        in_seg = (tg >= t0 * SR.TILE) & (tg < t0 * SR.TILE + seg.shape[1])
        assert bool((in_seg & (tg // SR.TILE - t0 < where)).any()) and bool((in_seg & (tg // SR.TILE - t0 > where)).any())


@pytest.mark.parametrize("M,V,K", [(129, 520, 64), (300, 4104, 896), (17, 512, 96), (2536, 4104, 96), (5000, 4104, 64)])
def test_bits(lib, M, V, K):
    """same launch, same bits (whatever the scratch held); a row's bits depend neither on the other rows nor on other targets; lse on no
    target at all"""
    eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    x, W, tg = _random(M, V, K, seed=3)
    lp, lse = _score(lib, x, W, tg)
    lp2, lse2 = _score(lib, x, W, tg, scratch_fill=1e30)
    assert eq(lp, lp2) and eq(lse, lse2)
    keep = torch.arange(0, M, 3, device=DEV)
    x3, _, tg3 = _random(M, V, K, seed=4)
    x3[keep], tg3[keep] = x[keep], tg[keep]
    lp3, lse3 = _score(lib, x3, W, tg3)
    assert eq(lp3[keep], lp[keep]) and eq(lse3[keep], lse[keep]), "other rows' data changed a row's bits"
    tg4 = (tg + 1 + torch.arange(M, device=DEV)) % V
    tg4[::5] = -100
    _, lse4 = _score(lib, x, W, tg4)
    assert eq(lse4, lse), "a target changed lse"


def test_refusals(lib):
    x, W, tg = _random(16, 512, 64, seed=1)
    out = torch.zeros(16, device=DEV)
    scratch = torch.zeros(1 << 16, device=DEV)
    err = lambda: lib.fvhd_last_error()
    big = scratch.numel() * 4
    assert lib.fvhd_op_lm_score(_st(), _p(x), _p(W), _p(tg), 16, 508, 64, _p(out), None, _p(scratch), big) != 0 and b"V % 8" in err()
    assert lib.fvhd_op_lm_score(_st(), _p(x), _p(W), _p(tg), 16, 512, 48, _p(out), None, _p(scratch), big) != 0 and b"K % 32" in err()
    assert lib.fvhd_op_lm_score(_st(), _p(x), _p(W), _p(tg), 0, 512, 64, _p(out), None, _p(scratch), big) != 0 and b"M >= 1" in err()
    need = lib.fvhd_lm_score_scratch_bytes(16, 512, 64)
    assert lib.fvhd_op_lm_score(_st(), _p(x), _p(W), _p(tg), 16, 512, 64, _p(out), None, _p(scratch), need - 1) != 0 and b"scratch too small" in err()
    assert lib.fvhd_op_lm_score(_st(), _p(x), _p(W), None, 16, 512, 64, _p(out), None, _p(scratch), big) != 0 and b"NULL" in err()
    assert lib.fvhd_op_lm_score(_st(), _p(x), _p(W), _p(tg), 16, 512, 64, None, None, _p(scratch), big) != 0 and b"NULL" in err()
    assert lib.fvhd_lm_score_plan(16, 508, 64) == 0 and lib.fvhd_lm_score_plan(16, 512, 48) == 0 and lib.fvhd_lm_score_scratch_bytes(16, 508, 64) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0, "a refused call wrote its output"
