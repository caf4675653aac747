"""The decode step's kernels (csrc/llm_decode.hip) element by element against tests/decode_reference.py (plain torch fp64, pinned to
transformers on the CPU by tests/test_decode_reference.py).

Bound: the project's single-op budget  |got - want| <= 1e-2 |want| + 1e-2 rms(want_row)  with the rms PER BATCH ROW - the rows below are
given scales from 0.05 to 20, a pooled rms would hide the small ones.  (The decode attention keeps P in fp32, so it takes the same 1e-2;
the fp32 logits of the lm_head take the prefill tests' 2e-3.)  Exact cases (one-hot operands, single keys, planted ties) are compared bit
for bit or to one bf16 ulp.  Every output is allocated with a sentinel-filled guard: rows >= B and the tail must stay untouched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as R  # noqa: E402
from llm_testlib import (GEMM_SHAPES, SENT, lib,  # noqa: E402,F401
                         close_by_batch_row as _close, dec_attention as _attention, dec_gemm as _gemm, dec_lm_argmax as _lm,
                         guard_intact as _guard_intact, guarded_rows as _guarded, lowest_argmax as _lowest_argmax,
                         padded_mask as _padded_mask, ptr as _p, row_scales as _row_scales, stream as _st)

pytestmark = pytest.mark.gpu


# ---- 1. the weight-streaming GEMM ---------------------------------------------------------------------------------------------------
def _gemm_inputs(B, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn(B, K, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
    nw = (1 + 0.3 * torch.randn(K, device="cuda", generator=g)).float()
    resid = (torch.randn(B, N, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
    return x, W, nw, resid


@pytest.mark.parametrize("epi", ["resid", "swiglu"])
@pytest.mark.parametrize("B", list(range(1, 17)))
def test_dec_gemm_every_batch_size(lib, B, epi):
    """N = 80: five 16-row tiles, so the second workgroup has ONE active wave; K = 256 in two slices"""
    N, K = 80, 256
    x, W, nw, resid = _gemm_inputs(B, N, K, 100 + B)
    for norm in (nw, None):
        want = R.dec_gemm_ref(x, norm, 1e-6, W, resid, epi)
        for splits in (1, 2):
            got = _gemm(lib, epi, x, norm, W, resid, splits)          # (asserts the guard and the counters)
            _close(got, want, f"B={B} {epi} norm={norm is not None} splits={splits}")


ALL_SPLITS = (1, 2, 3, 4, 7, 16, 64)


@pytest.mark.parametrize("epi", ["resid", "swiglu"])
@pytest.mark.parametrize("N,K", GEMM_SHAPES)
def test_dec_gemm_elementwise(lib, N, K, epi):
    """rows of distinct scale (a GEMM that took another row's rstd, or another row, is far outside), with and without the folded norm,
    every split form: S == 1 with NULL scratch, an uneven last slice (K / 128 = 7 over 4), more splits than K chunks"""
    big = N * K > 3e7
    worst = 0.0
    for B in (1, 2, 7, 16):
        x, W, nw, resid = _gemm_inputs(B, N, K, N + K + B)
        for norm in (nw, None):
            want = R.dec_gemm_ref(x, norm, 1e-6, W, resid, epi)
            for splits in ((1, 7, 16) if big else ALL_SPLITS):
                got = _gemm(lib, epi, x, norm, W, resid, splits)
                worst = max(worst, _close(got, want, f"N={N} K={K} B={B} {epi} norm={norm is not None} splits={splits}"))
            again = _gemm(lib, epi, x, norm, W, resid, 7)
            first = _gemm(lib, epi, x, norm, W, resid, 7)
            assert torch.equal(again, first)                      # deterministic split-K
            if epi == "resid":                                    # the model's form: resid IS out
                for splits in (1, 4):
                    plain = _gemm(lib, epi, x, norm, W, resid, splits)
                    alias = _gemm(lib, epi, x, norm, W, resid, splits, alias=True)
                    assert torch.equal(plain, alias)
    print(f"dec_gemm N={N} K={K} {epi}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("N,K", [(16, 128), (32, 128), (48, 256), (80, 256), (912, 896), (928, 896), (4880, 4864), (4896, 896), (9728, 896)])
def test_dec_gemm_one_hot_exact(lib, N, K):
    """x[b] = e_{k(b)} with distinct k(b), integer weights (exact in bf16), no norm: RESID with a zero residual returns column k(b) of W
    EXACTLY, SWIGLU returns bf16(silu(W[2j, k]) * W[2j + 1, k]) to one bf16 ulp - for every split count.  This pins the lane-to-output
    map, the batch-row map and the gate / up pairing instead of averaging over them.  Gate weights stay within +-60 (up weights and the
    RESID weights within +-125): towards |gate| ~ 87 the fp32 exp of the fast sigmoid leaves its range and returns 0 where the true product
    is a bf16 denormal - a bit-distance check would fail there without a kernel defect."""
    g = torch.Generator(device="cuda").manual_seed(N + K)
    for B in (1, 5, 16):
        ks = [(b * (K // B) + 3 * b + 1) % K for b in range(B)]
        assert len(set(ks)) == B
        x = torch.zeros(B, K, device="cuda", dtype=torch.bfloat16)
        x[torch.arange(B), ks] = 1.0
        W = torch.randint(-125, 126, (N, K), device="cuda", generator=g).to(torch.bfloat16)
        zero = torch.zeros(B, N, device="cuda", dtype=torch.bfloat16)
        want = W[:, ks].t().contiguous()
        for splits in ALL_SPLITS:
            got = _gemm(lib, "resid", x, None, W, zero, splits)
            assert torch.equal(got, want), (B, splits, int((got != want).sum()))
        Wg = W.clone()
        Wg[0::2] = torch.randint(-60, 61, (N // 2, K), device="cuda", generator=g).to(torch.bfloat16)
        col = Wg[:, ks].t().double()
        wb = (torch.nn.functional.silu(col[:, 0::2]) * col[:, 1::2]).to(torch.bfloat16)
        for splits in ALL_SPLITS:
            got = _gemm(lib, "swiglu", x, None, Wg, None, splits)
            gi, wi = got.view(torch.int16).int(), wb.view(torch.int16).int()
            ok = ((gi - wi).abs() <= 1) | ((got == 0) & (wb == 0))
            assert bool(ok.all()), (B, splits, int((~ok).sum()))


# ---- 2. q|k|v + rope + cache append ---------------------------------------------------------------------------------------------------
QKV_SHAPES = [(14, 2, 64, 896), (12, 2, 128, 1536), (28, 4, 128, 3584), (2, 1, 64, 128)]


@pytest.mark.parametrize("nh,nkv,hd,H", QKV_SHAPES)
@pytest.mark.parametrize("B", [1, 3, 16])
def test_dec_qkv_elementwise_and_cache_untouched(lib, nh, nkv, hd, H, B):
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    g = torch.Generator(device="cuda").manual_seed(hd + B + H)
    N, cap, P = (nh + 2 * nkv) * hd, 40, 8192
    x = (torch.randn(B, H, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
    W = (torch.randn(N, H, device="cuda", generator=g) / H ** 0.5).to(torch.bfloat16)
    bias = 0.1 * torch.randn(N, device="cuda", generator=g)
    nw = (1 + 0.3 * torch.randn(H, device="cuda", generator=g)).float()
    pos = torch.arange(B, device="cuda", dtype=torch.long) * 421 + 5
    pos[0] = 0
    if B > 1:
        pos[-1] = 9000                                            # beyond the table: computed on the fly
    table = rope_table(P, hd, 1e6, "cuda")
    qw, kw, vw = R.dec_qkv_ref(x, nw, 1e-6, W, bias, pos, nh, nkv, hd, 1e6)
    worst = 0.0
    for slot in (0, 17, cap - 1, cap):
        for splits in (1, 4, 7):
            kc = torch.full((B, nkv, cap, hd), SENT, device="cuda", dtype=torch.int16)
            vc = torch.full((B, nkv, cap, hd), SENT + 1, device="cuda", dtype=torch.int16)
            qbuf, q = _guarded(nh * hd, B)
            length = torch.tensor([slot], device="cuda", dtype=torch.int32)
            part = torch.empty(splits * N * 16, device="cuda") if splits > 1 else None
            cnt = torch.zeros((N // 16 + 3) // 4, device="cuda", dtype=torch.int32) if splits > 1 else None
            _lib.check(lib.fvhd_op_dec_qkv(_st(), _p(x), B, H, _p(nw), 1e-6, _p(W), _p(bias), _p(q), _p(pos), _p(table), P, 1e6, _p(kc), _p(vc), cap,
                                           _p(length), nh, nkv, hd, _p(part), _p(cnt), splits), "dec_qkv")
            torch.cuda.synchronize()
            what = f"B={B} slot={slot} splits={splits}"
            worst = max(worst, _close(q.view(B, nh, hd), qw, "q " + what))
            assert _guard_intact(qbuf, B * nh * hd) and (cnt is None or int(cnt.abs().sum()) == 0)
            others = torch.ones(cap, dtype=torch.bool, device="cuda")
            if slot < cap:
                others[slot] = False
                worst = max(worst, _close(kc.view(torch.bfloat16)[:, :, slot], kw, "k " + what))
                worst = max(worst, _close(vc.view(torch.bfloat16)[:, :, slot], vw, "v " + what))
            assert bool((kc[:, :, others] == SENT).all()) and bool((vc[:, :, others] == SENT + 1).all()), "cache written outside the slot: " + what
    print(f"dec_qkv nh={nh} hd={hd} H={H} B={B}: worst err / bound {worst:.3f}")


# ---- 3. single-query attention over the cache ------------------------------------------------------------------------------------------
ATT_LENGTHS = [(1, 64), (63, 64), (64, 64), (65, 200), (285, 2304), (2304, 2304)]
ATT_SPLITS = (1, 2, 9, 32)


@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 12, 2), (64, 4, 2)])
@pytest.mark.parametrize("length,cap", ATT_LENGTHS)
@pytest.mark.parametrize("B", [1, 2, 16])
def test_dec_attention_elementwise(lib, hd, nh, nkv, length, cap, B):
    g = torch.Generator(device="cuda").manual_seed(hd * 7 + length + B)
    q = (torch.randn(B, nh * hd, device="cuda", generator=g) * torch.linspace(0.5, 2.0, B, device="cuda")[:, None]).to(torch.bfloat16)
    kc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    vc = (torch.randn(B, nkv, cap, hd, device="cuda", generator=g) * _row_scales(B, g)[:, None, None, None]).to(torch.bfloat16)
    worst = 0.0
    for side in ("left", "right"):
        mask = _padded_mask(B, cap, length, side)
        if B == 16:
            mask[5] = 0                                           # one row with no valid key at all
        want = R.dec_attention_ref(q, kc, vc, mask, length)
        for splits in ATT_SPLITS:
            got = _attention(lib, q, kc, vc, mask, length, splits)
            worst = max(worst, _close(got, want, f"{side} length={length} cap={cap} B={B} splits={splits}"))
            if B == 16:
                assert int(got[5].view(torch.int16).abs().sum()) == 0, "the row without a valid key is not exact zeros"
            assert torch.equal(got, _attention(lib, q, kc, vc, mask, length, splits))
    print(f"dec_attention hd={hd} nh={nh} length={length} cap={cap} B={B}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 12, 2)])
@pytest.mark.parametrize("length,cap", [(1, 64), (65, 200), (285, 2304), (2304, 2304)])
def test_dec_attention_exact_cases(lib, hd, nh, nkv, length, cap):
    B = 3
    g = torch.Generator(device="cuda").manual_seed(hd + length)
    q = torch.randn(B, nh * hd, device="cuda", generator=g).to(torch.bfloat16)
    kc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    vc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    rep = nh // nkv
    # one valid key per row (first / middle / last of the length): softmax of one score is exactly 1, the output IS that v row
    only = [0, (2 * length) // 3, length - 1]
    mask = torch.zeros(B, cap, device="cuda", dtype=torch.uint8)
    for b in range(B):
        mask[b, only[b]] = 1
    want = torch.stack([vc[b, :, only[b]].repeat_interleave(rep, 0).reshape(nh * hd) for b in range(B)])
    for splits in ATT_SPLITS:
        got = _attention(lib, q, kc, vc, mask, length, splits)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), ("one valid key", splits)
    # all valid keys identical: equal scores, the output is the mean of the valid v rows (one bf16 rounding of the fp64 mean, 2^-8 relative, plus the fp32
    # accumulation of <= 2304 terms of |v| <~ 5: 4e-6)
    mask = _padded_mask(B, cap, length, "left", step=70)
    kc2 = kc[:, :, :1].expand(B, nkv, cap, hd).contiguous()
    mean = torch.stack([vc[b, :, :length][:, mask[b, :length] != 0].double().mean(1).repeat_interleave(rep, 0).reshape(nh * hd) for b in range(B)])
    for splits in ATT_SPLITS:
        got = _attention(lib, q, kc2, vc, mask, length, splits).double()
        err = (got - mean).abs()
        assert bool((err <= 2.0 ** -8 * mean.abs() + 4e-6).all()), ("identical keys", splits, float(err.max()))


@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 12, 2)])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_dec_attention_large_score_spread(lib, hd, nh, nkv, where):
    """q scaled by 8 (scores with a standard deviation of 8) and one key aligned with q (score 28, about the
    largest of the 2000 random ones, so several keys share the mass) first, in a middle slice, or last: the
    online-softmax rescale runs across blocks, waves and slices, upwards and downwards"""
    B, length, cap = 2, 2000, 2304
    g = torch.Generator(device="cuda").manual_seed(hd + len(where))
    qv = 8.0 * torch.randn(B, 1, hd, device="cuda", generator=g)
    q = qv.expand(B, nh, hd).reshape(B, nh * hd).to(torch.bfloat16).contiguous()          # every head asks the same question
    kc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    vc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    mask = _padded_mask(B, cap, length, "left")
    first = [int(mask[b].nonzero()[0, 0]) for b in range(B)]
    for b in range(B):
        j = {"first": first[b], "middle": 1111, "last": length - 1}[where]
        kc[b, :, j] = (3.5 * qv[b, 0] / qv[b, 0].norm()).to(torch.bfloat16)       # score 3.5 |q| hd^-0.5 = 28
    want = R.dec_attention_ref(q, kc, vc, mask, length)
    for splits in ATT_SPLITS:
        got = _attention(lib, q, kc, vc, mask, length, splits)
        _close(got, want, f"spread {where} splits={splits}")


# ---- 4. lm_head + argmax -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,H", [(151936, 896), (151936, 1536), (152064, 3584), (16, 896), (4112, 896), (4128, 896), (65552, 1536)])
@pytest.mark.parametrize("B", [1, 16])
def test_dec_lm_argmax_elementwise_and_ties(lib, V, H, B):
    """V = 4112 is 257 tiles and 65552 is 4097: the last workgroup has one active wave; V = 4128 (258 tiles): two"""
    g = torch.Generator(device="cuda").manual_seed(V + H + B)
    x = (torch.randn(B, H, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
    W = (torch.randn(V, H, device="cuda", generator=g) / H ** 0.5).to(torch.bfloat16)
    nw = (1 + 0.3 * torch.randn(H, device="cuda", generator=g)).float()
    xa = R.normed_operand(x, nw, 1e-6)
    want = torch.cat([xa @ W[i:i + 32768].double().t() for i in range(0, V, 32768)], 1)
    lg, ids = _lm(lib, x, nw, W)
    worst = _close(lg, want, f"logits V={V} H={H} B={B}", rtol=2e-3, atol_rms=2e-3)
    print(f"dec_lm_argmax V={V} H={H} B={B}: worst err / bound {worst:.3f}")
    assert torch.equal(ids, _lowest_argmax(lg))
    _, ids2 = _lm(lib, x, nw, W, logits=False)                    # the logits=False path of generate
    assert torch.equal(ids, ids2)
    # planted ties: row 0's winning weight row, moved to chosen index pairs - the lowest index must win each time
    best = int(ids[0])
    wrow = W[best].clone()
    pairs = [(1, 2), (0, 9), (5, 15)]                             # one lane's 4 values; index 0; two lanes of a tile
    if V >= 4112:
        pairs += [(1029, 1030), (645, 661), (700, 3000), (0, 2000), (V - 40, V - 1), (V - 1, V - 1), (V - 2, V - 1)]
        #          a lane group    two waves   two workgroups  index 0    the ragged tail ...
    W[best] = 0
    for lo, hi in pairs:
        keep = W[[lo, hi]].clone()
        W[lo], W[hi] = wrow, wrow
        lg, ids = _lm(lib, x, nw, W)
        assert float(lg[0, lo]) == float(lg[0, hi]) == float(lg[0].max()), (lo, hi)
        assert int(ids[0]) == lo, (lo, hi, int(ids[0]))
        assert torch.equal(ids, _lowest_argmax(lg))
        _, ids2 = _lm(lib, x, nw, W, logits=False)
        assert torch.equal(ids, ids2)
        W[[lo, hi]] = keep
