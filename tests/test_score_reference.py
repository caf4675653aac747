"""CPU: pins tests/score_reference.py (the fp64 reference of scoring, its plan mirror, the planted inputs), `score_targets` against
transformers' own label shift, and the session's chunk and label builder.  No device is touched."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_reference as SR  # noqa: E402
from ml_fastvlm_amd import _lib  # noqa: E402
from ml_fastvlm_amd.builder import session_score_chunk  # noqa: E402
from ml_fastvlm_amd.qwen2_prefill import label_aligned, score_targets  # noqa: E402


def test_reference_is_cross_entropy_in_fp64():
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(37, 64, generator=g) * 3).to(torch.bfloat16)
    W = (torch.randn(520, 64, generator=g) / 8).to(torch.bfloat16)
    tg = torch.randint(0, 520, (37,), generator=g)
    tg[5] = -100
    lse, lp, z = SR.reference(x, W, tg)
    ce = torch.nn.functional.cross_entropy(z, tg, reduction="none", ignore_index=-100)
    assert z.dtype == torch.float64 and torch.allclose(-lp, ce, rtol=0, atol=1e-12) and lp[5] == 0
    assert torch.allclose(lse, z.exp().sum(-1).log(), rtol=0, atol=1e-12)
    tg[6] = 520
    assert math.isnan(SR.reference(x, W, tg)[1][6])
    # the bound covers an fp32 evaluation in torch's own order, and is not vacuous: a dropped column of a peaked row breaks it
    bz, bl, bp = SR.bounds(x, W, lse)
    z32 = x.float() @ W.float().t()
    assert bool(((z32.double() - z).abs().amax(-1) <= bz).all())
    assert bool(((torch.logsumexp(z32, -1).double() - lse).abs() <= bl).all())
    assert float(bl.max()) < 1e-3 and bool((bp > bl).all())


def test_plan_mirror_is_the_librarys():
    lib = _lib.score_lib()
    for M in (1, 17, 128, 129, 300, 1024, 1025, 2536, 70000):
        for V in (8, 512, 520, 4104, 151936, 152064):
            for K in (32, 64, 96, 896, 3584):
                S = SR.plan(M, V, K)
                assert lib.fvhd_lm_score_plan(M, V, K) == S and 1 <= S <= 64
                assert lib.fvhd_lm_score_scratch_bytes(M, V, K) == 16 * S * M
                firsts, ntile = SR.segment_tiles(V, S)
                assert firsts[0] == 0 and all(b > a for a, b in zip(firsts, firsts[1:])) and firsts[-1] < ntile      # no empty segment
    for M, V, K in ((0, 512, 64), (4, 516, 64), (4, 512, 48), (4, 0, 64), (4, 512, 0)):
        assert SR.plan(M, V, K) == 0 == lib.fvhd_lm_score_plan(M, V, K)
    assert 448 < SR.plan(2536, 151936, 896) * ((2536 + 127) // 128) <= 512     # the benchmark's shape: resident at once at two workgroups per CU


def test_edge_columns_and_planted_rows():
    cols = SR.edge_columns(300, 4104, 64)
    assert cols[0] == 0 and cols[-1] == 4103 and {127, 128, 4095, 4096, 4100}.issubset(cols)
    g = torch.Generator().manual_seed(1)
    cols = SR.edge_columns(40, 520, 64)
    assert {0, 127, 128, 511, 512, 519}.issubset(cols) and len(cols) >= 16
    x, W, peak = SR.planted(40, 520, 64, cols, g, "cpu")
    _, _, z = SR.reference(x, W, peak)
    top2 = z.topk(2, -1)
    assert torch.equal(top2.indices[:, 0], peak) and bool((top2.values[:, 0] == SR.PEAK).all()) and float((top2.values[:, 0] - top2.values[:, 1]).min()) > 20
    assert set(peak.tolist()) == set(cols)


@pytest.mark.parametrize("side", ["none", "left", "right"])
def test_score_targets_is_transformers_shift(side):
    g = torch.Generator().manual_seed(2)
    B, T, V = 4, 13, 50
    logits = torch.randn(B, T, V, generator=g).double()
    labels = torch.randint(0, V, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    for b in range(B):
        n = 2 * b
        if side == "left" and n:
            mask[b, :n] = 0
        if side == "right" and n:
            mask[b, T - n:] = 0
    labels[1, 4:8] = -100                                        # a run of ignored labels (a prompt inside the sequence)
    labels[2, -1] = -100
    # what a caller of forward(labels=...) passes: -100 on the padding, and on the first real token (nothing predicts it)
    hf_labels = labels.masked_fill(mask == 0, -100)
    first = mask.argmax(1)
    hf_labels[torch.arange(B), first] = -100
    want = SR.hf_token_logprobs(logits, hf_labels)
    tg = score_targets(labels, None if side == "none" else mask)
    assert tg.dtype == torch.long and tg.shape == (B, T) and bool((tg[:, -1] == -100).all())
    lp = torch.log_softmax(logits, -1).gather(2, tg.clamp_min(0)[..., None])[..., 0]
    got = label_aligned(torch.where(tg >= 0, lp, torch.zeros_like(lp)))
    assert torch.allclose(got, want, rtol=0, atol=1e-12)
    assert bool((got[:, 0] == 0).all()) and bool((got[hf_labels == -100] == 0).all()) and bool((got[mask == 0] == 0).all())
    # transformers' loss = the mean over the scored tokens
    scored = label_aligned(tg >= 0)
    loss = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), hf_labels[:, 1:].reshape(-1), ignore_index=-100)
    assert abs(float(-got.sum() / scored.sum()) - float(loss)) < 1e-12
    # THE ONE DIVERGENCE from transformers: a caller who masks only the padding (not the first real token) gets that token scored by
    # transformers - from a padding position, a distribution conditioned on nothing - and not by score_targets.  Exactly that token:
    padding_only = labels.masked_fill(mask == 0, -100)
    theirs = SR.hf_token_logprobs(logits, padding_only)
    differs = (theirs != got)
    expect = torch.zeros_like(differs)
    for b in range(B):
        if int(first[b]) > 0 and int(labels[b, first[b]]) >= 0:
            expect[b, first[b]] = True
    assert torch.equal(differs, expect) and bool((got[expect] == 0).all()) and bool((theirs[expect] < 0).all())
    assert int(expect.sum()) == (3 if side == "left" else 0)      # rows 1 - 3 of the left-padded case, nowhere else
    with pytest.raises(ValueError):
        score_targets(labels[0])
    with pytest.raises(ValueError):
        score_targets(labels, mask[:, :-1])


def test_session_chunk_and_labels():
    pending = torch.tensor([7, 8, 9])
    inp = torch.tensor([[20, 21], [22, 23], [24, 25]])
    cont = torch.tensor([[30, 31, 32, 33], [40, 0, 41, 0], [50, 0, 0, 0]])
    cmask = torch.tensor([[1, 1, 1, 1], [1, 0, 1, 0], [1, 0, 0, 0]])
    ids, mask, labels, where = session_score_chunk(pending, inp, cont, cmask, pad_token_id=99)
    assert ids.tolist() == [[7, 20, 21, 30, 31, 32, 33], [99, 99, 8, 22, 23, 40, 41], [99, 99, 99, 9, 24, 25, 50]]
    assert mask.tolist() == [[1] * 7, [0] * 2 + [1] * 5, [0] * 3 + [1] * 4]
    assert labels.tolist() == [[-100] * 3 + [30, 31, 32, 33], [-100] * 5 + [40, 41], [-100] * 6 + [50]]
    assert where.tolist() == [[3, 4, 5, 6], [5, -1, 6, -1], [6, -1, -1, -1]]
    assert bool((mask[:, -1] == 1).all())                        # no row ends in padding: extend reads the next position off the last column
    # the shifted targets score exactly the continuation tokens, each from the position before it
    tg = score_targets(labels, mask)
    assert tg.tolist() == [[-100, -100, 30, 31, 32, 33, -100], [-100] * 4 + [40, 41, -100], [-100] * 5 + [50, -100]]
    ids0, mask0, labels0, where0 = session_score_chunk(pending[:1], None, cont[:1])
    assert ids0.tolist() == [[7, 30, 31, 32, 33]] and where0.tolist() == [[1, 2, 3, 4]] and score_targets(labels0, mask0).tolist() == [[30, 31, 32, 33, -100]]
    with pytest.raises(ValueError):
        session_score_chunk(pending[:2], inp, cont)
    with pytest.raises(ValueError):
        session_score_chunk(pending, inp, cont, torch.zeros_like(cont))
