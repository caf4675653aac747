"""tests/extend_reference.py on the CPU: the restriction of the concatenated attention against a direct computation, the rewind and
position models against hand-made cases, and the headroom of every input family of tests/test_gpu_extend_ops.py under its bound."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_reference as E  # noqa: E402
import prefill_reference as R  # noqa: E402


def test_the_reference_is_the_softmax_over_past_and_chunk():
    """rows >= P of attention_ref on the concatenation against a direct fp64 softmax written out per chunk query"""
    B, P, T, nh, nkv, hd = 2, 9, 5, 4, 2, 64
    qkv, _ = R.family("plain", B, P + T, nh, nkv, hd, seed=3)
    kvalid = torch.ones(B, P + T, dtype=torch.uint8)
    kvalid[0, :3] = 0
    kvalid[1, P + 1] = 0
    want, empty = E.attention_extend_ref(qkv, kvalid, B, P, T, nh, nkv, hd)
    q, k, v = R.split_heads(qkv, B, P + T, nh, nkv, hd)
    assert not bool(empty.any())
    for b in range(B):
        for t in range(T):
            for h in range(nh):
                vis = [j for j in range(P + t + 1) if kvalid[b, j]]
                s = torch.stack([(q[b, h, P + t].double() * k[b, h // 2, j].double()).sum() for j in vis]) / math.sqrt(hd)
                o = (torch.softmax(s, 0)[:, None] * torch.stack([v[b, h // 2, j].double() for j in vis])).sum(0)
                assert float((o - want[b, t, h]).abs().max()) <= 1e-12


def test_a_chunk_query_without_a_visible_key_is_empty_and_zero():
    B, P, T = 1, 4, 3
    qkv, _ = R.family("plain", B, P + T, 4, 2, 64, seed=4)
    kvalid = torch.zeros(B, P + T, dtype=torch.uint8)
    kvalid[0, P + 1] = 1
    want, empty = E.attention_extend_ref(qkv, kvalid, B, P, T, 4, 2, 64)
    assert empty.tolist() == [[True, False, False]] and bool((want[0, 0] == 0).all())


def test_rewind_model():
    mask = torch.tensor([[1, 1, 1, 1, 1, 1, 0, 0], [0, 0, 1, 1, 0, 1, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0]], dtype=torch.uint8)
    pos = torch.tensor([6, 3, 6])
    m, p, n, st = E.rewind_model(mask, pos, 6, [4, 3, 6])
    assert st == 0 and n == 6
    assert m.tolist() == [[1, 1, 1, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 0, 0]]
    assert p.tolist() == [4, 1, 6]                             # row 1 drops slots 3, 4, 5 of which TWO were valid
    m, p, n, st = E.rewind_model(mask, pos, 6, [2, 2, 0])
    assert st == 0 and n == 2 and p.tolist() == [2, 0, 0] and int(m[:, 2:].sum()) == 0
    for keep in ([7, 0, 0], [0, -1, 0]):
        m, p, n, st = E.rewind_model(mask, pos, 6, keep)
        assert st == 4 and n == 6 and torch.equal(m, mask) and torch.equal(p, pos)


def test_default_positions_continue_cumsum_minus_one():
    """the model against transformers' rule on the whole row: cumsum(mask) - 1 over [past | chunk], taken at the chunk's valid tokens"""
    past = torch.tensor([[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]])
    chunk = torch.tensor([[0, 1, 1, 1], [1, 1, 0, 1]])
    nxt = past.sum(1)                                           # the next position of a row = its valid tokens so far
    got = E.extend_positions_model(nxt, chunk.to(torch.uint8), 4)
    whole = torch.cat([past, chunk], 1).cumsum(1) - 1
    assert torch.equal(got[chunk != 0], whole[:, 5:][chunk != 0])
    assert got.tolist() == [[3, 3, 4, 5], [5, 6, 7, 7]]
    assert E.extend_positions_model(torch.tensor([7]), None, 3).tolist() == [[7, 8, 9]]


@pytest.mark.parametrize("hd,nh,nkv", E.HEADS + [(128, 4, 2)])
def test_every_family_leaves_headroom_under_the_attention_bound(hd, nh, nkv):
    """the GPU test's inputs through the CPU model of the kernel's arithmetic (tiles aligned to slot 0), rows >= P, against the fp64
    reference: err / bound <= 0.5 under ATT_RTOL = ATT_RMS = 2e-2 per row, for every family and every (P, T)"""
    worst = 0.0
    for P, T in E.PT:
        for i, (name, B, pad) in enumerate(E.op_families(P, T)):
            qkv, kvalid = R.family(name, B, P + T, nh, nkv, hd, seed=500 + 7 * P + T + i, pad=pad)
            want, empty = E.attention_extend_ref(qkv, kvalid, B, P, T, nh, nkv, hd)
            got = E.flash_extend_model(qkv, kvalid, B, P, T, nh, nkv, hd)
            assert bool((got[empty] == 0).all())
            bad, ratio = R._violations(got, want, R.ATT_RTOL, R.ATT_RMS, rows=~empty)
            assert bad == 0 and ratio <= 0.5, (name, P, T, ratio)
            worst = max(worst, ratio)
    print(f"extend headroom hd={hd} nh={nh}/{nkv}: worst err / bound {worst:.3f}")
