"""The three new operations of the verify step (csrc/llm_spec.hip) one at a time: attention for T queries on one cache row against the
single-query op (bit for bit) and torch fp32, the device's drafter against `prompt_lookup.propose`, and the accept step's bookkeeping."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import (SENT, check, dec_attention, guard_intact, guarded, guarded_rows, lib, ptr, rel, same_bits, stream)  # noqa: E402,F401

pytestmark = pytest.mark.gpu

CAP = 320


# ---- attention for T queries -------------------------------------------------------------------------------------------------------------
def _multi(lib, q, kbuf, vbuf, ks, vs, mask, length, T, nh, nkv, hd, splits):
    """one fvhd_op_dec_attention_multi launch into a guarded output -> (out [T, nh * hd] (a copy), counters)"""
    obuf, out = guarded_rows(nh * hd, T)
    ln = torch.tensor([length], device="cuda", dtype=torch.int32)
    part = torch.empty(T * nh * splits * (hd + 2), device="cuda") if splits > 1 else None
    cnt = torch.zeros(nh, device="cuda", dtype=torch.int32) if splits > 1 else None
    check(lib.fvhd_op_dec_attention_multi(stream(), ptr(q), ptr(kbuf), ptr(vbuf), ptr(ks), ptr(vs), ptr(mask), ptr(out), T, nh, nkv, hd, CAP, ptr(ln),
                                          ptr(part), ptr(cnt), splits), "attention_multi")
    torch.cuda.synchronize()
    assert guard_intact(obuf, T * nh * hd), "rows >= T or the guard tail were written"
    assert cnt is None or int(cnt.abs().sum()) == 0, "counters not back at zero"
    return out.clone()


@pytest.mark.parametrize("T", [2, 5, 16])
@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 28, 4), (64, 4, 2)])
def test_attention_multi(lib, hd, nh, nkv, T):
    g = torch.Generator(device="cuda").manual_seed(hd * 31 + nh + T)
    rep = nh // nkv
    for length in (1, 62, 63, 255, 285):                          # the new keys straddle a 64-key block and a slice edge (5 slices of 64)
        q = torch.randn(T, nh * hd, device="cuda", generator=g).to(torch.bfloat16)
        kbuf, kc = guarded(nkv * CAP, hd, "cuda")
        vbuf, vc = guarded(nkv * CAP, hd, "cuda")
        kc.copy_(torch.randn(nkv * CAP, hd, device="cuda", generator=g))
        vc.copy_(torch.randn(nkv * CAP, hd, device="cuda", generator=g))
        ks = torch.randn(T, nkv, hd, device="cuda", generator=g).to(torch.bfloat16)
        vs = torch.randn(T, nkv, hd, device="cuda", generator=g).to(torch.bfloat16)
        npad = min(max(length // 5, 1), length - 1)              # left padding; the step's embed has set bytes [length, length + T)
        mask = torch.zeros(1, CAP, device="cuda", dtype=torch.uint8)
        mask[0, npad:length + T] = 1
        k0, v0 = kc.clone(), vc.clone()
        # the cache that already holds the T new keys: what T plain steps would have left
        kfull, vfull = k0.view(1, nkv, CAP, hd).clone(), v0.view(1, nkv, CAP, hd).clone()
        kfull[0, :, length:length + T] = ks.transpose(0, 1)
        vfull[0, :, length:length + T] = vs.transpose(0, 1)
        for splits in (1, 5):
            kc.copy_(k0)
            vc.copy_(v0)
            out = _multi(lib, q, kbuf, vbuf, ks, vs, mask, length, T, nh, nkv, hd, splits)
            # (c) slots [length, length + T) hold the staged rows, every other slot and the guard rows keep their bytes
            assert torch.equal(kc.view(nkv, CAP, hd), kfull[0]) and torch.equal(vc.view(nkv, CAP, hd), vfull[0]), (length, splits)
            assert guard_intact(kbuf, nkv * CAP) and guard_intact(vbuf, nkv * CAP)
            # (d) a second run (the staged rows are in the cache now) gives the same bits
            again = _multi(lib, q, kbuf, vbuf, ks, vs, mask, length, T, nh, nkv, hd, splits)
            assert same_bits(out, again), (length, splits)
            for t in range(T):
                # (a) row t = the single-query op at length + t + 1, bit for bit
                plain = dec_attention(lib, q[t:t + 1].contiguous(), kfull, vfull, mask, length + t + 1, splits)
                assert same_bits(out[t:t + 1], plain), (length, splits, t, rel(out[t:t + 1], plain))
            # (b) the fp32 torch expression of test_gpu_decode.py::test_dec_attention, per query
            kf = kfull[0].float().repeat_interleave(rep, 0)
            vf = vfull[0].float().repeat_interleave(rep, 0)
            s = torch.einsum("thd,hkd->thk", q.float().view(T, nh, hd), kf) * hd ** -0.5
            keys = torch.arange(CAP, device="cuda")
            seen = (mask[0] != 0)[None] & (keys[None] < length + 1 + torch.arange(T, device="cuda")[:, None])
            s = s.masked_fill(~seen[:, None], float("-inf"))
            want = torch.einsum("thk,hkd->thd", torch.softmax(s, -1), vf).reshape(T, nh * hd)
            assert rel(out, want) <= 1e-2, (length, splits, rel(out, want))


def test_attention_multi_past_the_capacity_does_nothing(lib):
    hd, nh, nkv, T = 64, 4, 2, 5
    q = torch.randn(T, nh * hd, device="cuda").to(torch.bfloat16)
    kbuf, kc = guarded(nkv * CAP, hd, "cuda")
    vbuf, vc = guarded(nkv * CAP, hd, "cuda")
    kc.zero_()
    vc.zero_()
    ks = torch.randn(T, nkv, hd, device="cuda").to(torch.bfloat16)
    mask = torch.ones(1, CAP, device="cuda", dtype=torch.uint8)
    obuf, out = guarded_rows(nh * hd, T)
    ln = torch.tensor([CAP - T + 1], device="cuda", dtype=torch.int32)
    part = torch.empty(T * nh * 5 * (hd + 2), device="cuda")
    cnt = torch.zeros(nh, device="cuda", dtype=torch.int32)
    check(lib.fvhd_op_dec_attention_multi(stream(), ptr(q), ptr(kbuf), ptr(vbuf), ptr(ks), ptr(ks), ptr(mask), ptr(out), T, nh, nkv, hd, CAP, ptr(ln),
                                          ptr(part), ptr(cnt), 5), "attention_multi")
    torch.cuda.synchronize()
    assert guard_intact(obuf, 0) and int(kc.float().abs().sum()) == 0 and int(vc.float().abs().sum()) == 0 and int(cnt.abs().sum()) == 0
    assert guard_intact(kbuf, nkv * CAP) and guard_intact(vbuf, nkv * CAP)


# ---- the drafter -----------------------------------------------------------------------------------------------------------------------
def test_lookup_draft_equals_propose(lib):
    from ml_fastvlm_amd.prompt_lookup import propose
    g = torch.Generator().manual_seed(5)
    lengths = [1, 2, 3, 255, 256, 257, 700] + [int(x) for x in torch.randint(1, 701, (193,), generator=g)]
    matched = 0
    for case, L in enumerate(lengths):
        seq = torch.randint(0, 5, (L,), generator=g, dtype=torch.int32)
        if case % 3 == 0:                                         # negative placeholders, an image token among them
            seq[torch.rand(L, generator=g) < 0.15] = -200
        max_ngram, K = case % 4 + 1, case % 15 + 1
        buf = torch.full((L + 8,), 3, dtype=torch.int32)          # the entries past the length hold matches that must not be seen
        buf[:L] = seq
        dseq = buf.cuda()
        ln = torch.tensor([L], device="cuda", dtype=torch.int32)
        out = torch.full((K + 4,), -7, device="cuda", dtype=torch.long)
        check(lib.fvhd_op_dec_lookup_draft(stream(), ptr(dseq), ptr(ln), max_ngram, K, ptr(out)), "lookup_draft")
        torch.cuda.synchronize()
        want = propose(seq.tolist(), max_ngram, K)
        assert out[:K].tolist() == want, (case, L, max_ngram, K, seq.tolist()[-8:])
        assert bool((out[K:] == -7).all())
        matched += want != [int(seq[-1])] * K
    assert matched > 100                                          # vocab 5: matches abound


# ---- the accept step -------------------------------------------------------------------------------------------------------------------
W_SEQ_LEN, W_WRITTEN, W_FINISHED, W_STEPS, W_TOKENS, W_LIMIT, W_N_EOS, W_EOS, WORDS = 0, 1, 2, 3, 4, 5, 6, 8, 24


def _accept(lib, T, n, eos_at=None, room=None, bare=False):
    """drafts right up to position n (n = T - 1: all right); eos_at: the emitted position that holds an EOS id; room: tokens left below the
    limit -> the state after the launch"""
    cap, L0, P0, SL, WR, seq_cap, out_cap = 96, 37, 41, 11, 5, 64, 48
    g = torch.Generator().manual_seed(T * 100 + n)
    ids = (torch.randperm(900, generator=g)[:T] + 10).long()     # distinct ids: an EOS id occurs once
    draft = ids[:T - 1].clone()
    if n < T - 1:
        draft[n] = ids[n] + 1
        draft[n + 1:] = torch.randint(0, 5, (T - 2 - n,), generator=g)          # what follows a wrong draft does not matter
    words = torch.zeros(WORDS, dtype=torch.int32)
    words[W_SEQ_LEN], words[W_WRITTEN], words[W_STEPS], words[W_TOKENS] = SL, WR, 3, 4
    words[W_LIMIT] = WR + (room if room is not None else 40)
    words[W_EOS:W_EOS + 16] = -1
    if eos_at is not None:
        words[W_N_EOS] = 2
        words[W_EOS], words[W_EOS + 1] = 5, int(ids[eos_at])
    seq = torch.full((seq_cap,), -9, dtype=torch.int32)
    out = torch.full((out_cap,), -9, dtype=torch.long)
    mask = torch.zeros(cap, dtype=torch.uint8)
    mask[3:L0 + T] = 1
    d = dict(ids=ids.cuda(), draft=draft.cuda(), words=None if bare else words.cuda(), seq=None if bare else seq.cuda(), out=None if bare else out.cuda(),
             emitted=torch.full((2,), -9, device="cuda", dtype=torch.int32), last=torch.tensor([77, -9], device="cuda"),
             pos=torch.tensor([P0, -9], device="cuda"), len=torch.tensor([L0, -9], device="cuda", dtype=torch.int32), mask=mask.cuda())
    check(lib.fvhd_op_dec_lookup_accept(stream(), ptr(d["draft"]), ptr(d["ids"]), T, ptr(d["words"]), ptr(d["seq"]), seq_cap, ptr(d["out"]), out_cap,
                                        ptr(d["emitted"]), ptr(d["last"]), ptr(d["pos"]), ptr(d["len"]), ptr(d["mask"]), cap), "lookup_accept")
    torch.cuda.synchronize()
    d.update(L0=L0, P0=P0, SL=SL, WR=WR, mask0=mask)
    return d


def _check_state(d, T, e, finished=None):
    ids = d["ids"].cpu()
    assert d["emitted"].tolist() == [e, -9]
    assert d["last"].tolist() == [int(ids[e - 1]), -9] and d["pos"].tolist() == [d["P0"] + e, -9] and d["len"].tolist() == [d["L0"] + e, -9]
    want = d["mask0"].clone()
    want[d["L0"] + e:d["L0"] + T] = 0                             # the bytes of the rejected drafts, cleared again
    assert torch.equal(d["mask"].cpu(), want)
    if d["words"] is not None:
        w = d["words"].tolist()
        assert (w[W_SEQ_LEN], w[W_WRITTEN], w[W_FINISHED], w[W_STEPS], w[W_TOKENS]) == (d["SL"] + e, d["WR"] + e, int(finished), 4, 4 + e)
        seq, out = d["seq"].cpu(), d["out"].cpu()
        assert seq[d["SL"]:d["SL"] + e].tolist() == ids[:e].tolist() and out[d["WR"]:d["WR"] + e].tolist() == ids[:e].tolist()
        seq[d["SL"]:d["SL"] + e] = -9
        out[d["WR"]:d["WR"] + e] = -9
        assert bool((seq == -9).all()) and bool((out == -9).all())               # nothing else was appended


@pytest.mark.parametrize("T", [2, 8, 16])
def test_lookup_accept(lib, T):
    for n in range(T):
        _check_state(_accept(lib, T, n, bare=True), T, n + 1)                     # a bare verify step: no words, nothing appended
        _check_state(_accept(lib, T, n), T, n + 1, finished=False)
        for p in sorted({0, n // 2, n}):                                          # an EOS at the first, a middle and the last emitted position
            _check_state(_accept(lib, T, n, eos_at=p), T, p + 1, finished=True)
        if n + 1 < T:                                                             # an EOS id among the rows that were not emitted: not seen
            _check_state(_accept(lib, T, n, eos_at=n + 1), T, n + 1, finished=False)
        for room in sorted({1, n + 1, n + 2}):                                    # the token limit cuts the run and finishes the generation
            _check_state(_accept(lib, T, n, room=room), T, min(n + 1, room), finished=room <= n + 1)
