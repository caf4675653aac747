"""Verify steps and prompt-lookup decoding on the library (Qwen2Generator.verify / lookup_greedy, csrc/llm_spec.hip) against the plain
greedy steps of the same generator: the same tokens under torch.equal, and every logits row with the bits of the sequential step."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import models as _models, prompt as _prompt, ptr as _p, same_bits, stream as _st  # noqa: E402

pytestmark = pytest.mark.gpu

P, NEW, CAP = 37, 21, 96          # prompt length, new tokens of the recorded greedy run, cache capacity (prompt + new + 15 drafts and room)
CASES = {"0.5B": dict(name="0.5B", layers=2), "7B": dict(name="7B", layers=1), "0.5B-e4m3": dict(name="0.5B", layers=2, quantised=True)}
_cache = {}


def _case(key):
    """per model, computed once and left unchanged: the generator, a left-padded prompt, its greedy tokens g [NEW] and the sequential
    logits seq[i] (argmax = g[i]): seq[0] from start(), seq[i] from the step() that feeds g[i - 1]"""
    if key not in _cache:
        from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
        kw = dict(CASES[key])
        quantised = kw.pop("quantised", False)
        m16, ref = _models(kw["name"], seed=1, layers=kw["layers"], quantised=quantised)
        gen = Qwen2Generator.from_hf(m16, 2, CAP, weights="fp8_e4m3" if quantised else "bf16")
        e, mask = _prompt(ref, 2, P, "left", seed=14)
        e, mask = e[1:2].to(torch.bfloat16).contiguous(), mask[1:2].contiguous()     # row 1: three padded positions on the left
        with torch.no_grad():
            g = gen.greedy(e, mask, None, max_new_tokens=NEW, pad_token_id=0)
            lg, ids = gen.start(e, mask)
            seq = [lg[0].clone()]
            for _ in range(NEW - 1):
                lg, ids = gen.step()
                seq.append(lg[0].clone())
        assert g.shape == (1, NEW) and torch.equal(torch.stack(seq).argmax(-1), g[0])
        _cache[key] = dict(model=m16, gen=gen, e=e, mask=mask, g=g[0].clone(), seq=seq)
        del ref
    return _cache[key]


def _simulate(look, g, K, max_ngram):
    """the verify steps a lookup generation of the known greedy tokens g takes when every step drafts `propose`'s K tokens"""
    from ml_fastvlm_amd.prompt_lookup import propose
    g = g.tolist()
    seq = ([] if look is None else look.reshape(-1).tolist()) + g[:1]
    written, steps = 1, 0
    while written < len(g):
        drafts = propose(seq, max_ngram, K)
        n = 0
        while n < K and written + n < len(g) and drafts[n] == g[written + n]:
            n += 1
        e = min(n + 1, len(g) - written)
        seq += g[written:written + e]
        written += e
        steps += 1
    return steps


@pytest.mark.parametrize("key", list(CASES))
@pytest.mark.parametrize("T", [2, 5, 16])
def test_every_draft_right(key, T):
    c = _case(key)
    gen, g, seq = c["gen"], c["g"], c["seq"]
    gen.spec_reserve(16)
    got = [g[:1]]
    with torch.no_grad():
        gen.start(c["e"], c["mask"])
        for k in range((NEW - 1) // T):
            lg, ids, emitted = gen.verify(g[k * T + 1:(k + 1) * T].contiguous())
            assert int(emitted) == T and gen.cache_state() == (P + (k + 1) * T, 0)
            got.append(ids.clone())
            for t in range(T):                                    # row t fed g[k T + t]: the sequential step's logits, bit for bit
                assert same_bits(lg[t], seq[k * T + t + 1]), (key, T, k, t, (lg[t] - seq[k * T + t + 1]).abs().max().item())
    got = torch.cat(got)
    assert torch.equal(got, g[:got.shape[0]]) and got.shape[0] == 1 + (NEW - 1) // T * T


@pytest.mark.parametrize("key", list(CASES))
def test_first_wrong_draft_at_j(key):
    c = _case(key)
    gen, g, seq = c["gen"], c["g"], c["seq"]
    T, V = 8, gen.pre.vocab
    gen.spec_reserve(16)
    for j in range(T):                                            # j = T - 1: no draft is wrong
        drafts = g[1:T].clone()
        if j < T - 1:
            drafts[j] = (drafts[j] + 1) % V
        with torch.no_grad():
            gen.start(c["e"], c["mask"])
            lg, ids, emitted = gen.verify(drafts)
            assert int(emitted) == j + 1 and torch.equal(ids[:j + 1], g[1:j + 2]), (key, j, ids.tolist())
            assert gen.cache_state() == (P + j + 1, 0)
            for t in range(j + 1):
                assert same_bits(lg[t], seq[t + 1]), (key, j, t)
            # a plain step afterwards feeds g[j + 1] at length P + j + 1: the k / v of the rejected drafts above the length must not leak
            lg1, ids1 = gen.step()
            assert same_bits(lg1[0], seq[j + 2]) and int(ids1) == int(g[j + 2]), (key, j)
            assert gen.cache_state() == (P + j + 2, 0)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("key", list(CASES))
def test_lookup_greedy_equals_greedy(key, graph):
    c = _case(key)
    gen, g = c["gen"], c["g"]
    V = gen.pre.vocab
    rnd = torch.randint(0, V, (50,), generator=torch.Generator().manual_seed(3)).cuda()
    with_g = torch.cat([rnd[:20], torch.tensor([-200], device="cuda"), g, rnd[20:]])[None]     # [1, n] with an image placeholder
    kw = dict(max_new_tokens=NEW, prompt_lookup_num_tokens=7, max_matching_ngram_size=2, graph=graph, poll_every=3, return_stats=True)
    with torch.no_grad():
        for look, accepted in ((None, None), (rnd, False), (with_g, True)):
            got, st = gen.lookup_greedy(c["e"], c["mask"], None, lookup_ids=look, **kw)
            print(key, "graph" if graph else "eager", "lookup ids:", None if look is None else look.numel(), st)
            assert got.shape == (1, NEW) and torch.equal(got[0], g), (key, got.tolist(), g.tolist())
            # the step count is the drafting rule's, exactly: what `propose` would have drafted against the known tokens.  (These
            # synthetic models repeat themselves, so even with no or random lookup ids some drafts from the generated tokens are right.)
            want_steps = _simulate(look, g, 7, 2)
            assert st["tokens"] == NEW and st["steps"] == want_steps <= NEW - 1, (st, want_steps)
            if accepted:
                assert st["steps"] < st["tokens"] - 1             # something was accepted
    # fewer new tokens than one step could emit: the limit cuts the run
    with torch.no_grad():
        got, st = gen.lookup_greedy(c["e"], c["mask"], None, lookup_ids=with_g, max_new_tokens=3, prompt_lookup_num_tokens=15, graph=graph,
                                    return_stats=True)
    assert torch.equal(got[0], g[:3]) and st["tokens"] == 3 and st["steps"] in (1, 2)
    assert gen.cache_state()[1] == 0


@pytest.mark.parametrize("key", ["0.5B", "7B"])
def test_lookup_greedy_stops_at_eos(key):
    c = _case(key)
    gen, g = c["gen"], c["g"]
    k = NEW // 2
    eos = [int(g[k]), int(g[NEW - 2])]
    with torch.no_grad():
        want = gen.greedy(c["e"], c["mask"], None, max_new_tokens=NEW, eos_token_id=eos, pad_token_id=0)
        for look in (None, g[None]):
            got = gen.lookup_greedy(c["e"], c["mask"], None, lookup_ids=look, max_new_tokens=NEW, prompt_lookup_num_tokens=4, eos_token_id=eos,
                                    pad_token_id=0, poll_every=2)
            assert got.shape[1] <= k + 1 and torch.equal(got, want), (got.tolist(), want.tolist())
        # the first token is an EOS id: nothing but it
        got = gen.lookup_greedy(c["e"], c["mask"], None, max_new_tokens=NEW, eos_token_id=int(g[0]))
        assert torch.equal(got[0], g[:1])


def test_capacity_and_refusals():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    c = _case("0.5B")
    g = c["g"]
    small = Qwen2Generator.from_hf(c["model"], 2, P + 4)          # a context of its own: the shared generator keeps its cache
    small.spec_reserve(8)
    with torch.no_grad():
        small.start(c["e"], c["mask"])
        lg, ids, emitted = small.verify(g[1:2].contiguous())       # 2 rows fit: P + 2 <= P + 4
        assert int(emitted) == 2 and small.cache_state() == (P + 2, 0)
        small._spec_logits.fill_(float("nan"))
        small._spec_ids.fill_(-5)
        small._spec_emitted.fill_(-5)
        small.verify(g[3:10].contiguous())                         # 8 rows: P + 2 + 8 > P + 4 - error 1, nothing written
        assert small.cache_state() == (P + 2, 1)
        assert bool(torch.isnan(small._spec_logits).all()) and bool((small._spec_ids == -5).all()) and int(small._spec_emitted) == -5
        with pytest.raises(_lib.FvhdError, match="KV cache is full"):
            small.verify(g[3:4].contiguous())
        # a draft id outside [0, vocab): error 2 on the device word and on the host word, nothing advances
        small.start(c["e"], c["mask"])
        bad = g[1:4].clone()
        bad[1] = small.pre.vocab
        small._spec_emitted.fill_(-5)
        small.verify(bad)
        assert small.cache_state() == (P, 2) and int(small._spec_emitted) == -5
        with pytest.raises(_lib.FvhdError, match="token id outside"):
            small.verify(g[1:2].contiguous())
        # a restart clears the error; the sequence decodes as before
        small.start(c["e"], c["mask"])
        lg, ids, emitted = small.verify(g[1:2].contiguous())
        assert int(emitted) == 2 and torch.equal(ids, g[1:3]) and small.cache_state() == (P + 2, 0)
        # refusals that name their reason: sampling, processors, a started batch above 1
        small.set_sampling(True, 1.0, 0, 1.0, 0)
        with pytest.raises(_lib.FvhdError, match="sampling is on"):
            small.verify(g[3:4].contiguous())
        small.set_sampling(False)
        small.set_logits_processors(repetition_penalty=1.2)
        with pytest.raises(ValueError, match="logits processors are set"):
            small.verify(g[3:4].contiguous())
        lib = _lib.lookup_lib()                                    # the library refuses the same when called directly
        assert lib.fvhd_llm_verify(small.pre._h, _p(g[3:4].contiguous()), 2, None, None, None, _st()) != 0
        assert b"logits processors are on" in lib.fvhd_last_error()
        small.set_logits_processors()
        small.start(torch.cat([c["e"], c["e"]]), torch.cat([c["mask"], c["mask"]]))
        with pytest.raises(ValueError, match="ONE sequence"):
            small.verify(g[1:2].contiguous())
        assert lib.fvhd_llm_verify(small.pre._h, _p(g[1:2].contiguous()), 2, None, None, None, _st()) != 0
        assert b"ONE sequence" in lib.fvhd_last_error()
        assert lib.fvhd_llm_lookup_step(small.pre._h, 2, 2, _st()) != 0 and b"ONE sequence" in lib.fvhd_last_error()
