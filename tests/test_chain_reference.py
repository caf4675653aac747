"""tests/chain_reference.py against transformers' own LogitsProcessorList in `generate`'s order (CPU, no library): the composed reference
the GPU step-chain tests compare with must itself be the documented order, and must SEE a wrong order."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_reference as CR  # noqa: E402
import guidance_reference as GR  # noqa: E402
import llm_testlib as L  # noqa: E402
from logits_testlib import hf_chain, hf_guidance  # noqa: E402

V, R, STEPS, SCALE = 4096, 3, 8, 1.5
PROCESSORS = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4, eos_token_id=5, suppress_tokens=[7, 9])


def _bits(t):
    return t.contiguous().view(torch.int32)


def _raw(gen):
    """logits of the scale of a small model's, with the EOS id and a suppressed id on top of row 1 (the unconstrained one) so that
    their bans change the choice"""
    raw = 3.0 * torch.randn(2 * R, V, generator=gen)
    raw[1, 5] = 14.0
    raw[1, 7] = 13.0
    return raw


def _hf_list(cfg, auto, starts, prefix=True):
    from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        PrefixConstrainedLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    p = PROCESSORS
    procs = [cfg, RepetitionPenaltyLogitsProcessor(p["repetition_penalty"]), NoRepeatNGramLogitsProcessor(p["no_repeat_ngram_size"]),
             MinNewTokensLengthLogitsProcessor(0, p["min_new_tokens"], [p["eos_token_id"]]), SuppressTokensLogitsProcessor(p["suppress_tokens"])]
    if prefix:
        procs.append(PrefixConstrainedLogitsProcessor(auto.prefix_allowed_tokens_fn(starts), num_beams=1))
    return LogitsProcessorList(procs)


def test_the_composition_is_generates_processor_list():
    """8 steps at 3 rows, every edit on: the scores, the ids and the states of the reference are those of transformers' list - guidance,
    repetition penalty, n-gram ban, min-new-tokens, suppressed tokens, prefix constraint - on the same history"""
    gen = torch.Generator().manual_seed(0)
    auto = L.make_automaton(sizes=L.AUTOMATON_WIDE)
    starts = L.automaton_starts(R, auto.n_states)
    settings = CR.Settings(SCALE, PROCESSORS, auto)
    cfg, stub = hf_guidance(SCALE, R)
    hist = torch.zeros(R, 0, dtype=torch.long)
    states, fed = list(starts), None
    banned_eos, changed = [], 0
    for i in range(STEPS + 1):
        raw = _raw(gen)
        stub.uncond = raw[R:]
        guided = cfg(hist, raw[:R].clone())                      # transformers' own fp32 guided rows; the reference checks them against fp64
        got = CR.chain_reference(raw, hist, states, settings, guided=guided, fed=fed)
        # (an empty history: the prefix processor of some transformers versions cannot view it - the start states' mask itself)
        want = _hf_list(cfg, auto, starts, prefix=i > 0)(hist, raw[:R].clone())
        if i == 0:
            want = torch.where(auto.mask(starts), want, torch.full_like(want, -math.inf))
        assert torch.equal(_bits(got.scores), _bits(want)), i
        assert torch.equal(got.greedy, L.lowest_argmax(want)), i
        assert got.states == [auto.walk(s, row)[0] for s, row in zip(starts, hist.tolist())], i
        banned_eos.append(bool(want[1, 5] == -math.inf))
        changed += int(not torch.equal(got.greedy, L.lowest_argmax(guided)))
        states, fed = got.states, got.greedy
        hist = torch.cat([hist, fed[:, None]], 1)
    m = PROCESSORS["min_new_tokens"]
    assert banned_eos[:m + 1] == [True] * m + [False] and changed >= 1      # the EOS ban ends where transformers ends it
    assert starts[1] == -1 and any(s != -1 for s in starts)


def test_each_subset_of_the_edits_is_its_own_sublist():
    """with an edit off the reference leaves its stage out, and nothing else"""
    gen = torch.Generator().manual_seed(1)
    auto = L.make_automaton(sizes=L.AUTOMATON_WIDE)
    starts = L.automaton_starts(R, auto.n_states)
    hist = torch.randint(10, V, (R, 5), generator=gen)
    hist[:, 3] = hist[:, 1]                                      # a repeated token: a bigram the n-gram ban acts on
    hist[:, 4] = hist[:, 0]
    raw = _raw(gen)
    cfg, stub = hf_guidance(SCALE, R)
    stub.uncond = raw[R:]
    guided = cfg(hist, raw[:R].clone())
    after = list(starts)                                         # (a start / extend: the rows are in their start states)
    seen = set()
    for gd in (False, True):
        for proc in (False, True):
            for con in (False, True):
                x = guided.clone() if gd else raw[:R].clone()
                got = CR.chain_reference(raw if gd else raw[:R], hist, starts, CR.Settings(SCALE if gd else None, PROCESSORS if proc else None,
                                                                                           auto if con else None),
                                         guided=guided if gd else None)
                if proc:
                    x = hf_chain(hist, x, **CR.hf_keywords(PROCESSORS))
                if con:
                    x = torch.where(auto.mask(after), x, torch.full_like(x, -math.inf))
                assert torch.equal(_bits(got.scores), _bits(x)) and got.states == (after if con else None), (gd, proc, con)
                seen.add(tuple(_bits(got.scores).flatten().tolist()))
    assert len(seen) == 8                                        # every edit moved a score


def test_the_order_shows_in_the_scores():
    """guidance applied BEHIND the repetition penalty gives other scores on the same input: the reference is not blind to the order it
    exists to pin"""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor
    gen = torch.Generator().manual_seed(2)
    raw = _raw(gen)
    hist = torch.randint(10, V, (R, 4), generator=gen)
    cfg, stub = hf_guidance(SCALE, R)
    stub.uncond = raw[R:]
    settings = CR.Settings(SCALE, dict(repetition_penalty=1.3), None)
    right = CR.chain_reference(raw, hist, None, settings, guided=cfg(hist, raw[:R].clone()))
    wrong = cfg(hist, RepetitionPenaltyLogitsProcessor(1.3)(hist, raw[:R].clone()))
    assert not torch.equal(_bits(right.scores), _bits(wrong))
    moved = (right.scores != wrong).sum(1)
    assert bool((moved >= hist.shape[1]).all())                  # the penalty reaches a row's log-partition: far more than the history's ids move
    assert float((right.scores - wrong).abs().max()) > 0.1       # and by far more than the bound of the guided rows


def test_the_inputs_are_checked():
    gen = torch.Generator().manual_seed(3)
    raw = _raw(gen)
    auto = L.make_automaton(sizes=L.AUTOMATON_WIDE)
    guided = GR.guided_reference(raw, SCALE).float()
    with pytest.raises(AssertionError, match="max .err. / bound"):
        CR.chain_reference(raw, None, None, CR.Settings(SCALE), guided=guided + 1e-3)
    with pytest.raises(AssertionError, match="fewer than two finite scores"):
        one = L.make_automaton(sizes=(3, 5, 40, 2000, 7, 1))      # state 5 allows one token
        CR.chain_reference(raw[:R], None, [5, 5, 5], CR.Settings(None, None, one))
    with pytest.raises(AssertionError):
        CR.chain_reference(raw, None, None, CR.Settings(None), guided=guided)
    assert CR.chain_reference(raw, None, [0] * R, CR.Settings(SCALE, None, auto), guided=guided).states == [0] * R
