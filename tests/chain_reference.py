"""TEST INFRASTRUCTURE ONLY - the composed reference of the step's logits-to-token chain (`choose_tokens`, csrc/llm_step.hip): the
edits on the raw fp32 logits of one start / step / extend in the documented order, each from a helper the suite already trusts.

    1. guidance          the guided rows are an ARGUMENT (the op's output, or transformers' own processor's), asserted within the
                         derived bound of the fp64 reference (`guidance_reference.check`): the only edit that is not exact
    2. the processors    transformers' own RepetitionPenalty, NoRepeatNGram, MinNewTokensLength and SuppressTokens (`logits_testlib.hf_chain`)
                         on the tokens fed since the start
    3. the constraint    where(TokenAutomaton.mask(states), x, -inf) with the states behind the step's fed token

Everything behind guidance is exact in fp32, so the composed scores are compared BIT FOR BIT; the greedy id is their lowest argmax.
Plain torch and transformers on the CPU, no library.  PINNING: tests/test_chain_reference.py (against transformers' LogitsProcessorList
in `generate`'s order, and that the order shows in the scores)."""
import math
import os
import sys
from typing import NamedTuple, Optional

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_reference as GR  # noqa: E402
from llm_testlib import lowest_argmax  # noqa: E402
from logits_testlib import hf_chain  # noqa: E402


class Settings(NamedTuple):
    """what is on: guidance_scale None = off; processors: the keywords of `Qwen2Generator.set_logits_processors` or None; automaton: a
    `TokenAutomaton` or None"""
    guidance_scale: Optional[float] = None
    processors: Optional[dict] = None
    automaton: object = None


class Chain(NamedTuple):
    scores: torch.Tensor           # fp32 [R, V]: the composed scores the choice is made on (what the step keeps in rows [0, R))
    greedy: torch.Tensor           # int64 [R]: their argmax, the lowest index on ties
    states: Optional[list]         # the automaton states the rows are in behind the fed token (None without a constraint)


def hf_keywords(processors):
    """the keywords of set_logits_processors -> those of `hf_chain`"""
    p = dict(processors)
    eos = p.get("eos_token_id")
    eos = None if eos is None else ([int(eos)] if isinstance(eos, int) else [int(e) for e in eos])
    return dict(p=float(p.get("repetition_penalty", 1.0)), n=int(p.get("no_repeat_ngram_size", 0)), m=int(p.get("min_new_tokens", 0)), eos=eos,
                suppress=list(p.get("suppress_tokens") or []) or None)


def chain_reference(raw, history, states, settings, guided=None, fed=None):
    """raw: the raw fp32 logits [rows, V] of the call; under guidance rows = 2 R (row R + g the unconditional sequence of row g) and
    `guided` fp32 [R, V] holds the guided rows, else rows = R.  history: int64 [R, g], the tokens fed to rows [0, R) since the start, this
    step's included (read by the processors only).  states: the R automaton states BEFORE this call's fed token; fed: int64 [R], the token
    this step was fed, or None for a start / extend, whose rows are in the states given (their start states).  -> Chain.
    Asserts that every row keeps at least two finite scores: a row with fewer has no defined choice (an assertion about the inputs)."""
    raw = raw.detach().float().cpu()
    V = raw.shape[1]
    if settings.guidance_scale is not None:
        assert raw.shape[0] % 2 == 0 and guided is not None, "guidance: 2 R raw rows and the guided rows"
        R = raw.shape[0] // 2
        x = guided.detach().float().cpu().clone()
        assert x.shape == (R, V), (x.shape, R, V)
        assert GR.check(raw, settings.guidance_scale, x, "chain_reference: the guided rows") <= 1.0
    else:
        assert guided is None, "guided rows without a guidance scale"
        R = raw.shape[0]
        x = raw.clone()
    if settings.processors:
        hist = history.detach().cpu().long()
        assert hist.dim() == 2 and hist.shape[0] == R, (hist.shape, R)
        x = hf_chain(hist, x, **hf_keywords(settings.processors))
    after = None
    auto = settings.automaton
    if auto is not None:
        assert len(states) == R, (len(states), R)
        after = [int(s) for s in states] if fed is None else [auto.next(int(s), int(t))[0] for s, t in zip(states, fed.tolist())]
        x = torch.where(auto.mask(after), x, torch.full_like(x, -math.inf))
    assert not bool(torch.isnan(x).any())
    kept = torch.isfinite(x).sum(1)
    assert bool((kept >= 2).all()), f"rows with fewer than two finite scores after all edits: {kept.tolist()}"
    return Chain(x, lowest_argmax(x), after)
