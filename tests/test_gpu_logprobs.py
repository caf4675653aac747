"""Log-probabilities of generated tokens end to end (`greedy` / `sample(..., logprobs=n)`, fvhd_llm_set_logprobs / fvhd_llm_logprobs,
`GenerationSession.generate(logprobs=)`), on the small models of llm_testlib (vocab 4096).

Yardstick: an EAGER `start` / `extend` + `step(ids, logits=True)` loop - existing code - fed the very tokens the run produced returns the
logits of every step; tests/logprobs_reference.py applied to them (fp64) is what every `token_logprobs` / `top_*` entry must equal: ids
exactly, log-probabilities within the op test's derived bound (`logprobs_reference.logprob_bound`)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprobs_reference as LR  # noqa: E402
from llm_testlib import models, prompt  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NINF = float("-inf")
P, NEW, CAP = 21, 6, 64


@functools.lru_cache(maxsize=None)
def _model():
    return models("0.5B", seed=1, layers=2)


@functools.lru_cache(maxsize=None)
def _generator(weights="bf16", batch=17):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _model()
    return ref, Qwen2Generator.from_hf(m16, batch, CAP, weights=weights)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(x.shape == y.shape and torch.equal(x if x.dtype == torch.long else _bits(x), y if y.dtype == torch.long else _bits(y))
               for x, y in zip(a, b))


def _yardstick(gen, first, tokens):
    """the logits every token of `tokens` [B, n] was chosen from: `first()` (an eager start / extend with logits) gives column 0's, an
    eager step on column t - 1 gives column t's -> n x fp32 [B, vocab] (copies)"""
    lg, _ = first()
    out = [lg.clone()]
    for t in range(1, tokens.shape[1]):
        lg, _ = gen.step(tokens[:, t - 1].contiguous(), logits=True)
        out.append(lg.clone())
    torch.cuda.synchronize()
    return out


def _live(tokens, eos):
    """[B, n] bool: column t of row b is a real token (no EOS before it)"""
    if eos is None:
        return torch.ones_like(tokens, dtype=torch.bool)
    hit = (tokens == eos).long().cumsum(1)
    return (hit - (tokens == eos).long()) == 0


def _check_run(tokens, lp, logits_per_col, n, eos=None, what=""):
    """every column against the reference on the yardstick's logits; finished rows hold 0 / -1 / -inf -> the largest |err| / bound"""
    B, cols = tokens.shape
    assert lp.token_logprobs.shape == (B, cols) and lp.top_ids.shape == (B, cols, n) and lp.top_logprobs.shape == (B, cols, n)
    assert lp.token_logprobs.dtype == torch.float32 and lp.top_ids.dtype == torch.long and lp.top_logprobs.dtype == torch.float32
    live = _live(tokens, eos).cpu()
    worst = 0.0
    for t in range(cols):
        rows = live[:, t].nonzero()[:, 0]
        dead = (~live[:, t]).nonzero()[:, 0]
        if rows.numel():
            r = rows.to(tokens.device)
            ref = LR.Reference(logits_per_col[t][r], tokens[r, t], n)
            worst = max(worst, ref.check(n, lp.token_logprobs[r, t], lp.top_ids[r, t], lp.top_logprobs[r, t], what=f"{what} column {t}"))
        if dead.numel():
            d = dead.to(tokens.device)
            assert bool((lp.token_logprobs[d, t] == 0).all()) and bool((lp.top_ids[d, t] == -1).all()) and bool((lp.top_logprobs[d, t] == NINF).all()), \
                f"{what} column {t}: a finished row does not hold 0 / -1 / -inf"
    print(f"logprobs bound: {what} B={B} n={n}: max |err| / bound = {worst:.4f}")
    return worst


@pytest.mark.parametrize("weights,B", [("bf16", 1), ("bf16", 3), ("bf16", 17), ("fp8_e4m3", 3), ("mxfp4", 3)])
def test_greedy_logprobs_against_the_eager_loop(weights, B):
    """tokens bit-equal to greedy(); graph and eager equal bits; every entry (the first token of `start` included) is the reference's"""
    ref, gen = _generator(weights)
    e, mask = prompt(ref, B, P, "left", seed=5)
    e = e.to(torch.bfloat16)
    kw = dict(max_new_tokens=NEW, eos_token_id=None, pad_token_id=0)
    plain = gen.greedy(e, mask, None, **kw)
    assert isinstance(plain, torch.Tensor)
    tokens, lp = gen.greedy(e, mask, None, logprobs=4, **kw)
    assert torch.equal(tokens, plain) and tokens.shape == (B, NEW)
    tokens_e, lp_e = gen.greedy(e, mask, None, logprobs=4, graph=False, **kw)
    assert torch.equal(tokens_e, tokens) and _same(lp, lp_e), "graph replay and the eager run differ"
    logits = _yardstick(gen, lambda: gen.start(e, mask, None, logits=True), tokens)
    assert _check_run(tokens, lp, logits, 4, what=f"greedy {weights}") <= 1.0
    # greedy without processors: the chosen token IS the most likely one (lowest id on ties, both rules)
    assert torch.equal(lp.top_ids[:, :, 0], tokens) and torch.equal(_bits(lp.top_logprobs[:, :, 0]), _bits(lp.token_logprobs))
    assert bool((lp.token_logprobs <= 0).all()) and bool((lp.top_logprobs[:, :, :-1] >= lp.top_logprobs[:, :, 1:]).all())
    # n = 0 and n = 16: the same token_logprobs, bit for bit
    t0, lp0 = gen.greedy(e, mask, None, logprobs=0, **kw)
    t16, lp16 = gen.greedy(e, mask, None, logprobs=16, **kw)
    assert torch.equal(t0, plain) and torch.equal(t16, plain) and lp0.top_ids.shape == (B, NEW, 0) and lp0.top_logprobs.shape == (B, NEW, 0)
    assert torch.equal(_bits(lp0.token_logprobs), _bits(lp.token_logprobs)) and torch.equal(_bits(lp16.token_logprobs), _bits(lp.token_logprobs))
    assert torch.equal(lp16.top_ids[:, :, :4], lp.top_ids)
    assert _check_run(t16, lp16, logits, 16, what=f"greedy {weights}") <= 1.0


def test_sample_logprobs_are_of_the_logits_before_the_warpers():
    ref, gen = _generator()
    B = 3
    e, mask = prompt(ref, B, P, "left", seed=6)
    e = e.to(torch.bfloat16)
    kw = dict(max_new_tokens=NEW, temperature=0.7, top_k=20, top_p=0.9, seed=1234, eos_token_id=None, pad_token_id=0)
    plain = gen.sample(e, mask, None, **kw)
    tokens, lp = gen.sample(e, mask, None, logprobs=5, **kw)
    assert torch.equal(tokens, plain)
    tokens_e, lp_e = gen.sample(e, mask, None, logprobs=5, graph=False, **kw)
    assert torch.equal(tokens_e, tokens) and _same(lp, lp_e)
    logits = _yardstick(gen, lambda: gen.start(e, mask, None, logits=True), tokens)      # (greedy settings: the same logits for the same fed ids)
    assert _check_run(tokens, lp, logits, 5, what="sample") <= 1.0


def test_continue_cache_includes_the_first_token_of_extend():
    ref, gen = _generator()
    B, T = 3, 9
    e_past, m_past = prompt(ref, B, P, "left", seed=7)
    e_chunk, m_chunk = prompt(ref, B, T, "left", seed=8)
    e_past, e_chunk = e_past.to(torch.bfloat16), e_chunk.to(torch.bfloat16)
    kw = dict(max_new_tokens=NEW, eos_token_id=None, pad_token_id=0, continue_cache=True)
    gen.start(e_past, m_past)
    plain = gen.greedy(e_chunk, m_chunk, None, **kw)
    gen.start(e_past, m_past)
    tokens, lp = gen.greedy(e_chunk, m_chunk, None, logprobs=4, **kw)
    assert torch.equal(tokens, plain)
    gen.start(e_past, m_past)
    logits = _yardstick(gen, lambda: gen.extend(e_chunk, m_chunk, None, logits=True), tokens)
    assert _check_run(tokens, lp, logits, 4, what="continue_cache") <= 1.0


def test_with_processors_the_numbers_are_those_of_the_processed_scores():
    ref, gen = _generator()
    B = 3
    e, mask = prompt(ref, B, P, "left", seed=9)
    e = e.to(torch.bfloat16)
    kw = dict(max_new_tokens=NEW, eos_token_id=None, pad_token_id=0)
    _, lp_plain = gen.greedy(e, mask, None, logprobs=5, **kw)
    sup = sorted(set(lp_plain.top_ids[:, 0, :2].flatten().tolist()))       # the two most likely first tokens of every row: they matter
    proc = dict(repetition_penalty=1.3, suppress_tokens=sup)
    plain = gen.greedy(e, mask, None, **kw, **proc)
    tokens, lp = gen.greedy(e, mask, None, logprobs=5, **kw, **proc)
    assert torch.equal(tokens, plain) and gen._processors is None
    assert not bool(torch.isin(lp.top_ids, torch.tensor(sup, device=DEV)).any()), "a suppressed token is among the top ids"
    assert bool(torch.isfinite(lp.top_logprobs).all()) and bool(torch.isfinite(lp.token_logprobs).all())
    gen.set_logits_processors(**proc)
    try:
        logits = _yardstick(gen, lambda: gen.start(e, mask, None, logits=True), tokens)   # the processed scores (set_logits_processors)
    finally:
        gen.set_logits_processors()
    assert all(bool((lg[:, sup] == NINF).all()) for lg in logits)
    assert _check_run(tokens, lp, logits, 5, what="processors") <= 1.0
    assert not torch.equal(_bits(lp.token_logprobs), _bits(lp_plain.token_logprobs))


def test_a_row_that_finishes_early_holds_zero_minus_one_minus_inf():
    ref, gen = _generator()
    B, new = 3, 8
    e, mask = prompt(ref, B, P, "left", seed=10)
    e = e.to(torch.bfloat16)
    free = gen.greedy(e, mask, None, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
    eos = int(free[1, 2])                                        # row 1 ends at its third token (or earlier)
    kw = dict(max_new_tokens=new, eos_token_id=eos, pad_token_id=0)
    plain = gen.greedy(e, mask, None, **kw)
    tokens, lp = gen.greedy(e, mask, None, logprobs=3, **kw)
    assert torch.equal(tokens, plain)
    live = _live(tokens, eos)
    n_b = live.sum(1)
    assert int(n_b[1]) <= 3 < int(n_b.max()), n_b.tolist()
    logits = _yardstick(gen, lambda: gen.start(e, mask, None, logits=True), tokens)
    assert _check_run(tokens, lp, logits, 3, eos=eos, what="early eos") <= 1.0
    real = torch.where(live, lp.token_logprobs, torch.zeros_like(lp.token_logprobs)).sum(1)
    assert torch.equal(_bits(lp.token_logprobs.sum(1)), _bits(real)), "sum(1) is not the sum over the row's real tokens"


def test_the_setting_is_off_after_a_run_and_the_refusals():
    from ml_fastvlm_amd import _lib
    ref, gen = _generator()
    B = 3
    e, mask = prompt(ref, B, P, "left", seed=11)
    e = e.to(torch.bfloat16)
    gen.greedy(e, mask, None, max_new_tokens=3, eos_token_id=None, pad_token_id=0, logprobs=2)
    assert isinstance(gen.greedy(e, mask, None, max_new_tokens=3, eos_token_id=None, pad_token_id=0), torch.Tensor)
    tok = torch.zeros((B,), device=DEV)
    ti, tl = torch.zeros((B, 17), device=DEV, dtype=torch.long), torch.zeros((B, 17), device=DEV)
    with pytest.raises(_lib.FvhdError, match="is off"):
        gen.logprobs(0, tok)                                     # NULL logits with the setting off
    lg, _ = gen.start(e, mask, None, logits=True)
    gen.logprobs(2, tok, ti[:, :2].contiguous(), tl[:, :2].contiguous(), logits=lg)      # the caller's logits: allowed with the setting off
    gen.set_logprobs(True)
    try:
        with pytest.raises(_lib.FvhdError, match="did not leave its logits"):
            gen.logprobs(0, tok)                                 # the last call wrote the caller's buffer
        gen.start(e, mask, None, logits=False)
        gen.logprobs(0, tok)
        with pytest.raises(_lib.FvhdError, match=r"\[0, 16\]"):
            gen.logprobs(17, tok, ti, tl)
        gen.rewind([P - 1] * B)
        with pytest.raises(_lib.FvhdError, match="rewind"):
            gen.logprobs(0, tok)
    finally:
        gen.set_logprobs(False)
    torch.cuda.synchronize()


def test_a_session_returns_one_generation_logprobs_per_turn():
    from ml_fastvlm_amd import GenerationLogprobs, GenerationSession
    m16, _ = _model()
    s = GenerationSession(m16, batch=1, capacity=96)
    g = torch.Generator(device=DEV).manual_seed(12)
    for n_ids, new in ((19, 5), (7, 4)):
        ids = torch.randint(0, 4096, (1, n_ids), device=DEV, generator=g)
        tokens, lp = s.generate(ids, max_new_tokens=new, eos_token_id=None, pad_token_id=0, logprobs=2)
        assert isinstance(lp, GenerationLogprobs) and tokens.shape == (1, new)
        assert lp.token_logprobs.shape == (1, new) and lp.top_ids.shape == (1, new, 2) and lp.top_logprobs.shape == (1, new, 2)
        assert torch.equal(lp.top_ids[:, :, 0], tokens) and bool((lp.token_logprobs <= 0).all()) and bool(torch.isfinite(lp.top_logprobs).all())
