"""Extending a started KV cache end to end (fvhd_llm_extend / fvhd_llm_cache_rewind, Qwen2Generator.extend / .rewind, continue_cache,
ml_fastvlm_amd.GenerationSession) against transformers.

Oracle: transformers' Qwen2ForCausalLM in fp32 on the same bf16-rounded weights, run on the CONCATENATED sequence ([past | chunk] embeddings
or ids, the concatenated mask, positions cumsum(mask) - 1) - it never sees a cache of ours.  Budgets: the last-position logits of
start + extend within what compare_prefill asks of a prefill's (rel-L2 <= 2e-2, cos >= 0.9995); greedy token streams equal wherever the
oracle's top-2 margin exceeds DELTA (`agree`)."""
import ctypes as C
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import DELTA, agree, lib, metrics, models, prompt, sample as op_sample  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
LAYERS = {"0.5B": 2, "7B": 1}


@functools.lru_cache(maxsize=None)
def _model(name, quantised=False):
    """(bf16 model, fp32 oracle, prefill context), built once per module run"""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, ref = models(name, seed=1, quantised=quantised, layers=LAYERS[name])
    return m16, ref, Qwen2Prefill.from_hf(m16, weights="fp8_e4m3" if quantised else "bf16")


def _generator(name, batch, capacity, quantised=False):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref, pre = _model(name, quantised)
    return m16, ref, Qwen2Generator.from_hf(m16, batch, capacity, prefill=pre, weights=pre.weight_format)


def _oracle(ref, e_full, mask_full, new):
    """greedy continuation of the concatenated embeddings -> (sequences [B, new], scores: new x [B, vocab]; scores[0] = the last-position logits)"""
    with torch.no_grad():
        r = ref.generate(inputs_embeds=e_full, attention_mask=mask_full, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                         output_scores=True, return_dict_in_generate=True)
    return r.sequences, r.scores


def _oracle_ids(ref, ids, new):
    with torch.no_grad():
        r = ref.generate(input_ids=ids, attention_mask=torch.ones_like(ids), max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                         output_scores=True, return_dict_in_generate=True)
    return r.sequences[:, ids.shape[1]:], r.scores


def _logits_close(got, want, what):
    rel, cos, _ = metrics(got, want)
    print(f"{what}: last-position logits rel-L2 {rel:.3e} cos {cos:.6f}")
    assert rel <= 2e-2 and cos >= 0.9995, (what, rel, cos)


CASES = [("0.5B", 1, 40, 7, False), ("0.5B", 3, 40, 7, False), ("0.5B", 1, 70, 130, False), ("0.5B", 3, 70, 130, False),
         ("7B", 1, 40, 7, False), ("7B", 3, 70, 130, False), ("0.5B", 3, 70, 130, True)]


@pytest.mark.parametrize("name,B,P,T,quantised", CASES)
def test_start_then_extend_equals_the_concatenated_sequence(name, B, P, T, quantised):
    """start(P) + extend(T), rows 1 and 2 with left padding in the prompt AND in the chunk (a hole in the middle of their key rows):
    the logits of the chunk's last position against the oracle's on [past | chunk], then 8 greedy steps token for token"""
    new = 9
    m16, ref, gen = _generator(name, B, P + T + new, quantised)
    e_past, m_past = prompt(ref, B, P, "left", seed=5)
    e_chunk, m_chunk = prompt(ref, B, T, "left", seed=6)
    want_seq, scores = _oracle(ref, torch.cat([e_past, e_chunk], 1), torch.cat([m_past, m_chunk], 1), new)
    gen.start(e_past.to(torch.bfloat16), m_past)
    lg, ids = gen.extend(e_chunk.to(torch.bfloat16), m_chunk)
    _logits_close(lg, scores[0], f"{name} B={B} start({P}) + extend({T}){' e4m3' if quantised else ''}")
    ours = [ids.clone()]
    for _ in range(new - 1):
        ours.append(gen.step(logits=False)[1].clone())
    n = agree(torch.stack(ours, 1), want_seq, scores)
    assert gen.cache_state() == (P + T + new - 1, 0) and gen.length() == P + T + new - 1
    print(f"steps compared per row: {n}")


def test_extend_twice_and_the_same_calls_give_the_same_bits():
    """start(30), extend(20), extend(20) against the oracle on all 70 positions; the same call sequence again gives torch.equal logits"""
    B, new = 3, 1
    m16, ref, gen = _generator("0.5B", B, 80)
    parts = [prompt(ref, B, n, "left", seed=20 + i) for i, n in enumerate((30, 20, 20))]
    _, scores = _oracle(ref, torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), new)
    runs = []
    for _ in range(2):
        gen.start(parts[0][0].to(torch.bfloat16), parts[0][1])
        gen.extend(parts[1][0].to(torch.bfloat16), parts[1][1])
        lg, ids = gen.extend(parts[2][0].to(torch.bfloat16), parts[2][1])
        runs.append((lg.clone(), ids.clone()))
        assert gen.cache_state() == (70, 0)
    _logits_close(runs[0][0], scores[0], "start(30) + extend(20) + extend(20)")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_rewind_then_the_same_steps_give_the_same_bits():
    """4 decode steps on explicit ids, rewind by 4, the same ids again: bit-identical logits; a row with left padding keeps its positions"""
    B, P = 3, 25
    m16, ref, gen = _generator("0.5B", B, 64)
    e, mask = prompt(ref, B, P, "left", seed=8)
    fed = torch.randint(0, 4096, (4, B), device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    gen.start(e.to(torch.bfloat16), mask)
    first = [gen.step(fed[i].contiguous())[0].clone() for i in range(4)]
    assert gen.cache_state() == (P + 4, 0)
    gen.rewind([P] * B)
    assert gen.cache_state() == (P, 0) and gen.length() == P
    again = [gen.step(fed[i].contiguous())[0].clone() for i in range(4)]
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    # a rewind per row: rows keep different lengths, the longest sets the length
    gen.rewind(torch.tensor([P + 4, P + 1, P], dtype=torch.int64))
    assert gen.cache_state() == (P + 4, 0)
    gen.rewind(torch.tensor([P + 5, P, P], device=DEV, dtype=torch.int32))
    assert gen.cache_state() == (P + 4, 4)                        # out of range: nothing changed, error word 4
    from ml_fastvlm_amd import _lib
    with pytest.raises(_lib.FvhdError, match="keep length"):
        gen.step(fed[0].contiguous())


def test_greedy_continue_cache_replayed_equals_eager():
    """greedy(continue_cache=True): the captured and replayed run equals the eager one token for token and in the final cache state, and
    both agree with the oracle; the host's length needs no synchronisation after the replays"""
    B, P, T, new = 2, 33, 9, 10
    m16, ref, gen = _generator("0.5B", B, P + T + new)
    e_past, m_past = prompt(ref, B, P, "left", seed=11)
    e_chunk, m_chunk = prompt(ref, B, T, "left", seed=12)
    want_seq, scores = _oracle(ref, torch.cat([e_past, e_chunk], 1), torch.cat([m_past, m_chunk], 1), new)
    out = []
    for graph in (True, False):
        gen.start(e_past.to(torch.bfloat16), m_past)
        toks = gen.greedy(e_chunk.to(torch.bfloat16), m_chunk, None, max_new_tokens=new, eos_token_id=None, pad_token_id=0, graph=graph,
                          continue_cache=True)
        assert gen._length == P + T + new - 1
        out.append((toks, gen.cache_state()))
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] == (P + T + new - 1, 0)
    agree(out[0][0], want_seq, scores)
    with pytest.raises(ValueError, match="need a cache of"):
        gen.greedy(e_chunk.to(torch.bfloat16), m_chunk, None, max_new_tokens=2, continue_cache=True)


def _ids(n, rows, seed):
    return torch.randint(0, 4096, (rows, n), device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def test_session_three_turns_one_row():
    """B = 1, three turns on token ids (a stock Qwen2: no vision tower): every turn agrees with the oracle's greedy continuation of the full
    concatenated ids, and the session's length is the oracle's cached length (everything but the pending token)"""
    from ml_fastvlm_amd import GenerationSession
    m16, ref, _ = _model("0.5B")
    s = GenerationSession(m16, batch=1, capacity=160)
    full = torch.zeros((1, 0), device=DEV, dtype=torch.long)
    for turn, (n_ids, new) in enumerate(((37, 6), (9, 7), (21, 5))):
        ids = _ids(n_ids, 1, 30 + turn)
        got = s.generate(ids, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
        full = torch.cat([full, ids], 1)
        want, scores = _oracle_ids(ref, full, new)
        assert got.shape == (1, new)
        agree(got, want, scores)
        full = torch.cat([full, got], 1)
        assert s.length == full.shape[1] - 1 and s.gen.cache_state() == (full.shape[1] - 1, 0)
    s.reset()
    assert s.length == 0


def test_session_three_rows_with_an_early_eos():
    """B = 3; the EOS is the id the oracle emits at step 2 of row 1, so that row finishes early and the run feeds it pad tokens while the
    others go on.  The session rewinds every row to what it really holds: the next turn agrees with the oracle for ALL rows (per row:
    its own prompt + its own answer up to its EOS + its new ids)."""
    from ml_fastvlm_amd import GenerationSession
    m16, ref, _ = _model("0.5B")
    B, new = 3, 8
    ids1 = _ids(24, B, 40)
    want1, scores1 = _oracle_ids(ref, ids1, new)
    eos = int(want1[1, 2])
    s = GenerationSession(m16, batch=B, capacity=96)
    got1 = s.generate(ids1, max_new_tokens=new, eos_token_id=eos, pad_token_id=0)
    n_b = []
    for b in range(B):
        row = got1[b].tolist()
        n_b.append(row.index(eos) + 1 if eos in row else len(row))
        agree(got1[b:b + 1, :n_b[b]], want1[b:b + 1, :n_b[b]], [sc[b:b + 1] for sc in scores1[:n_b[b]]])
    assert n_b[1] <= 3 < max(n_b), n_b                           # the planted EOS ended row 1 early (or the margin rule let it end earlier)
    assert s.length == 24 + max(n_b) - 1
    ids2 = _ids(11, B, 41)
    got2 = s.generate(ids2, max_new_tokens=6, eos_token_id=None, pad_token_id=0)
    for b in range(B):
        full = torch.cat([ids1[b:b + 1], got1[b:b + 1, :n_b[b]], ids2[b:b + 1]], 1)
        want, scores = _oracle_ids(ref, full, 6)
        agree(got2[b:b + 1], want, scores)


def test_fork_one_image_four_questions():
    """one started row forked into 4, then four different chunks: row r agrees with the B = 1 session on prefix + chunk r (the oracle's
    margins decide where a difference is allowed)"""
    from ml_fastvlm_amd import GenerationSession
    m16, ref, _ = _model("0.5B")
    prefix, new = _ids(45, 1, 50), 6
    chunks = _ids(8, 4, 51)
    s = GenerationSession(m16, batch=4, capacity=96)
    first = s.generate(prefix, max_new_tokens=1, eos_token_id=None, pad_token_id=0)
    s.fork(4)
    assert s.rows == 4 and s.length == 45
    got = s.generate(chunks, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
    for r in range(4):
        one = GenerationSession(m16, batch=1, capacity=96)
        assert torch.equal(one.generate(prefix, max_new_tokens=1, eos_token_id=None, pad_token_id=0), first)
        alone = one.generate(chunks[r:r + 1], max_new_tokens=new, eos_token_id=None, pad_token_id=0)
        want, scores = _oracle_ids(ref, torch.cat([prefix, first, chunks[r:r + 1]], 1), new)
        agree(got[r:r + 1], want, scores)
        agree(alone, want, scores)
        agree(got[r:r + 1], alone, scores)


def test_identical_chunks_in_forked_rows_give_identical_bits():
    m16, ref, gen = _generator("0.5B", 4, 80)
    e, _ = prompt(ref, 1, 50, "left", seed=60)
    c, _ = prompt(ref, 1, 13, "left", seed=61)
    gen.start(e.to(torch.bfloat16))
    gen.beam_reserve()
    gen.cache_gather(torch.zeros(4, device=DEV, dtype=torch.long), 1)
    lg, ids = gen.extend(c.to(torch.bfloat16).expand(4, -1, -1).contiguous())
    for r in range(1, 4):
        assert torch.equal(lg[r], lg[0]) and int(ids[r]) == int(ids[0])
    assert gen.cache_state() == (63, 0)


def test_sampling_on_the_extend_logits(lib):
    """sample(continue_cache=True) with a fixed seed repeats, and its first token is the sampler's choice on the extend's logits with the
    Philox counter n = the new length"""
    B, P, T, new, seed = 2, 30, 12, 6, 1234
    m16, ref, gen = _generator("0.5B", B, P + T + new)
    e_past, m_past = prompt(ref, B, P, "left", seed=70)
    e_chunk, m_chunk = prompt(ref, B, T, "left", seed=71)
    runs = []
    for _ in range(2):
        gen.start(e_past.to(torch.bfloat16), m_past)
        runs.append(gen.sample(e_chunk.to(torch.bfloat16), m_chunk, None, max_new_tokens=new, temperature=0.9, top_k=40, top_p=0.95, seed=seed,
                               eos_token_id=None, pad_token_id=0, continue_cache=True))
    assert torch.equal(runs[0], runs[1])
    gen.start(e_past.to(torch.bfloat16), m_past)
    gen.set_sampling(True, 0.9, 40, 0.95, seed)
    try:
        lg, ids = gen.extend(e_chunk.to(torch.bfloat16), m_chunk)
        lg, ids = lg.clone(), ids.clone()
    finally:
        gen.set_sampling(False)
    want, _ = op_sample(lib, lg, 0.9, 40, 0.95, seed=seed, n=P + T)
    assert torch.equal(ids, want) and torch.equal(runs[0][:, 0], want)


def test_refusals_and_the_capacity():
    from ml_fastvlm_amd import _lib
    B = 2
    m16, ref, gen = _generator("0.5B", B, 40)
    l = _lib.extend_lib()
    e, mask = prompt(ref, B, 20, "left", seed=80)
    x = e.to(torch.bfloat16)
    one = C.c_void_p(16)
    # no started sequence (a fresh cache)
    with pytest.raises(RuntimeError, match="no started sequence"):
        gen.extend(x)
    assert l.fvhd_llm_extend(gen.pre._h, _lib.ptr(x), _lib.BF16, None, None, 20, None, None, None) != 0 and b"no started sequence" in l.fvhd_last_error()
    assert l.fvhd_llm_cache_rewind(gen.pre._h, one, None) != 0 and b"no started sequence" in l.fvhd_last_error()
    gen.start(x, mask)
    # batch mismatch, chunk length
    with pytest.raises(ValueError, match="started batch is 2"):
        gen.extend(x[:1])
    assert l.fvhd_llm_extend(gen.pre._h, _lib.ptr(x), _lib.BF16, None, None, 0, None, None, None) != 0 and b"T must be >= 1" in l.fvhd_last_error()
    assert l.fvhd_llm_extend(gen.pre._h, _lib.ptr(x), _lib.BF16, None, None, 41, None, None, None) != 0 and b"exceeds the capacity" in l.fvhd_last_error()
    # processors on: Python and the library both refuse, extend and rewind
    gen.set_logits_processors(repetition_penalty=1.3)
    try:
        with pytest.raises(ValueError, match="logits processors are set"):
            gen.extend(x)
        assert l.fvhd_llm_extend(gen.pre._h, _lib.ptr(x), _lib.BF16, None, None, 20, None, None, _lib.stream_ptr(gen.device)) != 0
        assert b"logits processors are on" in l.fvhd_last_error()
        k = torch.zeros(B, device=DEV, dtype=torch.int32)
        assert l.fvhd_llm_cache_rewind(gen.pre._h, _lib.ptr(k), _lib.stream_ptr(gen.device)) != 0 and b"logits processors are on" in l.fvhd_last_error()
    finally:
        gen.set_logits_processors()
    # length + T = capacity works; one more token: nothing is written, error word 1, the next call reports it
    gen.start(x, mask)
    lg, ids = gen.extend(x, mask)
    kept = (lg.clone(), ids.clone())
    assert gen.cache_state() == (40, 0)
    gen.extend(x[:, :1].contiguous(), logits=False)
    assert gen.cache_state() == (40, 1)
    assert torch.equal(gen._ids[:B], kept[1])                     # the chosen ids were not replaced
    with pytest.raises(_lib.FvhdError, match="capacity"):
        gen.extend(x[:, :1].contiguous())
    gen.start(x, mask)                                            # a start clears the word
    assert gen.cache_state() == (20, 0)
