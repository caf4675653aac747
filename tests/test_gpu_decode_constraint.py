"""Constrained decoding on contexts (fvhd_llm_set_constraint, Qwen2Generator.set_constraint / greedy / sample(constraint=...), include/fvhd.h
"LLM constrained decoding").  The oracle is `TokenAutomaton` on the host (its mask is pinned against transformers' processor in
tests/test_constraints.py) applied to the logits of an UNCONSTRAINED twin generator fed the same ids: every comparison is of bits or of
ids, no tolerance appears in this file."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from llm_testlib import lib  # noqa: E402,F401
from ml_fastvlm_amd import _lib  # noqa: E402
from ml_fastvlm_amd.constraints import FREE, TokenAutomaton  # noqa: E402

pytestmark = pytest.mark.gpu

V = 4096
T = 12

# shared with the step-chain tests and tools/decode_bits.py: defined once in llm_testlib
_bits = L.bits
SIZES, WIDE = L.AUTOMATON_SIZES, L.AUTOMATON_WIDE
make_automaton = L.make_automaton
_starts = L.automaton_starts
_op_logprobs = L.op_logprobs


@pytest.fixture(scope="module")
def small():
    return L.models("0.5B", seed=1)


@pytest.fixture(scope="module")
def auto():
    return make_automaton()


def _prompt_for(ref, B, T=T):
    if B <= 3:
        e, mask = L.prompt(ref, B, T, "left", seed=5, draw_on="cpu")
    else:
        e, mask = L.wide_prompt(ref, B, T, seed=5)
    return e.to(torch.bfloat16), mask


def _starts(B, n_states):
    """rows in different start states, row 1 unconstrained"""
    return [FREE if b == 1 else (b * 5 + 1) % n_states for b in range(B)]


def _masked(auto, states, raw):
    """the oracle: where(mask(states), the twin's logits, -inf) -> (its bits, the values)"""
    m = auto.mask(states).to(raw.device)
    want = torch.where(m, raw, torch.full_like(raw, -math.inf))
    return torch.where(m, _bits(raw), _bits(torch.full_like(raw, -math.inf))), want


def _gen(m16, B, cap, weights="bf16"):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    return Qwen2Generator.from_hf(m16, B, cap, weights=weights)


def _twin_run(m16, ref, auto, B, steps=9, processors=None):
    e, mask = _prompt_for(ref, B)
    A, U = _gen(m16, B, T + steps + 1), _gen(m16, B, T + steps + 1)
    starts = _starts(B, auto.n_states)
    if processors:
        A.set_logits_processors(**processors)
        U.set_logits_processors(**processors)
    A.set_constraint(auto, starts)
    changed = 0
    with torch.no_grad():
        lgA, idsA = A.start(e, mask)
        lgU, _ = U.start(e, mask)
        states = list(starts)
        for i in range(steps + 1):
            if i:
                fed = idsA.clone()
                lgA, idsA = A.step(fed if i % 2 else None)       # both sources of the fed token: the caller's ids, the previous choice
                lgU, _ = U.step(fed)
                states = [auto.next(s, int(t))[0] for s, t in zip(states, fed.tolist())]
            st, fl = A.constraint_state()
            assert st.tolist() == states and fl.tolist() == [0] * B, i      # the state after the last FED token; a chosen token never violates
            bits, want = _masked(auto, states, lgU)
            assert torch.equal(_bits(lgA), bits), i              # banned = -inf, allowed = the twin's bits
            assert torch.equal(idsA, L.lowest_argmax(want)), i
            assert all(s == FREE or int(t) in auto.allowed(s) for s, t in zip(states, idsA.tolist()))
            changed += int(not torch.equal(idsA, L.lowest_argmax(lgU)))
    assert changed >= 1                                          # the constraint really changed a choice
    assert states[1] == FREE and any(s != FREE for s in starts)
    A.set_constraint()
    A.set_logits_processors()
    return A


@pytest.mark.parametrize("B", [2, 40])
def test_twin_generators_tied_width(small, auto, B):
    _twin_run(small[0], small[1], auto, B)


def test_twin_generators_untied_7b_width(auto):
    m16, ref = L.models("7B", seed=1, layers=2)
    _twin_run(m16, ref, auto, 2)


def test_with_processors_the_mask_is_applied_to_the_processed_scores(small):
    """repetition_penalty and no_repeat_ngram_size on in both twins: the constrained logits are the mask on the processors-only twin's"""
    _twin_run(small[0], small[1], make_automaton(seed=4, sizes=WIDE), 3, processors=dict(repetition_penalty=1.3, no_repeat_ngram_size=2))


def test_graph_replay_equals_eager_and_every_row_is_accepted(small, auto):
    m16, ref = small
    B, new = 17, 12
    e, mask = _prompt_for(ref, B)
    gen = _gen(m16, B, T + new)
    starts = _starts(B, auto.n_states)
    kw = dict(max_new_tokens=new, pad_token_id=0, constraint=auto, constraint_start=starts)
    a = gen.greedy(e, mask, None, graph=True, **kw)
    b = gen.greedy(e, mask, None, graph=False, **kw)
    c = gen.greedy(e, mask, None, graph=True, **kw)
    assert torch.equal(a, b) and torch.equal(a, c)
    for s, row in zip(starts, a.tolist()):
        assert not auto.walk(s, row)[1], (s, row)
    assert gen._constraint is None
    plain = gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0)
    assert not torch.equal(plain, a)
    sa = gen.sample(e, mask, None, graph=True, seed=3, top_k=0, **kw)
    sb = gen.sample(e, mask, None, graph=False, seed=3, top_k=0, **kw)
    assert torch.equal(sa, sb)
    for s, row in zip(starts, sa.tolist()):
        assert not auto.walk(s, row)[1], (s, row)


def test_five_choices_and_eos(small):
    m16, ref = small
    B, eos, pad = 6, 7, 0
    g = torch.Generator().manual_seed(11)
    choices = [(10 + torch.randint(0, V - 10, (n,), generator=g)).tolist() for n in (1, 2, 3, 2, 3)]
    choices[3][0] = choices[2][0]                                # two choices share their first token
    a = TokenAutomaton.from_sequences(choices, V, eos_token_id=eos)
    e, mask = _prompt_for(ref, B)
    gen = _gen(m16, B, T + 8)
    for graph in (True, False):
        out = gen.greedy(e, mask, None, max_new_tokens=8, eos_token_id=eos, pad_token_id=pad, graph=graph, poll_every=3, constraint=a)
        assert out.shape[1] <= 4                                 # the longest choice and its EOS: the run stops there
        for row in out.tolist():
            n = row.index(eos)
            assert row[:n] in choices and all(t == pad for t in row[n + 1:]), row


@pytest.mark.parametrize("seed", [1, 22, 2 ** 40 + 5])
def test_sampling_draws_from_the_masked_logits(lib, small, auto, seed):
    """the id equals the sampler op's on the expected masked logits with the same seed, row and n"""
    m16, ref = small
    B, steps = 3, 8
    e, mask = _prompt_for(ref, B)
    A, U = _gen(m16, B, T + steps + 1), _gen(m16, B, T + steps + 1)
    starts = _starts(B, auto.n_states)
    temperature, top_k, top_p = 0.9, 30, 0.95
    A.set_sampling(True, temperature, top_k, top_p, seed)
    A.set_constraint(auto, starts)
    try:
        with torch.no_grad():
            lgA, idsA = A.start(e, mask)
            lgU, _ = U.start(e, mask)
            states = list(starts)
            for i in range(steps + 1):
                if i:
                    fed = idsA.clone()
                    lgA, idsA = A.step(fed)
                    lgU, _ = U.step(fed)
                    states = [auto.next(s, int(t))[0] for s, t in zip(states, fed.tolist())]
                bits, want = _masked(auto, states, lgU)
                assert torch.equal(_bits(lgA), bits), i          # the sampler reads the logits const
                ids, _ = L.sample(lib, want.contiguous(), temperature, top_k, top_p, seed=seed, n=A.length())
                assert torch.equal(idsA, ids), (i, idsA.tolist(), ids.tolist())
    finally:
        A.set_constraint()
        A.set_sampling(False)


def test_logprobs_renormalise_over_the_allowed_set(lib, small, auto):
    """logprobs=5 at a state with 3 allowed tokens (state 0 leads back to itself): three finite entries, two -inf"""
    m16, ref = small
    B, new = 3, 4
    e, mask = _prompt_for(ref, B)
    gen, U = _gen(m16, B, T + new), _gen(m16, B, T + new)
    assert len(auto.allowed(0)) == 3
    tokens, lp = gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0, logprobs=5, constraint=auto, constraint_start=0)
    with torch.no_grad():
        for i in range(new):
            lgU, _ = U.start(e, mask) if i == 0 else U.step(tokens[:, i - 1].contiguous())
            _, want = _masked(auto, [0] * B, lgU)
            tok, top, top_lp = _op_logprobs(lib, want.contiguous(), tokens[:, i].contiguous(), 5)
            assert torch.equal(_bits(lp.token_logprobs[:, i]), _bits(tok)), i
            assert torch.equal(lp.top_ids[:, i, :3], top[:, :3]) and torch.equal(_bits(lp.top_logprobs[:, i, :3]), _bits(top_lp[:, :3])), i
            assert bool(torch.isfinite(lp.top_logprobs[:, i, :3]).all()) and bool((lp.top_logprobs[:, i, 3:] == -math.inf).all()), i
            assert all(sorted(r) == auto.allowed(0) for r in lp.top_ids[:, i, :3].tolist())
            # the three probabilities sum to one (fp32 rounding of three exp: a sanity line, the bits above are the check)
            assert bool(torch.isfinite(lp.token_logprobs[:, i]).all())


def test_extend_reinitialises_the_states(small, auto):
    from ml_fastvlm_amd import GenerationSession
    m16, ref = small
    s = GenerationSession(m16, batch=2, capacity=80)
    ids1 = torch.randint(10, V, (2, 9), generator=torch.Generator().manual_seed(1)).cuda()
    ids2 = torch.randint(10, V, (2, 4), generator=torch.Generator().manual_seed(2)).cuda()
    a1 = s.generate(ids1, max_new_tokens=5, pad_token_id=0, constraint=auto, constraint_start=[2, 3])
    for st, row in zip([2, 3], a1.tolist()):
        assert not auto.walk(st, row)[1], row
    a2 = s.generate(ids2, max_new_tokens=5, pad_token_id=0, constraint=auto, constraint_start=[0, 4])      # its own start states, not where turn 1 ended
    assert all(t in auto.allowed(0) for t in a2[0].tolist()) and not auto.walk(4, a2[1].tolist())[1]
    a3 = s.generate(ids2, max_new_tokens=5, pad_token_id=0)      # an unconstrained turn: the unconstrained launches
    assert s.gen._constraint is None
    with pytest.raises(_lib.FvhdError, match="no constraint is on"):
        s.gen.constraint_state()
    assert a3.shape[0] == 2


def test_every_refusal_names_its_reason(lib, small, auto):
    m16, ref = small
    e, mask = _prompt_for(ref, 1)
    gen = _gen(m16, 1, T + 24)
    h, st = gen.pre._h, L.stream
    gen.beam_reserve()
    gen.spec_reserve(4, 8)
    gen.start(e, mask)                                           # started WITHOUT the constraint
    gen.set_constraint(auto)
    with pytest.raises(_lib.FvhdError, match="started without it"):
        gen.step(None)
    with pytest.raises(_lib.FvhdError, match="no sequence was started under the constraint"):
        gen.constraint_state()
    gen.start(e, mask)
    gen.step(None)

    def refused(rc):
        assert rc != 0
        return lib.fvhd_last_error().decode()

    keep = torch.tensor([T], dtype=torch.int32, device="cuda")
    rows = torch.zeros(1, dtype=torch.long, device="cuda")
    f = torch.zeros(1, V, device="cuda")
    out = torch.zeros(8, device="cuda", dtype=torch.long)
    sc = torch.zeros(1, 2, device="cuda")
    msg = refused(lib.fvhd_llm_cache_rewind(h, L.ptr(keep), st()))
    assert "fvhd_llm_cache_rewind: a constraint is on (fvhd_llm_set_constraint)" in msg and "not rewound" in msg
    msg = refused(lib.fvhd_llm_cache_gather(h, L.ptr(rows), 1, 1, st()))
    assert "fvhd_llm_cache_gather: a constraint is on" in msg and "not reordered" in msg
    msg = refused(lib.fvhd_llm_beam_topk(h, L.ptr(f), L.ptr(sc), 1, 2, 2, L.ptr(sc), L.ptr(out), st()))
    assert "fvhd_llm_beam_topk: a constraint is on" in msg
    drafts = torch.zeros(3, dtype=torch.long, device="cuda")
    msg = refused(lib.fvhd_llm_verify(h, L.ptr(drafts), 4, None, L.ptr(out), None, st()))
    assert "fvhd_llm_verify: a constraint is on" in msg and "does not advance" in msg
    eos = (C.c_int32 * 1)(7)
    msg = refused(lib.fvhd_llm_lookup_begin(h, None, 0, C.cast(eos, C.c_void_p), 1, 8, L.ptr(out), st()))
    assert "fvhd_llm_lookup_begin: a constraint is on" in msg
    msg = refused(lib.fvhd_llm_lookup_step(h, 4, 2, st()))
    assert "fvhd_llm_lookup_step: a constraint is on" in msg
    # the generator's own refusals, before it calls in
    for call, why in ((lambda: gen.rewind([T]), "not rewound"), (lambda: gen.cache_gather(rows, 1), "not reordered"),
                      (lambda: gen.verify(drafts), "does not advance"), (lambda: gen.beam_search(e, mask, num_beams=2, max_new_tokens=2), "beam search"),
                      (lambda: gen.lookup_greedy(e, mask, max_new_tokens=4, prompt_lookup_num_tokens=3), "does not advance")):
        with pytest.raises(ValueError, match="a constraint is set .*" + why):
            call()
    # validation, by message: the library checks what the Python class checks
    off, tok, tgt, start = (C.c_int32 * 3)(0, 2, 3), (C.c_int32 * 3)(1, 4, 0), (C.c_int32 * 3)(1, -1, 0), (C.c_int32 * 1)(0)
    p = lambda a: C.cast(a, C.c_void_p)      # noqa: E731
    assert lib.fvhd_llm_set_constraint(h, p(off), 2, p(tok), p(tgt), 3, p(start), 1) == 0
    for arrays, args, what in (
            (dict(tok=(C.c_int32 * 3)(1, V, 0)), {}, f"token {V} of edge 1 (state 0) is outside [0, vocab = {V})"),
            (dict(tgt=(C.c_int32 * 3)(1, -1, 2)), {}, "target 2 of edge 2 (state 1) is outside [-1, n_states = 2)"),
            (dict(tok=(C.c_int32 * 3)(4, 4, 0)), {}, "state 0 are not strictly ascending at edge 1"),
            (dict(off=(C.c_int32 * 3)(0, 3, 3), tok=(C.c_int32 * 3)(1, 4, 5)), {}, "state 1 has no edge"),
            (dict(off=(C.c_int32 * 3)(1, 2, 3)), {}, "offsets must start at 0"),
            (dict(off=(C.c_int32 * 3)(0, 2, 2)), {}, "offsets[n_states] = 2 is not n_edges = 3"),
            (dict(start=(C.c_int32 * 1)(2)), {}, "start state 2 of row 0"),
            ({}, dict(n_start=3), "n_start = 3 must be 1"),
            ({}, dict(n_states=(1 << 24) + 1), "exceed the limit of 16777216 states")):
        a = {**dict(off=off, tok=tok, tgt=tgt, start=start), **arrays}
        n = {**dict(n_states=2, n_edges=3, n_start=1), **args}
        msg = refused(lib.fvhd_llm_set_constraint(h, p(a["off"]), n["n_states"], p(a["tok"]), p(a["tgt"]), n["n_edges"], p(a["start"]), n["n_start"]))
        assert what in msg, (what, msg)
    # set during capture: refused by message, and the capture survives
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(gen.device)
    s.wait_stream(torch.cuda.current_stream(gen.device))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            with pytest.raises(ValueError, match="refused while a stream is being captured"):
                gen.set_constraint(auto)
            with pytest.raises(ValueError, match="refused while a stream is being captured"):
                gen.set_constraint()
    torch.cuda.current_stream(gen.device).wait_stream(s)
    gen.set_constraint()
    gen.rewind([T])                                              # off again: the calls run
    assert gen.cache_state() == (T, 0)


def test_a_captured_step_replays_the_tables_it_was_captured_with(small, auto):
    m16, ref = small
    B = 2
    e, mask = _prompt_for(ref, B)
    gen, U = _gen(m16, B, T + 8), _gen(m16, B, T + 8)
    other = make_automaton(seed=9)
    assert set(other.allowed(0)).isdisjoint(auto.allowed(0))
    gen.set_constraint(auto, 0)
    with torch.no_grad():
        _, ids = gen.start(e, mask)
        U.start(e, mask)
        fed = ids.clone()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(gen.device)
        s.wait_stream(torch.cuda.current_stream(gen.device))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                lg, out = gen.step(fed)
        torch.cuda.current_stream(gen.device).wait_stream(s)
        gen.set_constraint(other, 0)                             # tables B: A's are retired, not overwritten or freed
        g.replay()
        torch.cuda.synchronize()
        lgU, _ = U.step(fed)
        bits, want = _masked(auto, [0] * B, lgU)
        assert torch.equal(_bits(lg), bits) and torch.equal(out, L.lowest_argmax(want))
        assert all(int(t) in auto.allowed(0) for t in out.tolist())
        # an eager step now runs under tables B (state 0 of either automaton leads back to state 0)
        fed2 = out.clone()
        lg2, out2 = gen.step(fed2)
        lgU, _ = U.step(fed2)
        bits, want = _masked(other, [FREE if int(t) not in other.allowed(0) else 0 for t in fed2.tolist()], lgU)
        assert torch.equal(_bits(lg2), bits)
    assert gen.constraint_state()[1].tolist() == [1] * B          # A's tokens are not edges of B's state 0: violated, FREE
    gen.set_constraint()


def test_a_step_behind_the_error_word_writes_nothing(small, auto):
    m16, ref = small
    B = 2
    e, mask = _prompt_for(ref, B)
    gen = _gen(m16, B, T + 1)                                    # room for ONE decode step
    gen.set_constraint(auto, [2, 3])
    with torch.no_grad():
        _, ids = gen.start(e, mask)
        lg, ids = gen.step(ids.clone())
        st1, fl1 = gen.constraint_state()
        held = lg.clone()
        fed = ids.clone()
        lg.fill_(1.5)
        gen.step(fed)                                            # past the capacity: the embed sets the error word, every launch behind it returns
    assert gen.cache_state() == (T + 1, 1)
    st2, fl2 = gen.constraint_state()
    assert torch.equal(st1, st2) and torch.equal(fl1, fl2)
    assert bool((gen._logits[:B] == 1.5).all()) and held.shape == (B, V)
    gen.set_constraint()


@pytest.mark.parametrize("weights", ["fp8_e4m3", "mxfp4"])
def test_quantised_contexts_place_the_launch_the_same_way(small, auto, weights):
    m16, ref = small
    B, new = 3, 8
    e, mask = _prompt_for(ref, B)
    gen = _gen(m16, B, T + new, weights=weights)
    starts = _starts(B, auto.n_states)
    kw = dict(max_new_tokens=new, pad_token_id=0, constraint=auto, constraint_start=starts)
    a = gen.greedy(e, mask, None, graph=True, **kw)
    b = gen.greedy(e, mask, None, graph=False, **kw)
    assert torch.equal(a, b)
    for s, row in zip(starts, a.tolist()):
        assert not auto.walk(s, row)[1], (s, row)
    assert any(s != FREE for s in starts)
