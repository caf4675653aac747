"""Beam search with logits processors and a constraint on the library (`Qwen2Generator.beam_search(repetition_penalty=..., constraint=...)`,
include/fvhd.h "LLM beam search with processors") against transformers' own beam search on the fp32 oracle of the same bf16-rounded weights.

The method is tests/test_gpu_beam.py's: token-for-token equality only where the oracle's decisions are clear (seeds found on the CPU,
tools/beam_processor_margins.py) and the processors BITE (the oracle without them returns other tokens); for any margins, every returned
hypothesis must carry the oracle's PROCESSED score of that very token sequence - which a history that did not follow its beam does not
survive.  With processors that are on but can never edit, the result is plain beam search's, bit for bit."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_processors_reference as R  # noqa: E402
from llm_testlib import DELTA, bits, check, models, prompt, ptr, stream, wide_prompt  # noqa: E402

from ml_fastvlm_amd.beam import BeamSearchState  # noqa: E402

pytestmark = pytest.mark.gpu

CAPACITY = 32
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
# of prompt(ref, 1, 12, "left", seed, draw_on="cpu"), model seed 1, under PROC: what `tools/beam_processor_margins.py --seeds 0-1500
# --num-beams 2` marks
CLEAR_SEEDS_K2 = [943, 988, 1367, 1466]
# four beams need the top FIVE candidates of every step clear, which is rare on a random stand-in (about one prompt in 20 000 at three new
# tokens): (model seed, prompt seed, new tokens) of what `--num-beams 4 --new-tokens 3 --model-seed 12 / 11 --seeds 0-9250` marks
CLEAR_K4 = [(12, 7389, 3), (11, 5168, 3)]
# ... under the constraint of beam_processors_reference.trie(), num_beams 3: --trie --repetition-penalty 1 / 1.3 --no-repeat-ngram-size 0
TRIE_SEEDS = [0, 3, 11]
TRIE_PENALTY_SEEDS = [12, 20]


@pytest.fixture(scope="module")
def setup():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = models("0.5B", seed=1)
    ref.generation_config.eos_token_id = None
    ref.generation_config.pad_token_id = None
    gen = Qwen2Generator.from_hf(m16, 64, CAPACITY)
    return m16, ref, gen


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


# ---- c. a neutral setting: no tolerance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("G, K", [(1, 2), (3, 4), (16, 4)])
def test_processors_that_cannot_edit_leave_plain_beam_search(setup, G, K, graph):
    """no_repeat_ngram_size above max_new_tokens never bans, an unconstrained start state never masks: the step still normalises the rows,
    runs the processor launch, carries the histories and takes the pre-normalised top-K - and returns plain beam search's tokens and scores
    under torch.equal.  (Fixed seeds; a tie that straddles a row's top-C boundary could legitimately differ - none here does.)"""
    m16, ref, gen = setup
    new = 6
    e, mask = wide_prompt(ref, G, 13, seed=40 + G) if G > 3 else prompt(ref, G, 13, "left", 40 + G)
    kw = dict(num_beams=K, max_new_tokens=new, num_return_sequences=K, pad_token_id=0, return_scores=True, graph=graph)
    plain = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    neutral = gen.beam_search(e.to(torch.bfloat16), mask, None, no_repeat_ngram_size=new + 5, **kw)
    assert same(neutral, plain), (neutral, plain)
    free = gen.beam_search(e.to(torch.bfloat16), mask, None, constraint=R.trie(), constraint_start=-1, **kw)
    assert same(free, plain)
    assert gen.cache_state()[1] == 0
    # the run restored everything: the generator refuses and enqueues as before
    assert gen._beam_scoring is False and gen._processors is None and gen._constraint is None
    assert same(gen.beam_search(e.to(torch.bfloat16), mask, None, **kw), plain)


def test_settings_outside_the_call_keep_their_refusals(setup):
    m16, ref, gen = setup
    e, mask = prompt(ref, 1, 12, "left", 3)
    gen.set_logits_processors(repetition_penalty=1.2)
    try:
        with pytest.raises(ValueError, match="not implemented under beam search"):
            gen.beam_search(e.to(torch.bfloat16), mask, None, num_beams=2, max_new_tokens=4)
        with pytest.raises(ValueError, match="their token history is not reordered"):
            gen.cache_gather(torch.zeros(2, device="cuda", dtype=torch.long), 1)
    finally:
        gen.set_logits_processors()
    with pytest.raises(ValueError):                               # a run that fails inside (a mask of the wrong shape) restores the settings too
        gen.beam_search(e.to(torch.bfloat16), mask[:, :5], None, num_beams=2, max_new_tokens=4, repetition_penalty=1.2)
    assert gen._beam_scoring is False and gen._processors is None
    plain = gen.beam_search(e.to(torch.bfloat16), mask, None, num_beams=2, max_new_tokens=4, pad_token_id=0)      # ... and plain beams run on
    assert plain.shape == (1, 4)


# ---- d. against transformers where the oracle is clear -------------------------------------------------------------------------------
def clear_case(ref, gen, seed, K, new):
    p = PROC["repetition_penalty"]
    e, mask = prompt(ref, 1, 12, "left", seed, draw_on="cpu")
    want = R.oracle(ref, e, mask, K, new, **PROC)
    margin, replayed = R.oracle_margin(want, 1, K, new)
    print(f"seed {seed} K {K}: the oracle's smallest gap among the top {K + 1} candidates {margin:.3f}")
    assert torch.equal(replayed, want.sequences)
    assert margin > 2 * DELTA * p, f"seed {seed}: margin {margin:.4f} <= {2 * DELTA * p}: not a clear case"
    assert not torch.equal(R.oracle(ref, e, mask, K, new).sequences, want.sequences), f"seed {seed}: the processors do not bite"
    kw = dict(num_beams=K, max_new_tokens=new, pad_token_id=0, return_scores=True, **PROC)
    tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    assert torch.equal(tokens, want.sequences), (tokens, want.sequences)
    assert float((scores - want.sequences_scores).abs().max()) <= DELTA * p, (scores, want.sequences_scores)
    assert same(gen.beam_search(e.to(torch.bfloat16), mask, None, graph=False, **kw), (tokens, scores))
    assert gen.cache_state()[1] == 0
    return e, mask, tokens, scores


@pytest.mark.parametrize("seed", CLEAR_SEEDS_K2)
def test_two_beams_equal_transformers_where_the_oracle_is_clear(setup, seed):
    m16, ref, gen = setup
    clear_case(ref, gen, seed, 2, 6)


@pytest.mark.parametrize("model_seed, seed, new", CLEAR_K4)
def test_four_beams_equal_transformers_where_the_oracle_is_clear(model_seed, seed, new):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = models("0.5B", seed=model_seed)
    ref.generation_config.eos_token_id = None
    ref.generation_config.pad_token_id = None
    clear_case(ref, Qwen2Generator.from_hf(m16, 4, CAPACITY), seed, 4, new)


# ---- e. every returned hypothesis carries the oracle's processed score ---------------------------------------------------------------
@pytest.mark.parametrize("lp", [0.0, 1.0])
def test_every_returned_hypothesis_has_the_oracle_processed_score_of_its_tokens(setup, lp):
    m16, ref, gen = setup
    G, K, new, pad, p = 3, 4, 10, 4095, PROC["repetition_penalty"]
    e, mask = prompt(ref, G, 14, "left", 7)
    kw = dict(num_beams=K, max_new_tokens=new, length_penalty=lp, num_return_sequences=K, pad_token_id=pad, return_scores=True, **PROC)
    plain = gen.beam_search(e.to(torch.bfloat16), mask, None, **{k: v for k, v in kw.items() if k not in PROC})
    tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    assert tokens.shape == (G * K, new) and not torch.equal(tokens, plain[0]), "the processors change nothing here"
    for r in range(G * K):                                        # no_repeat_ngram_size = 2: no bigram twice
        row = tokens[r].tolist()
        pairs = list(zip(row, row[1:]))
        assert len(set(pairs)) == len(pairs), (r, row)
    lengths = torch.full((G * K,), new, device=tokens.device)
    rows = torch.arange(G, device=tokens.device).repeat_interleave(K)
    total = R.teacher_forced_processed(ref, e[rows], mask[rows], tokens, lengths, R.hf_processors(num_beams=K, device="cuda", **PROC))
    assert bool(torch.isfinite(total).all()), "a returned token was banned on its own prefix"
    want = total / lengths.float() ** lp
    bound = DELTA * p * lengths.float() / lengths.float() ** lp   # the test_gpu_beam.py bound per token, scaled by p: the penalty multiplies
    err = (scores - want).abs()                                   # a log-probability's error
    print(f"length_penalty {lp}: max |score - oracle's processed score| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (scores, want)
    by_prompt = scores.view(G, K)
    assert bool((by_prompt[:, :-1] >= by_prompt[:, 1:]).all()), by_prompt
    assert gen.cache_state()[1] == 0


# ---- f. a constraint under beams ---------------------------------------------------------------------------------------------------
def allowed_answers():
    return {tuple(s) for s in R.TRIE_SEQUENCES}


def answers_of(tokens, eos, pad):
    out = []
    for row in tokens.tolist():
        assert eos in row, row                                    # every hypothesis ended at the EOS edge of an answer
        n = row.index(eos)
        assert all(t == pad for t in row[n + 1:]), row
        out.append(tuple(row[:n]))
    return out


@pytest.mark.parametrize("seed, penalty", [(s, 1.0) for s in TRIE_SEEDS] + [(s, 1.3) for s in TRIE_PENALTY_SEEDS])
def test_constrained_beams_return_allowed_answers_and_equal_transformers(setup, seed, penalty):
    m16, ref, gen = setup
    K, new, eos, pad = 3, 6, R.TRIE_EOS, 4095                     # (a pad id of 0 is "falsy" in transformers: it would fill with the EOS id)
    A = R.trie()
    e, mask = prompt(ref, 1, 12, "left", seed, draw_on="cpu")
    want = R.oracle(ref, e, mask, K, new, eos_token_id=eos, pad_token_id=pad, num_return_sequences=K, repetition_penalty=penalty,
                    prefix_allowed_tokens_fn=A.prefix_allowed_tokens_fn())
    margin, _ = R.oracle_margin(want, 1, K, new, eos_token_id=eos)
    assert margin > 2 * DELTA * penalty, f"seed {seed}: margin {margin:.4f}: not a clear case"
    kw = dict(num_beams=K, max_new_tokens=new, num_return_sequences=K, eos_token_id=eos, pad_token_id=pad, return_scores=True, constraint=A,
              repetition_penalty=penalty)
    tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    got = answers_of(tokens, eos, pad)
    assert all(a in allowed_answers() for a in got) and len(set(got)) == K, got
    for a in got:                                                 # ... each accepted by the automaton itself
        state, violated = A.walk(0, list(a) + [eos])
        assert state == -1 and not violated
    n = want.sequences.shape[1]
    assert torch.equal(tokens, want.sequences), (tokens, want.sequences)
    assert float((scores - want.sequences_scores).abs().max()) <= DELTA * penalty, (scores, want.sequences_scores)
    assert same(gen.beam_search(e.to(torch.bfloat16), mask, None, graph=False, **kw), (tokens, scores)) and n <= new
    assert gen._constraint is None and gen.cache_state()[1] == 0


def test_constraint_states_follow_their_beams(setup):
    """beam_search's constrained step written out on the generator's own calls, three prompts each from its own start state.  Behind EVERY
    step, row r of `constraint_state()` is where the automaton itself stands after walking, from the prompt's start state, the tokens of
    the running sequence that row r holds (all of them fed, the last by this step) - with the same violation flag.  The beams of a prompt
    diverge at once, so a state that stayed on its row, or followed the wrong parent, differs.  The finished hypotheses end in accepting
    states: the walk over an answer and its EOS edge ends FREE without a violation."""
    m16, ref, gen = setup
    G, K, new, eos, pad = 3, 3, 6, R.TRIE_EOS, 4095
    rows, dev = G * K, "cuda"
    A = R.trie()
    e, mask = prompt(ref, G, 14, "left", 5)
    starts = [0, A.next(0, 11)[0], 0]                             # the root; behind "11" (its three answers); the root
    state = BeamSearchState(G, K, gen.pre.vocab, new, num_return_sequences=K, eos_token_id=eos, pad_token_id=pad, device=dev)
    cs = torch.zeros((G, state.keep), device=dev)
    ci = torch.zeros((G, state.keep), device=dev, dtype=torch.long)
    gen.beam_reserve()
    gen._set_greedy()
    gen.set_beam_scoring(True)
    gen.set_constraint(A, starts)
    checked = moved = 0
    try:
        lg, _ = gen.start(e.to(torch.bfloat16), mask, None, logits=True)
        st0, fl0 = gen.constraint_state()
        assert st0.tolist() == starts and not bool(fl0.any())
        first = lg.repeat_interleave(K, dim=0).contiguous()
        gen.cache_gather(torch.arange(rows, device=dev) // K, G)
        gen.beam_topk(first, state.running_beam_scores, state.keep, cs, ci)
        state.update(cs, ci)
        for i in range(1, new):
            if state.finished():
                break
            moved += int((state.parent != state.identity).sum())
            gen.cache_gather(state.parent, rows)
            lg, _ = gen.step(state.fed_ids, logits=True)
            got_s, got_f = gen.constraint_state()
            seqs = state.running_sequences.view(rows, new)[:, :i].tolist()
            for r in range(rows):
                want_s, violated = A.walk(starts[r // K], seqs[r])
                assert (int(got_s[r]), bool(got_f[r] & 1)) == (want_s, violated), (i, r, seqs[r], got_s.tolist(), got_f.tolist())
                checked += 1
            gen.beam_topk(lg, state.running_beam_scores, state.keep, cs, ci)
            state.update(cs, ci)
    finally:
        gen.set_constraint()
        gen.set_beam_scoring(False)
    assert checked >= 3 * rows and moved > 0, (checked, moved)   # rows did change their parents on the way
    tokens, _ = state.result()
    prefixes = [(), (11,), ()]
    for r, a in enumerate(answers_of(tokens, eos, pad)):
        assert prefixes[r // K] + a in allowed_answers(), (r, a)
        assert A.walk(starts[r // K], list(a) + [eos]) == (-1, False)
    assert gen.cache_state()[1] == 0


# ---- g. sampled beams with processors ---------------------------------------------------------------------------------------------------
def test_sampled_beams_with_processors_repeat_under_one_seed(setup):
    m16, ref, gen = setup
    e, mask = prompt(ref, 3, 12, "left", 21)
    kw = dict(num_beams=4, max_new_tokens=6, num_return_sequences=4, pad_token_id=0, return_scores=True, do_sample=True, temperature=0.7, top_k=50,
              top_p=0.9, **PROC)
    a = gen.beam_search(e.to(torch.bfloat16), mask, None, seed=5, **kw)
    assert same(gen.beam_search(e.to(torch.bfloat16), mask, None, seed=5, graph=False, **kw), a)
    assert not torch.equal(gen.beam_search(e.to(torch.bfloat16), mask, None, seed=6, **kw)[0], a[0])
    for row in a[0].tolist():                                     # the draw never takes a banned token
        pairs = list(zip(row, row[1:]))
        assert len(set(pairs)) == len(pairs), row


def composed_zero_noise(gen, lib, e, mask, K, new, proc):
    """beam_search's processed step written out on the generator's own calls, with the SAMPLED chain at zero noise and T = 1 as its top-K"""
    G, rows, dev, V, T = e.shape[0], e.shape[0] * K, e.device, gen.pre.vocab, e.shape[1]
    state = BeamSearchState(G, K, V, new, pad_token_id=0, device=dev)
    cs = torch.zeros((G, state.keep), device=dev)
    ci = torch.zeros((G, state.keep), device=dev, dtype=torch.long)
    noise = torch.zeros((rows, V), device=dev)

    def topk(logits, n):
        check(lib.fvhd_op_dec_beam_sample_pre(stream(), ptr(logits), ptr(state.running_beam_scores), G, K, state.keep, V, 1.0, 0, 1.0, 2, 0, n, ptr(noise),
                                              None, None, ptr(cs), ptr(ci)), "fvhd_op_dec_beam_sample_pre")
        state.update(cs, ci)
    gen.beam_reserve()
    gen._set_greedy()
    gen.set_beam_scoring(True)
    gen.set_logits_processors(**proc)
    try:
        lg, _ = gen.start(e, mask, None, logits=True)
        first = lg.repeat_interleave(K, dim=0).contiguous()
        gen.cache_gather(torch.arange(rows, device=dev) // K, G)
        topk(first, T)
        for i in range(new - 1):
            gen.cache_gather(state.parent, rows)
            lg, _ = gen.step(state.fed_ids, logits=True)
            topk(lg, T + i + 1)
    finally:
        gen.set_logits_processors()
        gen.set_beam_scoring(False)
    return state.result()


@pytest.mark.parametrize("seed", CLEAR_SEEDS_K2[:2])
def test_zero_noise_at_unit_temperature_is_the_greedy_result(setup, seed):
    from ml_fastvlm_amd import _lib
    m16, ref, gen = setup
    e, mask = prompt(ref, 1, 12, "left", seed, draw_on="cpu")
    greedy = gen.beam_search(e.to(torch.bfloat16), mask, None, num_beams=2, max_new_tokens=6, pad_token_id=0, return_scores=True, **PROC)
    drawn = composed_zero_noise(gen, _lib.beam_processors_lib(), e.to(torch.bfloat16), mask, 2, 6, PROC)
    assert same(drawn, greedy), (drawn, greedy)


# ---- h. the patched generate ---------------------------------------------------------------------------------------------------------
def test_patched_generate_runs_processed_beam_search_on_the_library():
    """builder._make_library_generate(beam_search=True, beam_processors=True) on a stand-in of LlavaQwen2ForCausalLM:
    generate(num_beams=2, repetition_penalty=..., no_repeat_ngram_size=...) raises no warning and equals Qwen2Generator.beam_search on the
    same spliced inputs; without the flag it falls back with the reason it always gave"""
    from transformers import Qwen2ForCausalLM
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd import splice as S

    class StandIn(Qwen2ForCausalLM):
        def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images, image_sizes=None):
            o = S.multimodal_splice(input_ids, position_ids, attention_mask, labels, images, self.get_input_embeddings().weight, "right", None)
            return o[0], o[1], o[2], past_key_values, o[4], o[5]

        @torch.no_grad()
        def generate(self, inputs=None, images=None, image_sizes=None, **kwargs):
            raise AssertionError("the reference's generate was called")

    m16, _ = models("0.5B", seed=10)
    model = StandIn(m16.config).eval()
    model.load_state_dict(m16.state_dict())
    model = model.to("cuda", torch.bfloat16)
    orig = StandIn.generate
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(10, 4000, (2, 12), generator=g)
    ids[:, 3] = -200                                              # IMAGE_TOKEN_INDEX
    ids = ids.cuda()
    feats = (0.5 * torch.randn(2, 16, 896, generator=g)).to("cuda", torch.bfloat16)
    call = dict(images=feats, image_sizes=[(256, 256)] * 2, do_sample=False, temperature=None, num_beams=2, max_new_tokens=8, use_cache=True,
                pad_token_id=0, eos_token_id=None, **PROC)
    model.generation_config.eos_token_id = None
    try:
        StandIn.generate = builder._make_library_generate(orig, beam_search=True, beam_processors=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = model.generate(ids, **call)
        _, pos, am, _, emb, _ = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, feats)
        gen = builder.generator_context(model, 4, emb.shape[1] + 8)
        want = gen.beam_search(emb, am, pos, num_beams=2, max_new_tokens=8, pad_token_id=0, **PROC)
        plain = gen.beam_search(emb, am, pos, num_beams=2, max_new_tokens=8, pad_token_id=0)
        assert got.shape == (2, 8) and torch.equal(got, want) and not torch.equal(want, plain)
        lib_t, lib_s = builder.beam_generate(model, ids, images=feats, num_beams=2, max_new_tokens=8, pad_token_id=0, return_scores=True, **PROC)
        assert torch.equal(lib_t, want) and lib_s.shape == (2,)
        StandIn.generate = builder._make_library_generate(orig, beam_search=True)
        with pytest.warns(UserWarning, match="stays on the reference.*repetition_penalty=1.3"), pytest.raises(AssertionError, match="reference's generate"):
            model.generate(ids, **call)
    finally:
        StandIn.generate = orig
