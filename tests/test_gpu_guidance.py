"""Classifier-free guidance end to end (`Qwen2Generator.greedy` / `.sample(guidance_scale=...)`, fvhd_llm_set_guidance, include/fvhd.h "LLM
classifier-free guidance").  The oracle is a TWIN generator without guidance on the same 2 G-row batch, teacher-forced with the guided
run's tokens: a row's bits do not depend on the batch it is decoded in, so the twin's raw logits are the guided run's, and the guided
scores follow from them - in fp64 (tests/guidance_reference.py) for the choice, through the op itself for the bits, and through
transformers' own processors for the compositions."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_reference as GR  # noqa: E402
import llm_testlib as L  # noqa: E402
import logprobs_reference as LR  # noqa: E402
from llm_testlib import lib  # noqa: E402,F401
from logits_testlib import hf_chain, hf_guidance  # noqa: E402
from ml_fastvlm_amd import _lib  # noqa: E402
from ml_fastvlm_amd.constraints import TokenAutomaton  # noqa: E402
from ml_fastvlm_amd.qwen2_decode import Qwen2Generator, guidance_batch  # noqa: E402

pytestmark = pytest.mark.gpu

V = 4096
NEW = 12
TC, TU = L.GUIDANCE_TC, L.GUIDANCE_TU      # prompt and negative-prompt lengths: the negative half is left-padded by 3 more

# shared with the step-chain tests: defined once in llm_testlib
_bits, _inputs, _op = L.bits, L.guidance_inputs, L.op_guidance


@pytest.fixture(scope="module")
def small():
    return L.models("0.5B", seed=1)


def _gen(m16, rows, weights="bf16"):
    return Qwen2Generator.from_hf(m16, rows, TC + NEW, weights=weights)


def _teacher(U, batch, tokens):
    """the twin without guidance on the 2 G-row batch, fed the mirrored tokens -> its raw logits [2 G, V] per step (copies)"""
    with torch.no_grad():
        lg, _ = U.start(*batch)
        yield lg.clone()
        for i in range(1, tokens.shape[1]):
            fed = tokens[:, i - 1].contiguous()
            lg, _ = U.step(torch.cat([fed, fed]))
            yield lg.clone()


# ---- twin ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,weights,G,s", [("0.5B", "bf16", 1, 1.5), ("0.5B", "bf16", 3, 3.0), ("0.5B", "bf16", 17, 1.5), ("0.5B", "bf16", 3, -1.0),
                                             ("7B", "fp8_e4m3", 3, 1.5), ("0.5B", "mxfp4", 3, 0.5)])
def test_every_token_is_the_fp64_argmax_of_the_twins_guided_scores(lib, name, weights, G, s):
    m16, _ = L.models(name, seed=1, layers=2 if name == "7B" else None)
    e, m, ne, nm = _inputs(m16, G, seed=G)
    A, U = _gen(m16, 2 * G, weights), _gen(m16, 2 * G, weights)
    tokens = A.greedy(e, m, None, max_new_tokens=NEW, pad_token_id=0, guidance_scale=s, negative_inputs_embeds=ne, negative_attention_mask=nm)
    assert tokens.shape == (G, NEW) and A._guidance is None
    batch = guidance_batch(e, m, None, ne, nm, None)
    for i, raw in enumerate(_teacher(U, batch, tokens)):
        want = L.lowest_argmax(GR.guided_reference(raw, s))
        assert torch.equal(tokens[:, i].cpu(), want), (i, tokens[:, i].tolist(), want.tolist())


def test_the_guided_runs_kept_logits_have_the_twins_bits(lib, small):
    """start and two steps under set_guidance against the twin: rows [G, 2 G) are the twin's raw rows, rows [0, G) the op on the twin's
    logits, the ids are mirrored, and the guided rows lie within the bound of the fp64 reference"""
    m16, _ = small
    G, s = 3, 1.5
    batch = guidance_batch(*_inputs(m16, G, seed=7)[:2], None, *_inputs(m16, G, seed=7)[2:], None)
    A, U = _gen(m16, 2 * G), _gen(m16, 2 * G)
    A.set_guidance(s)
    try:
        with torch.no_grad():
            lgA, idsA = A.start(*batch)
            lgU, _ = U.start(*batch)
            for i in range(3):
                if i:
                    fed = idsA.clone()
                    assert torch.equal(fed[:G], fed[G:])
                    lgA, idsA = A.step(fed if i % 2 else None)
                    lgU, _ = U.step(fed)
                assert torch.equal(_bits(lgA[G:]), _bits(lgU[G:])), i
                guided = _op(lib, lgU, s)
                assert torch.equal(_bits(lgA[:G]), _bits(guided)), i
                assert GR.check(lgU, s, guided, f"step {i}") <= 1.0
                assert torch.equal(idsA[:G], L.lowest_argmax(guided)) and torch.equal(idsA[:G], idsA[G:]), i
    finally:
        A.set_guidance()


# ---- oracle --------------------------------------------------------------------------------------------------------------------------------
# row seeds (of `_oracle_row`, model seed 1, s = 1.5) where the CPU fp32 oracle's GUIDED top-2 margin exceeds 2 * (2 |s| + 1) * DELTA = 0.16
# at EVERY one of the 12 steps (the smallest margins over the 12 steps: 0.40, 0.40, 0.37; searched over seeds 0 .. 399, ten qualify: 6, 149,
# 155, 217, 244, 289, 304, 344, 345, 378).  A row's tokens do not depend on the batch it is generated in, so the three rows form one batch.
# There bf16 rounding - an error of up to DELTA in each log-softmax row, (2 |s| + 1) DELTA in the guided scores - cannot legitimately pick
# another token: the outputs must be equal token for token, and no step is left out.
GUIDED_SEEDS = [217, 345, 289]
ORACLE_SCALE = 1.5


def _oracle_row(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(10, V, (1, TC), generator=g), torch.randint(10, V, (1, TU), generator=g)


def test_transformers_own_generate_with_guidance_on_the_fp32_oracle(small):
    m16, ref = small
    rows = [_oracle_row(s) for s in GUIDED_SEEDS]
    ids, nids = torch.cat([r[0] for r in rows]).cuda(), torch.cat([r[1] for r in rows]).cuda()
    G, s = len(rows), ORACLE_SCALE
    delta = (2 * abs(s) + 1) * L.DELTA
    with torch.no_grad():
        out = ref.generate(inputs_embeds=ref.get_input_embeddings()(ids), attention_mask=torch.ones_like(ids), guidance_scale=s, negative_prompt_ids=nids,
                           negative_prompt_attention_mask=torch.ones_like(nids), max_new_tokens=NEW, do_sample=False, output_scores=True,
                           return_dict_in_generate=True, pad_token_id=0, eos_token_id=None)
        emb = m16.get_input_embeddings()
        ours = _gen(m16, 2 * G).greedy(emb(ids), None, None, max_new_tokens=NEW, pad_token_id=0, guidance_scale=s, negative_inputs_embeds=emb(nids))
    assert out.sequences.shape == (G, NEW) and len(out.scores) == NEW
    assert L.agree(ours, out.sequences, out.scores, delta=delta) == [NEW] * G      # every margin exceeds delta: all 12 steps compared


# ---- identical negative prompt, graph, sampling -------------------------------------------------------------------------------------------
def test_an_identical_negative_prompt_gives_plain_greedys_tokens(small):
    m16, _ = small
    G = 3
    e, m, ne, nm = _inputs(m16, G, seed=3, same=True)
    A, P = _gen(m16, 2 * G), _gen(m16, G)
    plain = P.greedy(e, m, None, max_new_tokens=NEW, pad_token_id=0)
    for s in (3.0, -1.0):
        guided = A.greedy(e, m, None, max_new_tokens=NEW, pad_token_id=0, guidance_scale=s, negative_inputs_embeds=ne, negative_attention_mask=nm)
        assert torch.equal(guided, plain), s


def test_graph_equals_eager_and_a_seed_repeats(small):
    m16, _ = small
    G = 3
    e, m, ne, nm = _inputs(m16, G, seed=4)
    A = _gen(m16, 2 * G)
    kw = dict(max_new_tokens=NEW, pad_token_id=0, guidance_scale=1.5, negative_inputs_embeds=ne, negative_attention_mask=nm)
    a = A.greedy(e, m, None, graph=True, **kw)
    b = A.greedy(e, m, None, graph=False, **kw)
    assert torch.equal(a, b) and a.shape == (G, NEW)
    assert not torch.equal(a, _gen(m16, G).greedy(e, m, None, max_new_tokens=NEW, pad_token_id=0))      # guidance changed a choice
    sa = A.sample(e, m, None, seed=5, graph=True, **kw)
    assert torch.equal(A._ids[:G], A._ids[G:2 * G])              # the drawn ids of rows g and G + g
    sb = A.sample(e, m, None, seed=5, graph=False, **kw)
    sc = A.sample(e, m, None, seed=6, graph=True, **kw)
    assert torch.equal(sa, sb) and not torch.equal(sa, sc) and A._guidance is None


# ---- composition: processors, constraint, logprobs -----------------------------------------------------------------------------------------
def _automaton():
    """4 states of 300 tokens each, wandering among themselves (no FREE edge)"""
    g = torch.Generator().manual_seed(2)
    offsets, tokens, targets = [0], [], []
    for _ in range(4):
        ids = torch.randperm(V, generator=g)[:300].sort().values.tolist()
        tokens += ids
        targets += torch.randint(0, 4, (300,), generator=g).tolist()
        offsets.append(len(tokens))
    return TokenAutomaton(offsets, tokens, targets, V)


@pytest.mark.parametrize("what", ["processors", "constraint"])
def test_transformers_own_processors_on_the_guided_scores_choose_the_same_tokens(lib, small, what):
    """UnbatchedCFG fed the twin's unconditional logits through a stub, then RepetitionPenalty and NoRepeatNGram, or PrefixConstrained, in
    transformers' order; the guided scores are the op's on the twin's logits, checked against fp64 under the bound"""
    from transformers.generation.logits_process import PrefixConstrainedLogitsProcessor
    m16, _ = small
    G, s = 3, 1.5
    e, m, ne, nm = _inputs(m16, G, seed=8)
    A, U = _gen(m16, 2 * G), _gen(m16, 2 * G)
    auto, starts = _automaton(), [0, 1, 2]
    kw = dict(repetition_penalty=1.3, no_repeat_ngram_size=2) if what == "processors" else dict(constraint=auto, constraint_start=starts)
    tokens = A.greedy(e, m, None, max_new_tokens=NEW, pad_token_id=0, guidance_scale=s, negative_inputs_embeds=ne, negative_attention_mask=nm, **kw)

    cfg, stub = hf_guidance(s, G)
    changed = 0
    for i, raw in enumerate(_teacher(U, guidance_batch(e, m, None, ne, nm, None), tokens)):
        guided = _op(lib, raw, s)
        assert GR.check(raw, s, guided, f"step {i}") <= 1.0
        hist = tokens[:, :i].cpu()
        stub.uncond = raw[G:].cpu()
        hf = cfg(hist, raw[:G].cpu().clone())                   # transformers' own fp32 guided scores: within the same bound
        assert GR.check(raw, s, hf, f"transformers step {i}") <= 1.0
        if what == "processors":
            want = hf_chain(hist, guided.cpu(), p=1.3, n=2)
        elif i == 0:                                             # (the processor cannot view an empty history: the start states' mask itself)
            want = torch.where(auto.mask(starts), guided.cpu(), torch.full_like(guided.cpu(), float("-inf")))
        else:
            fn = lambda b, sent: auto.allowed(auto.walk(starts[b], sent.tolist())[0])      # noqa: E731
            want = PrefixConstrainedLogitsProcessor(fn, num_beams=1)(hist, guided.cpu().clone())
        assert torch.equal(tokens[:, i].cpu(), L.lowest_argmax(want)), i
        changed += int(not torch.equal(tokens[:, i].cpu(), L.lowest_argmax(guided.cpu())))
    assert changed >= 1                                          # the processors really changed a choice


def test_logprobs_are_the_log_softmax_of_the_guided_scores(lib, small):
    m16, _ = small
    G, s = 3, 1.5
    e, m, ne, nm = _inputs(m16, G, seed=9)
    A, U = _gen(m16, 2 * G), _gen(m16, 2 * G)
    tokens, lp = A.greedy(e, m, None, max_new_tokens=6, pad_token_id=0, logprobs=5, guidance_scale=s, negative_inputs_embeds=ne,
                          negative_attention_mask=nm)
    assert lp.token_logprobs.shape == (G, 6) and lp.top_ids.shape == (G, 6, 5)
    for i, raw in enumerate(_teacher(U, guidance_batch(e, m, None, ne, nm, None), tokens)):
        guided = _op(lib, raw, s)
        worst = LR.check_against(guided, tokens[:, i], 5, lp.token_logprobs[:, i], lp.top_ids[:, i], lp.top_logprobs[:, i], f"step {i}")
        assert worst <= 1.0 and torch.equal(lp.top_ids[:, i, 0], tokens[:, i])


# ---- off -----------------------------------------------------------------------------------------------------------------------------------
def test_on_then_off_equals_never_on(small):
    m16, _ = small
    G = 3
    e, m, ne, nm = _inputs(m16, G, seed=10)
    A, B = _gen(m16, 2 * G), _gen(m16, 2 * G)
    A.greedy(e, m, None, max_new_tokens=4, pad_token_id=0, guidance_scale=2.0, negative_inputs_embeds=ne, negative_attention_mask=nm)
    assert A._guidance is None
    batch = guidance_batch(e, m, None, ne, nm, None)
    assert torch.equal(A.greedy(*batch, max_new_tokens=NEW, pad_token_id=0), B.greedy(*batch, max_new_tokens=NEW, pad_token_id=0))
    with torch.no_grad():
        for gen in (A, B):
            gen.start(*batch)
        la, ia = A.step(None)
        lb, ib = B.step(None)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(ia, ib)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason(lib, small):
    m16, _ = small
    e, m, ne, nm = _inputs(m16, 1, seed=11)
    batch = guidance_batch(e, m, None, ne, nm, None)
    gen = _gen(m16, 3)
    h, st = gen.pre._h, L.stream
    gen.beam_reserve()
    gen.spec_reserve(4, 8)
    gen.start(*batch)                                            # two rows, started without guidance
    gen.set_guidance(1.5)

    def refused(rc):
        assert rc != 0
        return lib.fvhd_last_error().decode()

    keep = torch.tensor([TC, TC], dtype=torch.int32, device="cuda")
    rows = torch.zeros(2, dtype=torch.long, device="cuda")
    f, sc = torch.zeros(2, V, device="cuda"), torch.zeros(1, 2, device="cuda")
    out = torch.zeros(8, device="cuda", dtype=torch.long)
    drafts = torch.zeros(3, dtype=torch.long, device="cuda")
    eos = (C.c_int32 * 1)(7)
    try:
        msg = refused(lib.fvhd_llm_cache_rewind(h, L.ptr(keep), st()))
        assert "fvhd_llm_cache_rewind: guidance is on (fvhd_llm_set_guidance)" in msg and "equal lengths" in msg
        msg = refused(lib.fvhd_llm_cache_gather(h, L.ptr(rows), 2, 2, st()))
        assert "fvhd_llm_cache_gather: guidance is on" in msg and "pairing" in msg
        assert "fvhd_llm_beam_topk: guidance is on" in refused(lib.fvhd_llm_beam_topk(h, L.ptr(f), L.ptr(sc), 1, 2, 2, L.ptr(sc), L.ptr(out), st()))
        assert "fvhd_llm_verify: guidance is on" in refused(lib.fvhd_llm_verify(h, L.ptr(drafts), 4, None, L.ptr(out), None, st()))
        assert "fvhd_llm_lookup_begin: guidance is on" in refused(lib.fvhd_llm_lookup_begin(h, None, 0, C.cast(eos, C.c_void_p), 1, 8, L.ptr(out), st()))
        assert "fvhd_llm_lookup_step: guidance is on" in refused(lib.fvhd_llm_lookup_step(h, 4, 2, st()))
        # an odd batch: the library's message, then the generator's own
        x3 = torch.cat([batch[0], batch[0][:1]])
        m3, p3 = torch.cat([batch[1], batch[1][:1]]).to(torch.uint8).contiguous(), torch.cat([batch[2], batch[2][:1]]).contiguous()
        ids3 = torch.zeros(3, dtype=torch.long, device="cuda")
        msg = refused(lib.fvhd_llm_start(h, L.ptr(x3.contiguous()), _lib.dtype_code(x3.dtype), L.ptr(m3), L.ptr(p3), 3, x3.shape[1], None, L.ptr(ids3), st()))
        assert "fvhd_llm_start: guidance is on (fvhd_llm_set_guidance) and the batch is odd (3 rows)" in msg
        with pytest.raises(ValueError, match="the batch is odd"):
            gen.start(x3, torch.cat([batch[1], batch[1][:1]]), p3)
        for call, why in ((lambda: gen.rewind([TC, TC]), "equal lengths"), (lambda: gen.cache_gather(rows, 2), "pairing"),
                          (lambda: gen.beam_search(e, m, num_beams=2, max_new_tokens=2), "beam search"),
                          (lambda: gen.lookup_greedy(e, m, max_new_tokens=4, prompt_lookup_num_tokens=3), "do not take guidance")):
            with pytest.raises(ValueError, match="guidance is set .*" + why):
                call()
        assert "finite" in refused(lib.fvhd_llm_set_guidance(h, float("nan")))
    finally:
        gen.set_guidance()
    gen.step(None)                                               # off again: the started rows decode as before
