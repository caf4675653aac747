"""Beam-search sampling on the library (`Qwen2Generator.beam_search(do_sample=True)`, csrc/llm_beam.hip): graph replay against the eager run and
against the step written out here (step -> fvhd_op_dec_beam_sample at that cache length -> BeamSearchState.update -> cache_gather), and -
whatever the draws were - every returned hypothesis against the fp32 oracle's teacher-forced score of that very token sequence, with every
chosen token inside the oracle's kept set (or within DELTA of its threshold): a wrong reorder or wrong bookkeeping does not survive that."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_sample_reference as R  # noqa: E402
from llm_testlib import DELTA, bits, check, models, prompt, ptr, stream  # noqa: E402

from ml_fastvlm_amd.beam import BeamSearchState  # noqa: E402

pytestmark = pytest.mark.gpu

CAPACITY, NEW, T_PROMPT = 32, 6, 12


@pytest.fixture(scope="module")
def setup():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = models("0.5B", seed=1)
    gen = Qwen2Generator.from_hf(m16, 64, CAPACITY)
    return ref, gen, _lib.beam_sample_lib()


def composed(gen, e, mask, K, new, topk, **state_kw):
    """beam_search's step written out: topk(logits, running scores, keep, out scores, out index, n) is the only part that differs"""
    G, rows, dev = e.shape[0], e.shape[0] * K, e.device
    state = BeamSearchState(G, K, gen.pre.vocab, new, device=dev, **state_kw)
    cand_v = torch.zeros((G, state.keep), device=dev)
    cand_i = torch.zeros((G, state.keep), device=dev, dtype=torch.long)
    gen.beam_reserve()
    gen.set_sampling(False)
    lg, _ = gen.start(e.to(torch.bfloat16), mask, None, logits=True)
    logits = lg.repeat_interleave(K, dim=0).contiguous()
    gen.cache_gather(torch.arange(rows, device=dev) // K, G)
    topk(logits, state.running_beam_scores, state.keep, cand_v, cand_i, gen.cache_state()[0])
    state.update(cand_v, cand_i)
    for _ in range(new - 1):
        gen.cache_gather(state.parent, rows)
        logits, _ = gen.step(state.fed_ids, logits=True)
        topk(logits, state.running_beam_scores, state.keep, cand_v, cand_i, gen.cache_state()[0])
        state.update(cand_v, cand_i)
    return state.result()


def op_topk(lib, T, top_k, top_p, m, seed):
    def topk(logits, scores, keep, out_v, out_i, n):
        G, K = scores.shape
        check(lib.fvhd_op_dec_beam_sample(stream(), ptr(logits), ptr(scores), G, K, keep, logits.shape[1], T, top_k, top_p, m, seed, n, None, None, None,
                                          ptr(out_v), ptr(out_i)), "fvhd_op_dec_beam_sample")
    return topk


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("K", [2, 4])
def test_graph_replay_equals_the_eager_run_and_the_composed_step(setup, K, G):
    ref, gen, lib = setup
    e, mask = prompt(ref, G, T_PROMPT, "left", 21 + G)
    kw = dict(num_beams=K, max_new_tokens=NEW, num_return_sequences=K, pad_token_id=0, return_scores=True, do_sample=True, temperature=0.7, top_k=50,
              top_p=0.95, seed=1234 + K)
    tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    assert gen.cache_state() == (T_PROMPT + NEW - 1, 0)
    eager_t, eager_s = gen.beam_search(e.to(torch.bfloat16), mask, None, graph=False, **kw)
    assert torch.equal(eager_t, tokens) and torch.equal(bits(eager_s), bits(scores))
    want_t, want_s = composed(gen, e, mask, K, NEW, op_topk(lib, 0.7, 50, 0.95, 2, 1234 + K), num_return_sequences=K, pad_token_id=0)
    assert torch.equal(want_t, tokens) and torch.equal(bits(want_s), bits(scores))
    assert tokens.shape == (G * K, NEW) and bool(torch.isfinite(scores).all())


def test_two_seeds_draw_different_tokens_and_one_seed_repeats(setup):
    ref, gen, _ = setup
    e, mask = prompt(ref, 3, T_PROMPT, "left", 5)
    kw = dict(num_beams=4, max_new_tokens=NEW, num_return_sequences=4, pad_token_id=0, do_sample=True, temperature=1.0, top_k=0)
    a = gen.beam_search(e.to(torch.bfloat16), mask, None, seed=1, **kw)
    b = gen.beam_search(e.to(torch.bfloat16), mask, None, seed=2, **kw)
    c = gen.beam_search(e.to(torch.bfloat16), mask, None, seed=1, **kw)
    assert not torch.equal(a, b) and torch.equal(a, c)
    torch.manual_seed(11)                                         # seed None: from torch's generator, as in `sample`
    d = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    torch.manual_seed(11)
    assert torch.equal(gen.beam_search(e.to(torch.bfloat16), mask, None, **kw), d)


def test_top_k_one_runs_because_min_keep_takes_over(setup):
    ref, gen, _ = setup
    e, mask = prompt(ref, 3, T_PROMPT, "left", 6)
    kw = dict(num_beams=4, max_new_tokens=NEW, pad_token_id=0, return_scores=True, do_sample=True, temperature=0.5, top_k=1, seed=3)
    tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    assert tokens.shape == (3, NEW) and gen.cache_state() == (T_PROMPT + NEW - 1, 0) and bool(torch.isfinite(scores).all())
    eager_t, eager_s = gen.beam_search(e.to(torch.bfloat16), mask, None, graph=False, **kw)
    assert torch.equal(eager_t, tokens) and torch.equal(bits(eager_s), bits(scores))


def oracle_positions(ref, e, mask, tokens):
    """the oracle's logits at the positions that chose tokens[r, i], teacher-forced on the prompt row r and tokens[r, :i] -> fp32 [rows, n, V]"""
    n = tokens.shape[1]
    x = torch.cat((e, ref.get_input_embeddings()(tokens.clamp(min=0))), dim=1)
    am = torch.cat((mask, torch.ones_like(tokens)), dim=1)
    pos = (am.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        return ref(inputs_embeds=x, attention_mask=am, position_ids=pos).logits[:, -n - 1:-1].float()


@pytest.mark.parametrize("n_eos", [0, 1, 3])
@pytest.mark.parametrize("T,lp", [(1.0, 1.0), (0.2, 0.0)])
def test_every_returned_hypothesis_has_the_oracle_score_of_its_tokens(setup, T, lp, n_eos):
    ref, gen, _ = setup
    G, K, pad, top_k = 3, 4, 4095, 50
    e, mask = prompt(ref, G, T_PROMPT, "left", 7)
    kw = dict(num_beams=K, max_new_tokens=NEW, length_penalty=lp, num_return_sequences=K, pad_token_id=pad, return_scores=True, do_sample=True,
              temperature=T, top_k=top_k, seed=77)
    free, _ = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    # EOS ids from the EOS-free run: tokens its hypotheses took at their second and third positions - the finished-beam path runs
    eos = [int(free[0, 1]), int(free[K, 2]), int(free[2 * K, 1])][:n_eos]
    m = max(2, n_eos + 1)
    tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, eos_token_id=eos or None, **kw)
    assert gen.cache_state()[1] == 0
    assert tokens.shape[0] == G * K and scores.shape == (G * K,) and tokens.shape[1] <= NEW
    assert BeamSearchState(G, K, gen.pre.vocab, NEW, eos_token_id=eos or None).keep == (1 + max(1, n_eos)) * K
    n = tokens.shape[1]
    lengths = torch.full((G * K,), n, device=tokens.device)
    if eos:
        hit = torch.isin(tokens, torch.tensor(eos, device=tokens.device))
        lengths = torch.where(hit.any(-1), hit.float().argmax(-1) + 1, lengths)
        if lp == 0.0:                                             # (dividing by the length may rank every early ending below the full-length ones)
            assert bool((lengths < NEW).any()), "no hypothesis ended at an EOS id"
        for r in range(G * K):                                    # finished rows are padded, as in the greedy search
            assert bool((tokens[r, int(lengths[r]):] == pad).all()), (r, tokens[r])
    rows = torch.arange(G, device=tokens.device).repeat_interleave(K)
    x = oracle_positions(ref, e[rows], mask[rows], tokens)       # [G K, n, V]
    live = torch.arange(n, device=tokens.device)[None, :] < lengths[:, None]
    logp = torch.log_softmax(x, dim=-1)
    tok = torch.gather(logp, 2, tokens.clamp(min=0)[:, :, None])[:, :, 0]
    Tf = float(torch.tensor(T, dtype=torch.float32))
    want = (tok * live).sum(-1) / Tf / lengths.float() ** lp
    bound = lengths.float() * DELTA / Tf / lengths.float() ** lp
    err = (scores - want).abs()
    # every chosen token lies in the oracle's kept set, or within DELTA (as a logit) of its threshold
    s = (x.double() / Tf).reshape(-1, x.shape[-1])
    _, theta = R.kept_set(s, top_k, 1.0, m)
    chosen = torch.gather(s, 1, tokens.clamp(min=0).reshape(-1, 1))[:, 0]
    slack = (theta - chosen).reshape(G * K, n)[live]
    print(f"T {T} length_penalty {lp} eos {eos}: max |score - oracle| / bound {float((err / bound).max()):.3f}, lengths {lengths.tolist()}, "
          f"largest (threshold - chosen) * T / DELTA {float(slack.max()) * Tf / DELTA:.3f}")
    assert bool((err <= bound).all()), (scores, want)
    assert float(slack.max()) * Tf <= DELTA
    by_prompt = scores.view(G, K)
    assert bool((by_prompt[:, :-1] >= by_prompt[:, 1:]).all()), by_prompt


def test_with_sampling_off_beam_search_returns_the_bits_it_returned(setup):
    ref, gen, _ = setup
    for G, K in ((1, 2), (3, 4)):
        e, mask = prompt(ref, G, T_PROMPT, "left", 9)

        def topk(logits, scores, keep, out_v, out_i, n):
            gen.beam_topk(logits, scores, keep, out_v, out_i)
        want_t, want_s = composed(gen, e, mask, K, NEW, topk, num_return_sequences=K, pad_token_id=0)
        kw = dict(num_beams=K, max_new_tokens=NEW, num_return_sequences=K, pad_token_id=0, return_scores=True)
        for extra in (dict(), dict(do_sample=False, temperature=0.3, top_k=3, top_p=0.5, seed=9)):      # the settings are not read
            tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw, **extra)
            assert torch.equal(tokens, want_t) and torch.equal(bits(scores), bits(want_s))


def test_refusals_on_the_device(setup):
    ref, gen, lib = setup
    e, mask = prompt(ref, 2, T_PROMPT, "left", 3)
    with pytest.raises(ValueError, match="temperature"):
        gen.beam_search(e.to(torch.bfloat16), mask, None, num_beams=2, max_new_tokens=4, do_sample=True, temperature=0.0)
    gen.beam_sample_reserve()
    lg = torch.zeros(4, gen.pre.vocab, device="cuda")
    sc, ov, oi = torch.zeros(2, 2, device="cuda"), torch.zeros(2, 4, device="cuda"), torch.zeros(2, 4, device="cuda", dtype=torch.long)
    with pytest.raises(ValueError, match="min_keep"):
        gen.beam_sample_topk(lg, sc, 4, ov, oi, min_keep=5)
    with pytest.raises(ValueError, match="expected a contiguous"):
        gen.beam_sample_topk(lg[:, :64], sc, 4, ov, oi)
    h = gen.pre._h
    assert lib.fvhd_llm_beam_sample_topk(h, ptr(lg), ptr(sc), 2, 2, 4, 1.0, 0, 1.5, 2, 0, ptr(ov), ptr(oi), stream()) != 0 and b"top_p" in lib.fvhd_last_error()
    assert lib.fvhd_llm_beam_sample_topk(h, ptr(lg), ptr(sc), 2, 2, 4, 1.0, 0, 1.0, 0, 0, ptr(ov), ptr(oi), stream()) != 0 and b"min_keep" in lib.fvhd_last_error()
    assert lib.fvhd_llm_beam_sample_topk(h, ptr(lg), ptr(sc), 2, 1, 4, 1.0, 0, 1.0, 2, 0, ptr(ov), ptr(oi), stream()) != 0 and b"num_beams" in lib.fvhd_last_error()
    gen.set_guidance(1.5)
    try:
        assert lib.fvhd_llm_beam_sample_topk(h, ptr(lg), ptr(sc), 2, 2, 4, 1.0, 0, 1.0, 2, 0, ptr(ov), ptr(oi), stream()) != 0
        assert b"fvhd_llm_beam_sample_topk" in lib.fvhd_last_error()
    finally:
        gen.set_guidance(1.0)
