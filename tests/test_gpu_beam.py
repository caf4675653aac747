"""Beam search on the library (`Qwen2Generator.beam_search`, ml_fastvlm_amd/beam.py, csrc/llm_beam.hip) against transformers' own beam
search on the fp32 oracle of the same bf16-rounded weights.

Token-for-token equality is asked only where the oracle's decisions are clear (every gap among the top K + 1 accumulated candidates
above 2 DELTA: bf16 rounding cannot legitimately choose otherwise); for any margins, every returned hypothesis must carry the score the
oracle gives that very token sequence - which a wrong cache reorder or wrong bookkeeping does not survive."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import DELTA, models, prompt  # noqa: E402

from ml_fastvlm_amd.beam import BeamSearchState  # noqa: E402

pytestmark = pytest.mark.gpu

CLEAR_SEEDS = [205, 206, 248, 111]          # of prompt(ref, 1, 12, "left", seed, draw_on="cpu"), model seed 1: tools/beam_margins.py
CAPACITY = 32


@pytest.fixture(scope="module")
def setup():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = models("0.5B", seed=1)
    ref.generation_config.eos_token_id = None
    ref.generation_config.pad_token_id = None
    gen = Qwen2Generator.from_hf(m16, 64, CAPACITY)
    return m16, ref, gen


def oracle(ref, e, mask, K, new, **kw):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ref.generate(inputs_embeds=e, attention_mask=mask, num_beams=K, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                            return_dict_in_generate=True, output_scores=True, **kw)


def oracle_margin(out, G, K, new):
    """the oracle's search replayed from its own per-step log-probabilities (`scores`: [G K, vocab] per step) -> the smallest gap among the
    top K + 1 accumulated candidates of any prompt at any step, and the replay's tokens"""
    V = out.scores[0].shape[-1]
    st = BeamSearchState(G, K, V, new, pad_token_id=0, device=out.scores[0].device)
    margin = float("inf")
    for logp in out.scores:
        acc = (logp.float().view(G, K, V) + st.running_beam_scores[:, :, None]).reshape(G, K * V)
        top = torch.topk(acc, st.keep)
        margin = min(margin, float((top.values[:, :K] - top.values[:, 1:K + 1]).min()))
        st.update(top.values.contiguous(), top.indices.contiguous())
    return margin, st.result()[0]


@pytest.mark.parametrize("seed", CLEAR_SEEDS)
def test_beam_search_equals_transformers_where_the_oracle_is_clear(setup, seed):
    m16, ref, gen = setup
    K, new = 2, 6
    e, mask = prompt(ref, 1, 12, "left", seed, draw_on="cpu")
    want = oracle(ref, e, mask, K, new)
    margin, replayed = oracle_margin(want, 1, K, new)
    print(f"seed {seed}: the oracle's smallest gap among the top {K + 1} candidates {margin:.3f}")
    assert torch.equal(replayed, want.sequences)
    assert margin > 2 * DELTA, f"seed {seed}: margin {margin:.4f} <= {2 * DELTA}: not a clear case"
    tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, num_beams=K, max_new_tokens=new, pad_token_id=0, return_scores=True)
    assert torch.equal(tokens, want.sequences), (tokens, want.sequences)
    assert float((scores - want.sequences_scores).abs().max()) <= DELTA, (scores, want.sequences_scores)
    eager_t, eager_s = gen.beam_search(e.to(torch.bfloat16), mask, None, num_beams=K, max_new_tokens=new, pad_token_id=0, return_scores=True,
                                       graph=False)
    assert torch.equal(eager_t, tokens) and torch.equal(eager_s.view(torch.int32), scores.view(torch.int32))
    assert gen.cache_state()[1] == 0


def teacher_forced(ref, e, mask, tokens, lengths):
    """the oracle's sum of log-probabilities over tokens[r, :lengths[r]] continuing prompt row r"""
    n = tokens.shape[1]
    x = torch.cat((e, ref.get_input_embeddings()(tokens.clamp(min=0))), dim=1)
    am = torch.cat((mask, torch.ones_like(tokens)), dim=1)
    pos = (am.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        logp = torch.log_softmax(ref(inputs_embeds=x, attention_mask=am, position_ids=pos).logits[:, -n - 1:-1].float(), dim=-1)
    tok = torch.gather(logp, 2, tokens.clamp(min=0)[:, :, None])[:, :, 0]
    keep = torch.arange(n, device=tokens.device)[None, :] < lengths[:, None]
    return (tok * keep).sum(-1)


@pytest.mark.parametrize("lp", [0.0, 1.0])
def test_every_returned_hypothesis_has_the_oracle_score_of_its_tokens(setup, lp):
    m16, ref, gen = setup
    G, K, new, pad = 3, 4, 10, 4095
    e, mask = prompt(ref, G, 14, "left", 7)
    kw = dict(num_beams=K, max_new_tokens=new, length_penalty=lp, num_return_sequences=K, pad_token_id=pad, return_scores=True)
    free, _ = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    eos = int(free[0, 2])                                         # the EOS-free best beam's third token: the finished-beam path runs
    for eos_id in (None, eos):
        tokens, scores = gen.beam_search(e.to(torch.bfloat16), mask, None, eos_token_id=eos_id, **kw)
        assert tokens.shape[0] == G * K and scores.shape == (G * K,) and tokens.shape[1] <= new
        n = tokens.shape[1]
        lengths = torch.full((G * K,), n, device=tokens.device)
        if eos_id is not None:
            hit = tokens == eos_id
            first = torch.where(hit.any(-1), hit.float().argmax(-1) + 1, lengths)
            lengths = first
            if lp == 0.0:                                         # (dividing by the length may rank every early ending below the full-length ones)
                assert bool((lengths < new).any()), "no hypothesis ended at the EOS id"
            for r in range(G * K):                                # finished rows are padded
                assert bool((tokens[r, int(lengths[r]):] == pad).all()), (r, tokens[r])
        rows = torch.arange(G, device=tokens.device).repeat_interleave(K)
        total = teacher_forced(ref, e[rows], mask[rows], tokens, lengths)
        want = total / lengths.float() ** lp
        bound = DELTA * lengths.float() / lengths.float() ** lp
        err = (scores - want).abs()
        print(f"length_penalty {lp} eos {eos_id}: max |score - oracle| / bound {float((err / bound).max()):.3f}, lengths {lengths.tolist()}")
        assert bool((err <= bound).all()), (scores, want)
        by_prompt = scores.view(G, K)
        assert bool((by_prompt[:, :-1] >= by_prompt[:, 1:]).all()), by_prompt
        assert gen.cache_state()[1] == 0


def test_sixteen_copies_take_the_wide_kernels_and_equal_one(setup):
    m16, ref, gen = setup
    e, mask = prompt(ref, 1, 12, "left", 205, draw_on="cpu")
    kw = dict(num_beams=4, max_new_tokens=6, num_return_sequences=4, pad_token_id=0, return_scores=True)
    one_t, one_s = gen.beam_search(e.to(torch.bfloat16), mask, None, **kw)
    t, s = gen.beam_search(e.to(torch.bfloat16).expand(16, -1, -1).contiguous(), mask.expand(16, -1).contiguous(), None, **kw)
    assert t.shape == (64, one_t.shape[1])
    for g in range(16):
        assert torch.equal(t[4 * g:4 * g + 4], one_t), g
        assert torch.equal(s[4 * g:4 * g + 4].view(torch.int32), one_s.view(torch.int32)), g


def test_refusals(setup):
    m16, ref, gen = setup
    e, mask = prompt(ref, 5, 12, "left", 3)
    e = e.to(torch.bfloat16)
    with pytest.raises(ValueError, match="65 rows"):
        gen.beam_search(e, mask, None, num_beams=13, max_new_tokens=4)
    with pytest.raises(ValueError, match="greedy"):
        gen.beam_search(e, mask, None, num_beams=1, max_new_tokens=4)
    with pytest.raises(ValueError, match="cache"):
        gen.beam_search(e, mask, None, num_beams=2, max_new_tokens=CAPACITY - 12 + 2)
    tokens = gen.beam_search(e, mask, None, num_beams=2, max_new_tokens=CAPACITY - 12 + 1, pad_token_id=0)      # the whole capacity
    assert tokens.shape == (5, CAPACITY - 12 + 1) and gen.cache_state() == (CAPACITY, 0)


def test_patched_generate_runs_beam_search_on_the_library():
    """builder._make_library_generate(beam_search=True) - what install_into_llava(generate=True, beam_search=True) installs - on a stand-in
    of LlavaQwen2ForCausalLM: generate(num_beams=2) raises no warning and equals Qwen2Generator.beam_search on the same spliced inputs"""
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
    StandIn.generate = builder._make_library_generate(orig, beam_search=True)
    try:
        g = torch.Generator().manual_seed(0)
        ids = torch.randint(10, 4000, (2, 12), generator=g)
        ids[:, 3] = -200                                          # IMAGE_TOKEN_INDEX
        ids = ids.cuda()
        feats = (0.5 * torch.randn(2, 16, 896, generator=g)).to("cuda", torch.bfloat16)
        call = dict(images=feats, image_sizes=[(256, 256)] * 2, do_sample=False, temperature=None, num_beams=2, max_new_tokens=8, use_cache=True,
                    pad_token_id=0, eos_token_id=None)
        model.generation_config.eos_token_id = None
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = model.generate(ids, **call)
        _, pos, am, _, emb, _ = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, feats)
        gen = builder.generator_context(model, 4, emb.shape[1] + 8)
        want = gen.beam_search(emb, am, pos, num_beams=2, max_new_tokens=8, pad_token_id=0)
        assert got.shape == (2, 8) and torch.equal(got, want)
        lib_t, lib_s = builder.beam_generate(model, ids, images=feats, num_beams=2, max_new_tokens=8, pad_token_id=0, return_scores=True)
        assert torch.equal(lib_t, want) and lib_s.shape == (2,)
    finally:
        StandIn.generate = orig
