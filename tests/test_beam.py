"""Beam search (include/fvhd.h version 505), the parts that need no GPU: `ml_fastvlm_amd.beam.BeamSearchState` against transformers' own
`_beam_search` on a tiny fp32 model, the binding's version rule and the builder's resolution of a generate(num_beams=...) call."""
import itertools
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402

from ml_fastvlm_amd.beam import BeamSearchState, beams_to_keep  # noqa: E402

N_NEW = 7
MARGIN = 1e-4


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(3)
    m = L.tiny_qwen2().eval()
    with torch.no_grad():
        for p in m.parameters():                                  # sharper distributions than the N(0, 0.02) init: margins well above fp32 noise
            if p.dim() == 2:
                p.mul_(6.0)
    m.generation_config.eos_token_id = None
    m.generation_config.pad_token_id = None
    ids = torch.randint(0, m.config.vocab_size, (2, 5), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        emb = m.get_input_embeddings()(ids)
    return m, emb


def oracle(m, emb, K, eos, **kw):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return m.generate(inputs_embeds=emb, attention_mask=torch.ones(emb.shape[:2], dtype=torch.long), num_beams=K, do_sample=False,
                          max_new_tokens=N_NEW, eos_token_id=eos, pad_token_id=63, return_dict_in_generate=True, output_scores=True, **kw)


def drive(m, emb, K, eos, **kw):
    """the class under test on the same model's log-probabilities: a full forward of every running row per step (no cache), log-softmax +
    running scores and topk in torch -> (tokens, scores, the smallest gap between neighbours among the top keep + 1 live candidates)"""
    G, V = emb.shape[0], m.config.vocab_size
    st = BeamSearchState(G, K, V, N_NEW, eos_token_id=eos, pad_token_id=63, **kw)
    rows = emb.repeat_interleave(K, dim=0)
    margin = float("inf")
    with torch.no_grad():
        for step in range(N_NEW):
            if st.finished():
                break
            if step:
                rows = torch.cat((rows[st.parent], m.get_input_embeddings()(st.fed_ids)[:, None, :]), dim=1)
            logp = torch.log_softmax(m(inputs_embeds=rows).logits[:, -1, :].float(), dim=-1)
            acc = (logp.view(G, K, V) + st.running_beam_scores[:, :, None]).reshape(G, K * V)
            top = torch.topk(acc, st.keep + 1)
            live = top.values[:, 1:] > -1e8
            gaps = (top.values[:, :-1] - top.values[:, 1:])[live]
            margin = min(margin, float(gaps.min()))
            st.update(top.values[:, :st.keep].contiguous(), top.indices[:, :st.keep].contiguous())
    tokens, scores = st.result()
    return tokens, scores, margin


@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_restatement_equals_transformers_beam_search(tiny, K):
    m, emb = tiny
    free = oracle(m, emb, K, None).sequences                     # the EOS ids come from the EOS-free output: they fire before the last step
    eos_sets = [None, int(free[0, 2]), [int(free[0, 2]), int(free[K if free.shape[0] > 2 else 1, 3])]]
    cases = list(itertools.product([0.0, 1.0, 2.0], [False, True, "never"], [1, K], eos_sets))
    skipped = 0
    for lp, early, n_ret, eos in cases:
        kw = dict(length_penalty=lp, early_stopping=early, num_return_sequences=n_ret)
        want = oracle(m, emb, K, eos, **kw)
        tokens, scores, margin = drive(m, emb, K, eos, **kw)
        if margin <= MARGIN:
            skipped += 1
            continue
        what = f"K={K} {kw} eos={eos}"
        assert tokens.shape == want.sequences.shape, (what, tokens.shape, want.sequences.shape)
        assert torch.equal(tokens, want.sequences), (what, tokens, want.sequences)
        assert torch.allclose(scores, want.sequences_scores, rtol=0, atol=1e-5), (what, scores, want.sequences_scores)
    assert skipped * 10 <= len(cases), f"{skipped} of {len(cases)} cases have an oracle margin <= {MARGIN}"


def test_eos_fires_before_the_last_step(tiny):
    """the EOS cases above are not vacuous: with the chosen id some returned hypothesis ends early and is padded"""
    m, emb = tiny
    free = oracle(m, emb, 2, None).sequences
    eos = int(free[0, 2])
    tokens, scores, _ = drive(m, emb, 2, eos, num_return_sequences=2)
    ended = (tokens == eos).any(dim=1)
    assert bool(ended.any())
    for row in tokens[ended]:
        first = int((row == eos).nonzero()[0, 0])
        assert bool((row[first + 1:] == 63).all())
    assert bool((scores.view(2, 2)[:, 0] >= scores.view(2, 2)[:, 1]).all())


def test_a_finished_search_ignores_further_updates(tiny):
    m, emb = tiny
    st = BeamSearchState(1, 2, 64, 2)
    v = torch.tensor([[-0.5, -1.0, -2.0, -3.0]])
    st.update(v, torch.tensor([[3, 5, 7, 9]]))
    assert not st.finished() and st.fed_ids.tolist() == [3, 5] and st.parent.tolist() == [0, 0]
    st.update(v - 1.0, torch.tensor([[64 + 1, 2, 64 + 4, 6]]))
    assert st.finished() and st.parent.tolist() == [0, 1]
    before = [t.clone() for t in (st.sequences, st.beam_scores, st.beam_indices, st.fed_ids, st.cur)]
    st.update(v, torch.tensor([[1, 2, 3, 4]]))
    assert all(torch.equal(a, b) for a, b in zip(before, (st.sequences, st.beam_scores, st.beam_indices, st.fed_ids, st.cur)))
    tokens, scores = st.result()
    assert tokens.tolist() == [[5, 1]] and abs(float(scores[0]) - (-1.5 / 2)) < 1e-6


def test_settings_are_checked():
    assert beams_to_keep(4, 0) == 8 and beams_to_keep(4, 1) == 8 and beams_to_keep(3, 2) == 9
    with pytest.raises(ValueError, match="num_beams"):
        BeamSearchState(1, 1, 64, 4)
    with pytest.raises(ValueError, match="num_return_sequences"):
        BeamSearchState(1, 2, 64, 4, num_return_sequences=3)
    with pytest.raises(ValueError, match="early_stopping"):
        BeamSearchState(1, 2, 64, 4, early_stopping="always")


# ---- builder ---------------------------------------------------------------------------------------------------------------------------
BEAMS = dict(do_sample=False, num_beams=4, max_new_tokens=8, use_cache=True)


def test_the_settings_resolve_num_beams_to_the_library_only_on_request():
    from ml_fastvlm_amd import builder
    m = L.tiny_qwen2()
    settings, reason = builder._library_generate_settings(m, dict(BEAMS))
    assert settings is None and "num_beams" in reason            # the default: as before
    settings, reason = builder._library_generate_settings(m, dict(BEAMS), beam_search=True)
    assert reason is None and settings["sampling"] is None
    assert settings["beam"] == dict(num_beams=4, length_penalty=1.0, early_stopping=False, num_return_sequences=1)
    settings, reason = builder._library_generate_settings(m, dict(BEAMS, num_return_sequences=3, length_penalty=0.5, early_stopping=True),
                                                          beam_search=True)
    assert reason is None and settings["beam"] == dict(num_beams=4, length_penalty=0.5, early_stopping=True, num_return_sequences=3)
    settings, reason = builder._library_generate_settings(m, dict(BEAMS, num_beams=1), beam_search=True)
    assert reason is None and settings["beam"] is None


@pytest.mark.parametrize("kw", [dict(do_sample=True), dict(num_beam_groups=2, diversity_penalty=0.5), dict(num_beam_groups=2),
                                dict(repetition_penalty=1.2), dict(return_dict_in_generate=True), dict(num_beams=32)])
def test_other_beam_modes_keep_a_fallback_reason(kw):
    from ml_fastvlm_amd import builder
    settings, reason = builder._library_generate_settings(L.tiny_qwen2(), dict(BEAMS, **kw), beam_search=True)
    assert settings is None and reason


def test_the_patched_generate_takes_the_library_for_num_beams(monkeypatch):
    from ml_fastvlm_amd import builder
    from types import SimpleNamespace
    tiny_model = L.tiny_qwen2()

    class OnDevice:                                               # what the patched generate looks at: a bf16 lm_head on a HIP device
        lm_head = SimpleNamespace(weight=SimpleNamespace(device=torch.device("cuda", 0), dtype=torch.bfloat16))
        _prepare_generation_config = staticmethod(tiny_model._prepare_generation_config)

    m = OnDevice()
    seen = []
    monkeypatch.setattr(builder, "_generate_on_library", lambda *a: seen.append(a) or "library")
    orig = lambda self, inputs, images, image_sizes, **kw: "reference"      # noqa: E731
    ids = torch.zeros((2, 3), dtype=torch.long)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert builder._make_library_generate(orig, beam_search=True)(m, ids, **BEAMS) == "library"
    assert seen[0][-1] == dict(num_beams=4, length_penalty=1.0, early_stopping=False, num_return_sequences=1)
    with pytest.warns(UserWarning, match="num_beams"):
        assert builder._make_library_generate(orig)(m, ids, **BEAMS) == "reference"
    wide = torch.zeros((17, 3), dtype=torch.long)                 # 17 x 4 = 68 rows
    with pytest.warns(UserWarning, match="68"):
        assert builder._make_library_generate(orig, beam_search=True)(m, wide, **BEAMS) == "reference"


def test_the_package_exports_the_new_names():
    import ml_fastvlm_amd as fv
    assert fv.beam_generate is not None and fv.BeamSearchState is BeamSearchState
    assert {"beam_generate", "BeamSearchState"} <= set(fv.__all__)


def test_install_into_llava_passes_the_beam_search_option():
    from oracle import ref_import
    if not ref_import.reference_available():
        pytest.skip("the reference checkout is not on this machine")
    ref_import.install_timm_stub()
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    import ml_fastvlm_amd as fv
    from ml_fastvlm_amd import builder
    lq = pytest.importorskip("llava.model.language_model.llava_qwen")
    import llava.model.llava_arch as arch
    import llava.model.multimodal_encoder.builder as enc_builder
    before = lq.LlavaQwen2ForCausalLM.generate
    saved = (enc_builder.build_vision_tower, arch.build_vision_tower, arch.LlavaMetaForCausalLM.encode_images)
    made = []
    real = builder._make_library_generate
    try:
        builder._make_library_generate = lambda orig, beam_search=False: made.append(beam_search) or real(orig, beam_search=beam_search)
        fv.install_into_llava(generate=True)
        fv.install_into_llava(generate=True, beam_search=True)
        assert made == [False, True]
        assert lq.LlavaQwen2ForCausalLM.generate._fvhd_orig is getattr(before, "_fvhd_orig", before)
    finally:                                                    # the tower patches of install_into_llava too: other tests import llava
        builder._make_library_generate = real
        lq.LlavaQwen2ForCausalLM.generate = before
        enc_builder.build_vision_tower, arch.build_vision_tower, arch.LlavaMetaForCausalLM.encode_images = saved
