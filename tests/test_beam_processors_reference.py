"""Beam search with logits processors, the parts that need no GPU: the composed reference of tests/beam_processors_reference.py against
transformers' own generate(num_beams=K, ...) in fp32 on the CPU, the `beam_processors` flag of `builder._library_generate_settings`,
the keyword checks of `Qwen2Generator.beam_search` that run before any device is touched, and the feature record."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_processors_reference as R  # noqa: E402
import llm_testlib as L  # noqa: E402

from ml_fastvlm_amd import builder  # noqa: E402


# ---- a. the composed reference ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(3)
    m = L.tiny_qwen2().eval()
    m.generation_config.eos_token_id = None
    m.generation_config.pad_token_id = None
    g = torch.Generator().manual_seed(5)
    e = torch.randn(2, 7, 64, generator=g)
    mask = torch.ones(2, 7, dtype=torch.long)
    mask[1, :2] = 0
    return m, e, mask


def logits_of(m, e, mask, K):
    rows = torch.arange(e.shape[0]).repeat_interleave(K)

    def fn(hist):
        x = torch.cat((e[rows], m.get_input_embeddings()(hist)), dim=1)
        am = torch.cat((mask[rows], torch.ones_like(hist)), dim=1)
        pos = (am.cumsum(-1) - 1).clamp(min=0)
        return m(inputs_embeds=x, attention_mask=am, position_ids=pos).logits[:, -1]
    return fn


CASES = [
    (2, dict(repetition_penalty=1.3, no_repeat_ngram_size=2)),
    (4, dict(repetition_penalty=1.3, no_repeat_ngram_size=2)),
    (3, dict(repetition_penalty=0.8)),
    (2, dict(no_repeat_ngram_size=1, suppress_tokens=[3, 9, 40])),
    (3, dict(min_new_tokens=4, repetition_penalty=1.2)),
]


@pytest.mark.parametrize("K, proc", CASES)
def test_composed_reference_equals_transformers(tiny, K, proc):
    m, e, mask = tiny
    new, G, V = 8, e.shape[0], 64
    plain = R.oracle(m, e, mask, K, new)
    eos = None
    if "min_new_tokens" in proc:
        eos = int(plain.sequences[0, 1])                          # an id the plain search picks early: the ban bites
    want = R.oracle(m, e, mask, K, new, eos_token_id=eos, **proc)
    assert not torch.equal(want.sequences, plain.sequences) or want.sequences.shape != plain.sequences.shape, "the processors change nothing here"
    steps = []
    tokens, scores = R.composed_beam_search(logits_of(m, e, mask, K), G, K, V, new, R.hf_processors(eos_token_id=eos, num_beams=K, **proc),
                                            eos_token_id=eos, pad_token_id=0, record=steps)
    assert torch.equal(tokens, want.sequences), (tokens, want.sequences)
    assert float((scores - want.sequences_scores).abs().max()) < 1e-5
    # transformers reports the same processed rows (its cache against the full forward here: rounding only)
    for ours, theirs in zip(steps, want.scores):
        same_bans = torch.equal(torch.isinf(ours), torch.isinf(theirs))
        assert same_bans and float((ours - theirs)[~torch.isinf(ours)].abs().max()) < 1e-4


def test_a_history_that_does_not_follow_its_parent_is_caught(tiny):
    """the reference with the reorder left out disagrees with transformers: the test above sees the reorder"""
    m, e, mask = tiny
    K, new, G, V = 4, 8, e.shape[0], 64
    proc = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
    want = R.oracle(m, e, mask, K, new, num_return_sequences=K, **proc)
    inner = R.hf_processors(num_beams=K, **proc)
    fn = logits_of(m, e, mask, K)
    st = R.BeamSearchState(G, K, V, new, num_return_sequences=K, pad_token_id=0)
    hist = torch.zeros((G * K, 0), dtype=torch.long)
    moved = False
    for step in range(new):
        if step:
            moved = moved or not torch.equal(st.parent, st.identity)
            hist = torch.cat((hist, st.fed_ids[:, None]), dim=1)  # NOT reordered; the model still sees the right sequences
        seqs = st.running_sequences.view(G * K, new)[:, :step]
        logp = inner(hist, torch.log_softmax(fn(seqs).float(), dim=-1))
        top = torch.topk((logp.view(G, K, V) + st.running_beam_scores[:, :, None]).reshape(G, K * V), st.keep)
        st.update(top.values.contiguous(), top.indices.contiguous())
    tokens, scores = st.result()
    assert moved and not (torch.equal(tokens, want.sequences) and float((scores - want.sequences_scores).abs().max()) < 1e-4)


# ---- the settings flag ------------------------------------------------------------------------------------------------------------------
BASE = dict(do_sample=False, max_new_tokens=8, use_cache=True)


def settings(kw, **flags):
    return builder._library_generate_settings(L.tiny_qwen2(), dict(BASE, **kw), **flags)


def test_the_flag_lets_the_four_settings_pass_under_beams():
    got, reason = settings(dict(num_beams=4, repetition_penalty=1.2, no_repeat_ngram_size=3), beam_search=True, beam_processors=True)
    assert reason is None and got["sampling"] is None
    assert got["beam"] == dict(num_beams=4, length_penalty=1.0, early_stopping=False, num_return_sequences=1, repetition_penalty=pytest.approx(1.2),
                               no_repeat_ngram_size=3, min_new_tokens=0, suppress_tokens=[])
    got, reason = settings(dict(num_beams=2, suppress_tokens=[5, 7], min_new_tokens=3, eos_token_id=9), beam_search=True, beam_processors=True)
    assert reason is None and got["beam"]["suppress_tokens"] == [5, 7] and got["beam"]["min_new_tokens"] == 3 and got["eos_token_id"] == 9
    assert "eos_token_id" not in got["beam"]
    got, reason = settings(dict(num_beams=2), beam_search=True, beam_processors=True)             # nothing asked: what it was
    assert reason is None and got["beam"] == dict(num_beams=2, length_penalty=1.0, early_stopping=False, num_return_sequences=1)
    got, reason = settings(dict(num_beams=2, repetition_penalty=1.2), beam_search=True, beam_processors=True, processors=True)
    assert reason is None and got["beam"]["repetition_penalty"] == pytest.approx(1.2) and got["processors"] is None
    got, reason = settings(dict(num_beams=2, do_sample=True, repetition_penalty=1.2), beam_search=True, beam_processors=True, beam_sample=True)
    assert reason is None and got["beam"]["do_sample"] is True and got["beam"]["repetition_penalty"] == pytest.approx(1.2)


def test_without_the_flag_such_a_call_keeps_its_reason():
    for flags in (dict(beam_search=True), dict(beam_search=True, processors=True)):
        got, reason = settings(dict(num_beams=2, repetition_penalty=1.2), **flags)
        assert got is None and "repetition_penalty" in reason
        got, reason = settings(dict(num_beams=2, no_repeat_ngram_size=2), **flags)
        assert got is None and "no_repeat_ngram_size" in reason
    got, reason = settings(dict(num_beams=2, repetition_penalty=1.2), beam_processors=True)      # no beam_search: beams fall back as ever
    assert got is None and "num_beams" in reason


@pytest.mark.parametrize("kw, word", [(dict(bad_words_ids=[[5]]), "bad_words_ids"), (dict(min_length=3), "min_length"),
                                      (dict(sequence_bias=[[[5], 1.0]]), "sequence_bias"), (dict(prefix_allowed_tokens_fn=lambda b, s: [1]), "prefix_allowed_tokens_fn"),
                                      (dict(do_sample=True, min_p=0.1), "min_p"), (dict(do_sample=True, typical_p=0.9), "typical_p"),
                                      (dict(do_sample=True, top_h=0.5), "top_h"), (dict(num_beam_groups=2, diversity_penalty=0.5), "num_beam_groups")])
def test_what_keeps_falling_back_under_the_flag(kw, word):
    got, reason = settings(dict(num_beams=2, repetition_penalty=1.2, **kw), beam_search=True, beam_processors=True, beam_sample=True,
                           sampling_warpers=True)
    assert got is None and (word in reason or "do not resolve" in reason), reason


def test_limits_of_the_library_fall_back_under_beams_too():
    got, reason = settings(dict(num_beams=2, suppress_tokens=list(range(30, 30 + 300))), beam_search=True, beam_processors=True)
    assert got is None and "logits processors" in reason


# ---- keyword validation, before any device ----------------------------------------------------------------------------------------------
def bare_generator():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen.pre = types.SimpleNamespace(vocab=64)
    gen.batch, gen.capacity, gen.device = 8, 32, torch.device("cpu")
    return gen


def test_keyword_checks_run_before_the_device():
    gen = bare_generator()
    x = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError, match="repetition_penalty must be finite and > 0"):
        gen.beam_search(x, num_beams=2, max_new_tokens=4, repetition_penalty=0.0)
    with pytest.raises(ValueError, match="suppress_tokens: every id must be in"):
        gen.beam_search(x, num_beams=2, max_new_tokens=4, suppress_tokens=[64])
    with pytest.raises(ValueError, match="constraint_start is given without a constraint"):
        gen.beam_search(x, num_beams=2, max_new_tokens=4, constraint_start=0)
    with pytest.raises(ValueError, match="greedy"):
        gen.beam_search(x, num_beams=1, max_new_tokens=4, repetition_penalty=1.2)
    gen._guidance = 2.0
    with pytest.raises(ValueError, match="beam search does not take guidance"):
        gen.beam_search(x, num_beams=2, max_new_tokens=4, repetition_penalty=1.2)
    gen._guidance = None
    gen._processors = dict(repetition_penalty=1.2)                # set outside the call: still refused, and told where they go
    with pytest.raises(ValueError, match="not implemented under beam search.*keywords of beam_search"):
        gen.beam_search(x, num_beams=2, max_new_tokens=4, repetition_penalty=1.2)
    with pytest.raises(ValueError, match=r"clear them with set_logits_processors\(\)$"):
        gen.beam_search(x, num_beams=2, max_new_tokens=4)


# ---- the feature record ----------------------------------------------------------------------------------------------------------------
def test_the_feature_record_and_its_gates():
    from ml_fastvlm_amd import _lib
    assert "beam_processors" in _lib.FEATURES_OPEN and _lib.FEATURE_TABLES[-1] is _lib.FEATURES_OPEN
    names = [n for t in _lib.FEATURE_TABLES for n in t]
    assert len(names) == len(set(names))                          # the tables share no name
    sigs = [n for t in _lib.FEATURE_TABLES for f in t.values() for n in f.sig] + list(_lib.BASE_SIGNATURES)
    assert len(sigs) == len(set(sigs))                            # no symbol under two features
    f = _lib.FEATURES_OPEN["beam_processors"]
    assert f.since is None and f.probe == "fvhd_llm_set_beam_scoring" and f.probe in f.sig and f.needs == "beam_sample"
    built = _lib.load()
    assert _lib.has("beam_processors") and _lib.require("beam_processors") is built and _lib.beam_processors_lib() is built
    for n in f.sig:
        assert getattr(built, n).argtypes is not None, n
    with pytest.raises(KeyError):
        _lib.has("no_such_feature")
