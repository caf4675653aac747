"""Logits processors of the decode step (include/fvhd.h version 506), the parts that need no GPU: `process_reference` against transformers'
own processors bit for bit, the builder's settings resolution with `processors=True`, the 506 gate of the binding and the argument checks
of the two new C entry points."""
import ctypes as C
import math
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from binding_stub import stub  # noqa: E402

from logits_testlib import hf_chain  # noqa: E402
from ml_fastvlm_amd.logits_processors import normalize, process_reference  # noqa: E402

V = 1001


def _scores(B, seed):
    g = torch.Generator().manual_seed(seed)
    s = 4.0 * torch.randn(B, V, generator=g)
    s[:, 5] = 0.0
    s[:, 6] = -0.0
    s[:, 7] = -math.inf
    s[:, 8] = -3.25
    s[:, 9] = 2.5
    return s


def _histories(n):
    """name -> int64 [2, g]: the issue's list, with tokens 5 .. 9 (zero, -0, -inf, negative, positive logits) among them"""
    g = torch.Generator().manual_seed(7)
    out = {"empty": torch.zeros(2, 0, dtype=torch.long), "one": torch.tensor([[5], [8]])}
    for name, k in (("n-1", n - 1), ("n", n)):
        if k >= 1:
            out[name] = torch.randint(0, 12, (2, k), generator=g)
    out["repeated"] = torch.tensor([[7] * 300, [9] * 300])
    # the suffix (3, 4, 6) occurs three times with the successors 8, 9, 5, then once more at the end
    a = [1, 3, 4, 6, 8, 2, 3, 4, 6, 9, 11, 3, 4, 6, 5, 10, 3, 4, 6]
    b = [7, 3, 4, 6, 9, 7, 3, 4, 6, 9, 7, 3, 4, 6, 0, 7, 3, 4, 6]
    out["suffix x3"] = torch.tensor([a, b])
    out["random"] = torch.randint(0, V, (2, 64), generator=g)
    return out


@pytest.mark.parametrize("p", [1.0, 1.3, 0.8])
@pytest.mark.parametrize("n", [0, 1, 2, 4])
def test_the_reference_equals_transformers_bit_for_bit(p, n):
    for name, h in _histories(max(n, 1)).items():
        s = _scores(h.shape[0], seed=h.shape[1])
        for m, eos, sup in ((0, None, None), (70, [8, 700], None), (3, [9], [5, 6, 1000]), (0, None, [7, 11])):
            kw = dict(p=p, n=n, m=m, eos=eos, suppress=sup)
            want = hf_chain(h, s, **kw)
            got = process_reference(h, s, repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m, eos_token_id=eos, suppress_tokens=sup)
            assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, kw)
    # the input is not edited
    s = _scores(2, 0)
    keep = s.clone()
    process_reference(torch.tensor([[5, 8], [9, 9]]), s, repetition_penalty=1.3, no_repeat_ngram_size=1)
    assert torch.equal(s.view(torch.int32), keep.view(torch.int32))


def test_a_repeated_token_is_penalised_once_and_a_ban_wins():
    s = _scores(1, 3)
    h = torch.tensor([[9] * 5 + [8] * 3])
    got = process_reference(h, s, repetition_penalty=1.3, suppress_tokens=[9])
    p = torch.tensor(1.3, dtype=torch.float32)
    assert got[0, 8] == s[0, 8] * p and got[0, 9] == -math.inf
    got = process_reference(h, s, repetition_penalty=1.3)
    assert got[0, 9] == s[0, 9] / p


def test_normalize_names_the_limits():
    assert normalize() is None and normalize(1.0, 0, 0, eos_token_id=[1, 2], suppress_tokens=[]) is None
    assert normalize(min_new_tokens=3) is None                   # no EOS id: nothing to ban
    assert normalize(1.2, None, None, 5, None) == dict(repetition_penalty=1.2, no_repeat_ngram_size=0, min_new_tokens=0, eos_token_id=[],
                                                       suppress_tokens=[])
    assert normalize(min_new_tokens=2, eos_token_id=7)["eos_token_id"] == [7]
    with pytest.raises(ValueError, match="at most 16"):
        normalize(min_new_tokens=2, eos_token_id=list(range(17)))
    with pytest.raises(ValueError, match="at most 256"):
        normalize(suppress_tokens=list(range(257)))
    with pytest.raises(ValueError, match="vocab"):
        normalize(suppress_tokens=[64], vocab=64)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="repetition_penalty"):
            normalize(bad)
    with pytest.raises(ValueError, match=">= 0"):
        normalize(no_repeat_ngram_size=-1)


# ---- builder ---------------------------------------------------------------------------------------------------------------------------
BASE = dict(do_sample=False, max_new_tokens=8, use_cache=True)
OFF = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=[])


@pytest.mark.parametrize("kw,want", [
    (dict(repetition_penalty=1.2), dict(OFF, repetition_penalty=1.2)),
    (dict(no_repeat_ngram_size=3), dict(OFF, no_repeat_ngram_size=3)),
    (dict(min_new_tokens=3, eos_token_id=[5, 6]), dict(OFF, min_new_tokens=3)),
    (dict(suppress_tokens=[1, 2, 3]), dict(OFF, suppress_tokens=[1, 2, 3])),
    (dict(repetition_penalty=0.8, no_repeat_ngram_size=2, min_new_tokens=4, eos_token_id=9, suppress_tokens=[7]),
     dict(repetition_penalty=0.8, no_repeat_ngram_size=2, min_new_tokens=4, suppress_tokens=[7])),
])
@pytest.mark.parametrize("sample", [False, True])
def test_the_settings_take_the_four_processors_on_request(kw, want, sample):
    from ml_fastvlm_amd import builder
    m = L.tiny_qwen2()
    call = dict(BASE, **kw, **(dict(do_sample=True, temperature=0.7, top_k=20, top_p=0.9) if sample else {}))
    settings, reason = builder._library_generate_settings(m, dict(call))
    assert settings is None and any(k in reason for k in kw)      # the default: as before
    settings, reason = builder._library_generate_settings(m, dict(call), processors=True)
    assert reason is None, reason
    assert settings["processors"] == want and settings["beam"] is None
    assert (settings["sampling"] == dict(temperature=0.7, top_k=20, top_p=0.9)) if sample else settings["sampling"] is None
    if "eos_token_id" in kw:
        assert settings["eos_token_id"] == kw["eos_token_id"]


def test_all_off_resolves_to_no_processors():
    from ml_fastvlm_amd import builder
    m = L.tiny_qwen2()
    settings, reason = builder._library_generate_settings(m, dict(BASE), processors=True)
    assert reason is None and settings["processors"] is None
    settings, reason = builder._library_generate_settings(m, dict(BASE))
    assert reason is None and "processors" not in settings        # without the flag the dict is what it was


@pytest.mark.parametrize("kw", [dict(num_beams=2, repetition_penalty=1.2), dict(num_beams=2, no_repeat_ngram_size=2),
                                dict(bad_words_ids=[[3, 4]]), dict(min_length=3), dict(min_new_tokens=3, eos_token_id=list(range(17))),
                                dict(suppress_tokens=list(range(40)) * 6 + list(range(17))), dict(suppress_tokens=[64]),
                                dict(begin_suppress_tokens=[3]), dict(sequence_bias={(3,): 1.0}), dict(encoder_repetition_penalty=1.2)])
def test_everything_else_keeps_a_fallback_reason(kw):
    from ml_fastvlm_amd import builder
    for beam_search in (False, True):
        settings, reason = builder._library_generate_settings(L.tiny_qwen2(), dict(BASE, **kw), beam_search=beam_search, processors=True)
        assert settings is None and reason, kw


def test_the_patched_generate_passes_the_processors(monkeypatch):
    from types import SimpleNamespace
    from ml_fastvlm_amd import builder
    tiny_model = L.tiny_qwen2()

    class OnDevice:                                               # what the patched generate looks at: a bf16 lm_head on a HIP device
        lm_head = SimpleNamespace(weight=SimpleNamespace(device=torch.device("cuda", 0), dtype=torch.bfloat16))
        config = tiny_model.config
        _prepare_generation_config = staticmethod(tiny_model._prepare_generation_config)

    m = OnDevice()
    seen = []
    monkeypatch.setattr(builder, "_generate_on_library", lambda *a, **kw: seen.append((a, kw)) or "library")
    orig = lambda self, inputs, images, image_sizes, **kw: "reference"      # noqa: E731
    ids = torch.zeros((2, 3), dtype=torch.long)
    call = dict(BASE, repetition_penalty=1.2, no_repeat_ngram_size=3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert builder._make_library_generate(orig, logits_processors=True)(m, ids, **call) == "library"
        assert builder._make_library_generate(orig, logits_processors=True)(m, ids, **BASE) == "library"
    assert seen[0][1] == dict(processors=dict(OFF, repetition_penalty=1.2, no_repeat_ngram_size=3))
    assert seen[1][1] == {}                                       # nothing on: the call of version 505, argument for argument
    with pytest.warns(UserWarning, match="repetition_penalty"):
        assert builder._make_library_generate(orig)(m, ids, **call) == "reference"


def test_generate_on_library_hands_the_processors_to_the_generator(monkeypatch):
    from ml_fastvlm_amd import builder
    calls = []

    class Gen:
        def greedy(self, *a, **kw):
            calls.append(("greedy", kw))

        def sample(self, *a, **kw):
            calls.append(("sample", kw))

    monkeypatch.setattr(builder, "generator_context", lambda model, B, cap: Gen())
    m = L.tiny_qwen2()
    ids = torch.zeros((1, 4), dtype=torch.long)
    proc = dict(OFF, no_repeat_ngram_size=2)
    builder._generate_on_library(m, ids, None, None, None, None, 4, 1, 0, None, None, processors=proc)
    builder._generate_on_library(m, ids, None, None, None, None, 4, 1, 0, dict(temperature=1.0, top_k=0, top_p=1.0), None, processors=proc)
    builder._generate_on_library(m, ids, None, None, None, None, 4, 1, 0)
    assert calls[0][0] == "greedy" and calls[0][1]["no_repeat_ngram_size"] == 2 and calls[0][1]["suppress_tokens"] == []
    assert calls[1][0] == "sample" and calls[1][1]["no_repeat_ngram_size"] == 2 and calls[1][1]["top_k"] == 0
    assert calls[2][0] == "greedy" and "no_repeat_ngram_size" not in calls[2][1]


# ---- binding ---------------------------------------------------------------------------------------------------------------------------
def test_a_505_library_loads_and_processors_name_the_rebuild(monkeypatch):
    from ml_fastvlm_amd import _lib
    calls = []
    lib = stub(monkeypatch, 505, calls)
    assert lib.fvhd_version() == 505
    # a generator on that library: all-off settings are accepted silently, a processor names the rebuild
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen._processors, gen.device = None, torch.device("cpu")
    gen.pre = type("Pre", (), dict(vocab=64, _h=None))()
    gen.set_logits_processors()
    with pytest.raises(_lib.FvhdError, match="506"):
        gen.set_logits_processors(repetition_penalty=1.2)
    assert calls == []


def test_the_entry_points_reject_bad_arguments():
    from ml_fastvlm_amd import _lib
    lib = _lib.processors_lib()
    vp = C.c_void_p
    assert lib.fvhd_llm_set_logits_processors(None, 1.2, 0, 0, None, 0, None, 0) != 0
    assert b"NULL" in lib.fvhd_last_error()
    x = torch.zeros(2, 64)
    h = torch.zeros(2, 8, dtype=torch.int32)
    ids = (C.c_int32 * 300)(*([3] * 300))
    lg, hs, lst = vp(x.data_ptr()), vp(h.data_ptr()), C.cast(ids, vp)

    def op(logits=lg, B=2, V=64, hist=hs, cap=8, g=4, p=1.2, n=0, m=0, eos=None, n_eos=0, sup=None, n_sup=0):
        return lib.fvhd_op_dec_logits_process(None, logits, B, V, hist, cap, g, p, n, m, eos, n_eos, sup, n_sup)

    for kw, word in ((dict(logits=None), b"NULL"), (dict(hist=None), b"NULL"), (dict(B=0), b"B <= 64"), (dict(B=65), b"B <= 64"),
                     (dict(g=9), b"capacity"), (dict(g=-1), b"capacity"), (dict(p=0.0), b"repetition_penalty"),
                     (dict(p=math.nan), b"repetition_penalty"), (dict(n=-1), b"no_repeat_ngram_size"), (dict(m=-1), b"min_new_tokens"),
                     (dict(eos=lst, n_eos=17), b"at most 16"), (dict(sup=lst, n_sup=257), b"at most 256"), (dict(n_eos=2), b"NULL"),
                     (dict(sup=lst, n_sup=1, V=3), b"outside [0, vocab")):
        assert op(**kw) != 0, kw
        assert word in lib.fvhd_last_error(), (kw, lib.fvhd_last_error())
