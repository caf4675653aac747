"""Prompt-lookup decoding under sampling, without a device: the new entry points' argument checks, lookup_sample's refusals before
anything is touched, and the routing of transformers' `prompt_lookup_num_tokens` by `_library_generate_settings`."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402


def test_the_entry_points_reject_bad_arguments():
    from ml_fastvlm_amd import _lib
    lib = _lib.lookup_sample_lib()
    one = C.c_void_p(16)                                         # never dereferenced: every call below fails its argument checks
    assert lib.fvhd_llm_set_verify_sampling(None, 1) != 0 and b"ctx is NULL" in lib.fvhd_last_error()
    assert lib.fvhd_llm_lookup_logprobs(None, 5, one, one, one, None) != 0 and b"NULL" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_sample_rows(None, None, 4, 64, 1.0, 0, 1.0, 0, 0, 0, None, one, None, None, None, None) != 0
    assert b"fvhd_op_dec_sample_rows: NULL" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_sample_rows(None, one, 17, 64, 1.0, 0, 1.0, 0, 0, 0, None, one, None, None, None, None) != 0
    assert b"B <= 16" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_sample_rows(None, one, 4, 64, 1.0, 0, 1.0, 0, 0, -1, None, one, None, None, None, None) != 0
    assert b"n0" in lib.fvhd_last_error()
    for (T, k, p), what in [((0.0, 50, 0.9), b"temperature"), ((0.7, -1, 0.9), b"top_k"), ((0.7, 50, 1.5), b"top_p")]:
        assert lib.fvhd_op_dec_sample_rows(None, one, 4, 64, T, k, p, 0, 0, 0, None, one, None, None, None, None) != 0
        assert what in lib.fvhd_last_error(), (T, k, p)


def _bare_generator(batch=1, capacity=64, run_batch=1):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen._processors, gen.device, gen.batch, gen.capacity, gen._run_batch = None, torch.device("cpu"), batch, capacity, run_batch
    gen._spec_rows, gen._spec_logits, gen._spec_ids, gen._spec_emitted = 0, None, None, None
    gen.pre = type("Pre", (), dict(vocab=64, _h=None))()         # no context: any call into the library would fail on it
    return gen


def test_lookup_sample_refuses_before_it_touches_a_device():
    gen = _bare_generator()
    x = torch.zeros(1, 10, 8)
    with pytest.raises(ValueError, match="lookup_sample: prompt-lookup decoding takes ONE sequence"):
        gen.lookup_sample(torch.zeros(2, 10, 8), max_new_tokens=4)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="max_new_tokens"):
            gen.lookup_sample(x, max_new_tokens=bad)
    for T in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="lookup_sample: temperature"):
            gen.lookup_sample(x, max_new_tokens=4, temperature=T)
    for p in (-0.1, 1.5, math.nan):
        with pytest.raises(ValueError, match="lookup_sample: top_p"):
            gen.lookup_sample(x, max_new_tokens=4, top_p=p)
    with pytest.raises(ValueError, match="lookup_sample: top_k"):
        gen.lookup_sample(x, max_new_tokens=4, top_k=-1)
    for k in (0, 16, -1):                                        # K outside 1 .. 15: T = K + 1 rows outside [2, 16]
        with pytest.raises(ValueError, match="lookup_sample: a verify step takes 2 .. 16 rows"):
            gen.lookup_sample(x, max_new_tokens=4, prompt_lookup_num_tokens=k)
    with pytest.raises(ValueError, match="lookup_sample: max_matching_ngram_size"):
        gen.lookup_sample(x, max_new_tokens=4, max_matching_ngram_size=17)
    with pytest.raises(ValueError, match=r"cache of 65 positions, reserved 64"):
        gen.lookup_sample(x, max_new_tokens=48, prompt_lookup_num_tokens=7)
    for n in (-1, 17, 2.0, True):
        with pytest.raises(ValueError, match="logprobs"):
            gen.lookup_sample(x, max_new_tokens=4, logprobs=n)
        with pytest.raises(ValueError, match="logprobs"):
            gen.lookup_greedy(x, max_new_tokens=4, logprobs=n)
    gen._processors = dict(repetition_penalty=1.2)
    with pytest.raises(ValueError, match="logits processors are set"):
        gen.lookup_sample(x, max_new_tokens=4)


# ---- the patched generate: transformers' prompt_lookup_num_tokens ----------------------------------------------------------------------------
PREDICT = dict(do_sample=True, temperature=0.2, top_p=None, num_beams=1, max_new_tokens=256, use_cache=True)   # predict.py's generate()
LOOKUP = dict(prompt_lookup_num_tokens=7)


def _settings(kw, **flags):
    from ml_fastvlm_amd.builder import _library_generate_settings
    return _library_generate_settings(L.tiny_qwen2(), dict(kw), **flags)


def test_one_prompt_is_routed_to_the_lookup_greedy_and_sampled():
    got, reason = _settings(dict(PREDICT, do_sample=False, **LOOKUP), prompt_lookup=True, batch=1)
    assert reason is None and got["sampling"] is None and got["beam"] is None
    assert got["lookup"] == dict(prompt_lookup_num_tokens=7, max_matching_ngram_size=2)
    got, reason = _settings(dict(PREDICT, **LOOKUP, max_matching_ngram_size=3), prompt_lookup=True, batch=1)
    assert reason is None and got["sampling"] == dict(temperature=pytest.approx(0.2), top_k=50, top_p=1.0)
    assert got["lookup"] == dict(prompt_lookup_num_tokens=7, max_matching_ngram_size=3)
    got, reason = _settings(dict(PREDICT), prompt_lookup=True, batch=1)      # the flag alone changes nothing about a call without the keyword
    assert reason is None and got["lookup"] is None


@pytest.mark.parametrize("kw,flags,names", [
    (dict(), dict(batch=2), ("prompt_lookup_num_tokens=7", "batch of 2")),
    (dict(num_beams=2, do_sample=False), dict(batch=1), ("num_beams=2",)),
    (dict(num_beams=2, do_sample=False), dict(batch=1, beam_search=True), ("prompt_lookup_num_tokens=7", "num_beams=2")),
    (dict(repetition_penalty=1.2), dict(batch=1), ("repetition_penalty=1.2",)),
    (dict(repetition_penalty=1.2), dict(batch=1, processors=True), ("prompt_lookup_num_tokens=7", "repetition_penalty")),
    (dict(prompt_lookup_num_tokens=16), dict(batch=1), ("prompt_lookup_num_tokens=16", "1 .. 15")),
    (dict(max_matching_ngram_size=17), dict(batch=1), ("max_matching_ngram_size=17",)),
])
def test_anything_else_falls_back_and_names_why(kw, flags, names):
    got, reason = _settings(dict(PREDICT, **dict(LOOKUP, **kw)), prompt_lookup=True, **flags)
    assert got is None
    for n in names:
        assert n in reason, (n, reason)


def test_with_the_flag_off_the_keyword_falls_back_as_before():
    got, reason = _settings(dict(PREDICT, **LOOKUP))
    assert got is None and reason == "prompt_lookup_num_tokens=7"
    got, reason = _settings(dict(PREDICT))
    assert reason is None and "lookup" not in got


def test_the_patched_generate_takes_the_flag():
    import inspect
    from ml_fastvlm_amd import builder
    assert inspect.signature(builder.install_into_llava).parameters["prompt_lookup"].default is False
    assert inspect.signature(builder._make_library_generate).parameters["prompt_lookup"].default is False
