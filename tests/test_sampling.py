"""CPU-side contract of the token sampler (qwen2_decode.philox_uniform, _lib's 502 symbols, builder's generate settings): no GPU needed."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from binding_stub import stub  # noqa: E402


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, want):
    from ml_fastvlm_amd.qwen2_decode import philox4x32_10
    assert tuple(philox4x32_10(counter, key)) == want


def test_philox_uniform_is_an_fp32_value_in_unit_interval():
    from ml_fastvlm_amd.qwen2_decode import philox4x32_10, philox_uniform
    seed = 0x0123456789ABCDEF
    u = philox_uniform(seed, 3, 285)
    x0 = philox4x32_10((3, 285, 0, 0), (0x89ABCDEF, 0x01234567))[0]
    assert u == (x0 >> 8) / 2 ** 24 and 0.0 <= u < 1.0
    assert torch.tensor(u, dtype=torch.float32).item() == u


def test_sampling_entry_points_reject_bad_arguments():
    from ml_fastvlm_amd import _lib
    lib = _lib.sampling_lib()
    assert lib.fvhd_llm_set_sampling(None, 1, 0.7, 50, 0.9, 1) != 0
    assert b"NULL" in lib.fvhd_last_error()
    host = torch.zeros(4)                                       # never read: the arguments are refused first
    ids = torch.zeros(1, dtype=torch.long)
    p, q = C.c_void_p(host.data_ptr()), C.c_void_p(ids.data_ptr())
    for (T, k, top_p), what in [((0.0, 50, 0.9), b"temperature"), ((math.nan, 50, 0.9), b"temperature"), ((math.inf, 50, 0.9), b"temperature"),
                                ((0.7, 50, 1.5), b"top_p"), ((0.7, -1, 0.9), b"top_k"), ((0.7, 50, math.nan), b"top_p")]:
        assert lib.fvhd_op_dec_sample(None, p, 1, 4, T, k, top_p, 0, 0, None, q, None) != 0
        assert what in lib.fvhd_last_error(), (T, k, top_p)
    assert lib.fvhd_op_dec_sample(None, None, 1, 4, 1.0, 0, 1.0, 0, 0, None, q, None) != 0
    assert lib.fvhd_op_dec_sample(None, p, 17, 4, 1.0, 0, 1.0, 0, 0, None, q, None) != 0


def test_a_501_library_loads_and_sampling_names_the_rebuild(monkeypatch):
    """a library built before sampling (version 501, none of the 502 exports) still loads - greedy decoding works on it - and the
    sampling entry points raise FvhdError naming 502 instead of an AttributeError"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator

    lib = stub(monkeypatch, 501, [], without=("fvhd_llm_set_sampling", "fvhd_op_dec_sample"))
    assert lib.fvhd_version() == 501
    with pytest.raises(_lib.FvhdError, match="502"):
        _lib.sampling_lib()
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen.pre = None
    with pytest.raises(_lib.FvhdError, match="502"):
        gen.set_sampling(True, 0.7, 50, 0.9, 1)
    gen._set_greedy()                                           # greedy on a 501 library: nothing to set


PREDICT = dict(do_sample=True, temperature=0.2, top_p=None, num_beams=1, max_new_tokens=256, use_cache=True)   # predict.py's generate()


def test_settings_of_predict_py_run_on_the_library():
    from ml_fastvlm_amd.builder import _library_generate_settings
    got, reason = _library_generate_settings(L.tiny_qwen2(), dict(PREDICT))
    assert reason is None
    assert got["max_new_tokens"] == 256 and got["sampling"] == dict(temperature=pytest.approx(0.2), top_k=50, top_p=1.0)


def test_settings_greedy_and_the_model_generation_config():
    from ml_fastvlm_amd.builder import _library_generate_settings
    got, reason = _library_generate_settings(L.tiny_qwen2(), dict(PREDICT, do_sample=False))
    assert reason is None and got["sampling"] is None
    m = L.tiny_qwen2()
    m.generation_config.top_k = 20
    got, reason = _library_generate_settings(m, dict(PREDICT))
    assert reason is None and got["sampling"]["top_k"] == 20


@pytest.mark.parametrize("kw,name", [(dict(num_beams=2), "num_beams"), (dict(repetition_penalty=1.2), "repetition_penalty"),
                                     (dict(min_p=0.1), "min_p"), (dict(max_new_tokens=None), "max_new_tokens"),
                                     (dict(output_scores=True, return_dict_in_generate=True), "output_scores"),
                                     (dict(use_cache=False), "use_cache"), (dict(logits_processor=[lambda i, s: s]), "logits_processor"),
                                     (dict(min_new_tokens=3), "min_new_tokens"), (dict(num_return_sequences=2), "num_return_sequences")])
def test_settings_outside_the_library_fall_back_with_the_reason(kw, name):
    from ml_fastvlm_amd.builder import _library_generate_settings
    got, reason = _library_generate_settings(L.tiny_qwen2(), dict(PREDICT, **kw))
    assert got is None and name in reason


def test_library_generate_falls_back_on_a_cpu_model_with_one_warning():
    import warnings
    from ml_fastvlm_amd.builder import _make_library_generate
    calls = []

    def orig(self, inputs=None, images=None, image_sizes=None, **kwargs):
        calls.append(kwargs)
        return "reference"

    m = L.tiny_qwen2()
    gen = _make_library_generate(orig)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert gen(m, torch.zeros(1, 4, dtype=torch.long), **PREDICT) == "reference"
        assert gen(m, torch.zeros(1, 4, dtype=torch.long), **PREDICT) == "reference"
    assert len(calls) == 2 and calls[0]["temperature"] == 0.2
    assert len([x for x in w if "generate stays on the reference" in str(x.message)]) == 1
    with pytest.raises(NotImplementedError, match="inputs_embeds"):
        gen(m, inputs_embeds=torch.zeros(1, 4, 64))


def test_install_into_llava_generate_replaces_the_reference_generate():
    from oracle import ref_import
    if not ref_import.reference_available():
        pytest.skip("the reference checkout is not on this machine")
    import sys
    ref_import.install_timm_stub()
    if ref_import.REFERENCE_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REFERENCE_ROOT)
    import ml_fastvlm_amd as fv
    lq = pytest.importorskip("llava.model.language_model.llava_qwen")
    import llava.model.llava_arch as arch
    import llava.model.multimodal_encoder.builder as enc_builder
    before = lq.LlavaQwen2ForCausalLM.generate
    saved = (enc_builder.build_vision_tower, arch.build_vision_tower, arch.LlavaMetaForCausalLM.encode_images)
    try:
        fv.install_into_llava(generate=True)
        after = lq.LlavaQwen2ForCausalLM.generate
        assert getattr(after, "_fvhd_generate", False) and after._fvhd_orig is getattr(before, "_fvhd_orig", before)
        fv.install_into_llava(generate=True)                   # idempotent: wraps the reference's generate, never a wrapper
        assert lq.LlavaQwen2ForCausalLM.generate._fvhd_orig is after._fvhd_orig
    finally:                                                    # the tower patches of install_into_llava too: other tests import llava
        lq.LlavaQwen2ForCausalLM.generate = before
        enc_builder.build_vision_tower, arch.build_vision_tower, arch.LlavaMetaForCausalLM.encode_images = saved
