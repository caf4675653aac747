"""CPU: the host side of classifier-free guidance (include/fvhd.h "LLM classifier-free guidance") - the builder's settings resolution with
and without `guidance=True`, the fallback reasons, the Python-side refusals, the 2 G-row batch of a guided run, and the new symbols of the
built library."""
import inspect
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_reference as GR  # noqa: E402
import llm_testlib as L  # noqa: E402

import ml_fastvlm_amd  # noqa: E402
from ml_fastvlm_amd import _lib, builder  # noqa: E402
from ml_fastvlm_amd.qwen2_decode import Qwen2Generator, generation_position_ids, guidance_batch, normalize_guidance  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = torch.tensor([[3, 4, 5]])
BASE = dict(max_new_tokens=4, do_sample=False)


def _settings(kw, **flags):
    return builder._library_generate_settings(L.tiny_qwen2(), dict(BASE, **kw), **flags)


# ---- settings ----------------------------------------------------------------------------------------------------------------------------
def test_settings_accept_guidance_scale_under_the_flag_only():
    call = dict(guidance_scale=1.5, negative_prompt_ids=NEG, negative_prompt_attention_mask=torch.ones_like(NEG))
    settings, reason = _settings(call)
    assert settings is None and reason == "negative_prompt_ids is given"
    settings, reason = _settings(dict(guidance_scale=1.5))
    assert settings is None and reason == "guidance_scale=1.5"
    settings, reason = _settings(call, guidance=True, batch=1)
    assert reason is None and settings["sampling"] is None and settings["beam"] is None
    g = settings["guidance"]
    assert g["guidance_scale"] == 1.5 and g["negative_prompt_ids"] is NEG and torch.equal(g["negative_prompt_attention_mask"], torch.ones_like(NEG))
    # sampling composes; scale 1 / unset is off, with or without negative ids (transformers ignores them then)
    settings, reason = _settings(dict(call, do_sample=True, temperature=0.7), guidance=True, batch=1)
    assert reason is None and settings["sampling"]["temperature"] == 0.7 and settings["guidance"]["guidance_scale"] == 1.5
    for kw in (dict(), dict(guidance_scale=1.0), dict(negative_prompt_ids=NEG)):
        settings, reason = _settings(kw, guidance=True, batch=1)
        assert reason is None and settings["guidance"] is None, kw
    # without the flag the settings carry no such key
    assert "guidance" not in _settings(dict())[0]


def test_fallback_reasons_under_the_flag():
    def reason(kw, batch=1, **flags):
        settings, why = _settings(kw, guidance=True, batch=batch, **flags)
        assert settings is None
        return why

    assert "without negative_prompt_ids" in reason(dict(guidance_scale=1.5))
    assert "image placeholder" in reason(dict(guidance_scale=1.5, negative_prompt_ids=torch.tensor([[3, -200, 5]])))
    assert "at most 32" in reason(dict(guidance_scale=1.5, negative_prompt_ids=NEG.repeat(33, 1)), batch=33)
    assert "one negative prompt per prompt" in reason(dict(guidance_scale=1.5, negative_prompt_ids=NEG.repeat(2, 1)), batch=1)
    assert reason(dict(guidance_scale=1.5, negative_prompt_ids=NEG, num_beams=2)) == "num_beams=2"
    assert reason(dict(guidance_scale=1.5, negative_prompt_ids=NEG, num_beams=2), beam_search=True) == "guidance_scale=1.5"
    assert "prompt_lookup_num_tokens" in reason(dict(guidance_scale=1.5, negative_prompt_ids=NEG, prompt_lookup_num_tokens=3), prompt_lookup=True)
    assert reason(dict(guidance_scale=1.5, negative_prompt_ids=NEG, streamer=object())) == "streamer is given"


def test_the_flags_of_the_public_interface():
    assert inspect.signature(builder.install_into_llava).parameters["guidance"].default is False
    assert inspect.signature(builder._make_library_generate).parameters["guidance"].default is False
    for fn in (Qwen2Generator.greedy, Qwen2Generator.sample):
        p = inspect.signature(fn).parameters
        assert p["guidance_scale"].default is None and p["negative_inputs_embeds"].default is None
        assert p["negative_attention_mask"].default is None and p["negative_position_ids"].default is None
    p = inspect.signature(ml_fastvlm_amd.generate).parameters
    assert p["guidance_scale"].default is None and p["negative_prompt_ids"].default is None and p["negative_prompt_attention_mask"].default is None
    assert normalize_guidance(None) is None and normalize_guidance(1) is None and normalize_guidance(1.0) is None and normalize_guidance(-1) == -1.0
    for bad in (float("inf"), float("nan"), "2", True):
        with pytest.raises(ValueError, match="finite"):
            normalize_guidance(bad)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_python_side_refusals_name_their_reason():
    ids = torch.tensor([[1, 2, 3]])
    with pytest.raises(ValueError, match="without negative_prompt_ids"):
        ml_fastvlm_amd.generate(None, ids, guidance_scale=1.5)
    with pytest.raises(ValueError, match="at most 32"):
        ml_fastvlm_amd.generate(None, ids.repeat(33, 1), guidance_scale=1.5, negative_prompt_ids=NEG.repeat(33, 1))
    with pytest.raises(ValueError, match="prompt-lookup"):
        ml_fastvlm_amd.generate(None, ids, guidance_scale=1.5, negative_prompt_ids=NEG, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="beam search"):
        ml_fastvlm_amd.beam_generate(None, ids, guidance_scale=1.5)
    with pytest.raises(ValueError, match="beam search and the verify step do not take guidance"):
        builder._generate_on_library(None, None, None, None, None, None, 4, None, None, beam=dict(num_beams=2),
                                     guidance=dict(guidance_scale=1.5, negative_prompt_ids=NEG, negative_prompt_attention_mask=None))
    with pytest.raises(ValueError, match="sessions"):
        builder.GenerationSession.generate(None, ids, guidance_scale=1.5)
    with pytest.raises(ValueError, match="image placeholder"):
        builder._guidance_settings("generate", 1.5, torch.tensor([[3, -200]]), None, 1, text_only=True)
    assert builder._guidance_settings("generate", 1.5, torch.tensor([[3, -200]]), None, 1) is not None      # generate() splices it
    assert builder._guidance_settings("generate", None, None, None) is None


def _bare_generator(batch=64, guidance=None):
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen.batch, gen.capacity, gen._processors, gen._constraint, gen._guidance, gen._run_batch = batch, 64, None, None, guidance, 0
    return gen


def test_generator_refusals_touch_no_device():
    gen = _bare_generator()
    x = torch.zeros(2, 4, 8)
    with pytest.raises(ValueError, match="needs negative_inputs_embeds"):
        gen._guided_inputs("greedy", 1.5, x, None, None, None, None, None, False)
    with pytest.raises(ValueError, match="without a guidance_scale"):
        gen._guided_inputs("greedy", None, x, None, None, x, None, None, False)
    with pytest.raises(ValueError, match="at most 32 prompts"):
        gen._guided_inputs("greedy", 1.5, torch.zeros(33, 4, 8), None, None, torch.zeros(33, 2, 8), None, None, False)
    with pytest.raises(ValueError, match="one negative prompt per prompt"):
        gen._guided_inputs("greedy", 1.5, x, None, None, torch.zeros(3, 2, 8), None, None, False)
    with pytest.raises(ValueError, match="the reserved batch is 2"):
        _bare_generator(batch=2)._guided_inputs("sample", 1.5, x, None, None, x, None, None, False)
    assert gen._guided_inputs("greedy", 1.0, x, None, None, None, None, None, False) == (None, x, None, None)
    on = _bare_generator(guidance=1.5)
    with pytest.raises(ValueError, match="beam_search: guidance is set"):
        on.beam_search(x, num_beams=2)
    with pytest.raises(ValueError, match="lookup_greedy: guidance is set"):
        on._verify_refusal("lookup_greedy", 4)
    for who in ("rewind", "cache_gather"):
        with pytest.raises(ValueError, match=f"{who}: guidance is set"):
            on._guidance_refusal(who, "why")
    with pytest.raises(ValueError, match="the batch is odd"):
        on._note_choice(3)
    on._note_choice(6)
    assert on._choice_rows() == 3
    gen._run_batch = 3                                           # without guidance: the started batch, whatever a cache reorder makes of it
    gen._note_choice(3)
    assert gen._choice_rows() == 3
    gen._run_batch = 5
    assert gen._choice_rows() == 5


# ---- the 2 G-row batch -------------------------------------------------------------------------------------------------------------------
def test_the_batch_of_unequal_lengths():
    G, H = 2, 4
    e = torch.arange(G * 5 * H, dtype=torch.float32).view(G, 5, H) + 1
    m = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1]])
    ne = -(torch.arange(G * 3 * H, dtype=torch.float32).view(G, 3, H) + 1)
    nm = torch.tensor([[1, 1, 1], [0, 1, 1]])
    x2, m2, p2 = guidance_batch(e, m, None, ne, nm, None)
    want_x, want_m = GR.pair_batch(e, m, ne, nm)
    assert torch.equal(x2, want_x) and torch.equal(m2, want_m)
    assert m2.tolist() == [[1, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 1, 1]]
    # every half's real tokens keep the positions they have on their own: 0 .. n - 1, 0 on padding
    assert p2.tolist() == [[0, 1, 2, 3, 4], [0, 0, 0, 1, 2], [0, 0, 0, 1, 2], [0, 0, 0, 0, 1]]
    assert torch.equal(p2, generation_position_ids(m2, 4, 5))
    # the longer negative prompt pads the prompts; no masks = all valid; given position ids travel with their half
    x3, m3, p3 = guidance_batch(ne, None, None, e, None, torch.arange(5).repeat(G, 1) + 7)
    assert x3.shape == (4, 5, H) and m3.tolist() == [[0, 0, 1, 1, 1]] * 2 + [[1] * 5] * 2
    assert p3.tolist() == [[0, 0, 0, 1, 2]] * 2 + [[7, 8, 9, 10, 11]] * 2
    # a chunk for a started cache: no positions unless both halves bring theirs (extend continues every row)
    assert guidance_batch(e, m, None, ne, nm, None, positions=False)[2] is None
    with pytest.raises(ValueError, match=r"negative_attention_mask must be \[2, 3\]"):
        guidance_batch(e, m, None, ne, m, None)


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
NAMES = ("fvhd_dec_guidance_scratch_bytes", "fvhd_op_dec_guidance", "fvhd_llm_set_guidance")


def test_the_built_library_has_them_under_510():
    lib = _lib.guidance_lib()
    assert lib is _lib.load() and lib.fvhd_version() == 510
    for name in NAMES:
        assert hasattr(lib, name), name
    S = GR.slices(152064)
    assert lib.fvhd_dec_guidance_scratch_bytes(32, 152064) == 16384 + 2 * ((8 * 32 * S + 255) // 256 * 256) + 512
    assert lib.fvhd_dec_guidance_scratch_bytes(1, 5) == 16384 + 2 * 256 + 256
    assert lib.fvhd_dec_guidance_scratch_bytes(33, 64) == 0 and lib.fvhd_dec_guidance_scratch_bytes(1, 0) == 0
    assert _lib.MAX_GUIDANCE_PROMPTS == GR.MAX_PROMPTS == 32


def test_header_and_sources_declare_them_once():
    hdr = open(os.path.join(ROOT, "include", "fvhd.h")).read()
    assert "#define FVHD_VERSION 510" in hdr
    for name in NAMES:
        assert len(re.findall(rf"^(?:int|size_t) {name}\(", hdr, flags=re.M)) == 1, name
    csrc = os.path.join(ROOT, "ml_fastvlm_amd", "csrc")
    decl = re.compile(r"^\s*(?:extern \"C\" )?int fvhd_launch_dec_guidance\(", flags=re.M)
    where = sorted(f for f in os.listdir(csrc) if f.endswith((".h", ".hip")) and decl.search(open(os.path.join(csrc, f)).read()))
    assert where == ["launchers.h", "llm_guidance.hip"], where


def test_argument_checks_without_a_device():
    lib = _lib.guidance_lib()
    assert lib.fvhd_llm_set_guidance(None, 1.5) != 0 and "NULL" in lib.fvhd_last_error().decode()
    assert lib.fvhd_op_dec_guidance(None, None, 1, 8, 1.5, None, 0) != 0 and "NULL" in lib.fvhd_last_error().decode()
