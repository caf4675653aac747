"""CPU: the host side of the log-probabilities of generated tokens - `normalize_logprobs`, the binding of a library built before the entry
points, the declarations in include/fvhd.h and csrc/launchers.h, the `logprobs` keyword of greedy / sample / generate, and the refusals the
library makes before it touches a device."""
import inspect
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ml_fastvlm_amd  # noqa: E402
from ml_fastvlm_amd import _lib  # noqa: E402
from ml_fastvlm_amd.qwen2_decode import GenerationLogprobs, Qwen2Generator, normalize_logprobs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normalize_logprobs_accepts_and_refuses():
    assert normalize_logprobs(None) is None and normalize_logprobs(None, 4) is None
    for n in (0, 1, 5, 16):
        assert normalize_logprobs(n) == n and normalize_logprobs(n, 151936) == n
    assert normalize_logprobs(4, 4) == 4
    for bad in (1.0, "5", True, [3], torch.tensor(3)):
        with pytest.raises(ValueError, match="int"):
            normalize_logprobs(bad)
    for bad in (-1, 17, 1000):
        with pytest.raises(ValueError, match=r"\[0, 16\]"):
            normalize_logprobs(bad)
    with pytest.raises(ValueError, match="vocabulary"):
        normalize_logprobs(5, 4)
    assert _lib.MAX_LOGPROBS == 16


def test_the_header_declares_the_four_functions_and_the_launcher_once():
    hdr = open(os.path.join(ROOT, "include", "fvhd.h")).read()
    assert "#define FVHD_VERSION 510" in hdr
    for name in ("fvhd_dec_logprobs_scratch_bytes", "fvhd_op_dec_logprobs", "fvhd_llm_set_logprobs", "fvhd_llm_logprobs"):
        assert len(re.findall(r"^(?:int|size_t) " + name + r"\(", hdr, flags=re.M)) == 1, name
    csrc = os.path.join(ROOT, "ml_fastvlm_amd", "csrc")
    decl = re.compile(r"^\s*(?:extern \"C\" )?int fvhd_launch_dec_logprobs\(", flags=re.M)
    assert len(decl.findall(open(os.path.join(csrc, "launchers.h")).read())) == 1
    # the definition, and no second prototype anywhere else
    where = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and decl.search(open(os.path.join(csrc, f)).read())]
    assert where == ["launchers.h", "llm_logprobs.hip"], where


def test_the_scratch_size_is_the_documented_one():
    lib = _lib.logprobs_lib()
    pad = lambda x: (x + 255) // 256 * 256      # noqa: E731
    for B, V, n in ((1, 1, 0), (1, 17, 5), (3, 4096, 16), (64, 152064, 16), (17, 151936, 1)):
        S = 64 if V >= 131072 else (V + 2047) // 2048
        assert lib.fvhd_dec_logprobs_scratch_bytes(B, V, n) == 16384 + 2 * pad(4 * B * S) + pad(8 * B * S * n)
    for B, V, n in ((0, 8, 0), (65, 8, 0), (1, 0, 0), (1, 8, -1), (1, 8, 17)):
        assert lib.fvhd_dec_logprobs_scratch_bytes(B, V, n) == 0


def test_the_op_refuses_bad_arguments_with_a_message():
    """host pointers and a NULL stream: a launch would fault, the refusal comes first"""
    import ctypes as C
    lib = _lib.logprobs_lib()
    buf = (C.c_char * 4096)()
    p = C.cast(buf, C.c_void_p)

    def refused(*args):
        assert lib.fvhd_op_dec_logprobs(None, *args) != 0
        return lib.fvhd_last_error().decode()

    assert "NULL" in refused(None, p, 1, 8, 0, p, None, None, p, 4096)
    assert "NULL" in refused(p, p, 1, 8, 0, p, None, None, None, 4096)
    assert "B" in refused(p, p, 65, 8, 0, p, None, None, p, 4096)
    assert "V" in refused(p, p, 1, 0, 0, p, None, None, p, 4096)
    assert "top_n" in refused(p, p, 1, 64, 17, p, p, p, p, 4096)
    assert "exceeds" in refused(p, p, 1, 4, 5, p, p, p, p, 4096)
    assert "top_ids_out" in refused(p, p, 1, 8, 2, p, None, p, p, 4096)
    assert "scratch_bytes" in refused(p, p, 1, 8, 2, p, p, p, p, 512)
    assert lib.fvhd_llm_set_logprobs(None, 1) != 0 and "NULL" in lib.fvhd_last_error().decode()
    assert lib.fvhd_llm_logprobs(None, None, 0, p, None, None, None) != 0 and "NULL" in lib.fvhd_last_error().decode()


def test_greedy_sample_and_generate_take_logprobs():
    from ml_fastvlm_amd import builder
    for fn in (Qwen2Generator.greedy, Qwen2Generator.sample, ml_fastvlm_amd.generate, builder.GenerationSession.generate, builder._generate_on_library):
        p = inspect.signature(fn).parameters
        assert "logprobs" in p and p["logprobs"].default is None, fn
    assert "GenerationLogprobs" in ml_fastvlm_amd.__all__ and ml_fastvlm_amd.GenerationLogprobs is GenerationLogprobs
    assert GenerationLogprobs._fields == ("token_logprobs", "top_ids", "top_logprobs")


def test_generate_refuses_a_bad_logprobs_before_it_looks_at_the_model():
    with pytest.raises(ValueError, match=r"\[0, 16\]"):
        ml_fastvlm_amd.generate(None, None, logprobs=17)
    with pytest.raises(ValueError, match="prompt-lookup"):
        ml_fastvlm_amd.generate(None, None, logprobs=2, prompt_lookup_num_tokens=3)
