"""The decode's batch limit (64 sequences per step, include/fvhd.h version 503): constants, refusals before any pointer is read, the
502-library path and the generate fallback's reason.  No GPU."""
import ctypes as C
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from binding_stub import stub  # noqa: E402


def test_constants_and_versions():
    from ml_fastvlm_amd import _lib
    lib = _lib.load()
    assert _lib.MAX_DECODE_BATCH == 64
    assert _lib.WIDE_BATCH_VERSION == 503 <= lib.fvhd_version()
    assert _lib.ABI_VERSION == 501 and _lib.SAMPLING_VERSION == 502


def test_cache_reserve_names_the_limit():
    from ml_fastvlm_amd import _lib
    lib = _lib.load()
    assert lib.fvhd_llm_cache_reserve(None, 65, 8) != 0
    assert b"64" in lib.fvhd_last_error()
    assert lib.fvhd_llm_cache_reserve(None, 0, 8) != 0


def test_single_ops_refuse_65_rows_before_reading_anything():
    """host pointers and a NULL stream: a launch would fault, the refusal comes first and names the limit"""
    from ml_fastvlm_amd import _lib
    lib = _lib.load()
    host = torch.zeros(128)
    idb = torch.zeros(65, dtype=torch.long)
    p, q = C.c_void_p(host.data_ptr()), C.c_void_p(idb.data_ptr())
    for epi in (_lib.EPI_RESID, _lib.EPI_SWIGLU):
        assert lib.fvhd_op_dec_gemm(None, epi, p, 65, None, 1e-6, p, 16, 128, p, p, None, None, 1) != 0
        assert b"B <= 64" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_lm_argmax(None, p, 65, None, 1e-6, p, 16, 128, None, q, p, p) != 0
    assert b"B <= 64" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_qkv(None, p, 65, 128, None, 1e-6, p, p, p, q, p, 16, 1e6, p, p, 8, p, 1, 1, 64, None, None, 1) != 0
    assert b"B <= 64" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_attention(None, p, p, p, p, p, 65, 1, 1, 64, 8, p, None, None, 1) != 0
    assert b"B <= 64" in lib.fvhd_last_error()
    # the sampler on its own keeps its contract of 16 rows
    assert _lib.sampling_lib().fvhd_op_dec_sample(None, p, 17, 4, 1.0, 0, 1.0, 0, 0, None, q, None) != 0
    assert b"B <= 16" in lib.fvhd_last_error()


def test_a_502_library_loads_and_a_wide_batch_names_the_rebuild(monkeypatch):
    """a library built before the batch tiles (version 502) still loads, the greedy set-up of a generator of up to 16 sequences works
    on it, and a wider batch raises FvhdError naming 503 instead of the library's own refusal"""
    from types import SimpleNamespace
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    reserved = []

    lib = stub(monkeypatch, 502, [], fvhd_llm_cache_reserve=lambda h, batch, cap: reserved.append((batch, cap)) or 0)
    assert lib.fvhd_version() == 502
    assert _lib.sampling_lib() is lib and _lib.decode_lib(1) is lib and _lib.decode_lib(16) is lib
    with pytest.raises(_lib.FvhdError, match="503"):
        _lib.decode_lib(17)
    pre = SimpleNamespace(_h=None, device=torch.device("cpu"), vocab=32, tie_word_embeddings=True)
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    gen = Qwen2Generator(pre, 16, 8)                              # 16 sequences: set up on the old library
    assert reserved == [(16, 8)] and gen.batch == 16
    gen._set_greedy()
    for batch in (17, 64):
        with pytest.raises(_lib.FvhdError, match="503"):
            Qwen2Generator(pre, batch, 8)
    assert reserved == [(16, 8)]                                  # the wide requests never reached the library


def test_more_than_64_sequences_is_refused_in_python_too():
    from ml_fastvlm_amd import _lib
    with pytest.raises(_lib.FvhdError, match="64"):
        _lib.decode_lib(65)


def test_batch_reason():
    from ml_fastvlm_amd.builder import _batch_reason
    assert _batch_reason(1) is None and _batch_reason(17) is None and _batch_reason(64) is None
    assert _batch_reason(65) == "batch 65 > 64"


def test_library_generate_falls_back_above_64_rows_with_the_batch_as_the_reason():
    from ml_fastvlm_amd.builder import _make_library_generate
    calls = []

    def orig(self, inputs=None, images=None, image_sizes=None, **kwargs):
        calls.append(inputs.shape[0])
        return "reference"

    m = L.tiny_qwen2()                                                   # a CPU model: the batch is checked before the device
    gen = _make_library_generate(orig)
    kw = dict(do_sample=False, num_beams=1, max_new_tokens=4, use_cache=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert gen(m, torch.zeros(65, 4, dtype=torch.long), **kw) == "reference"
    msgs = [str(x.message) for x in w if "generate stays on the reference" in str(x.message)]
    assert calls == [65] and len(msgs) == 1 and "batch 65 > 64" in msgs[0], msgs
    with warnings.catch_warnings(record=True) as w:                # 17 .. 64 rows: the batch is no reason any more (here the device is)
        warnings.simplefilter("always")
        assert gen(m, torch.zeros(17, 4, dtype=torch.long), **kw) == "reference"
    msgs = [str(x.message) for x in w if "generate stays on the reference" in str(x.message)]
    assert len(msgs) == 1 and "batch" not in msgs[0] and "HIP device" in msgs[0], msgs
