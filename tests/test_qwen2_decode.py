"""CPU-side contract of the Qwen2 decode (ml_fastvlm_amd/qwen2_decode.py, builder.generate, _lib): no GPU needed."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from binding_stub import Everything, stub  # noqa: E402


def test_stale_library_fails_with_the_abi_message(monkeypatch):
    """_lib.load() compares fvhd_version() BEFORE it declares symbols: a library built before this binding's exports reports the ABI
    mismatch, not an AttributeError for the first symbol it lacks"""
    from ml_fastvlm_amd import _lib

    with pytest.raises(_lib.FvhdError, match="ABI version 500"):    # a library of version 500 that exports nothing else
        stub(monkeypatch, 500, [], without=Everything())


def test_binding_declares_the_decode_exports():
    from ml_fastvlm_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 501 and lib.fvhd_version() >= 501
    for n in ("fvhd_llm_cache_reserve", "fvhd_llm_start", "fvhd_llm_decode", "fvhd_llm_cache_state", "fvhd_llm_set_tied_embeddings",
              "fvhd_op_dec_gemm", "fvhd_op_dec_qkv", "fvhd_op_dec_attention", "fvhd_op_dec_lm_argmax"):
        assert getattr(lib, n).argtypes is not None, n


def test_decode_entry_points_reject_bad_arguments():
    from ml_fastvlm_amd import _lib
    lib = _lib.load()
    assert lib.fvhd_llm_cache_reserve(None, 1, 8) != 0
    assert lib.fvhd_llm_decode(None, None, None, None, None) != 0
    assert lib.fvhd_llm_start(None, None, 0, None, None, 1, 1, None, None, None) != 0
    assert lib.fvhd_op_dec_gemm(None, 4, None, 1, None, 1e-6, None, 16, 128, None, None, None, None, 1) != 0
    assert b"NULL" in lib.fvhd_last_error()


@pytest.mark.parametrize("kw,name", [(dict(do_sample=True), "do_sample"), (dict(num_beams=4), "num_beams"),
                                     (dict(repetition_penalty=1.2), "repetition_penalty"), (dict(num_beam_groups=2), "num_beam_groups")])
def test_generate_refuses_other_decoding_strategies(kw, name):
    import ml_fastvlm_amd as fv
    with pytest.raises(NotImplementedError, match=name):
        fv.generate(None, torch.zeros(1, 4, dtype=torch.long), **kw)


def test_generate_refuses_non_bf16_models():
    import ml_fastvlm_amd as fv
    with pytest.raises(ValueError, match="bf16 model on a HIP device"):
        fv.generate(L.tiny_qwen2(), torch.zeros(1, 4, dtype=torch.long), max_new_tokens=2)


@pytest.mark.parametrize("kind", ["left", "right", "none", "nomask"])
def test_position_ids_follow_transformers(kind):
    from transformers.generation.utils import GenerationMixin
    from ml_fastvlm_amd.qwen2_decode import generation_position_ids
    B, T = 3, 7
    mask = torch.ones(B, T, dtype=torch.long)
    if kind == "left":
        mask[1, :2] = 0
        mask[2, :5] = 0
    elif kind == "right":
        mask[1, 5:] = 0
        mask[2, 2:] = 0
    emb = torch.zeros(B, T, 8)
    kwargs = {} if kind == "nomask" else {"attention_mask": mask}
    want = GenerationMixin._prepare_position_ids_for_generation(None, emb, kwargs)
    got = generation_position_ids(None if kind == "nomask" else mask, B, T)
    assert torch.equal(got, want.expand(B, T))
    # the next step: the last column + 1, per row (a right-padded row continues at 0 + 1)
    if kind == "right":
        assert got[2, -1].item() + 1 == 1
