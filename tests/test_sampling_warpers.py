"""CPU-side contract of the sampling warpers min_p / typical_p / epsilon_cutoff / eta_cutoff (fvhd_llm_set_sampling_warpers,
qwen2_decode.normalize_warpers, builder's generate settings under sampling_warpers=True): no GPU needed."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from binding_stub import stub  # noqa: E402

PREDICT = dict(do_sample=True, temperature=0.2, top_p=None, num_beams=1, max_new_tokens=256, use_cache=True)   # predict.py's generate()


def test_entry_points_refuse_bad_values_and_name_them():
    from ml_fastvlm_amd import _lib
    lib = _lib.sampling_warpers_lib()
    assert lib.fvhd_llm_set_sampling_warpers(None, 0.0, 1.0, 0.0, 0.0) != 0 and b"NULL" in lib.fvhd_last_error()
    host, ids, info = torch.zeros(4), torch.zeros(1, dtype=torch.long), torch.zeros(8)      # never read: the arguments are refused first
    p, q, r = (C.c_void_p(t.data_ptr()) for t in (host, ids, info))
    for w, what in [((1.5, 1.0, 0.0, 0.0), b"min_p"), ((-0.1, 1.0, 0.0, 0.0), b"min_p"), ((math.nan, 1.0, 0.0, 0.0), b"min_p"),
                    ((0.0, 0.0, 0.0, 0.0), b"typical_p"), ((0.0, 1.5, 0.0, 0.0), b"typical_p"), ((0.0, math.nan, 0.0, 0.0), b"typical_p"),
                    ((0.0, 1.0, 1.0, 0.0), b"epsilon_cutoff"), ((0.0, 1.0, -0.5, 0.0), b"epsilon_cutoff"), ((0.0, 1.0, math.nan, 0.0), b"epsilon_cutoff"),
                    ((0.0, 1.0, 0.0, 1.0), b"eta_cutoff"), ((0.0, 1.0, 0.0, math.nan), b"eta_cutoff")]:
        assert lib.fvhd_op_dec_sample_warpers(None, p, 1, 4, 1.0, 0, 1.0, *w, 0, 0, 0, 0, None, q, r) != 0
        assert what in lib.fvhd_last_error(), w
    assert lib.fvhd_op_dec_sample_warpers(None, p, 1, 4, 0.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 0, 0, 0, 0, None, q, r) != 0 and b"temperature" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_sample_warpers(None, p, 1, 4, 1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 0, 0, 0, 0, None, q, None) != 0      # info is its output
    assert lib.fvhd_op_dec_sample_warpers(None, p, 65, 4, 1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 0, 0, 0, 0, None, q, r) != 0
    assert lib.fvhd_op_dec_sample_warpers(None, p, 17, 4, 1.0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 0, 1, 0, 0, None, q, r) != 0        # one sequence: T <= 16


def test_normalize_warpers():
    from ml_fastvlm_amd.qwen2_decode import WARPERS_OFF, normalize_warpers
    assert normalize_warpers("t") is None and normalize_warpers("t", **WARPERS_OFF) is None
    assert normalize_warpers("t", min_p=None, typical_p=1, epsilon_cutoff=0, eta_cutoff=0.0) is None
    assert normalize_warpers("t", min_p=0.1) == dict(WARPERS_OFF, min_p=0.1)
    assert normalize_warpers("t", typical_p=0.9, eta_cutoff=1e-3) == dict(WARPERS_OFF, typical_p=0.9, eta_cutoff=1e-3)
    for bad, word in [(dict(min_p=1.5), "min_p"), (dict(min_p=-1), "min_p"), (dict(min_p="a"), "min_p"), (dict(min_p=True), "min_p"),
                      (dict(typical_p=0.0), "typical_p"), (dict(typical_p=2), "typical_p"), (dict(epsilon_cutoff=1.0), "epsilon_cutoff"),
                      (dict(eta_cutoff=-0.1), "eta_cutoff"), (dict(eta_cutoff=math.nan), "eta_cutoff")]:
        with pytest.raises(ValueError, match=f"who: {word}"):
            normalize_warpers("who", **bad)


def test_a_library_built_before_the_warpers_names_the_rebuild(monkeypatch):
    """such a library loads and samples; set_sampling with the warpers off does not ask it for the new symbol, with one on it names the rebuild"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    calls = []
    lib = stub(monkeypatch, 510, calls, without=("fvhd_llm_set_sampling_warpers",))
    assert _lib.has("sampling") and not _lib.has("sampling_warpers") and "fvhd_op_dec_sample_warpers" not in vars(lib)
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen.pre = type("P", (), {"_h": None})()
    gen.set_sampling(True, 0.7, 50, 0.9, 1)
    gen.set_sampling(True, 0.7, 50, 0.9, 1, min_p=0.0, typical_p=1.0)
    for kw in (dict(min_p=0.1), dict(typical_p=0.5), dict(epsilon_cutoff=1e-3), dict(eta_cutoff=1e-3)):
        with pytest.raises(_lib.FvhdError, match="built before the sampling warpers.*rebuild the library"):
            gen.set_sampling(True, 0.7, 50, 0.9, 1, **kw)
    with pytest.raises(ValueError, match="min_p"):                # the argument rule comes first, and needs no library
        gen.set_sampling(True, 0.7, 50, 0.9, 1, min_p=2.0)


def test_set_sampling_sets_all_four_every_time(monkeypatch):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    got = []
    stub(monkeypatch, 510, [], fvhd_llm_set_sampling_warpers=lambda h, *w: got.append(w) or 0)
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen.pre = type("P", (), {"_h": None})()
    gen.set_sampling(True, 0.7, 50, 0.9, 1, min_p=0.1, eta_cutoff=0.002)
    gen.set_sampling(False)
    assert got == [(0.1, 1.0, 0.0, 0.002), (0.0, 1.0, 0.0, 0.0)]


def test_settings_without_the_flag_keep_falling_back():
    from ml_fastvlm_amd.builder import _library_generate_settings
    for kw, word in [(dict(min_p=0.1), "min_p=0.1"), (dict(typical_p=0.9), "typical_p=0.9"), (dict(epsilon_cutoff=1e-3), "epsilon_cutoff"),
                     (dict(eta_cutoff=1e-3), "eta_cutoff"), (dict(top_h=0.5), "top_h")]:
        got, reason = _library_generate_settings(L.tiny_qwen2(), dict(PREDICT, **kw))
        assert got is None and word in reason, (kw, reason)


def test_settings_with_the_flag_carry_the_warpers():
    from ml_fastvlm_amd.builder import _library_generate_settings
    m = L.tiny_qwen2()
    got, reason = _library_generate_settings(m, dict(PREDICT, min_p=0.1), sampling_warpers=True)
    assert reason is None and got["sampling"] == dict(temperature=pytest.approx(0.2), top_k=50, top_p=1.0, min_p=pytest.approx(0.1))
    got, reason = _library_generate_settings(m, dict(PREDICT, min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3), sampling_warpers=True)
    assert reason is None and {k: got["sampling"][k] for k in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")} == \
        dict(min_p=pytest.approx(0.05), typical_p=pytest.approx(0.9), epsilon_cutoff=pytest.approx(3e-4), eta_cutoff=pytest.approx(2e-3))
    got, reason = _library_generate_settings(m, dict(PREDICT), sampling_warpers=True)       # nothing asked: what it was
    assert reason is None and got["sampling"] == dict(temperature=pytest.approx(0.2), top_k=50, top_p=1.0)


def test_values_that_mean_off_are_passed_as_off():
    """what transformers itself treats as off: typical_p >= 1, a cutoff outside (0, 1), min_p = 0"""
    from ml_fastvlm_amd.builder import _library_generate_settings
    m = L.tiny_qwen2()
    for kw in (dict(typical_p=1.0), dict(epsilon_cutoff=0.0), dict(eta_cutoff=0.0), dict(min_p=0.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=1.5)):
        got, reason = _library_generate_settings(m, dict(PREDICT, **kw), sampling_warpers=True)
        if got is None:                                           # a value transformers' own config validation refuses: its generate reports it
            assert "do not resolve" in reason, (kw, reason)
            continue
        assert sorted(got["sampling"]) == ["temperature", "top_k", "top_p"], (kw, got["sampling"])


def test_what_keeps_falling_back_under_the_flag():
    from ml_fastvlm_amd.builder import _library_generate_settings
    m = L.tiny_qwen2()
    got, reason = _library_generate_settings(m, dict(PREDICT, top_h=0.5), sampling_warpers=True)
    assert got is None and "top_h" in reason
    got, reason = _library_generate_settings(m, dict(PREDICT, top_h=0.5, min_p=0.1), sampling_warpers=True)
    assert got is None and "top_h" in reason
    got, reason = _library_generate_settings(m, dict(PREDICT, do_sample=False, num_beams=4, min_p=0.1), sampling_warpers=True, beam_search=True)
    assert got is None and "min_p" in reason                      # the warpers are not used in beam search
    got, reason = _library_generate_settings(m, dict(PREDICT, do_sample=False, min_p=0.1), sampling_warpers=True)
    assert reason is None and got["sampling"] is None             # greedy: transformers ignores the warpers, so does the library


def test_the_feature_record_and_its_gates(monkeypatch):
    """`_lib.FEATURES_LATER["sampling_warpers"]`: what tests/test_lib_features.py checks of every entry of the pinned table"""
    from ml_fastvlm_amd import _lib
    assert list(_lib.FEATURES_LATER) == ["sampling_warpers"] and not set(_lib.FEATURES_LATER) & set(_lib.FEATURES)
    f = _lib.FEATURES_LATER["sampling_warpers"]
    assert f.since is None and f.probe == "fvhd_llm_set_sampling_warpers" and f.probe in f.sig and f.needs == "sampling"
    sigs = [n for t in (_lib.FEATURES, _lib.FEATURES_LATER) for g in t.values() for n in g.sig] + list(_lib.BASE_SIGNATURES)
    assert len(sigs) == len(set(sigs))                              # no symbol under two features
    built = _lib.load()                                             # the built library has it
    assert _lib.has("sampling_warpers") and _lib.require("sampling_warpers") is built and _lib.sampling_warpers_lib() is built
    for n in f.sig:
        assert getattr(built, n).argtypes is not None, n
    lib = stub(monkeypatch, 510, [])                                # a library that has it gets it declared
    assert _lib.has("sampling_warpers") and _lib.sampling_warpers_lib() is lib
    for n, (res, args) in f.sig.items():
        assert n in vars(lib) and (getattr(lib, n).restype, getattr(lib, n).argtypes) == (res, args), n
    lib = stub(monkeypatch, 510, [], without=(f.probe,))            # one built before it loads, keeps everything older, names the rebuild
    assert _lib.load() is lib and not _lib.has("sampling_warpers") and not set(f.sig) & set(vars(lib))
    for other, g in _lib.FEATURES.items():
        assert _lib.has(other) and set(g.sig) <= set(vars(lib)), other
    for gate in (lambda: _lib.require("sampling_warpers"), _lib.sampling_warpers_lib):
        with pytest.raises(_lib.FvhdError, match="rebuild the library") as e:
            gate()
        assert f"built before {f.phrase}" in str(e.value) and "ABI version 510" in str(e.value) and f.names in str(e.value)
    stub(monkeypatch, _lib.SAMPLING_VERSION - 1, [])                # without sampling itself: sampling's message
    with pytest.raises(_lib.FvhdError, match="needs 502 - rebuild"):
        _lib.sampling_warpers_lib()
