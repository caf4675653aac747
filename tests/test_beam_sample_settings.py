"""CPU-side contract of beam-search sampling (fvhd_llm_beam_sample_topk, Qwen2Generator.beam_search(do_sample=True), builder's generate
settings under beam_sample=True): no GPU needed."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from binding_stub import stub  # noqa: E402

PREDICT = dict(do_sample=True, temperature=0.2, top_p=None, num_beams=4, max_new_tokens=256, use_cache=True)   # predict.py --num_beams 4


def test_predicts_call_resolves_to_sampled_beam_settings_under_the_flag():
    from ml_fastvlm_amd.builder import _library_generate_settings
    got, reason = _library_generate_settings(L.tiny_qwen2(), dict(PREDICT), beam_search=True, beam_sample=True)
    assert reason is None and got["sampling"] is None
    assert got["beam"] == dict(num_beams=4, length_penalty=1.0, early_stopping=False, num_return_sequences=1, do_sample=True,
                               temperature=pytest.approx(0.2), top_k=50, top_p=1.0)
    got, reason = _library_generate_settings(L.tiny_qwen2(), dict(PREDICT, top_p=0.9, top_k=0, num_return_sequences=2), beam_search=True, beam_sample=True)
    assert reason is None and got["beam"]["top_k"] == 0 and got["beam"]["top_p"] == pytest.approx(0.9) and got["beam"]["num_return_sequences"] == 2


def test_without_the_flag_the_call_falls_back_with_todays_reason():
    from ml_fastvlm_amd.builder import _library_generate_settings
    m = L.tiny_qwen2()
    got, reason = _library_generate_settings(m, dict(PREDICT), beam_search=True)
    assert got is None and reason == "do_sample=True with num_beams=4 (beam sampling)"
    got, reason = _library_generate_settings(m, dict(PREDICT))                      # no beam search at all: as ever
    assert got is None and "num_beams=4" in reason
    got, reason = _library_generate_settings(m, dict(PREDICT), beam_sample=True)    # the flag alone does not switch beam search on
    assert got is None and "num_beams=4" in reason
    # and greedy beam search is what it was, with or without the flag
    want, _ = _library_generate_settings(m, dict(PREDICT, do_sample=False, temperature=None), beam_search=True)
    got, reason = _library_generate_settings(m, dict(PREDICT, do_sample=False, temperature=None), beam_search=True, beam_sample=True)
    assert reason is None and got == want and sorted(got["beam"]) == ["early_stopping", "length_penalty", "num_beams", "num_return_sequences"]
    # one beam under the flag: plain sampling, as before
    got, reason = _library_generate_settings(m, dict(PREDICT, num_beams=1), beam_search=True, beam_sample=True)
    assert reason is None and got["beam"] is None and got["sampling"] == dict(temperature=pytest.approx(0.2), top_k=50, top_p=1.0)


def test_what_keeps_falling_back_under_the_flag():
    from ml_fastvlm_amd.builder import _library_generate_settings
    m = L.tiny_qwen2()
    for kw, word in [(dict(min_p=0.1), "min_p"), (dict(typical_p=0.9), "typical_p"), (dict(epsilon_cutoff=1e-3), "epsilon_cutoff"),
                     (dict(eta_cutoff=1e-3), "eta_cutoff"), (dict(top_h=0.5), "top_h"), (dict(repetition_penalty=1.2), "repetition_penalty"),
                     (dict(num_beam_groups=2, diversity_penalty=0.5), "num_beam_groups"), (dict(guidance_scale=1.5), "guidance_scale"),
                     (dict(prompt_lookup_num_tokens=3), "prompt_lookup_num_tokens")]:
        got, reason = _library_generate_settings(m, dict(PREDICT, **kw), beam_search=True, beam_sample=True, sampling_warpers=True, processors=True)
        assert got is None and word in reason, (kw, reason)
    got, reason = _library_generate_settings(m, dict(PREDICT, temperature=0.0), beam_search=True, beam_sample=True)
    assert got is None                                            # do_sample with temperature 0: transformers' own complaint, or ours


def test_beam_search_and_beam_generate_refuse_bad_sampling_arguments():
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    gen = Qwen2Generator.__new__(Qwen2Generator)
    e = torch.zeros(1, 4, 8)
    for kw, word in [(dict(temperature=0.0), "temperature"), (dict(temperature=math.inf), "temperature"), (dict(temperature="a"), "temperature"),
                     (dict(top_k=-1), "top_k"), (dict(top_k=2.5), "top_k"), (dict(top_p=1.5), "top_p"), (dict(top_p=-0.1), "top_p"),
                     (dict(seed=1.5), "seed")]:
        with pytest.raises(ValueError, match=f"beam_search: {word}"):
            gen.beam_search(e, num_beams=2, max_new_tokens=4, do_sample=True, **kw)
        if "seed" not in kw:
            with pytest.raises(ValueError, match=f"beam_generate: {word}"):
                builder.beam_generate(L.tiny_qwen2(), torch.zeros(1, 4, dtype=torch.long), num_beams=2, max_new_tokens=4, do_sample=True, **kw)
    with pytest.raises(ValueError, match="greedy"):
        gen.beam_search(e, num_beams=1, max_new_tokens=4, do_sample=True)
    out_v, out_i = torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.long)
    for kw, word in [(dict(temperature=-1.0), "temperature"), (dict(min_keep=0), "min_keep"), (dict(min_keep=5), "min_keep"), (dict(min_keep=True), "min_keep")]:
        with pytest.raises(ValueError, match=f"beam_sample_topk: {word}"):
            gen.beam_sample_topk(torch.zeros(2, 16), torch.zeros(1, 2), 4, out_v, out_i, **kw)


def test_entry_points_refuse_bad_values_and_name_them():
    from ml_fastvlm_amd import _lib
    lib = _lib.beam_sample_lib()
    assert lib.fvhd_llm_beam_sample_reserve(None) != 0 and b"NULL" in lib.fvhd_last_error()
    assert lib.fvhd_llm_beam_sample_topk(None, None, None, 1, 2, 4, 1.0, 0, 1.0, 2, 0, None, None, None) != 0 and b"NULL" in lib.fvhd_last_error()
    host = torch.zeros(64 + 4)
    off = (-host.data_ptr() // 4) % 4                              # a 16-byte aligned window of host memory: never read, the arguments are refused first
    x = host[off:off + 64]
    sc, ov, oi = torch.zeros(2), torch.zeros(4), torch.zeros(4, dtype=torch.long)
    p, q, r, s = (C.c_void_p(t.data_ptr()) for t in (x, sc, ov, oi))

    def call(G=1, K=2, keep=4, V=32, T=1.0, top_k=0, top_p=1.0, m=2, n=0):
        return lib.fvhd_op_dec_beam_sample(None, p, q, G, K, keep, V, T, top_k, top_p, m, 0, n, None, None, None, r, s)
    for kw, what in [(dict(T=0.0), b"temperature"), (dict(T=math.nan), b"temperature"), (dict(top_k=-1), b"top_k"), (dict(top_p=1.5), b"top_p"),
                     (dict(m=0), b"min_keep"), (dict(m=5), b"min_keep"), (dict(n=-1), b"n must be"), (dict(K=1), b"num_beams"), (dict(K=17), b"num_beams"),
                     (dict(keep=65, V=4096), b"keep"), (dict(V=40), b"V % 16"), (dict(G=33), b"groups * num_beams"), (dict(keep=20, V=16), b"keep <= V")]:
        assert call(**kw) != 0, kw
        assert what in lib.fvhd_last_error(), (kw, lib.fvhd_last_error())
    assert lib.fvhd_op_dec_beam_sample(None, None, q, 1, 2, 4, 32, 1.0, 0, 1.0, 2, 0, 0, None, None, None, r, s) != 0 and b"NULL" in lib.fvhd_last_error()


def test_a_library_built_before_the_feature_names_the_rebuild(monkeypatch):
    """such a library loads and runs greedy beam search; only the sampled call asks for the new symbols and names the rebuild"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    lib = stub(monkeypatch, 510, [], without=("fvhd_llm_beam_sample_topk",))
    assert _lib.has("beam") and not _lib.has("beam_sample") and "fvhd_op_dec_beam_sample" not in vars(lib) and _lib.beam_lib() is lib
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen.pre = type("P", (), {"_h": None, "vocab": 16})()
    gen.device = torch.device("cpu")
    with pytest.raises(_lib.FvhdError, match="built before beam-search sampling.*rebuild the library"):
        gen.beam_sample_topk(torch.zeros(2, 16), torch.zeros(1, 2), 4, torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.long))


def test_the_feature_record_and_its_gates(monkeypatch):
    from ml_fastvlm_amd import _lib
    assert list(_lib.FEATURES_LATEST) == ["beam_sample"] and not set(_lib.FEATURES_LATEST) & (set(_lib.FEATURES) | set(_lib.FEATURES_LATER))
    f = _lib.FEATURES_LATEST["beam_sample"]
    assert f.since is None and f.probe == "fvhd_llm_beam_sample_topk" and f.probe in f.sig and f.needs == "beam"
    sigs = [n for t in (_lib.FEATURES, _lib.FEATURES_LATER, _lib.FEATURES_LATEST) for g in t.values() for n in g.sig] + list(_lib.BASE_SIGNATURES)
    assert len(sigs) == len(set(sigs))                              # no symbol under two features
    built = _lib.load()                                             # the built library has it
    assert _lib.has("beam_sample") and _lib.require("beam_sample") is built and _lib.beam_sample_lib() is built
    for n in f.sig:
        assert getattr(built, n).argtypes is not None, n
    lib = stub(monkeypatch, 510, [])                                # a library that has it gets it declared
    assert _lib.has("beam_sample") and _lib.beam_sample_lib() is lib
    for n, (res, args) in f.sig.items():
        assert n in vars(lib) and (getattr(lib, n).restype, getattr(lib, n).argtypes) == (res, args), n
    lib = stub(monkeypatch, 510, [], without=(f.probe,))            # one built before it loads, keeps everything older
    assert _lib.load() is lib and not _lib.has("beam_sample") and not set(f.sig) & set(vars(lib))


def test_beam_search_draws_with_min_keep_from_the_eos_list(monkeypatch):
    """the step under do_sample calls beam_sample_topk with min_keep = n_eos + 1 (2 without EOS) and the run's seed, never beam_topk"""
    from ml_fastvlm_amd import beam
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    assert beam.beams_to_keep(4, 0) == 8 and beam.beams_to_keep(4, 3) == 16
    seen = []

    class Stop(Exception):
        pass

    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen.pre = type("P", (), {"_h": None, "vocab": 16})()
    gen.device, gen.batch, gen.capacity = torch.device("cpu"), 8, 32
    gen._logits = torch.zeros(8, 16)
    monkeypatch.setattr(Qwen2Generator, "beam_reserve", lambda self: None)
    monkeypatch.setattr(Qwen2Generator, "beam_sample_reserve", lambda self: seen.append("reserve"))
    monkeypatch.setattr(Qwen2Generator, "_set_greedy", lambda self: None)
    monkeypatch.setattr(Qwen2Generator, "start", lambda self, *a, **k: (torch.zeros(2, 16), None))
    monkeypatch.setattr(Qwen2Generator, "cache_gather", lambda self, *a: None)
    monkeypatch.setattr(Qwen2Generator, "beam_topk", lambda self, *a: (_ for _ in ()).throw(AssertionError("beam_topk under do_sample")))

    def topk(self, logits, scores, keep, out_v, out_i, **kw):
        seen.append((keep, kw))
        raise Stop
    monkeypatch.setattr(Qwen2Generator, "beam_sample_topk", topk)
    for eos, m in ((None, 2), (5, 2), ([5, 6, 7], 4)):
        with pytest.raises(Stop):
            gen.beam_search(torch.zeros(2, 4, 8), num_beams=4, max_new_tokens=4, eos_token_id=eos, do_sample=True, temperature=0.5, top_k=7, top_p=0.9, seed=99)
        keep, kw = seen[-1]
        assert keep == max(2, m) * 4 and kw == dict(temperature=0.5, top_k=7, top_p=0.9, min_keep=m, seed=99) and seen[-2] == "reserve"
    torch.manual_seed(3)
    with pytest.raises(Stop):
        gen.beam_search(torch.zeros(2, 4, 8), num_beams=4, max_new_tokens=4, do_sample=True)
    a = seen[-1][1]
    torch.manual_seed(3)
    with pytest.raises(Stop):
        gen.beam_search(torch.zeros(2, 4, 8), num_beams=4, max_new_tokens=4, do_sample=True)
    assert seen[-1][1] == a and a["top_k"] == 50 and a["temperature"] == 1.0 and 0 <= a["seed"] < 2 ** 63     # seed None: torch.manual_seed repeats it
