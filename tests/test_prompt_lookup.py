"""Prompt-lookup decoding without a GPU: the drafting rule (`ml_fastvlm_amd.prompt_lookup.propose`, the specification of the device's
drafter), the binding's version gate, and the refusals that `Qwen2Generator` raises before any device is touched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from binding_stub import stub  # noqa: E402

from ml_fastvlm_amd.prompt_lookup import propose  # noqa: E402


# ---- the drafting rule -----------------------------------------------------------------------------------------------------------------
def test_no_match_fills_with_the_last_token():
    assert propose([1, 2, 3, 4], 2, 3) == [4, 4, 4]


def test_a_match_only_at_n_1():
    # the 2-gram (9, 3) occurs once (the suffix itself); the 1-gram 3 occurred at index 1
    assert propose([5, 3, 7, 8, 9, 3], 2, 3) == [7, 8, 9]


def test_the_longer_ngram_wins_over_a_later_shorter_match():
    # (1, 2) matches at 0 (-> 7); the 1-gram 2 also matches later at 4 (-> 9): n = 2 is tried first
    assert propose([1, 2, 7, 0, 2, 9, 1, 2], 2, 1) == [7]
    assert propose([1, 2, 7, 0, 2, 9, 1, 2], 1, 1) == [9]


def test_of_two_matches_the_later_one_wins():
    assert propose([1, 2, 5, 6, 1, 2, 8, 9, 1, 2], 2, 2) == [8, 9]


def test_a_continuation_that_runs_into_the_buffers_end():
    # the match at 1 is followed by (3, 4, 3) only: the rest is the last token
    assert propose([0, 3, 4, 3], 1, 5) == [4, 3, 3, 3, 3]
    # the suffix itself (i + n == len) is not a match: 7 occurs nowhere before
    assert propose([1, 7], 1, 2) == [7, 7]


def test_negative_ids_never_match_and_never_become_drafts():
    # inside the suffix window: (-200, 4) is skipped at n = 2 although it occurs at 0; n = 1 matches 4 at index 1
    assert propose([-200, 4, 6, -200, 4], 2, 2) == [6, 4]
    # inside the continuation: the drafts end before the placeholder
    assert propose([1, 2, 3, -200, 5, 1, 2], 2, 4) == [3, 2, 2, 2]
    # a continuation that starts with one: the match still ends the search, with no draft from it
    assert propose([2, -200, 9, 2], 1, 2) == [2, 2]
    # a negative last token: no suffix without it, so no match at any n (the fill is the last token as it is)
    assert propose([3, -1, 3, -1], 2, 2) == [-1, -1]


def test_buffers_of_length_1_and_2():
    assert propose([5], 2, 3) == [5, 5, 5]
    assert propose([5, 5], 2, 3) == [5, 5, 5]                     # n = 1: 5 at index 0 is followed by 5, then the buffer ends
    assert propose([5, 6], 4, 2) == [6, 6]


def test_k_1_and_k_15():
    seq = list(range(20)) + [0]
    assert propose(seq, 3, 1) == [1]
    assert propose(seq, 3, 15) == list(range(1, 16))
    assert propose([4, 0], 3, 15) == [0] * 15


def test_the_limits_are_checked():
    for kw in (dict(max_ngram=0, K=1), dict(max_ngram=17, K=1), dict(max_ngram=1, K=0), dict(max_ngram=1, K=16)):
        with pytest.raises(ValueError, match="max_ngram"):
            propose([1, 2], **kw)
    with pytest.raises(ValueError, match="empty"):
        propose([], 1, 1)


def test_propose_against_a_brute_force_restatement():
    g = torch.Generator().manual_seed(0)
    for _ in range(300):
        L = int(torch.randint(1, 40, (1,), generator=g))
        seq = (torch.randint(0, 4, (L,), generator=g) - (torch.rand(L, generator=g) < 0.1).long() * 7).tolist()
        n_max, K = int(torch.randint(1, 5, (1,), generator=g)), int(torch.randint(1, 16, (1,), generator=g))
        want = None
        for n in range(min(n_max, L - 1), 0, -1):
            hits = [i for i in range(L - n) if seq[i:i + n] == seq[L - n:] and all(t >= 0 for t in seq[L - n:])]
            if hits:
                want = []
                for t in seq[max(hits) + n:max(hits) + n + K]:
                    if t < 0:
                        break
                    want.append(t)
                break
        want = (want or []) + [seq[-1]] * (K - len(want or []))
        assert propose(seq, n_max, K) == want, (seq, n_max, K)


# ---- binding ---------------------------------------------------------------------------------------------------------------------------
def test_a_506_library_loads_and_lookup_names_the_rebuild(monkeypatch):
    from ml_fastvlm_amd import _lib
    calls = []
    lib = stub(monkeypatch, 506, calls)
    assert lib.fvhd_version() == 506
    gen = _bare_generator()
    with pytest.raises(_lib.FvhdError, match="507"):
        gen.spec_reserve(4)
    assert calls == []


def test_the_entry_points_reject_bad_arguments():
    import ctypes as C
    from ml_fastvlm_amd import _lib
    lib = _lib.lookup_lib()
    one = C.c_void_p(16)                                         # never dereferenced: every call below fails its argument checks
    assert lib.fvhd_llm_spec_reserve(None, 4, 0) != 0 and b"fvhd_llm_cache_reserve" in lib.fvhd_last_error()
    assert lib.fvhd_llm_verify(None, one, 4, None, None, None, None) != 0 and b"NULL" in lib.fvhd_last_error()
    assert lib.fvhd_llm_lookup_step(None, 4, 2, None) != 0 and b"NULL" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_attention_multi(None, one, one, one, one, one, one, one, 1, 4, 2, 64, 64, one, None, None, 1) != 0
    assert b"T <= 16" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_attention_multi(None, one, one, one, one, one, one, one, 4, 4, 2, 32, 64, one, None, None, 1) != 0
    assert b"head_dim" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_attention_multi(None, one, one, one, one, one, one, one, 4, 4, 2, 64, 64, one, None, None, 2) != 0
    assert b"splits" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_lookup_draft(None, one, one, 0, 3, one) != 0 and b"max_ngram" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_lookup_draft(None, one, one, 2, 16, one) != 0 and b"K <= 15" in lib.fvhd_last_error()
    assert lib.fvhd_op_dec_lookup_accept(None, one, one, 17, None, None, 0, None, 0, None, one, one, one, one, 8) != 0
    assert b"T <= 16" in lib.fvhd_last_error()


# ---- the generator's refusals ------------------------------------------------------------------------------------------------------------
def _bare_generator(batch=1, capacity=64, run_batch=1):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen._processors, gen.device, gen.batch, gen.capacity, gen._run_batch = None, torch.device("cpu"), batch, capacity, run_batch
    gen._spec_rows, gen._spec_logits, gen._spec_ids, gen._spec_emitted = 0, None, None, None
    gen.pre = type("Pre", (), dict(vocab=64, _h=None))()
    return gen


def test_lookup_greedy_refuses_what_it_does_not_cover():
    gen = _bare_generator()
    x = torch.zeros(1, 10, 8)
    with pytest.raises(ValueError, match="ONE sequence"):
        gen.lookup_greedy(torch.zeros(2, 10, 8), max_new_tokens=4)
    for k in (0, 16, -1):                                         # T = k + 1 outside [2, 16]
        with pytest.raises(ValueError, match="2 .. 16 rows"):
            gen.lookup_greedy(x, max_new_tokens=4, prompt_lookup_num_tokens=k)
    with pytest.raises(ValueError, match="max_matching_ngram_size"):
        gen.lookup_greedy(x, max_new_tokens=4, max_matching_ngram_size=0)
    # capacity: prompt + max_new_tokens + T - 1 (the last step's drafts need their slots)
    with pytest.raises(ValueError, match=r"cache of 65 positions, reserved 64"):
        gen.lookup_greedy(x, max_new_tokens=48, prompt_lookup_num_tokens=7)
    with pytest.raises(ValueError, match="max_new_tokens"):
        gen.lookup_greedy(x, max_new_tokens=0)
    gen._processors = dict(repetition_penalty=1.2)
    with pytest.raises(ValueError, match="logits processors are set"):
        gen.lookup_greedy(x, max_new_tokens=4)
    with pytest.raises(ValueError, match="logits processors are set"):
        gen.verify(torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match="logits processors are set"):
        gen.spec_reserve(4)


def test_verify_refuses_a_batch_and_a_bad_row_count():
    gen = _bare_generator(batch=4, run_batch=3)
    with pytest.raises(ValueError, match="ONE sequence - the started batch is 3"):
        gen.verify(torch.zeros(3, dtype=torch.long))
    gen = _bare_generator(run_batch=0)
    with pytest.raises(ValueError, match="start"):
        gen.verify(torch.zeros(3, dtype=torch.long))
    gen = _bare_generator()
    with pytest.raises(ValueError, match="2 .. 16 rows"):
        gen.verify(torch.zeros(16, dtype=torch.long))            # 17 rows
    with pytest.raises(ValueError, match="2 .. 16 rows"):
        gen.verify(torch.zeros(0, dtype=torch.long))             # 1 row: that is step()
    with pytest.raises(ValueError, match="int64"):
        gen.verify(torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="spec_reserve"):
        gen.verify(torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError, match="2 .. 16 rows"):
        gen.spec_reserve(17)


def test_generate_passes_the_keyword_on_and_refuses_a_batch(monkeypatch):
    from ml_fastvlm_amd import builder
    calls = []

    class Gen:
        def lookup_greedy(self, *a, **kw):
            calls.append(("lookup", kw))
            return "L"

        def greedy(self, *a, **kw):
            calls.append(("greedy", kw))
            return "G"

    caps = []
    monkeypatch.setattr(builder, "generator_context", lambda model, batch, capacity, weights=None: caps.append((batch, capacity)) or Gen())
    emb = torch.nn.Embedding(16, 8)
    m = type("M", (), dict(get_input_embeddings=lambda self: emb))()
    ids = torch.tensor([[1, 2, 3, 4, 5]])
    look = dict(prompt_lookup_num_tokens=5, max_matching_ngram_size=3, lookup_ids=ids)
    assert builder._generate_on_library(m, ids, None, None, None, None, 9, 1, 0, lookup=look) == "L"
    assert builder._generate_on_library(m, ids, None, None, None, None, 9, 1, 0) == "G"
    assert calls[0][0] == "lookup" and calls[0][1]["prompt_lookup_num_tokens"] == 5 and calls[0][1]["lookup_ids"] is ids
    assert calls[0][1]["max_new_tokens"] == 9 and calls[0][1]["eos_token_id"] == 1
    assert calls[1][0] == "greedy" and "lookup_ids" not in calls[1][1]
    assert caps == [(1, 5 + 9 + 5), (1, 5 + 9)]                   # the drafts of the last step need cache slots too

    class LM:
        lm_head = type("H", (), dict(weight=torch.zeros(1, dtype=torch.bfloat16, device="meta")))()
    with pytest.raises(ValueError, match="bf16 model on a HIP device"):
        builder.generate(LM(), ids, prompt_lookup_num_tokens=4)   # the keyword is accepted (no NotImplementedError for an unknown setting)
    with pytest.raises(ValueError, match="ONE prompt per call"):
        builder.generate(LM(), torch.zeros(2, 5, dtype=torch.long), prompt_lookup_num_tokens=4)
