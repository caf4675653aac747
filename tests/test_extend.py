"""Extending a started KV cache, without a GPU: the refusals of the C entry points and of the Python methods (all raised
before any device is looked at) and GenerationSession's chunk building and keep-length bookkeeping on plain tensors."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ml_fastvlm_amd import GenerationSession, _lib  # noqa: E402
from ml_fastvlm_amd.builder import session_chunk, session_keep  # noqa: E402
from ml_fastvlm_amd.qwen2_decode import Qwen2Generator  # noqa: E402


def test_the_entry_points_reject_bad_arguments():
    lib = _lib.extend_lib()
    one = C.c_void_p(16)                                        # a non-NULL pointer that no refused call may touch
    err = lambda: lib.fvhd_last_error()
    assert lib.fvhd_llm_extend(None, one, 2, None, None, 4, None, None, None) != 0 and b"NULL" in err()
    assert lib.fvhd_llm_cache_rewind(None, one, None) != 0 and b"NULL" in err()
    assert lib.fvhd_op_attention_extend(None, one, one, one, one, one, 1, 4, 4, 2, 32, 64, one) != 0 and b"head_dim" in err()
    assert lib.fvhd_op_attention_extend(None, one, one, one, one, one, 1, 0, 4, 2, 64, 64, one) != 0 and b"T <= capacity" in err()
    assert lib.fvhd_op_attention_extend(None, one, one, one, one, one, 1, 65, 4, 2, 64, 64, one) != 0 and b"T <= capacity" in err()
    assert lib.fvhd_op_attention_extend(None, one, one, one, one, one, 1, 4, 5, 2, 64, 64, one) != 0 and b"multiple of n_kv_heads" in err()
    assert lib.fvhd_op_attention_extend(None, one, one, one, one, one, 1, 4, 4, 2, 64, 64, None) != 0 and b"NULL" in err()
    assert lib.fvhd_op_cache_append(None, one, one, one, None, None, 1, 9, 4, 2, 64, 8, one, one) != 0 and b"T <= capacity" in err()
    assert lib.fvhd_op_cache_append(None, one, one, one, None, None, 1, 4, 4, 2, 60, 8, one, one) != 0 and b"head_dim % 8" in err()
    assert lib.fvhd_op_cache_append(None, one, one, one, None, None, 1, 4, 4, 2, 64, 8, one, None) != 0 and b"NULL" in err()
    assert lib.fvhd_op_extend_positions(None, one, None, one, 0, 4) != 0 and b"B >= 1" in err()
    assert lib.fvhd_op_cache_rewind(None, one, 65, one, one, 8, one, one) != 0 and b"rows <= 64" in err()
    assert lib.fvhd_op_cache_rewind(None, None, 1, one, one, 8, one, one) != 0 and b"NULL" in err()


# ---- the generator's refusals ------------------------------------------------------------------------------------------------------------
def _bare_generator(batch=4, capacity=64, run_batch=2, length=10):
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen._processors, gen.device, gen.batch, gen.capacity, gen._run_batch, gen._length = None, torch.device("cpu"), batch, capacity, run_batch, length
    gen.pre = type("Pre", (), dict(vocab=64, hidden=8, _h=None))()
    return gen


def test_extend_refuses_before_it_touches_a_device():
    x = torch.zeros(2, 5, 8)
    with pytest.raises(RuntimeError, match="no started sequence"):
        _bare_generator(run_batch=0).extend(x)
    with pytest.raises(ValueError, match="started batch is 2"):
        _bare_generator().extend(torch.zeros(3, 5, 8))
    with pytest.raises(ValueError, match="chunk length 65"):
        _bare_generator().extend(torch.zeros(2, 65, 8))
    with pytest.raises(ValueError, match=r"\[B, T, hidden\]"):
        _bare_generator().extend(torch.zeros(2, 8))
    gen = _bare_generator()
    gen._processors = dict(repetition_penalty=1.2)
    with pytest.raises(ValueError, match="logits processors are set"):
        gen.extend(x)
    with pytest.raises(ValueError, match="logits processors are set"):
        gen.rewind([1, 1])


def test_rewind_refuses_before_it_touches_a_device():
    with pytest.raises(RuntimeError, match="no started sequence"):
        _bare_generator(run_batch=0).rewind([1])
    with pytest.raises(ValueError, match="one int32 / int64 entry per started row"):
        _bare_generator().rewind([1, 2, 3])
    with pytest.raises(ValueError, match="one int32 / int64 entry per started row"):
        _bare_generator().rewind(torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match=r"must lie in \[0, the cache length 10\]"):
        _bare_generator().rewind([3, 11])
    with pytest.raises(ValueError, match="must lie in"):
        _bare_generator().rewind(torch.tensor([-1, 2]))


def test_continue_cache_checks_the_capacity_against_the_tracked_length():
    gen = _bare_generator(capacity=64, length=40)
    with pytest.raises(ValueError, match=r"the cached 40 \+ chunk 20 \+ 8 new tokens need a cache of 67 positions, reserved 64"):
        gen._run(torch.zeros(2, 20, 8), None, None, 8, None, None, False, 16, continue_cache=True)
    with pytest.raises(RuntimeError, match="no started sequence"):
        _bare_generator(run_batch=0)._run(torch.zeros(2, 20, 8), None, None, 8, None, None, False, 16, continue_cache=True)
    assert gen.length() == 40                                   # known: no device is asked


# ---- the session's bookkeeping -----------------------------------------------------------------------------------------------------------
def test_session_chunk_is_left_padding_then_pending_then_the_new_ids():
    ids, mask = session_chunk(torch.tensor([7, 8, 9]), torch.tensor([[1, 2, 3], [4, 0, 0], [0, 5, 6]]), torch.tensor([[1, 1, 1], [1, 0, 0], [0, 1, 1]]), 99)
    assert ids.tolist() == [[7, 1, 2, 3], [99, 99, 8, 4], [99, 9, 5, 6]]
    assert mask.tolist() == [[1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1]]
    ids, mask = session_chunk(torch.tensor([7]), torch.tensor([[1, 2]]))
    assert ids.tolist() == [[7, 1, 2]] and mask.tolist() == [[1, 1, 1]]
    with pytest.raises(ValueError, match="the session holds 2"):
        session_chunk(torch.tensor([7, 8]), torch.tensor([[1, 2]]))


def test_session_keep_counts_up_to_and_including_the_first_eos():
    # row 0: EOS (9) as its 2nd token, then the pads the run fed; row 1: no EOS; row 2: EOS first
    tokens = torch.tensor([[5, 9, 0, 0], [1, 2, 3, 4], [9, 0, 0, 0]])
    keep, pending = session_keep(50, tokens, 9)
    assert keep == [51, 53, 50] and pending.tolist() == [9, 4, 9]
    keep, pending = session_keep(50, tokens, [3, 9])
    assert keep == [51, 52, 50] and pending.tolist() == [9, 3, 9]
    keep, pending = session_keep(7, tokens, None)
    assert keep == [10, 10, 10] and pending.tolist() == [0, 4, 0]
    # the cache after n - 1 decode steps holds 50 + 3 slots: every keep is inside it
    assert max(session_keep(50, tokens, 9)[0]) <= 50 + tokens.shape[1] - 1


def test_a_session_starts_empty_and_fork_needs_one_row():
    s = GenerationSession(object(), batch=4, capacity=128)
    assert s.rows == 0 and s.length == 0
    with pytest.raises(ValueError, match="ONE started row"):
        s.fork(2)
    s._pending = torch.tensor([3])
    with pytest.raises(ValueError, match="exceed the session's batch 4"):
        s.fork(5)
    s.reset()
    assert s.rows == 0
