"""The order rules of the cache calls, without a GPU: the version that carries them, the generator's refusals behind a rewind / cache_gather
(raised before any device is looked at, on test_extend.py's bare generator)."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ml_fastvlm_amd import _lib  # noqa: E402
from ml_fastvlm_amd.qwen2_decode import Qwen2Generator  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STALE = "before the cache reorder / rewind"


def _bare_generator(batch=4, capacity=64, run_batch=1, length=10, stale=True):
    gen = Qwen2Generator.__new__(Qwen2Generator)
    gen._processors, gen.device, gen.batch, gen.capacity, gen._run_batch, gen._length = None, torch.device("cpu"), batch, capacity, run_batch, length
    gen._ids_stale, gen._spec_rows = stale, 16
    gen.pre = type("Pre", (), dict(vocab=64, hidden=8, _h=None))()
    return gen


def test_the_library_carries_the_order_rules():
    # a behaviour change without a new symbol: the minor version, and the header says what changed
    src = open(os.path.join(ROOT, "include", "fvhd.h")).read()
    assert int(re.search(r"#define\s+FVHD_VERSION\s+(\d+)", src).group(1)) == 510 == _lib.load().fvhd_version()
    assert "510 changes behaviour without a new" in src


def test_step_without_ids_and_verify_are_refused_behind_a_rewind_or_gather():
    gen = _bare_generator()
    with pytest.raises(ValueError, match=STALE) as err:
        gen.step()
    assert "extend()" in str(err.value) and "explicit ids" in str(err.value)      # the two ways on
    with pytest.raises(ValueError, match=STALE):
        gen.step(None, logits=False)
    with pytest.raises(ValueError, match=STALE):
        gen.verify(torch.zeros(4, dtype=torch.long))
    # the other refusals of verify come first, as before: a started batch above 1, the row count
    with pytest.raises(ValueError, match="ONE sequence"):
        _bare_generator(run_batch=2).verify(torch.zeros(4, dtype=torch.long))
    with pytest.raises(ValueError, match="2 .. 16 rows"):
        gen.verify(torch.zeros(16, dtype=torch.long))
    with pytest.raises(RuntimeError, match="call start"):
        _bare_generator(run_batch=0).step()


def test_explicit_ids_pass_the_rule():
    """step(ids) is not refused by the order rule: on the bare generator it gets as far as the argument check of the ids themselves"""
    gen = _bare_generator()
    with pytest.raises(ValueError, match="contiguous int64 tensor"):
        gen.step(torch.zeros(3, dtype=torch.long))               # (the wrong shape: [1] is expected)
    assert gen._ids_stale                                        # a refused call clears nothing


def test_with_processors_set_the_generator_refuses_every_call_that_moves_the_cache():
    """rewind, extend, verify and - the history is not reordered either - cache_gather, each before any device is looked at"""
    gen = _bare_generator(stale=False)
    gen._processors = dict(repetition_penalty=1.3)
    with pytest.raises(ValueError, match="their token history is not reordered"):
        gen.cache_gather(torch.zeros(3, dtype=torch.long), 1)
    with pytest.raises(ValueError, match="their token history is not rewound"):
        gen.rewind([5])
    with pytest.raises(ValueError, match="their token history has no ids for an embedded chunk"):
        gen.extend(torch.zeros(1, 2, 8))
    with pytest.raises(ValueError, match="does not maintain their token history"):
        gen.verify(torch.zeros(4, dtype=torch.long))
    assert gen._run_batch == 1 and not gen._ids_stale            # a refused call changes nothing


def test_a_generator_without_the_flag_is_not_stale():
    gen = _bare_generator(stale=False)
    del gen._ids_stale                                           # an object made before the flag existed
    gen._stale_ids_refusal("step")
