"""CPU: pins tests/guidance_reference.py - the fp64 reference of classifier-free guidance against transformers' own
UnbatchedClassifierFreeGuidanceLogitsProcessor, its two special cases, and the shape of the derived bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_reference as GR  # noqa: E402
import logprobs_reference as LR  # noqa: E402


class _Out(dict):
    logits = property(lambda self: self["logits"])


class _Stub:
    """a "model" whose forward returns fixed logits [G, 1, V]: what the processor asks for the unconditional sequence"""

    def __init__(self, logits):
        self.fixed = logits
        self.calls = 0

    def __call__(self, input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        self.calls += 1
        return _Out(logits=self.fixed[:, None, :], past_key_values=None)


def _rows(G, V, seed):
    g = torch.Generator().manual_seed(seed)
    scale = torch.logspace(-1.3, 1.3, 2 * G)[torch.randperm(2 * G, generator=g)]
    return torch.randn(2 * G, V, generator=g) * scale[:, None]


def _hf(x, s):
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    G = x.shape[0] // 2
    stub = _Stub(x[G:])
    ids = torch.zeros((G, 3), dtype=torch.long)
    proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(s, stub, unconditional_ids=ids, unconditional_attention_mask=torch.ones_like(ids))
    return proc(ids, x[:G].clone()), stub


@pytest.mark.parametrize("s", [0.5, 1.5, 3.0, -1.0])
@pytest.mark.parametrize("G,V", [(1, 5), (3, 2049), (2, 4099)])
def test_transformers_processor_in_fp32_lies_within_the_bound_of_the_fp64_reference(G, V, s):
    x = _rows(G, V, seed=G * 1000 + V)
    got, stub = _hf(x, s)
    assert stub.calls == 1 and got.dtype == torch.float32
    worst = GR.check(x, s, got, f"transformers G={G} V={V} s={s}")
    assert 0.0 <= worst <= 1.0


def test_scale_one_is_the_plain_log_softmax():
    x = _rows(2, 1001, seed=1)
    got, stub = _hf(x, 1.0)
    assert stub.calls == 0                                       # transformers: "off" never asks the model
    assert torch.equal(got, torch.nn.functional.log_softmax(x[:2], dim=-1))
    lc = GR.log_softmax64(x[:2])
    assert float((GR.guided_reference(x, 1.0) - lc).abs().max()) <= 1e-12
    # and the reference's log-softmax is the log-probabilities reference's
    ids = torch.tensor([3, 7])
    tok, _, _ = LR.logprobs_reference(x[:2], ids, 0)
    assert torch.equal(tok, lc.gather(1, ids[:, None])[:, 0])


@pytest.mark.parametrize("s", [0.5, 3.0, -1.0])
def test_identical_rows_give_lc_exactly(s):
    x = _rows(2, 2049, seed=2)
    x[2:] = x[:2]
    assert torch.equal(GR.guided_reference(x, s), GR.log_softmax64(x[:2]))


def test_the_bound_follows_its_derivation():
    """positive, never below the log-softmax bound of the unconditional row, growing with |s|, symmetric in the sign of s; the scale is the
    fp32 value; the slice counts are the kernel's"""
    x = _rows(2, 4099, seed=3)
    ref = GR.Reference(x)
    b1, b3, bm3 = ref.bound(1.5), ref.bound(3.0), ref.bound(-3.0)
    assert bool((b1 > 0).all()) and bool((b3 > b1).all()) and bool((b1 >= ref.e_u).all())
    # s and -s differ in |guided| alone: the rounding of the last sum
    last = (1 + 2.0 ** -10) * GR.U * (ref.guided(3.0).abs() - ref.guided(-3.0).abs())
    assert torch.allclose(b3 - bm3, last, rtol=1e-6, atol=1e-18)
    assert GR.fp32_scale(0.1) != 0.1 and GR.fp32_scale(1.5) == 1.5
    assert [GR.slices(v) for v in (1, 2048, 2049, 129024, 129025, 152064)] == [1, 1, 2, 63, 64, 64]
    assert [GR.apply_slices(v) for v in (1, 2048, 2049, 152064)] == [1, 1, 2, 75]
    # a wrong element is caught
    got = ref.guided(1.5).clone()
    got[1, 17] += 4 * float(b1[1, 17])
    with pytest.raises(AssertionError, match="bound"):
        ref.check(1.5, got)


def test_pair_batch_left_pads_both_halves_to_the_longer_length():
    e, m = torch.ones(2, 5, 4), torch.ones(2, 5, dtype=torch.long)
    m[1, :2] = 0
    ne, nm = 2 * torch.ones(2, 3, 4), torch.ones(2, 3, dtype=torch.long)
    x2, m2 = GR.pair_batch(e, m, ne, nm)
    assert x2.shape == (4, 5, 4) and m2.tolist() == [[1, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 1, 1, 1]]
    assert bool((x2[2:, :2] == 0).all()) and bool((x2[2:, 2:] == 2).all()) and bool((x2[:2] == 1).all())
