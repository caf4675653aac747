"""tests/prefill_reference.py pinned on the CPU: its fp64 restatements against oracle/qwen2_oracle.py in fp32 (itself pinned to the
installed `transformers` by tests/test_qwen2_prefill.py), and the HEADROOM of every input family of tests/test_gpu_prefill_ops.py under
that file's bound: a CPU model of the attention kernel's arithmetic (64-key tiles, P and the denominator in bf16-rounded P, one output
rounding) must stay within HALF of  2e-2 |want| + 2e-2 rms(row)  per (b, t, head) row, the census case within 2^-7 |want|.  These are
conditions on the INPUTS (a family that needed the whole budget for the arithmetic the kernel is allowed would test nothing), not
tolerances of the kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_reference as R  # noqa: E402
from oracle import qwen2_oracle as QO  # noqa: E402


def test_rmsnorm_ref_equals_the_oracle():
    g = torch.Generator().manual_seed(0)
    for M, H in ((5, 136), (3, 896)):
        x = (torch.randn(M, H, generator=g) * torch.logspace(-3, 1.3, M)[:, None]).to(torch.bfloat16)
        w = 1 + 0.3 * torch.randn(H, generator=g)
        want = QO.rmsnorm(x.float(), w, 1e-6)
        got = R.rmsnorm_ref(x, w, 1e-6)
        assert got.dtype == torch.float64
        assert torch.allclose(got, want.double(), rtol=1e-5, atol=1e-30)


@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 3, 1)])
def test_rope_ref_equals_the_oracle(hd, nh, nkv):
    g = torch.Generator().manual_seed(hd)
    B, T = 2, 19
    qkv = torch.randn(B * T, (nh + 2 * nkv) * hd, generator=g).to(torch.bfloat16)
    pos = torch.stack([torch.randperm(300, generator=g)[:T] for _ in range(B)])
    q, k, v = R.split_heads(qkv.float(), B, T, nh, nkv, hd)
    cos, sin = QO.rope_cos_sin(pos, hd, 1e6)
    qr, kr = QO.apply_rope(q, k, cos, sin)
    got = R.rope_ref(qkv, pos.reshape(-1), nh, nkv, hd, 1e6)
    assert got.dtype == torch.float64
    gq, gk, gv = R.split_heads(got.reshape(B * T, -1), B, T, nh, nkv, hd)
    assert torch.allclose(gq, qr.double(), rtol=1e-5, atol=1e-5) and torch.allclose(gk, kr.double(), rtol=1e-5, atol=1e-5)
    assert torch.equal(gv, v.double())


@pytest.mark.parametrize("name", ["plain", "qscale", "left", "holes"])
def test_attention_ref_equals_the_oracle_on_unmasked_rows(name):
    B, T, nh, nkv, hd = 4, 150, 4, 2, 64
    qkv, kvalid = R.family(name, B, T, nh, nkv, hd, seed=3)
    q, k, v = R.split_heads(qkv, B, T, nh, nkv, hd)
    got, empty = R.attention_ref(q, k, v, kvalid)
    want = QO.attention(q.float(), k.float(), v.float(), kvalid).view(B, T, nh, hd)
    assert got.dtype == torch.float64
    rows = ~empty
    if name == "left":
        assert bool(empty.any()) and bool((got[empty] == 0).all())           # the contract of rows with no visible key
        assert torch.equal(empty, torch.cumsum(kvalid != 0, 1) == 0)
    else:
        assert name == "holes" or not bool(empty.any())
    scale = want[rows].abs().max()
    assert float((got[rows] - want[rows].double()).abs().max()) <= 1e-5 * float(scale)


def test_flash_model_is_exact_on_a_single_key_and_zero_without_one():
    B, T, nh, nkv, hd = 1, 130, 2, 1, 64
    qkv, _ = R.family("qscale", B, T, nh, nkv, hd, seed=1)
    kvalid = torch.zeros(B, T, dtype=torch.uint8)
    kvalid[0, 70] = 1
    q, k, v = R.split_heads(qkv, B, T, nh, nkv, hd)
    out = R.flash_model(q, k, v, kvalid)
    assert bool((out[0, :70] == 0).all())
    assert torch.equal(out[0, 70:], v[0, 0, 70].expand(T - 70, nh, hd))


# (family, B, padding counts).  The model's error on the flat rows (q scale 0.05: hundreds of keys of equal weight, each P rounded to 8 bits) is
# close to normal with a standard deviation of ~0.08 of the bound, so the LARGEST ratio grows with the number of elements drawn: the
# batches stay at 4 sequences (2 M elements at T = 1025, hd = 128), the seven padding counts in two batches.
HEADROOM = [("plain", 2, None), ("qscale", 2, None), ("ascending", 2, None), ("descending", 2, None), ("planted", 4, None), ("holes", 4, None),
            ("left", 4, 0), ("left", 4, 3), ("right", 4, 0), ("right", 4, 3), ("census", 2, None)]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("T", [257, 1025])
@pytest.mark.parametrize("name,B,first", HEADROOM)
def test_input_families_leave_headroom_under_the_gpu_bound(name, B, first, T, hd):
    nh, nkv = 4, 2
    pad = R.padding_counts(T)[first:first + 4] if first is not None else None
    qkv, kvalid = R.family(name, B, T, nh, nkv, hd, seed=T + hd + (first or 0), pad=pad)
    q, k, v = R.split_heads(qkv, B, T, nh, nkv, hd)
    want, empty = R.attention_ref(q, k, v, kvalid)
    model = R.flash_model(q, k, v, kvalid)
    assert bool((model[empty] == 0).all())
    if name == "census":
        bad, worst = R._violations(model, want, 2.0 ** -7, 0.0, rows=~empty)
        print(f"census T={T} hd={hd}: model err / (2^-7 |want|) {worst:.3f}")
        assert bad == 0 and worst <= 1.0
    else:
        bad, worst = R._violations(model, want, R.ATT_RTOL, R.ATT_RMS, rows=~empty)
        print(f"{name} T={T} hd={hd} pad={pad}: model err / bound {worst:.3f}")
        assert bad == 0 and worst <= 0.5, worst
