"""The prefill's kernels (csrc/llm.hip, and w8_unpack_kernel of csrc/llm_w8.hip as the prefill uses it) element by element against
tests/prefill_reference.py (plain torch fp64 on the bf16-rounded operands, pinned to oracle/qwen2_oracle.py on the CPU by
tests/test_prefill_reference.py, which also shows that every input family used here leaves the kernel's allowed arithmetic half the bound).

Bounds, all PER ROW (one (b, t, head) vector of hd values; one row of rmsnorm / rope) - the rows are given scales that differ by orders of
magnitude, a pooled rms would hide the small ones:
  attention   |err| <= 2e-2 |want| + 2e-2 rms(want row)    the project's attention budget (P is rounded to bf16 for the PV MFMA)
  rmsnorm     |err| <= 2^-7 |want|                         one rounding to bf16 (half an ulp <= 2^-8), fp32 statistics
  rope        |err| <= 2^-7 (|a| + |b|) per rotated pair   one rounding to bf16
  exact cases (single visible key, NULL against all-ones mask, in place against out of place, one launch against another, bf16 against
  fp32 / fp16 embeddings, e4m3 against bf16 weights holding the same values) bit for bit; the census case to 2^-7 |want|.
Every output is allocated with a sentinel-filled guard behind its rows; inputs are compared with their bits before the launch.

MEASURED (MI355X, the worst err / bound per family as the tests print it; profiles/r11_prefill_tests_pytest.log):
  attention, lengths at the edges (q-row scales)   0.470 (T = 193, hd 128); long sequences 0.364 / 0.340 (T = 1025), 0.371 / 0.450 (T = 2304)
  attention, masks                                 left padding 0.356, right padding 0.368, holes 0.335
  attention, moving maximum                        ascending 0.360, descending 0.404, planted winner 0.365
  attention, census                                0.496 of 2^-7 |want|, i.e. 2^-8: the rounding of the output alone
  attention, single visible key / NULL mask / relaunch / one sequence alone: identical bits
  rmsnorm                                          0.498 of 2^-7 |want| (half a bf16 ulp); in place = out of place bit for bit
  rope                                             0.480 of 2^-7 (|a| + |b|)
  last-row logits                                  6.3e-5 of the 2e-3 bound
  embed dtypes, workspace history, e4m3 against bf16 on dequantised weights: identical bits
The CPU model of the kernel's arithmetic (tests/test_prefill_reference.py) reaches 0.41 on the same families: the largest ratios come from the
flat rows (q scale 0.05, hundreds of keys of equal weight, every P rounded to 8 bits), where the error is close to normal with a standard
deviation of ~0.08 of the bound and the maximum grows with the number of elements compared.  No measured attention ratio exceeds 0.5; one
that did would be worth a look before anything else.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_reference as R  # noqa: E402
from llm_testlib import (CONFIGS, lib,  # noqa: E402,F401
                         check as _check, compare_prefill, ptr as _p, qwen2_cfg, qwen2_model, stream as _st)

pytestmark = pytest.mark.gpu

DEV = "cuda"
THETA = 1e6



# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def _attn(lib, qkv, kvalid, B, T, nh, nkv, hd):
    """one fvhd_op_attention_causal launch into a guarded buffer -> out [B, T, nh, hd] bf16 (a copy).  Asserts that the B*T rows are all
    that was written and that qkv / key_valid keep their bits."""
    rows = B * T
    assert qkv.shape == (rows, (nh + 2 * nkv) * hd) and qkv.dtype == torch.bfloat16 and qkv.is_contiguous()
    assert kvalid is None or (kvalid.shape == (B, T) and kvalid.dtype == torch.uint8 and kvalid.is_contiguous())
    buf, out = R.guarded(rows, nh * hd, DEV)
    before = qkv.clone()
    mask_before = None if kvalid is None else kvalid.clone()
    _check(lib.fvhd_op_attention_causal(_st(), _p(qkv), _p(out), _p(kvalid), B, T, nh, nkv, hd), "attention")
    torch.cuda.synchronize()
    assert R.guard_intact(buf, rows), "rows behind B*T were written"
    assert R.same_bits(qkv, before), "the kernel wrote into its input"
    assert kvalid is None or torch.equal(kvalid, mask_before)
    return out.clone().view(B, T, nh, hd)


def _attn_check(lib, qkv, kvalid, B, T, nh, nkv, hd, what):
    """launch, compare the rows with a visible key against attention_ref at the attention bound, the others against zero -> (out, worst)"""
    got = _attn(lib, qkv, kvalid, B, T, nh, nkv, hd)
    q, k, v = R.split_heads(qkv, B, T, nh, nkv, hd)
    want, empty = R.attention_ref(q, k, v, kvalid)
    assert bool(torch.isfinite(got.float()).all()), f"{what}: non-finite output"
    assert bool((got[empty] == 0).all()), f"{what}: a row without a visible key is not zero"
    worst = R._close(got, want, what, R.ATT_RTOL, R.ATT_RMS, rows=~empty)
    return got, worst


EDGE_T = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]
EDGE_CASES = [(T, hd, nh, nkv, 3) for T in EDGE_T for hd, nh, nkv in ((64, 14, 2), (128, 12, 2))] + \
             [(T, hd, nh, nkv, 1) for T in (1025, 2304) for hd, nh, nkv in ((64, 4, 2), (128, 4, 4))] + [(129, 128, 28, 4, 3)]


@pytest.mark.parametrize("T,hd,nh,nkv,B", EDGE_CASES)
def test_attention_lengths_at_the_tile_and_workgroup_edges(lib, T, hd, nh, nkv, B):
    """sequence lengths on either side of the 64-key tile and of the 128-query workgroup, and long ones; q rows of distinct scale 0.05 .. 8,
    v of distinct scale per kv head and per key.  Two launches give the same bits; one sequence alone (another grid, another block remap)
    gives the bits it has inside the batch."""
    qkv, _ = R.family("qscale", B, T, nh, nkv, hd, seed=1000 + T + hd + nh, device=DEV)
    got, worst = _attn_check(lib, qkv, None, B, T, nh, nkv, hd, f"T={T} hd={hd} nh={nh}/{nkv}")
    print(f"attention edges T={T} hd={hd} nh={nh}/{nkv} B={B}: worst err / bound {worst:.3f}")
    again = _attn(lib, qkv, None, B, T, nh, nkv, hd)
    assert R.same_bits(got, again), "two launches differ"
    if B > 1:
        b = 1
        alone = _attn(lib, qkv[b * T:(b + 1) * T].contiguous(), None, 1, T, nh, nkv, hd)
        assert R.same_bits(alone[0], got[b]), "a sequence launched alone differs from the same sequence inside the batch"


MASK_SHAPES = [(64, 4, 2), (128, 4, 2)]


@pytest.mark.parametrize("hd,nh,nkv", MASK_SHAPES)
def test_attention_null_mask_equals_all_ones(lib, hd, nh, nkv):
    B, T = 4, 257
    qkv, _ = R.family("qscale", B, T, nh, nkv, hd, seed=7 + hd, device=DEV)
    a = _attn(lib, qkv, None, B, T, nh, nkv, hd)
    b = _attn(lib, qkv, torch.ones(B, T, device=DEV, dtype=torch.uint8), B, T, nh, nkv, hd)
    c = _attn(lib, qkv, torch.full((B, T), 255, device=DEV, dtype=torch.uint8), B, T, nh, nkv, hd)      # any non-zero byte is "valid"
    assert R.same_bits(a, b) and R.same_bits(a, c)


@pytest.mark.parametrize("hd,nh,nkv", MASK_SHAPES)
@pytest.mark.parametrize("kind", ["left", "right", "holes"])
def test_attention_masks(lib, kind, hd, nh, nkv):
    """T = 257, B = 4 with another mask per sequence: left / right padding of 1, 63, 64, 65, 128, 129 and T - 1 keys (in two batches), the
    whole key tile 64..127 invalid, half of all keys invalid at random.  Rows with a visible key against attention_ref, rows without one
    exactly zero, everything finite, the guard intact."""
    B, T = 4, 257
    counts = R.padding_counts(T)
    assert counts == [1, 63, 64, 65, 128, 129, 256]
    batches = [None] if kind == "holes" else [counts[:4], counts[3:]]
    worst = 0.0
    for i, pad in enumerate(batches):
        qkv, kvalid = R.family(kind, B, T, nh, nkv, hd, seed=40 + hd + i, device=DEV, pad=pad)
        got, w = _attn_check(lib, qkv, kvalid, B, T, nh, nkv, hd, f"{kind} {pad} hd={hd}")
        worst = max(worst, w)
        empty = (torch.cumsum(kvalid != 0, 1) == 0)
        if kind == "left":
            assert [int(e.sum()) for e in empty] == pad           # the zero rows are there, and they are these
        if kind == "right":
            assert not bool(empty.any())
    print(f"attention masks {kind} hd={hd}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("T", [257, 1025])
@pytest.mark.parametrize("kind", ["ascending", "descending", "planted"])
def test_attention_moving_maximum(lib, kind, T, hd):
    """ascending: a ramp of 40 logits along the keys - every later tile raises every row's running maximum (the alpha rescale, ~10 logits
    per tile at T = 257); descending: the maximum sits in tile 0, alpha == 1 from the second tile on (the skip path); planted: one key 60
    logits above the rest in the first tile, a middle tile, the last queries' diagonal tile and at the last query's own position"""
    nh, nkv = 4, 2
    B = 4 if kind == "planted" else 2
    qkv, _ = R.family(kind, B, T, nh, nkv, hd, seed=60 + T + hd, device=DEV)
    got, worst = _attn_check(lib, qkv, None, B, T, nh, nkv, hd, f"{kind} T={T} hd={hd}")
    print(f"attention {kind} T={T} hd={hd}: worst err / bound {worst:.3f}")
    if kind == "planted":                                         # the inputs do what they claim: the planted key takes (nearly) all the weight
        q, k, v = R.split_heads(qkv, B, T, nh, nkv, hd)
        for b, j in enumerate(R.planted_keys(T)):
            s = (q[b].double() @ k[b].double().repeat_interleave(nh // nkv, 0).transpose(-1, -2)) * hd ** -0.5      # [nh, T, T]
            others = s[:, j:, :].clone()
            others[:, :, j] = -math.inf
            others = others.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool, device=DEV))[j:], -math.inf)
            assert float((s[:, j:, j] - others.amax(-1)).min()) > 15.0          # e^-15 x 1024 keys: < 1e-3 of the weight


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("T", [129, 257, 1025])
def test_attention_census_counts_every_visible_key_once(lib, T, hd):
    """q = 0: every visible key has P = 1 exactly; v[j] = e_{j mod hd}; 70 % of the keys valid at random.  out[t, d] = the number of visible
    keys j <= t with j mod hd = d over the number of visible keys: counts (exact in fp32), ONE division (1 / l, then the product: two fp32
    roundings) and the rounding to bf16 - within 2^-7 |want| (one bf16 ulp).  A key dropped or counted twice at a tile or workgroup edge
    changes a count by one: with at most T / hd <= 17 keys per count that is >= 6 % of the value."""
    nh, nkv, B = 4, 2, 2
    qkv, kvalid = R.family("census", B, T, nh, nkv, hd, seed=80 + T + hd, device=DEV)
    got = _attn(lib, qkv, kvalid, B, T, nh, nkv, hd)
    q, k, v = R.split_heads(qkv, B, T, nh, nkv, hd)
    want, empty = R.attention_ref(q, k, v, kvalid)
    # the reference against the counts themselves
    valid = (kvalid != 0)
    onehot = torch.nn.functional.one_hot(torch.arange(T, device=DEV) % hd, hd).double()
    counts = torch.cumsum(valid[:, :, None] * onehot[None], 1)                                           # [B, T, hd]
    frac = counts / counts.sum(-1, keepdim=True).clamp_min(1)
    assert float((want - frac[:, :, None, :]).abs().max()) <= 1e-12
    assert bool((got[empty] == 0).all())
    worst = R._close(got, want, f"census T={T} hd={hd}", 2.0 ** -7, 0.0, rows=~empty)
    print(f"attention census T={T} hd={hd}: worst err / (2^-7 |want|) {worst:.3f}")


@pytest.mark.parametrize("hd,nh,nkv", MASK_SHAPES)
def test_attention_single_visible_key_is_returned_bit_for_bit(lib, hd, nh, nkv):
    """key_valid one-hot at j (first, a middle, the last tile): P = exp2(0) = 1, l = 1, so every query t >= j returns v[j] of its kv head
    bit for bit, every t < j zero"""
    T = 257
    js = [5, 130, 256]
    B = len(js)
    qkv, _ = R.family("qscale", B, T, nh, nkv, hd, seed=90 + hd, device=DEV)
    kvalid = torch.zeros(B, T, device=DEV, dtype=torch.uint8)
    for b, j in enumerate(js):
        kvalid[b, j] = 1
    got = _attn(lib, qkv, kvalid, B, T, nh, nkv, hd)
    _, _, v = R.split_heads(qkv, B, T, nh, nkv, hd)
    for b, j in enumerate(js):
        assert bool((got[b, :j] == 0).all()), (b, j)
        want = v[b, :, j].repeat_interleave(nh // nkv, 0)[None].expand(T - j, nh, hd)
        assert R.same_bits(got[b, j:], want.contiguous()), (b, j, int((got[b, j:] != want).sum()))


def test_attention_argument_checks(lib):
    """nh % nkv != 0, head_dim 96, B = 0, T = 0: an error code, and nothing launched (the output keeps the sentinel)"""
    B, T, nh, nkv, hd = 2, 20, 4, 2, 64
    qkv = torch.randn(B * T, (nh + 2 * nkv) * 128, device=DEV).to(torch.bfloat16)
    buf, out = R.guarded(B * T, nh * 128, DEV)
    for args in ((B, T, 3, 2, hd), (B, T, nh, nkv, 96), (0, T, nh, nkv, hd), (B, 0, nh, nkv, hd), (B, T, nh, 0, hd)):
        assert lib.fvhd_op_attention_causal(_st(), _p(qkv), _p(out), _p(None), *args) != 0, args
        assert lib.fvhd_last_error()
    torch.cuda.synchronize()
    assert R.guard_intact(buf, 0)
    _check(lib.fvhd_op_attention_causal(_st(), _p(qkv), _p(out), _p(None), B, T, nh, nkv, 128), "attention")      # the context is still usable
    torch.cuda.synchronize()
    assert R.guard_intact(buf, B * T) and bool(torch.isfinite(out.float()).all())


# ---- rmsnorm -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("H", [8, 64, 136, 512, 520, 896, 1536, 3584])
def test_rmsnorm_elementwise_in_place_and_guard(lib, H, M):
    """widths that leave lanes idle (8: one lane; 136: 17 lanes; 520: one lane in the second pass), row counts around the 4 rows of a
    workgroup; rows of distinct scale 1e-3 .. 20 (at 1e-3 eps is half the variance) and one all-zero row"""
    g = torch.Generator(device=DEV).manual_seed(H * 7 + M)
    scales = torch.logspace(-3, math.log10(20.0), M, device=DEV)[torch.randperm(M, device=DEV, generator=g)] if M > 1 else torch.tensor([20.0], device=DEV)
    x = (torch.randn(M, H, device=DEV, generator=g) * scales[:, None]).to(torch.bfloat16)
    zero_row = 1 if M > 1 else None
    if zero_row is not None:
        x[zero_row] = 0
    w = (1 + 0.3 * torch.randn(H, device=DEV, generator=g)).float()
    want = R.rmsnorm_ref(x, w, 1e-6)
    xbuf, xin = R.guarded(M, H, DEV)
    xin.copy_(x)
    ybuf, y = R.guarded(M, H, DEV)
    _check(lib.fvhd_op_rmsnorm(_st(), _p(xin), _p(y), _p(w), M, H, 1e-6), "rmsnorm")
    torch.cuda.synchronize()
    assert R.guard_intact(ybuf, M) and R.guard_intact(xbuf, M) and R.same_bits(xin, x)
    worst = R._close(y, want, f"rmsnorm {M}x{H}", 2.0 ** -7, 0.0)
    if zero_row is not None:
        assert bool((y[zero_row] == 0).all())
    _check(lib.fvhd_op_rmsnorm(_st(), _p(xin), _p(xin), _p(w), M, H, 1e-6), "rmsnorm in place")
    torch.cuda.synchronize()
    assert R.same_bits(xin, y), "in place differs from out of place"
    assert R.guard_intact(xbuf, M)
    print(f"rmsnorm M={M} H={H}: worst err / (2^-7 |want|) {worst:.3f}")


# ---- rope --------------------------------------------------------------------------------------------------------------------------------
def _rope_pair_check(got, want, src, nh, nkv, hd, what):
    """got bf16 / want fp64 / src bf16 [M, heads, hd]: |err| <= 2^-7 (|a| + |b|) per rotated pair (a, b) = (x[i], x[i + hd / 2]) -> worst ratio"""
    n = nh + nkv
    a, b = src[:, :n, :hd // 2].double().abs(), src[:, :n, hd // 2:].double().abs()
    bound = (2.0 ** -7 * (a + b)).repeat(1, 1, 2)
    err = (got[:, :n].double() - want[:, :n]).abs()
    assert bool(torch.isfinite(got.float()).all())
    bad = int((err > bound).sum())
    worst = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
    assert bad == 0, f"{what}: {bad} elements out of tolerance, worst err / bound {worst:.3g}"
    return worst


@pytest.mark.parametrize("cache", [True, False])
@pytest.mark.parametrize("B,T", [(1, 1), (3, 37), (2, 130)])
@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 28, 4), (128, 12, 2)])
def test_rope_elementwise_cache_layout_and_untouched_rows(lib, hd, nh, nkv, B, T, cache):
    """positions inside the table, drawn at random per row.  M = B*T - 5 rows are rotated (B*T when that is 1): the rows behind M, the v
    heads, the cache rows of the positions behind M and the guards keep their bits; the caches [B, nkv, T, hd] hold the rotated k rows and
    the v rows element for element"""
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    g = torch.Generator(device=DEV).manual_seed(hd + nh + B * T)
    rows, heads = B * T, nh + 2 * nkv
    M = rows - 5 if rows > 5 else rows
    P = T + 64
    width = heads * hd
    src = (torch.randn(rows, width, device=DEV, generator=g) * torch.logspace(-2, 1, rows, device=DEV)[torch.randperm(rows, device=DEV, generator=g)][:, None]).to(torch.bfloat16)
    pos = torch.randint(0, P, (rows,), device=DEV, generator=g)
    table = rope_table(P, hd, THETA, DEV)
    qbuf, qkv = R.guarded(rows, width, DEV)
    qkv.copy_(src)
    kbuf = vbuf = kc = vc = None
    if cache:
        kbuf, kc = R.guarded(B * nkv * T, hd, DEV)
        vbuf, vc = R.guarded(B * nkv * T, hd, DEV)
    _check(lib.fvhd_op_rope(_st(), _p(qkv), _p(pos), _p(table), _p(kc), _p(vc), M, T, nh, nkv, hd, P, THETA), "rope")
    torch.cuda.synchronize()
    want = R.rope_ref(src[:M], pos[:M], nh, nkv, hd, THETA)
    got = qkv.view(rows, heads, hd)
    worst = _rope_pair_check(got[:M], want, src[:M].view(M, heads, hd), nh, nkv, hd, f"rope hd={hd} {B}x{T}")
    assert R.same_bits(got[:M, nh + nkv:], src.view(rows, heads, hd)[:M, nh + nkv:]), "v heads were touched"
    assert R.same_bits(qkv[M:], src[M:]) and R.guard_intact(qbuf, rows), "rows behind M were touched"
    if cache:
        assert R.guard_intact(kbuf, B * nkv * T) and R.guard_intact(vbuf, B * nkv * T)
        kc4, vc4 = kc.view(B, nkv, T, hd), vc.view(B, nkv, T, hd)
        written = (torch.arange(rows, device=DEV) < M).view(B, 1, T).expand(B, nkv, T)
        rot = got.view(B, T, heads, hd)
        assert R.same_bits(kc4[written], rot[:, :, nh:nh + nkv].transpose(1, 2)[written]), "k cache != the rotated k rows"
        assert R.same_bits(vc4[written], rot[:, :, nh + nkv:].transpose(1, 2)[written]), "v cache != the v rows"
        assert bool((kc4.view(torch.int16)[~written] == R.SENT).all()) and bool((vc4.view(torch.int16)[~written] == R.SENT).all()), \
            "cache rows of positions behind M were written"
    print(f"rope hd={hd} nh={nh}/{nkv} {B}x{T} cache={cache}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("splits", [1, 2, 4])
def test_qkv_splitk_rope_equals_reduce_then_rope(lib, splits):
    """fvhd_op_qkv_splitk_rope at head_dim 128 with caches: bit-identical to its own partial sums added in slice order + bias, one rounding,
    then fvhd_op_rope - and that against rope_ref element-wise"""
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    hd, nh, nkv, K, B, T = 128, 4, 2, 256, 3, 37
    M, Mp, heads = B * T, 128, nh + 2 * nkv
    width, P = heads * hd, T + 64
    g = torch.Generator(device=DEV).manual_seed(splits)
    A = torch.randn(Mp, K, device=DEV, generator=g).to(torch.bfloat16)
    W = (torch.randn(width, K, device=DEV, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(width, device=DEV, generator=g)
    pos = torch.randint(0, P, (M,), device=DEV, generator=g)
    table = rope_table(P, hd, THETA, DEV)
    part = torch.zeros(splits, Mp, width, device=DEV, dtype=torch.float32)
    qbuf, qkv = R.guarded(M, width, DEV)
    kbuf, kc = R.guarded(B * nkv * T, hd, DEV)
    vbuf, vc = R.guarded(B * nkv * T, hd, DEV)
    _check(lib.fvhd_op_qkv_splitk_rope(_st(), _p(A), _p(W), _p(bias), _p(part), _p(qkv), _p(pos), _p(table), _p(kc), _p(vc), M, Mp, K, T, nh, nkv, hd,
                                       P, THETA, splits), "split qkv + rope")
    torch.cuda.synchronize()
    assert R.guard_intact(qbuf, M) and R.guard_intact(kbuf, B * nkv * T) and R.guard_intact(vbuf, B * nkv * T)
    acc = part[0].clone()
    for s in range(1, splits):
        acc += part[s]
    proj = (acc[:M] + bias).to(torch.bfloat16).contiguous()
    ref = proj.clone()
    kc2, vc2 = torch.zeros_like(kc), torch.zeros_like(vc)
    _check(lib.fvhd_op_rope(_st(), _p(ref), _p(pos), _p(table), _p(kc2), _p(vc2), M, T, nh, nkv, hd, P, THETA), "rope")
    torch.cuda.synchronize()
    assert R.same_bits(qkv, ref), "fused reduce + rope differs from reduce -> rope"
    assert R.same_bits(kc, kc2) and R.same_bits(vc, vc2), "KV cache"
    want = R.rope_ref(proj, pos, nh, nkv, hd, THETA)
    _rope_pair_check(qkv.view(M, heads, hd), want, proj.view(M, heads, hd), nh, nkv, hd, f"split-K rope splits={splits}")
    R._close(proj, A[:M].double() @ W.double().t() + bias.double(), "split q|k|v projection", 1e-2, 1e-2)     # the single-op budget, per row


# ---- the whole prefill -------------------------------------------------------------------------------------------------------------------
def _tiny():
    cfg = qwen2_cfg(hidden=128, layers=2, heads=2, kv=1, inter=256, vocab=512)
    m = qwen2_model(cfg, seed=4)
    m.load_state_dict({k: (v.to(torch.bfloat16).float() if v.dim() == 2 else v) for k, v in m.state_dict().items()})
    return cfg, m.to(DEV)


def _run(pre, x, mask=None, pos=None):
    """-> (logits, hidden states [B*T, H], k cache, v cache), all copies"""
    B, T = x.shape[:2]
    logits, kc, vc = pre(x, mask, pos, return_kv=True)
    hs = pre.hidden_states(B * T)
    torch.cuda.synchronize()
    return logits.clone(), hs, kc, vc


def _same_run(a, b):
    return torch.equal(a[0], b[0]) and all(R.same_bits(x, y) for x, y in zip(a[1:], b[1:]))


def _embeds(B, T, H, seed):
    """bf16 values that fp16 holds exactly as well (2^-10 <= |x| < 2^15)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B, T, H, device=DEV, generator=g)
    x = torch.where(x.abs() < 2.0 ** -10, torch.full_like(x, 2.0 ** -10), x).to(torch.bfloat16)
    assert torch.equal(x.to(torch.float16).to(torch.bfloat16), x)
    return x


def test_prefill_embed_dtypes_give_the_bits_of_bf16():
    """cast_rows_kernel: fp32 and fp16 inputs_embeds holding bf16 values give the bits of the bf16 call; unrounded fp32 gives the bits of
    x.to(bfloat16) (round to nearest even)"""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    cfg, m = _tiny()
    pre = Qwen2Prefill.from_hf(m)
    B, T = 3, 41
    x = _embeds(B, T, cfg.hidden_size, 11)
    mask = torch.ones(B, T, device=DEV, dtype=torch.long)
    mask[1, :7] = 0
    base = _run(pre, x, mask)
    assert bool(torch.isfinite(base[0]).all())
    assert _same_run(_run(pre, x.float(), mask), base), "fp32 embeddings"
    assert _same_run(_run(pre, x.to(torch.float16), mask), base), "fp16 embeddings"
    raw = torch.randn(B, T, cfg.hidden_size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(12))
    raw[0, 0, :4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20], device=DEV)    # ties to even, and just above one
    assert not torch.equal(raw.to(torch.bfloat16).float(), raw)
    assert _same_run(_run(pre, raw, mask), _run(pre, raw.to(torch.bfloat16), mask)), "unrounded fp32 embeddings"
    assert not torch.equal(_run(pre, raw, mask)[0], base[0])


def test_prefill_logits_are_those_of_the_last_row():
    """gather_rows_kernel: the logits equal lm_head(norm(hidden_states[b*T + T - 1])) recomputed in fp64 (the normed operand rounded to
    bf16 once, as the library holds it) at the fp32-logit bound of tests/test_qwen2_prefill.py, 2e-3 - and no other row's"""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    from oracle import qwen2_oracle as QO
    cfg, m = _tiny()
    pre = Qwen2Prefill.from_hf(m)
    B, T = 3, 40
    x = _embeds(B, T, cfg.hidden_size, 21) * torch.tensor([0.3, 1.0, 3.0], device=DEV, dtype=torch.bfloat16).view(B, 1, 1)
    logits, hs, _, _ = _run(pre, x)
    sd = m.state_dict()
    normed = QO.rmsnorm(hs.float(), sd["model.norm.weight"].float(), cfg.rms_norm_eps).to(torch.bfloat16).double()
    all_logits = (normed @ sd["lm_head.weight"].double().t()).view(B, T, -1)
    worst = R._close(logits, all_logits[:, T - 1], "logits of the last row", 2e-3, 2e-3)
    print(f"prefill last-row logits: worst err / bound {worst:.2e}")
    for t in (0, T - 2):                                          # the test can tell the rows apart
        assert R._violations(logits, all_logits[:, t], 2e-3, 2e-3)[0] > 0


def test_prefill_workspace_history_does_not_leak():
    """(2, 40), then the larger (3, 130), then (2, 40) again on one context: the bits of the first call.  The padding rows up to the
    256-row multiple then hold what the larger call left"""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    cfg, m = _tiny()
    pre = Qwen2Prefill.from_hf(m)
    small = _embeds(2, 40, cfg.hidden_size, 31)
    large = _embeds(3, 130, cfg.hidden_size, 32) * 5
    mask = torch.ones(2, 40, device=DEV, dtype=torch.long)
    mask[1, :9] = 0
    first = _run(pre, small, mask)
    big = _run(pre, large)
    assert bool(torch.isfinite(big[0]).all())
    assert _same_run(_run(pre, small, mask), first)
    fresh = Qwen2Prefill.from_hf(m)                               # and of a context that never saw the larger call
    assert _same_run(_run(fresh, small, mask), first)


@pytest.mark.parametrize("B,T", [(2, 128), (1, 257)])
def test_prefill_row_count_at_the_256_row_padding_edge(B, T):
    """B*T = 256 (no padding row) and 257 (255 of them) against transformers at the budgets of tests/test_qwen2_prefill.py"""
    compare_prefill(qwen2_cfg(hidden=128, layers=2, heads=2, kv=1, inter=256, vocab=512), B, T, "left", seed=6, layers_tol=1.5e-2)


@pytest.mark.parametrize("name", ["0.5B", "7B"])
def test_prefill_e4m3_weights_give_the_bits_of_bf16_on_dequantised_values(name):
    """a model whose matrices hold dequantised e4m3 values (codes * power-of-two row scale: exact in bf16, and they quantise to
    themselves): the "fp8_e4m3" context unpacks exactly the bf16 context's matrices and runs the same GEMMs on them - identical bits for
    logits, hidden states and the KV cache.  The only test that separates w8_unpack_kernel mode 0 from a nearly right one."""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    from ml_fastvlm_amd import quantize_rows_e4m3
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    kw = dict(CONFIGS[name], num_hidden_layers=2)
    cfg = Qwen2Config(vocab_size=4096, max_position_embeddings=4096, rope_theta=1e6, rms_norm_eps=1e-6, **kw)
    torch.manual_seed(5)
    with torch.device(DEV):
        m = Qwen2ForCausalLM(cfg).eval().to(torch.bfloat16)
    emb = m.get_input_embeddings().weight
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
            elif p is not emb or cfg.tie_word_embeddings:
                codes, scale = quantize_rows_e4m3(p)
                p.copy_((codes.float() * scale[:, None]).to(torch.bfloat16))
                assert torch.equal(p.float(), codes.float() * scale[:, None])
    B, T = 2, 24
    x = (0.5 * torch.randn(B, T, cfg.hidden_size, device=DEV)).to(torch.bfloat16)
    mask = torch.ones(B, T, device=DEV, dtype=torch.long)
    mask[1, :3] = 0
    pos = torch.clamp(torch.cumsum(mask, 1) - 1, min=0)
    p8 = Qwen2Prefill.from_hf(m, weights="fp8_e4m3")
    p16 = Qwen2Prefill.from_hf(m)
    assert p8.weight_format == "fp8_e4m3" and p16.weight_format == "bf16"
    a, b = _run(p8, x, mask, pos), _run(p16, x, mask, pos)
    assert bool(torch.isfinite(b[0]).all()) and float(b[0].abs().max()) > 0
    assert torch.equal(a[0], b[0]), f"logits: {int((a[0] != b[0]).sum())} of {a[0].numel()} differ"
    assert R.same_bits(a[1], b[1]), "hidden states"
    assert R.same_bits(a[2], b[2]) and R.same_bits(a[3], b[3]), "KV cache"
