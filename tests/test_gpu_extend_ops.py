"""The kernels of csrc/llm_extend.hip one at a time (fvhd_op_attention_extend / _cache_append / _extend_positions / _cache_rewind) against
tests/extend_reference.py: fp64 references compared per (b, t, head) row at the project's attention budget (2e-2 |want| + 2e-2 rms of the
row), bit identities where the contract is one, sentinel-filled caches (capacity > P + T, a spare cache row) and guarded outputs.

MEASURED (MI355X, the worst err / bound as the tests print it): attention over 8 (P, T) x 3 head shapes x 5 - 9 families 0.457 (q-row
scales, P = 5, T = 200, hd 128), masks <= 0.416, holes <= 0.369; census 0.438 of 2^-7 |want|; P = 0, single visible key, append, rewind,
positions: identical bits.  The CPU model of the arithmetic (tests/test_extend_reference.py) reaches 0.415 on the same families."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import extend_reference as E  # noqa: E402
import prefill_reference as R  # noqa: E402
from llm_testlib import SENT, check as _check, lib, ptr as _p, stream as _st  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _i32(v):
    return torch.tensor([v], device=DEV, dtype=torch.int32)


def _extend(lib, qkv_full, kvalid_full, B, P, T, nh, nkv, hd, cap=None, spare=1):
    """the op on the chunk rows of a concatenated sequence: caches with slots [0, P + T) filled, everything else the sentinel; the mask
    ones behind P + T -> out [B, T, nh, hd] bf16 (a copy).  Asserts that only the B*T rows were written and that no input changed."""
    N = P + T
    cap = N + 37 if cap is None else cap
    rows = E.chunk_rows(qkv_full, B, P, T)
    kc, vc = E.caches(qkv_full, B, N, nh, nkv, hd, cap, B + spare)
    mask = E.cache_mask(kvalid_full, B, N, cap, B + spare, DEV)
    buf, out = R.guarded(B * T, nh * hd, DEV)
    before = (rows.clone(), kc.clone(), vc.clone(), mask.clone())
    past = _i32(P)
    _check(lib.fvhd_op_attention_extend(_st(), _p(rows), _p(kc), _p(vc), _p(mask), _p(out), B, T, nh, nkv, hd, cap, _p(past)), "attention_extend")
    torch.cuda.synchronize()
    assert R.guard_intact(buf, B * T), "rows behind B*T were written"
    assert R.same_bits(rows, before[0]) and R.same_bits(kc, before[1]) and R.same_bits(vc, before[2]) and torch.equal(mask, before[3])
    return out.clone().view(B, T, nh, hd)


@pytest.mark.parametrize("hd,nh,nkv", E.HEADS)
@pytest.mark.parametrize("P,T", E.PT)
def test_attention_extend_against_the_concatenated_reference(lib, P, T, hd, nh, nkv):
    """every input family at length P + T (extend_reference.op_families): plain, q-row scales, a maximum that moves up / down the keys, a
    planted winner, left padding inside the past / reaching into the chunk (its first chunk queries are all-masked rows: zeros), right
    padding, whole key tiles invalid; B = 1, 3 and 4"""
    report = []
    for i, (name, B, pad) in enumerate(E.op_families(P, T)):
        qkv, kvalid = R.family(name, B, P + T, nh, nkv, hd, seed=500 + 7 * P + T + i, device=DEV, pad=pad)
        got = _extend(lib, qkv, kvalid, B, P, T, nh, nkv, hd)
        want, empty = E.attention_extend_ref(qkv, kvalid, B, P, T, nh, nkv, hd)
        assert bool((got[empty] == 0).all()), f"{name}: a chunk query without a visible key is not zero"
        worst = R._close(got, want, f"{name} P={P} T={T} hd={hd} nh={nh}/{nkv}", R.ATT_RTOL, R.ATT_RMS, rows=~empty)
        report.append(f"{name}{'' if pad is None else pad} {worst:.3f}")
    print(f"attention_extend P={P} T={T} hd={hd} nh={nh}/{nkv}: worst err / bound " + ", ".join(report))


@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 28, 4)])
@pytest.mark.parametrize("T", [1, 64, 129, 257])
def test_with_an_empty_past_the_bits_are_the_prefill_kernels(lib, T, hd, nh, nkv):
    """P = 0: the chunk is the whole sequence and the kernel performs llm_attention_kernel's operations in its order - identical bits,
    without a mask, with left padding and with whole tiles invalid"""
    B = 4
    masks = [None, R.family("left", B, T, nh, nkv, hd, seed=1)[1].to(DEV) if T > 1 else None, R.hole_masks(T, torch.Generator(device=DEV).manual_seed(2), DEV)]
    qkv, _ = R.family("qscale", B, T, nh, nkv, hd, seed=40 + T + hd, device=DEV)
    for kvalid in masks:
        buf, ref = R.guarded(B * T, nh * hd, DEV)
        _check(lib.fvhd_op_attention_causal(_st(), _p(qkv), _p(ref), _p(kvalid), B, T, nh, nkv, hd), "attention_causal")
        got = _extend(lib, qkv, kvalid, B, 0, T, nh, nkv, hd)
        assert R.same_bits(got, ref.view(B, T, nh, hd)), f"T={T} hd={hd} mask={'none' if kvalid is None else 'set'}"


@pytest.mark.parametrize("hd,nh,nkv", [(64, 4, 2), (128, 4, 2)])
def test_a_single_visible_key_is_returned_bit_for_bit(lib, hd, nh, nkv):
    """key_valid one-hot: P = exp2(0) = 1 and l = 1, so a chunk query that sees the key returns v[j] of its kv head bit for bit and one
    that does not returns zeros - a key in the first past tile, in the last past tile, the chunk's first token, a token inside the chunk"""
    P, T = 130, 70
    js = [5, 129, 130, 180]
    B = len(js)
    qkv, _ = R.family("qscale", B, P + T, nh, nkv, hd, seed=90 + hd, device=DEV)
    kvalid = torch.zeros(B, P + T, device=DEV, dtype=torch.uint8)
    for b, j in enumerate(js):
        kvalid[b, j] = 1
    got = _extend(lib, qkv, kvalid, B, P, T, nh, nkv, hd)
    v = R.split_heads(qkv, B, P + T, nh, nkv, hd)[2]
    for b, j in enumerate(js):
        t0 = max(j - P, 0)
        assert bool((got[b, :t0] == 0).all())
        want = v[b, :, j].repeat_interleave(nh // nkv, 0)[None].expand(T - t0, nh, hd)
        assert R.same_bits(got[b, t0:], want.contiguous()), (b, j)


@pytest.mark.parametrize("P,T,hd", [(70, 130, 64), (192, 65, 128)])
def test_census_counts_every_visible_key_once(lib, P, T, hd):
    """q = 0: every visible key has P = 1 exactly; v[j] = e_{j mod hd}; 70 % of the keys valid at random: out[t, d] = the visible keys
    j <= P + t with j mod hd = d over all visible ones - within 2^-7 |want| (one bf16 ulp); a key dropped or counted twice at the past /
    chunk seam, a tile or a workgroup edge changes a count by one"""
    nh, nkv, B, N = 4, 2, 2, P + T
    qkv, kvalid = R.family("census", B, N, nh, nkv, hd, seed=80 + P + hd, device=DEV)
    got = _extend(lib, qkv, kvalid, B, P, T, nh, nkv, hd)
    want, empty = E.attention_extend_ref(qkv, kvalid, B, P, T, nh, nkv, hd)
    onehot = torch.nn.functional.one_hot(torch.arange(N, device=DEV) % hd, hd).double()
    counts = torch.cumsum((kvalid != 0)[:, :, None] * onehot[None], 1)[:, P:]
    frac = counts / counts.sum(-1, keepdim=True).clamp_min(1)
    assert float((want - frac[:, :, None, :]).abs().max()) <= 1e-12
    assert bool((got[empty] == 0).all())
    worst = R._close(got, want, f"census P={P} T={T} hd={hd}", 2.0 ** -7, 0.0, rows=~empty)
    print(f"attention_extend census P={P} T={T} hd={hd}: worst err / (2^-7 |want|) {worst:.3f}")


def test_attention_extend_at_the_capacity_and_past_it(lib):
    """P + T = capacity works; P + T = capacity + 1 writes nothing"""
    hd, nh, nkv, B, P, T = 64, 4, 2, 2, 100, 30
    qkv, _ = R.family("qscale", B, P + T, nh, nkv, hd, seed=7, device=DEV)
    got = _extend(lib, qkv, None, B, P, T, nh, nkv, hd, cap=P + T)
    want, _ = E.attention_extend_ref(qkv, None, B, P, T, nh, nkv, hd)
    R._close(got, want, "P + T = capacity", R.ATT_RTOL, R.ATT_RMS)
    rows = E.chunk_rows(qkv, B, P, T)
    kc, vc = E.caches(qkv, B, P + T, nh, nkv, hd, P + T, B + 1)
    mask = E.cache_mask(None, B, P + T, P + T, B + 1, DEV)
    buf, out = R.guarded(B * T, nh * hd, DEV)
    past = _i32(P + 1)
    _check(lib.fvhd_op_attention_extend(_st(), _p(rows), _p(kc), _p(vc), _p(mask), _p(out), B, T, nh, nkv, hd, P + T, _p(past)), "attention_extend")
    torch.cuda.synchronize()
    assert R.guard_intact(buf, 0), "a launch past the capacity wrote output rows"


# ---- cache append ------------------------------------------------------------------------------------------------------------------------
def _append_case(hd, nh, nkv, B, P, T, cap, layers=2, spare=1, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    width = (nh + 2 * nkv) * hd
    rows = torch.randn(B * T, width, device=DEV, generator=g).to(torch.bfloat16)
    kc = torch.randn(layers, B + spare, nkv, cap, hd, device=DEV, generator=g).to(torch.bfloat16)
    vc = torch.randn(layers, B + spare, nkv, cap, hd, device=DEV, generator=g).to(torch.bfloat16)
    mask = torch.full((B + spare, cap), 7, device=DEV, dtype=torch.uint8)
    chunk = (torch.rand(B, T, device=DEV, generator=g) < 0.6).to(torch.uint8)
    return rows, kc, vc, mask, chunk


@pytest.mark.parametrize("hd,nh,nkv,B,P,T", [(64, 14, 2, 3, 63, 17), (128, 28, 4, 1, 130, 129), (64, 4, 2, 2, 0, 5), (128, 4, 2, 3, 257, 1)])
def test_cache_append_copies_the_rows_and_nothing_else(lib, hd, nh, nkv, B, P, T):
    """the appended slots equal the k / v heads of the rows bit for bit; slots < P, slots >= P + T, the spare row and the other layer keep
    their bits; the mask column is the chunk's mask (ones without one), written only when the mask pointer is given"""
    cap = P + T + 11
    rows, kc, vc, mask, chunk = _append_case(hd, nh, nkv, B, P, T, cap, seed=P + T)
    k0, v0, m0 = kc.clone(), vc.clone(), mask.clone()
    status = _i32(0)
    layer = 1
    past = _i32(P)
    _check(lib.fvhd_op_cache_append(_st(), _p(rows), _p(kc[layer]), _p(vc[layer]), _p(mask), _p(chunk), B, T, nh, nkv, hd, cap, _p(past), _p(status)), "append")
    torch.cuda.synchronize()
    x = rows.view(B, T, nh + 2 * nkv, hd)
    wk, wv, wm = k0.clone(), v0.clone(), m0.clone()
    wk[layer, :B, :, P:P + T] = x[:, :, nh:nh + nkv].transpose(1, 2)
    wv[layer, :B, :, P:P + T] = x[:, :, nh + nkv:].transpose(1, 2)
    wm[:B, P:P + T] = chunk
    assert R.same_bits(kc, wk) and R.same_bits(vc, wv) and torch.equal(mask, wm) and int(status) == 0
    # a later layer's launch: no mask pointer - the mask stays; no chunk mask - ones
    past = _i32(P)
    _check(lib.fvhd_op_cache_append(_st(), _p(rows), _p(kc[0]), _p(vc[0]), None, None, B, T, nh, nkv, hd, cap, _p(past), _p(status)), "append")
    past = _i32(P)
    _check(lib.fvhd_op_cache_append(_st(), _p(rows), _p(kc[0]), _p(vc[0]), _p(mask), None, B, T, nh, nkv, hd, cap, _p(past), _p(status)), "append")
    torch.cuda.synchronize()
    wk[0, :B, :, P:P + T] = wk[layer, :B, :, P:P + T]
    wv[0, :B, :, P:P + T] = wv[layer, :B, :, P:P + T]
    wm[:B, P:P + T] = 1
    assert R.same_bits(kc, wk) and R.same_bits(vc, wv) and torch.equal(mask, wm)


def test_cache_append_at_the_capacity_and_past_it(lib):
    """P + T = capacity works; P + T = capacity + 1 writes nothing anywhere and leaves error word 1, and while the word is set a launch
    that would fit does nothing either"""
    hd, nh, nkv, B, T, cap = 64, 4, 2, 2, 9, 40
    rows, kc, vc, mask, chunk = _append_case(hd, nh, nkv, B, cap - T, T, cap, layers=1, seed=3)
    k0, v0, m0 = kc.clone(), vc.clone(), mask.clone()
    status = _i32(0)
    past = _i32(cap - T)
    _check(lib.fvhd_op_cache_append(_st(), _p(rows), _p(kc), _p(vc), _p(mask), _p(chunk), B, T, nh, nkv, hd, cap, _p(past), _p(status)), "append")
    torch.cuda.synchronize()
    assert int(status) == 0 and R.same_bits(kc[0, :B, :, cap - T:], rows.view(B, T, -1, hd)[:, :, nh:nh + nkv].transpose(1, 2).contiguous())
    kc.copy_(k0), vc.copy_(v0), mask.copy_(m0)
    past = _i32(cap - T + 1)
    _check(lib.fvhd_op_cache_append(_st(), _p(rows), _p(kc), _p(vc), _p(mask), _p(chunk), B, T, nh, nkv, hd, cap, _p(past), _p(status)), "append")
    torch.cuda.synchronize()
    assert int(status) == 1 and R.same_bits(kc, k0) and R.same_bits(vc, v0) and torch.equal(mask, m0)
    past = _i32(0)
    _check(lib.fvhd_op_cache_append(_st(), _p(rows), _p(kc), _p(vc), _p(mask), _p(chunk), B, T, nh, nkv, hd, cap, _p(past), _p(status)), "append")
    torch.cuda.synchronize()
    assert int(status) == 1 and R.same_bits(kc, k0) and R.same_bits(vc, v0) and torch.equal(mask, m0)


# ---- rewind and positions ----------------------------------------------------------------------------------------------------------------
def _rewind(lib, mask, pos, length, keep, status=0):
    m, p = mask.to(DEV).clone(), pos.to(DEV).clone()
    ln, st = _i32(length), _i32(status)
    k = torch.tensor(keep, device=DEV, dtype=torch.int32)
    _check(lib.fvhd_op_cache_rewind(_st(), _p(k), len(keep), _p(m), _p(p), mask.shape[1], _p(ln), _p(st)), "rewind")
    torch.cuda.synchronize()
    return m.cpu(), p.cpu(), int(ln), int(st)


def test_rewind_matches_the_model(lib):
    """rows with left padding and with holes: the positions drop by the VALID slots only; more slots than one pass of the workgroup
    (length 700 > 256 threads); keep = length (nothing dropped) and keep = 0 (everything)"""
    g = torch.Generator().manual_seed(5)
    rows, cap, length = 5, 800, 700
    mask = (torch.rand(rows, cap, generator=g) < 0.7).to(torch.uint8)
    mask[0] = 1
    mask[1, :300] = 0
    mask[:, length:] = 0
    pos = mask[:, :length].long().sum(1)
    for keep in ([700, 650, 1, 0, 333], [10, 10, 10, 10, 10], [700] * 5):
        want = E.rewind_model(mask, pos, length, keep)
        got = _rewind(lib, mask, pos, length, keep)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[2:] == want[2:], keep
        assert got[2] == max(keep) and got[3] == 0


def test_rewind_out_of_range_changes_nothing_and_sets_error_word_4(lib):
    mask = torch.ones(3, 64, dtype=torch.uint8)
    mask[:, 40:] = 0
    pos = torch.tensor([40, 40, 40])
    for keep in ([41, 3, 3], [3, -1, 3]):
        m, p, n, st = _rewind(lib, mask, pos, 40, keep)
        assert st == 4 and n == 40 and torch.equal(m, mask) and torch.equal(p, pos)
    m, p, n, st = _rewind(lib, mask, pos, 40, [3, 3, 3], status=1)      # a pending error word: nothing happens
    assert st == 1 and n == 40 and torch.equal(m, mask) and torch.equal(p, pos)


@pytest.mark.parametrize("B,T", [(1, 1), (3, 17), (64, 130)])
def test_default_positions_match_the_model(lib, B, T):
    g = torch.Generator().manual_seed(B + T)
    nxt = torch.randint(0, 3000, (B,), generator=g)
    chunk = torch.ones(B, T, dtype=torch.uint8)
    for b in range(B):
        chunk[b, :(5 * b) % T] = 0                               # left-padded chunk rows
    nxt_d = nxt.to(DEV)
    for cv in (chunk, None):
        out = torch.full((B * T + 8,), -7, device=DEV, dtype=torch.long)
        cv_d = None if cv is None else cv.to(DEV)                # (named: a temporary would be freed before the launch reads it)
        _check(lib.fvhd_op_extend_positions(_st(), _p(nxt_d), _p(cv_d), _p(out), B, T), "positions")
        torch.cuda.synchronize()
        assert bool((out[B * T:] == -7).all())
        assert torch.equal(out[:B * T].view(B, T).cpu(), E.extend_positions_model(nxt, cv, T))
