"""The three device operations of beam search with processors, each on its own (include/fvhd.h "LLM beam search with processors",
csrc/llm_beam.hip): the row normalisation element by element against fp64, the reorder of the rows' histories and automaton states under
sentinel guards, and the top-K chains on pre-normalised rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_processors_reference as R  # noqa: E402
from llm_testlib import bits, check, ptr, stream  # noqa: E402

pytestmark = pytest.mark.gpu

SENT_F = 1.23e36
SENT_I = 0x7B3D7B3D
PAD = 64                       # guard elements on either side (256 bytes: the payload keeps the allocation's alignment)


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import _lib
    return _lib.beam_processors_lib()


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * PAD,), fill, device="cuda", dtype=dtype)
    return buf, buf[PAD:PAD + n]


def guards_intact(buf, fill):
    return bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all())


# ---- b1. the normalisation ---------------------------------------------------------------------------------------------------------------
def norm_rows(rows, V, seed, kinds=("plain", "spread", "banned")):
    """rows of logits: kind r % len(kinds) - `spread`: a range of thousands (most of the row underflows), `banned`: a third of it -inf"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = 3.0 * torch.randn(rows, V, device="cuda", generator=g)
    for r in range(rows):
        kind = kinds[r % len(kinds)]
        if kind == "spread":
            x[r] *= 1500.0
        elif kind == "banned":
            x[r, torch.rand(V, device="cuda", generator=g) < 0.33] = float("-inf")
    return x


def run_norm(lib, x):
    rows, V = x.shape
    buf, flat = guarded(rows * V, torch.float32, SENT_F)
    y = flat.view(rows, V)
    y.copy_(x)
    sbuf, sflat = guarded(rows * 2, torch.float32, SENT_F)
    check(lib.fvhd_op_dec_beam_norm(stream(), ptr(y), rows, V, ptr(sflat)), "fvhd_op_dec_beam_norm")
    torch.cuda.synchronize()
    assert guards_intact(buf, SENT_F) and guards_intact(sbuf, SENT_F)
    return y, sflat.view(rows, 2)


def check_norm(x, y, stats, what):
    """bit-equal to (x - M) - L of the op's own M, L; within the derived bound of fp64 -> the worst |err| / bound"""
    M, L = stats[:, :1], stats[:, 1:]
    assert torch.equal(M[:, 0], x.max(1).values), what
    assert torch.equal(bits((x - M) - L), bits(y)), what
    want, bound = R.norm_reference(x), R.norm_bound(x)
    fin = torch.isfinite(want)
    assert bool((y[~fin] == float("-inf")).all()) and bool(torch.isfinite(y[fin]).all()), what
    ratio = ((y.double() - want)[fin].abs() / bound[fin]).max()
    assert float(ratio) <= 1.0, f"{what}: max |err| / bound = {float(ratio):.3g}"
    return float(ratio)


@pytest.mark.parametrize("V", [4096, 4100, 151936])
@pytest.mark.parametrize("rows", [1, 16, 17, 64])
def test_normalisation_against_fp64_and_its_own_statistics(lib, rows, V):
    x = norm_rows(rows, V, 100 * rows + V % 97)
    y, stats = run_norm(lib, x)
    ratio = check_norm(x, y, stats, f"rows {rows} V {V}")
    print(f"beam_norm rows {rows} V {V}: max |err| / bound {ratio:.3f}")


@pytest.mark.parametrize("V", [4099, 4100, 17, 3])
@pytest.mark.parametrize("kind", ["plain", "spread", "banned"])
def test_normalisation_one_row_kind_and_rows_that_are_not_aligned(lib, kind, V):
    """V % 4 != 0: rows 1 and 2 do not start on 16 bytes and go element by element; V < 16: a slice of less than one thread's share"""
    x = norm_rows(3, V, 7 + V, kinds=(kind,))
    if kind == "banned":
        x[:, 0] = 0.5                                             # (a row keeps a finite entry)
    y, stats = run_norm(lib, x)
    check_norm(x, y, stats, f"{kind} V {V}")


@pytest.mark.parametrize("G, K", [(4, 4), (16, 4)])
def test_normalisation_statistics_are_the_plain_chains(lib, G, K):
    """M and L bit for bit what the plain top-K chain subtracts (fvhd_op_dec_beam_sample reports them): the same slices, the same order"""
    V, rows = 151936, G * K
    x = norm_rows(rows, V, 5)
    _, stats = run_norm(lib, x)
    info = torch.zeros(rows, 4, device="cuda")
    out_v, out_i = torch.zeros(G, 4, device="cuda"), torch.zeros(G, 4, device="cuda", dtype=torch.long)
    check(lib.fvhd_op_dec_beam_sample(stream(), ptr(x), ptr(torch.zeros(G, K, device="cuda")), G, K, 4, V, 1.0, 0, 1.0, 2, 0, 0, None, None, ptr(info),
                                      ptr(out_v), ptr(out_i)), "fvhd_op_dec_beam_sample")
    assert torch.equal(bits(info[:, 2:4]), bits(stats))


def test_normalisation_refusals(lib):
    x = torch.zeros(2, 64, device="cuda")
    assert lib.fvhd_op_dec_beam_norm(stream(), ptr(x), 65, 64, None) != 0
    assert lib.fvhd_op_dec_beam_norm(stream(), ptr(x), 2, 262145, None) != 0
    assert lib.fvhd_op_dec_beam_norm(stream(), None, 2, 64, None) != 0


# ---- b2. the history / state reorder ---------------------------------------------------------------------------------------------------
BATCH, CAP, VG = 8, 12, 4100
W = (VG + 31) // 32            # 129 words: the last one holds 4 bits


def history_rows(seed):
    """per row a token list: empty, at capacity, repeats (sign bits), the bitmap's tail word -> (hist, seen, count) as the step keeps them"""
    g = torch.Generator().manual_seed(seed)
    lists = [[], torch.randint(0, VG, (CAP,), generator=g).tolist(), [7, 7, 7, 4099, 7], [4099, 4096, 31, 32, 4096, 31], [5],
             torch.randint(0, 40, (9,), generator=g).tolist(), [4097, 0, 4097], torch.randint(0, VG, (CAP - 1,), generator=g).tolist()]
    hist = torch.full((BATCH, CAP), SENT_I, dtype=torch.int32)
    seen = torch.zeros((BATCH, W), dtype=torch.int64)
    count = torch.zeros((BATCH,), dtype=torch.int32)
    for r, toks in enumerate(lists):
        have = set()
        for i, t in enumerate(toks):
            hist[r, i] = t - (1 << 31) if t in have else t        # sign bit: a repeat
            have.add(t)
            seen[r, t >> 5] |= 1 << (t & 31)
        count[r] = len(toks)
    seen = torch.where(seen >= 1 << 31, seen - (1 << 32), seen).to(torch.int32)
    return hist, seen, count


def run_gather(lib, src, rows_in, with_hist=True, with_states=True):
    hist0, seen0, count0 = history_rows(3)
    g = torch.Generator().manual_seed(11)
    states0 = torch.randint(-1, 500, (BATCH,), generator=g, dtype=torch.int32)
    flags0 = torch.randint(0, 2, (BATCH,), generator=g, dtype=torch.int32)
    bufs = {}
    for name, t in (("hist", hist0), ("seen", seen0), ("count", count0), ("states", states0), ("flags", flags0)):
        buf, flat = guarded(t.numel(), torch.int32, SENT_I)
        flat.copy_(t.reshape(-1).cuda())
        bufs[name] = (buf, flat.view(t.shape), t)
    status = torch.zeros(1, device="cuda", dtype=torch.int32)
    src_d = torch.tensor(src, device="cuda", dtype=torch.long)
    p = {k: ptr(v[1]) for k, v in bufs.items()}
    code = lib.fvhd_op_dec_hist_gather(stream(), p["hist"] if with_hist else None, p["seen"] if with_hist else None, p["count"] if with_hist else None,
                                       p["states"] if with_states else None, p["flags"] if with_states else None, ptr(src_d), BATCH, rows_in, len(src),
                                       CAP, VG, ptr(status))
    check(code, "fvhd_op_dec_hist_gather")
    torch.cuda.synchronize()
    for name, (buf, _, _) in bufs.items():
        assert guards_intact(buf, SENT_I), name
    return {k: (v[1].cpu(), v[2]) for k, v in bufs.items()}, int(status)


def expect_gather(old, src, with_hist=True, with_states=True):
    want = {k: v.clone() for k, v in old.items()}
    for r, s in enumerate(src):
        if with_hist:
            n = int(old["count"][s])
            want["hist"][r, :n] = old["hist"][s, :n]              # entries behind the source's count keep the row's old bytes
            want["seen"][r] = old["seen"][s]
            want["count"][r] = old["count"][s]
        if with_states:
            want["states"][r] = old["states"][s]
            want["flags"][r] = old["flags"][s]
    return want


CASES = {
    "replication": ([0, 0, 0, 0, 1, 1, 1, 1], 2),                 # src = r // K: G = 2 prefilled rows become G K = 8
    "two_cycle": ([1, 0, 2, 3, 5, 4, 7, 6], 8),                   # swaps: the in-place hazard; rows 2, 3 are identity rows
    "mixed": ([2, 2, 3, 1, 1, 0], 8),                             # 6 of 8 rows; sources read after they were overwritten in place
    "identity": ([0, 1, 2, 3, 4, 5, 6, 7], 8),
    "empty_and_full": ([1, 0, 0, 1], 4),                          # the empty history and the one at capacity trade places
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("with_hist, with_states", [(True, True), (True, False), (False, True)])
def test_histories_and_states_follow_src(lib, name, with_hist, with_states):
    src, rows_in = CASES[name]
    got, status = run_gather(lib, src, rows_in, with_hist, with_states)
    want = expect_gather({k: v[1] for k, v in got.items()}, src, with_hist, with_states)
    assert status == 0
    for k in want:
        assert torch.equal(got[k][0], want[k]), (name, k)


@pytest.mark.parametrize("src", [[0, 1, 8, 3], [1, -1], [0, 0, 0, 0, 1, 1, 1, 2]])
def test_an_index_out_of_range_writes_only_the_error_word(lib, src):
    rows_in = 8 if src[-1] != 2 else 2                            # (2 is out of range for rows_in = 2)
    got, status = run_gather(lib, src, rows_in)
    assert status == 3
    for k, (now, before) in got.items():
        assert torch.equal(now, before), k


def test_gather_does_nothing_behind_an_error_word(lib):
    hist0, seen0, count0 = history_rows(3)
    h, s, c = hist0.cuda(), seen0.cuda(), count0.cuda()
    status = torch.full((1,), 1, device="cuda", dtype=torch.int32)
    src = torch.tensor([1, 0], device="cuda")
    check(lib.fvhd_op_dec_hist_gather(stream(), ptr(h), ptr(s), ptr(c), None, None, ptr(src), BATCH, 2, 2, CAP, VG, ptr(status)), "fvhd_op_dec_hist_gather")
    assert int(status) == 1 and torch.equal(h.cpu(), hist0) and torch.equal(s.cpu(), seen0) and torch.equal(c.cpu(), count0)


# ---- b3. the top-K chains on pre-normalised rows -----------------------------------------------------------------------------------------
def topk_inputs(G, K, V, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = 3.0 * torch.randn(G * K, V, device="cuda", generator=g)
    scores = -2.0 * torch.rand(G, K, device="cuda", generator=g)
    scores[:, -1] = -1e9                                          # a dead beam
    return x, scores


def outs(G, keep):
    return torch.zeros(G, keep, device="cuda"), torch.zeros(G, keep, device="cuda", dtype=torch.long)


@pytest.mark.parametrize("V", [4096, 151936])
@pytest.mark.parametrize("G, K", [(1, 2), (3, 4), (16, 4)])
def test_untouched_rows_give_the_plain_chain_bit_for_bit(lib, G, K, V):
    """normalise, then the pre-normalised chain = the plain chain on the raw logits: an entry no processor edits carries exactly the value
    the plain chain adds to the beam score.  (Fixed seeds; a tie that straddles a row's top-C boundary could legitimately differ between
    selection by raw and by normalised value - none of these seeds hits one.)"""
    keep = 2 * K
    x, scores = topk_inputs(G, K, V, 31 * G + K)
    want_v, want_i = outs(G, keep)
    check(lib.fvhd_op_dec_beam_topk(stream(), ptr(x), ptr(scores), G, K, keep, V, ptr(want_v), ptr(want_i)), "fvhd_op_dec_beam_topk")
    y = x.clone()
    check(lib.fvhd_op_dec_beam_norm(stream(), ptr(y), G * K, V, None), "fvhd_op_dec_beam_norm")
    got_v, got_i = outs(G, keep)
    check(lib.fvhd_op_dec_beam_topk_pre(stream(), ptr(y), ptr(scores), G, K, keep, V, ptr(got_v), ptr(got_i)), "fvhd_op_dec_beam_topk_pre")
    assert torch.equal(got_i, want_i) and torch.equal(bits(got_v), bits(want_v))
    # and against torch on the normalised rows: acc = x' + score, ties to the lower flat index
    acc = (y.view(G, K, V) + scores[:, :, None]).reshape(G, K * V)
    top = torch.topk(acc, keep)
    assert torch.equal(bits(got_v), bits(top.values))
    assert torch.equal(got_i, top.indices) or torch.equal(acc.gather(1, got_i), top.values)


@pytest.mark.parametrize("G, K", [(1, 2), (3, 4), (16, 4)])
def test_zero_noise_and_unit_temperature_draw_the_greedy_chain(lib, G, K):
    V, keep = 4096, 2 * K
    x, scores = topk_inputs(G, K, V, 17 + G)
    check(lib.fvhd_op_dec_beam_norm(stream(), ptr(x), G * K, V, None), "fvhd_op_dec_beam_norm")
    x[:, 5:900:7] = float("-inf")                                 # processed rows: bans ...
    x[:, 3] *= 1.3                                                # ... and a penalised entry
    want_v, want_i = outs(G, keep)
    check(lib.fvhd_op_dec_beam_topk_pre(stream(), ptr(x), ptr(scores), G, K, keep, V, ptr(want_v), ptr(want_i)), "fvhd_op_dec_beam_topk_pre")
    noise = torch.zeros_like(x)
    for top_k, top_p in ((0, 1.0), (50, 1.0), (0, 0.999999)):
        got_v, got_i = outs(G, keep)
        check(lib.fvhd_op_dec_beam_sample_pre(stream(), ptr(x), ptr(scores), G, K, keep, V, 1.0, top_k, top_p, keep, 0, 0, ptr(noise), None, None,
                                              ptr(got_v), ptr(got_i)), "fvhd_op_dec_beam_sample_pre")
        assert torch.equal(got_i, want_i) and torch.equal(bits(got_v), bits(want_v)), (top_k, top_p)


def test_banned_entries_are_never_candidates(lib):
    G, K, V, keep = 2, 2, 4096, 8
    x = torch.full((G * K, V), float("-inf"), device="cuda")
    x[0, 10], x[0, 4000], x[1, 77] = -0.5, -1.5, -0.25             # prompt 0: three allowed entries in all
    x[2, 5] = -0.125                                              # prompt 1: one; its second row allows nothing
    scores = torch.tensor([[0.0, -1.0], [-3.0, 0.0]], device="cuda")
    want_v = torch.tensor([[-0.5, -1.25, -1.5] + [float("-inf")] * 5, [-3.125] + [float("-inf")] * 7], device="cuda")
    want_i = torch.tensor([[10, V + 77, 4000, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0, 0, 0]], device="cuda")
    got_v, got_i = outs(G, keep)
    check(lib.fvhd_op_dec_beam_topk_pre(stream(), ptr(x), ptr(scores), G, K, keep, V, ptr(got_v), ptr(got_i)), "fvhd_op_dec_beam_topk_pre")
    assert torch.equal(got_v, want_v) and torch.equal(got_i, want_i)
    info = torch.zeros(G * K, 4, device="cuda")
    got_v, got_i = outs(G, keep)
    check(lib.fvhd_op_dec_beam_sample_pre(stream(), ptr(x), ptr(scores), G, K, keep, V, 1.0, 0, 1.0, 2, 0, 0, ptr(torch.zeros_like(x)), None, ptr(info),
                                          ptr(got_v), ptr(got_i)), "fvhd_op_dec_beam_sample_pre")
    assert torch.equal(got_v, want_v) and torch.equal(got_i, want_i)
    assert info[:, 1].tolist() == [2.0, 1.0, 1.0, 0.0]            # the kept counts: a -inf entry is never counted
