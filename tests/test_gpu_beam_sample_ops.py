"""Beam-search sampling on its own (csrc/llm_beam.hip "beam-search sampling", fvhd_op_dec_beam_sample) against the fp64 reference of
tests/beam_sample_reference.py and, with the noise switched off, bit for bit against the greedy chain (fvhd_op_dec_beam_topk).

The inputs are random logits whose rows differ in scale by 160x, with about 1 % of -inf entries.  Bounds: `beam_sample_reference.bound`
derives the bound on the device's key a + g and on the returned a from the kernel's order of operations; the Philox seeds of the selection
cases are those at which every adjacent gap among the reference's top keep + 1 keys exceeds twice that bound (tools/beam_sample_margins.py
finds them on the CPU; the test asserts it of its own inputs).  Each selection case prints the largest observed fraction of its bound
(profiles/beam_sample_bound.log keeps a run's lines)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_sample_reference as R  # noqa: E402
from llm_testlib import SENT, bits, check, guarded, lib, ptr, stream  # noqa: E402,F401

pytestmark = pytest.mark.gpu

VOCABS = [16, 4096, 4112, 151936, 262144]            # less than a slice, one slice, a slice edge + 16, the 0.5B vocabulary, the maximum
GKC = [(1, 2, 4), (3, 5, 10), (4, 16, 64), (32, 2, 4)]      # the last two: 64 rows = four blocks of the threshold search
SHAPES = [(V, G, K, C) for V in VOCABS for (G, K, C) in GKC if C <= V]      # (keep <= V: 64 picks do not fit 16 tokens)
TEMPERATURES = [1.0, 0.2]
N_STEP = 7                                           # the cache length of the draws
INF = float("inf")


def selection_settings(T, K, keep):
    """(top_k, top_p, min_keep) of a selection case: no filter at T = 1, predict.py's top_k with a top_p at T = 0.2; min_keep = n_eos + 1
    for the n_eos that gives this keep"""
    m = max(2, keep // K)
    return (0, 1.0, m) if T == 1.0 else (50, 0.9, m)


# (V, G, K, keep, T) -> the Philox seed of the case: tools/beam_sample_margins.py
SELECTION_SEEDS = {
    (16, 1, 2, 4, 1.0): 0, (16, 1, 2, 4, 0.2): 0, (16, 3, 5, 10, 1.0): 0, (16, 3, 5, 10, 0.2): 0, (16, 32, 2, 4, 1.0): 0, (16, 32, 2, 4, 0.2): 0,
    (4096, 1, 2, 4, 1.0): 0, (4096, 1, 2, 4, 0.2): 0, (4096, 3, 5, 10, 1.0): 0, (4096, 3, 5, 10, 0.2): 0, (4096, 4, 16, 64, 1.0): 0,
    (4096, 4, 16, 64, 0.2): 0, (4096, 32, 2, 4, 1.0): 0, (4096, 32, 2, 4, 0.2): 0,
    (4112, 1, 2, 4, 1.0): 0, (4112, 1, 2, 4, 0.2): 0, (4112, 3, 5, 10, 1.0): 0, (4112, 3, 5, 10, 0.2): 0, (4112, 4, 16, 64, 1.0): 1,
    (4112, 4, 16, 64, 0.2): 0, (4112, 32, 2, 4, 1.0): 0, (4112, 32, 2, 4, 0.2): 0,
    (151936, 1, 2, 4, 1.0): 0, (151936, 1, 2, 4, 0.2): 0, (151936, 3, 5, 10, 1.0): 0, (151936, 3, 5, 10, 0.2): 0, (151936, 4, 16, 64, 1.0): 0,
    (151936, 4, 16, 64, 0.2): 0, (151936, 32, 2, 4, 1.0): 0, (151936, 32, 2, 4, 0.2): 0,
    (262144, 1, 2, 4, 1.0): 0, (262144, 1, 2, 4, 0.2): 0, (262144, 3, 5, 10, 1.0): 0, (262144, 3, 5, 10, 0.2): 0, (262144, 4, 16, 64, 1.0): 1,
    (262144, 4, 16, 64, 0.2): 4, (262144, 32, 2, 4, 1.0): 0, (262144, 32, 2, 4, 0.2): 0,
}


def beam_sample(lib, logits, scores, G, K, C, T=1.0, top_k=0, top_p=1.0, m=2, seed=0, n=0, noise=None, noise_out=False):
    """one call into outputs with sentinel rows before and behind -> (values fp32 [G, C], indices int64 [G, C], info fp32 [rows, 4], g or None)"""
    rows, V = logits.shape
    vbuf, _ = guarded(G + 2, 2 * C, "cuda")
    ibuf, _ = guarded(G + 2, 4 * C, "cuda")
    nbuf, _ = guarded(rows + 2, 8, "cuda")
    vals, idx, info = vbuf[1:G + 1].view(torch.float32), ibuf[1:G + 1].view(torch.int64), nbuf[1:rows + 1].view(torch.float32)
    g = torch.full((rows * V + 64,), float("nan"), device="cuda") if noise_out else None
    check(lib.fvhd_op_dec_beam_sample(stream(), ptr(logits), ptr(scores), G, K, C, V, T, top_k, top_p, m, seed, n, ptr(noise), ptr(g), ptr(info),
                                      ptr(vals), ptr(idx)), "fvhd_op_dec_beam_sample")
    torch.cuda.synchronize()
    for buf, used in ((vbuf, G), (ibuf, G), (nbuf, rows)):
        assert bool((buf[0] == SENT).all()) and bool((buf[used + 1:] == SENT).all()), "a guard row was written"
    if g is not None:
        assert bool(torch.isnan(g[rows * V:]).all()), "noise_out was written past its end"
        g = g[:rows * V].view(rows, V).clone()
    return vals.clone(), idx.clone(), info.clone(), g


def greedy_topk(lib, logits, scores, G, K, C):
    vals = torch.empty(G, C, device="cuda")
    idx = torch.empty(G, C, device="cuda", dtype=torch.long)
    check(lib.fvhd_op_dec_beam_topk(stream(), ptr(logits), ptr(scores), G, K, C, logits.shape[1], ptr(vals), ptr(idx)), "fvhd_op_dec_beam_topk")
    torch.cuda.synchronize()
    return vals, idx


@pytest.mark.parametrize("V,G,K,C", SHAPES)
def test_without_noise_and_filters_it_is_the_greedy_chain_bit_for_bit(lib, V, G, K, C):
    x, scores = R.inputs(V, G, K, 1)
    x, scores = x.cuda(), scores.cuda()
    zero = torch.zeros_like(x)
    want_v, want_i = greedy_topk(lib, x, scores, G, K, C)
    assert bool(torch.isfinite(want_v).all())                    # (enough finite candidates: the greedy chain is defined)
    vals, idx, info, _ = beam_sample(lib, x, scores, G, K, C, noise=zero)
    assert torch.equal(idx, want_i) and torch.equal(bits(vals), bits(want_v))
    assert bool((info[:, 0] == -INF).all()) and torch.equal(info[:, 1].long(), (x > -INF).sum(-1))      # nothing binds: every finite logit is kept
    # a dead beam is an ordinary input, and the same call twice gives the same bits
    scores[:, 0] = -1e9
    want_v, want_i = greedy_topk(lib, x, scores, G, K, C)
    a = beam_sample(lib, x, scores, G, K, C, noise=zero)
    b = beam_sample(lib, x, scores, G, K, C, noise=zero)
    assert torch.equal(a[1], want_i) and torch.equal(bits(a[0]), bits(want_v))
    assert torch.equal(a[1], b[1]) and torch.equal(bits(a[0]), bits(b[0]))


def threshold_case(name, V=4112, rows=6):
    """-> (logits on the CPU, top_k, top_p, m, what decides theta)"""
    x, _ = R.inputs(V, 1, rows, 5)
    if name == "top_k >= V":
        return x, V + 5, 1.0, 2
    if name == "top_k < m":
        return x, 1, 1.0, 3
    if name == "top_p tiny":
        return x, 0, 1e-6, 4
    if name == "top_k then top_p":
        return x, 50, 0.9, 2
    if name == "top_p alone":
        return x, 0, 0.7, 2
    if name == "boundary tie":                                    # the top_k-th and the next three logits are equal: kept as a group
        for r in range(rows):
            order = torch.argsort(x[r], descending=True)
            x[r, order[9:13]] = float(x[r, order[9]])
        return x, 10, 1.0, 2
    if name == "tie at v_m":                                      # the m-th and (m + 1)-th are equal and top_p would keep one token
        for r in range(rows):
            order = torch.argsort(x[r], descending=True)
            x[r, order[2]] = x[r, order[1]]
        return x, 0, 1e-6, 2
    raise KeyError(name)


@pytest.mark.parametrize("T", [1.0, 0.2])
@pytest.mark.parametrize("name", ["top_k >= V", "top_k < m", "top_p tiny", "top_k then top_p", "top_p alone", "boundary tie", "tie at v_m"])
def test_thresholds_and_kept_counts_equal_the_reference(lib, name, T):
    x, top_k, top_p, m = threshold_case(name)
    rows, V = x.shape
    ref = R.reference(x, torch.zeros(1, rows), 1, rows, 2 * rows, T, top_k, top_p, m, noise=torch.zeros_like(x))
    if top_p < 1.0:                                               # the inputs' own margin: top-p's boundary is not within rounding of a token's mass
        s = ref["s"]
        p = torch.softmax(torch.where(s >= R.kept_set(s, top_k, 1.0, m)[1][:, None], s, torch.full_like(s, -INF)), -1)      # over the top-k survivors
        mass = torch.sort(p, -1, descending=True).values.cumsum(-1)
        assert float((mass - top_p).abs().min()) > 1e-5 or top_p < 1e-5
    xg = x.cuda()
    vals, idx, info, _ = beam_sample(lib, xg, torch.zeros(1, rows, device="cuda"), 1, rows, 2 * rows, T, top_k, top_p, m, noise=torch.zeros_like(xg))
    print(f"{name} T={T}: theta {info[:, 0].tolist()}, kept {info[:, 1].long().tolist()}")
    assert torch.equal(info[:, 1].long().cpu(), ref["count"])
    assert torch.equal(info[:, 0].double().cpu(), ref["theta"])
    assert bool((ref["count"] >= m).all())
    if name == "top_k >= V":
        assert bool((info[:, 0] == -INF).all())
    if name == "boundary tie":
        assert ref["count"].tolist() == [13] * rows
    if name in ("top_p tiny", "top_k < m"):
        assert ref["count"].tolist() == [m] * rows                # min_keep decides
    if name == "tie at v_m":
        assert ref["count"].tolist() == [3] * rows
    # M and L, in the order the greedy chain sums them: within the bound on L
    assert torch.equal(info[:, 2].cpu(), x.max(-1).values)
    L = -torch.log_softmax(x.double(), -1).max(-1).values        # log sum exp(x - M) = -(the log-probability of the maximum)
    assert float((info[:, 3].double().cpu() - L).abs().max()) <= R.DELTA_L


def test_a_row_with_fewer_than_min_keep_finite_logits_keeps_the_finite_ones(lib):
    V, K, C = 4096, 2, 6
    x = torch.full((K, V), -INF)
    x[0, 70], x[0, 4000] = 1.0, 0.5
    x[1, 9] = 2.0
    x = x.cuda()
    scores = torch.tensor([[0.0, -0.5]], device="cuda")
    vals, idx, info, _ = beam_sample(lib, x, scores, 1, K, C, 0.5, 50, 0.3, 3, noise=torch.zeros_like(x))
    assert info[:, 1].tolist() == [2.0, 1.0]
    assert idx[0].tolist() == [V + 9, 70, 4000, 0, 0, 0]          # a: 0 / 0.5 - 0.5, log(0.62) / 0.5, log(0.38) / 0.5; then the slots nothing fills
    assert bool((vals[0, 3:] == -INF).all()) and bool(torch.isfinite(vals[0, :3]).all())


@pytest.mark.parametrize("decides", ["top_k", "top_p", "min_keep"])
def test_noise_does_not_bring_back_a_filtered_token(lib, decides):
    V, G, K, C, T = 4112, 1, 2, 4, 0.7
    x, scores = R.inputs(V, G, K, 9)
    top_k, top_p, m = {"top_k": (5, 1.0, 2), "top_p": (0, 0.5, 2), "min_keep": (1, 1.0, 3)}[decides]
    ref = R.reference(x, scores, G, K, C, T, top_k, top_p, m, noise=torch.zeros_like(x))
    noise = torch.zeros_like(x)
    out = (~ref["kept"]) & (x > -INF)
    for r in range(K):                                            # + 1e6 on the best filtered-out token of each row, and on a -inf one
        cand = torch.where(out[r], ref["s"][r], torch.full_like(ref["s"][r], -INF))
        noise[r, int(cand.argmax())] = 1e6
        noise[r, int((x[r] == -INF).nonzero()[0])] = 1e6
    want = R.reference(x, scores, G, K, C, T, top_k, top_p, m, noise=noise)
    vals, idx, info, _ = beam_sample(lib, x.cuda(), scores.cuda(), G, K, C, T, top_k, top_p, m, noise=noise.cuda())
    assert torch.equal(info[:, 1].long().cpu(), ref["count"]) and torch.equal(info[:, 0].double().cpu(), ref["theta"])
    assert torch.equal(idx.cpu(), want["index"]) and torch.equal(want["index"], ref["index"])      # the picks of the run without that noise
    picked = torch.gather(ref["kept"].view(G, K * V), 1, idx.cpu())
    assert bool(picked.all())
    assert float((vals.double().cpu() - want["scores"]).abs().max()) <= R.bound(want, T)[1]


def test_noise_moves_picks_across_beams_and_ties_go_to_the_lower_flat_index(lib):
    V, G, K, C = 4112, 2, 3, 6
    x, scores = R.inputs(V, G, K, 4)
    x[x == -INF] = -3.0
    scores[:] = torch.tensor([[0.0, -30.0, -60.0]])              # without noise every pick is beam 0's
    xg, sg = x.cuda(), scores.cuda()
    zero = torch.zeros_like(xg)
    _, idx0, _, _ = beam_sample(lib, xg, sg, G, K, C, noise=zero)
    assert bool((idx0 < V).all())
    noise = torch.zeros_like(x)
    noise[2, 4100], noise[1, 17], noise[5, 4111], noise[3, 0] = 500.0, 400.0, 300.0, 100.0      # beams 2 and 1 of prompt 0, beams 2 and 0 of prompt 1
    want = R.reference(x, scores, G, K, C, 1.0, 0, 1.0, 2, noise=noise)
    vals, idx, _, _ = beam_sample(lib, xg, sg, G, K, C, noise=noise.cuda())
    assert idx[0, :2].tolist() == [2 * V + 4100, V + 17] and idx[1, :2].tolist() == [2 * V + 4111, 0]
    assert torch.equal(idx.cpu(), want["index"])
    assert float((vals.double().cpu() - want["scores"]).abs().max()) <= R.bound(want, 1.0)[1]      # the UNPERTURBED a, in draw order
    assert float(vals[0, 0]) < float(vals[0, 2])                  # ... which does not descend
    # ties in a + g: the beams of a prompt are equal rows with equal scores (the same M and L, bit for bit), two equal best logits in each, equal
    # noise -> six equal keys, taken in flat index order across slices and beams
    x2 = torch.full((2 * K, V), -5.0)
    x2[:K, 5] = x2[:K, 4100] = 2.0
    s2 = torch.zeros(2, K)
    got_v, got_i, _, _ = beam_sample(lib, x2.cuda(), s2.cuda(), 2, K, 5, noise=torch.full((2 * K, V), 0.25, device="cuda"))
    assert got_i[0].tolist() == [5, 4100, V + 5, V + 4100, 2 * V + 5]
    assert got_i[1].tolist() == [0, 1, 2, 3, 4]                   # prompt 1: every candidate ties
    assert bool((got_v[0] == got_v[0, 0]).all())


PHILOX_SEED = 1                                                   # see test_philox_noise: found on the CPU


def test_philox_noise(lib):
    """noise_out against g(u) in fp64 from the Python Philox over 64 x 4112 values, u within 2^-17 of both ends among them"""
    V, G, K, C, n = 4112, 32, 2, 4, 123456
    seed = (0xC0FFEE << 32) | PHILOX_SEED
    u = R.gumbel_uniform(R.gumbel_words(seed, G * K, n, V))
    assert u.min() < 2.0 ** -17 and u.max() > 1.0 - 2.0 ** -17, (u.min(), 1 - u.max())
    want = R.gumbel_noise(seed, G * K, n, V)
    x, scores = R.inputs(V, G, K, 2)
    _, _, _, g = beam_sample(lib, x.cuda(), scores.cuda(), G, K, C, 0.2, 50, 0.9, 2, seed=seed, n=n, noise_out=True)
    tol = R.ULPS_LOG * 2.0 ** -23 * (1.0 + want.abs())
    frac = ((g.double().cpu() - want).abs() / tol).max()
    lo, hi = int(u.argmin()), int(u.argmax())
    print(f"philox noise: max |g - g64| / bound {float(frac):.3f}; g at the smallest u {float(g.flatten()[lo]):.6f} (fp64 {float(want.flatten()[lo]):.6f}), "
          f"at the largest {float(g.flatten()[hi]):.6f} (fp64 {float(want.flatten()[hi]):.6f})")
    assert float(frac) <= 1.0
    # another n, another row offset in the counter: different noise
    _, _, _, g2 = beam_sample(lib, x.cuda(), scores.cuda(), G, K, C, 0.2, 50, 0.9, 2, seed=seed, n=n + 1, noise_out=True)
    assert float((g2 != g).float().mean()) > 0.99


@pytest.mark.parametrize("T", TEMPERATURES)
@pytest.mark.parametrize("V,G,K,C", SHAPES)
def test_selection_equals_the_reference_in_order(lib, V, G, K, C, T):
    top_k, top_p, m = selection_settings(T, K, C)
    seed = SELECTION_SEEDS[(V, G, K, C, T)]
    x, scores = R.inputs(V, G, K, 0)
    x, scores = x.cuda(), scores.cuda()
    ref = R.reference(x, scores, G, K, C, T, top_k, top_p, m, seed=seed, n=N_STEP, extra=1)
    b_key, b_a = R.bound(ref, T)
    keys = ref["keys"]
    gap = R.smallest_gap(keys)                                    # (a prompt whose filters leave fewer than keep + 1 candidates has fewer competitors)
    assert gap > 2 * b_key, f"the inputs' smallest gap among the top {C + 1} keys is {gap:.3g} <= 2 * {b_key:.3g}: tools/beam_sample_margins.py"
    vals, idx, info, g = beam_sample(lib, x, scores, G, K, C, T, top_k, top_p, m, seed=seed, n=N_STEP, noise_out=True)
    assert torch.equal(info[:, 1].long(), ref["count"]) and torch.equal(info[:, 0].double(), ref["theta"])
    assert torch.equal(idx, ref["index"][:, :C])
    err_a = float((vals.double() - ref["scores"][:, :C])[torch.isfinite(keys[:, :C])].abs().max())
    filled = torch.isfinite(keys[:, :C])
    assert torch.equal(torch.isfinite(vals), filled)              # a slot that cannot be filled holds (-inf, 0)
    dev_key = vals.double() + torch.gather(g.double().view(G, -1), 1, idx)
    err_key = float((dev_key - keys[:, :C])[filled].abs().max())
    print(f"beam_sample V={V} G={G} K={K} keep={C} T={T}: smallest gap {gap:.3g}, bound on a + g {b_key:.3g}, observed {err_key:.3g} "
          f"({err_key / b_key:.3f} of it); bound on a {b_a:.3g}, observed {err_a:.3g} ({err_a / b_a:.3f} of it)")
    assert err_a <= b_a and err_key <= b_key
    assert not math.isnan(err_key)
