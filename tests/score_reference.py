"""TEST INFRASTRUCTURE ONLY - the fp64 reference of scoring (csrc/llm_score.hip, include/fvhd.h "LLM scoring"), its DERIVED error bound,
the host mirror of the launch plan and the planted-peak inputs.  Importing it needs no GPU.

Reference: z = x . W^T, lse = logsumexp(z), logprob = z[target] - lse, all in fp64 from the bf16-ROUNDED operands (what the kernel reads).

Bound per row, u = 2^-24 (fp32 unit roundoff), A = max_v sum_k |x_k w_vk|:
    |err z|   <= K u A                            a sum of K exact bf16 x bf16 products in ANY fp32 order (MFMA, split or not)
    |err lse| <= K u A + V u + 8 u (1 + |lse|)    lse is 1-Lipschitz in z (max norm); the fp32 sum of V positive terms in any order has a
                                                  relative error <= V u, i.e. V u absolute on its log; exp, log and the final add are a
                                                  few ulp of values <= 1 + |lse|
    |err logprob| <= the sum of the two
PINNING: tests/test_score_reference.py (against torch.nn.functional.cross_entropy in fp64, and the plan against the library)."""
import math

import torch

U = 2.0 ** -24
TILE = 128              # vocabulary tile of llm_score.hip
ROWS = 128              # rows per workgroup
MAX_SEG = 64


def reference(x, W, targets):
    """x [M, K], W [V, K] (any float dtype, values already bf16-representable), targets int64 [M] -> (lse fp64 [M], logprob fp64 [M], z fp64
    [M, V]); logprob 0 at a negative target, NaN at a target >= V"""
    z = x.double() @ W.double().t()
    lse = torch.logsumexp(z, -1)
    V = W.shape[0]
    ok = (targets >= 0) & (targets < V)
    zt = z.gather(1, targets.clamp(0, V - 1)[:, None])[:, 0]
    lp = torch.where(ok, zt - lse, torch.zeros_like(lse))
    lp = torch.where(targets >= V, torch.full_like(lp, float("nan")), lp)
    return lse, lp, z


def bounds(x, W, lse, z_extra=None):
    """-> (bound on z, bound on lse, bound on logprob), fp64 [M] each; z_extra [M]: a further per-row error of every logit (an input
    rounding the caller accounts for), added to the z term"""
    K, V = x.shape[1], W.shape[0]
    A = (x.double().abs() @ W.double().abs().t()).amax(-1)
    bz = K * U * A
    if z_extra is not None:
        bz = bz + z_extra
    bl = bz + V * U + 8 * U * (1 + lse.abs())
    return bz, bl, bz + bl


def worst_ratio(got, want, bound):
    """max |got - want| / bound over finite `want`; asserts that `got` is finite there"""
    sel = torch.isfinite(want)
    assert bool(torch.isfinite(got.double()[sel]).all()), "non-finite output"
    return float(((got.double()[sel] - want[sel]).abs() / bound[sel]).max()) if bool(sel.any()) else 0.0


def plan(M, V, K):
    """host mirror of fvhd_lm_score_plan: segments S (0 = the shape is refused)"""
    if M < 1 or V < 8 or V % 8 or K < 32 or K % 32:
        return 0
    nrb, ntile = (M + ROWS - 1) // ROWS, (V + TILE - 1) // TILE
    return max(1, min(512 // nrb, MAX_SEG, ntile))


def segment_tiles(V, S):
    """first vocabulary tile of every segment, and the tile count: segment s walks tiles [s * ntile // S, (s + 1) * ntile // S)"""
    ntile = (V + TILE - 1) // TILE
    return [s * ntile // S for s in range(S)], ntile


def tiles_per_segment(M, V, K):
    """tile count of every segment of the plan in force"""
    S = plan(M, V, K)
    firsts, ntile = segment_tiles(V, S)
    return [b - a for a, b in zip(firsts, firsts[1:] + [ntile])]


def walk_columns(M, V, K):
    """for every segment that walks two or more tiles: a column in the middle of its FIRST tile, of its LAST tile and (three or more) of a
    tile between them - a peak there is met at the start of the walk (every later tile must leave the running maximum alone), at its end
    (the running sum is rescaled when it arrives) or in between"""
    S = plan(M, V, K)
    firsts, ntile = segment_tiles(V, S)
    cols = []
    for a, b in zip(firsts, firsts[1:] + [ntile]):
        if b - a >= 2:
            for t in sorted({a, (a + b - 1) // 2, b - 1}):
                cols.append(min(t * TILE + 70, V - 1))
    return cols


def edge_columns(M, V, K):
    """the columns where a dropped or doubled logit would hide: 0, V - 1, each side of every vocabulary-tile edge (the segment edges of the
    plan in force are among them - asserted), the middle of the ragged last tile, the wave / lane-group edges inside a tile and, where
    segments walk several tiles, `walk_columns`"""
    S = plan(M, V, K)
    firsts, ntile = segment_tiles(V, S)
    cols = {0, V - 1}
    cols.update(walk_columns(M, V, K))
    for t in range(1, ntile):
        cols.update((t * TILE - 1, t * TILE))
    for f in firsts[1:]:
        assert f * TILE - 1 in cols and f * TILE in cols
    last0 = (ntile - 1) * TILE
    cols.update((last0 + (V - last0) // 2, last0 + (V - last0) // 2 + 1))
    cols.update(c for c in (3, 4, 15, 16, 63, 64, 79, 80) if c < V)
    return sorted(c for c in cols if 0 <= c < V)


PEAK = 32.0             # the planted logit: > 20 nats above every other logit of its row (the others have a standard deviation of 0.5; the tests assert the gap)


def planted(M, V, K, cols, g, device):
    """rows whose logit at ONE column dominates: the first P = len(cols) <= K - 16 dimensions are "peak dimensions" - W[cols[i]] is PEAK on
    dimension i and 0 elsewhere, every other W row is 0 on the peak dimensions and small random on the rest; row m has a 1 on peak
    dimension m % P, 0 on the other peak dimensions and random values on the rest.  So z[m][cols[m % P]] = PEAK exactly and every other
    logit of the row is a small random number -> (x bf16 [M, K], W bf16 [V, K], peak column per row int64 [M])"""
    P = len(cols)
    assert 1 <= P <= K - 16
    x = torch.zeros(M, K, device=device)
    W = torch.zeros(V, K, device=device)
    W[:, P:] = torch.randn(V, K - P, device=device, generator=g) * (0.5 / math.sqrt(K - P))
    x[:, P:] = torch.randn(M, K - P, device=device, generator=g)
    ct = torch.tensor(cols, device=device)
    W[ct] = 0
    W[ct, torch.arange(P, device=device)] = PEAK
    which = torch.arange(M, device=device) % P
    x[torch.arange(M, device=device), which] = 1.0
    return x.to(torch.bfloat16), W.to(torch.bfloat16), ct[which]


def hf_token_logprobs(logits, labels):
    """transformers' own shift (`ForCausalLMLoss`: labels padded with -100 on the right and shifted left by one, cross entropy with
    ignore_index = -100, here per token): logits [B, T, V] fp64, labels [B, T] -> log-probs [B, T] indexed by the PREDICTED token (0 at
    t = 0 and at ignored labels)"""
    B, T, V = logits.shape
    shift = torch.nn.functional.pad(labels, (0, 1), value=-100)[:, 1:]
    ce = torch.nn.functional.cross_entropy(logits.reshape(B * T, V).double(), shift.reshape(B * T), ignore_index=-100, reduction="none").view(B, T)
    return torch.cat([torch.zeros_like(ce[:, :1]), -ce[:, :-1]], 1)
