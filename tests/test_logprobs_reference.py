"""CPU: pins tests/logprobs_reference.py - the fp64 reference of the log-probabilities op against torch.log_softmax / torch.topk on rows of
distinct values, its ordering rules by hand (ties, -inf, +-0, n = 0, n = V), and the error bound (it covers an fp32 evaluation, and a
dropped term breaks it).  No device is touched."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprobs_reference as LR  # noqa: E402

NINF = float("-inf")


def _distinct(B, V, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    grid = torch.linspace(-3 * scale, 3 * scale, V)              # distinct by construction, every row in an order of its own
    x = torch.stack([grid[torch.randperm(V, generator=g)] for _ in range(B)])
    assert all(x[b].unique().numel() == V for b in range(B))
    return x


def test_distinct_rows_are_log_softmax_and_topk():
    for B, V, n in ((1, 17, 5), (3, 257, 16), (5, 4096, 16), (2, 1001, 1)):
        x = _distinct(B, V, seed=V)
        ids = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(1))
        tok, top, top_lp = LR.logprobs_reference(x, ids, n)
        ls = torch.log_softmax(x.double(), dim=1)
        tk = torch.topk(x, n, dim=1)
        assert tok.dtype == torch.float64 and top.dtype == torch.long and top_lp.dtype == torch.float64
        assert torch.allclose(tok, ls.gather(1, ids[:, None])[:, 0], rtol=0, atol=1e-12)
        assert torch.equal(top, tk.indices) and torch.allclose(top_lp, ls.gather(1, tk.indices), rtol=0, atol=1e-12)
        assert bool((top_lp[:, :-1] >= top_lp[:, 1:]).all())
        assert torch.allclose(torch.exp(ls).sum(1), torch.ones(B, dtype=torch.float64), atol=1e-12)


def test_ties_go_to_the_lowest_ids():
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, 2.0, 0.5]])
    tok, top, top_lp = LR.logprobs_reference(x, torch.tensor([4]), 6)
    assert top.tolist() == [[1, 2, 4, 3, 5, 0]]
    lse = math.log(3 * math.exp(3) + 2 * math.exp(2) + math.exp(1) + math.exp(0.5))
    assert abs(tok.item() - (3 - lse)) < 1e-12
    assert torch.allclose(top_lp[0], torch.tensor([3 - lse] * 3 + [2 - lse] * 2 + [1 - lse], dtype=torch.float64), atol=1e-12)
    # a whole row of one value: ids 0 .. n - 1, each log(1 / V)
    tok, top, top_lp = LR.logprobs_reference(torch.full((2, 9), -7.25), torch.tensor([8, 0]), 9)
    assert top.tolist() == [list(range(9))] * 2 and torch.allclose(top_lp, torch.full((2, 9), -math.log(9), dtype=torch.float64), atol=1e-12)
    assert torch.allclose(tok, torch.full((2,), -math.log(9), dtype=torch.float64), atol=1e-12)


def test_minus_inf_contributes_nothing_and_ranks_last():
    x = torch.tensor([[NINF, 0.0, NINF, 1.0, NINF]])
    tok, top, top_lp = LR.logprobs_reference(x, torch.tensor([0]), 5)
    lse = math.log(1 + math.e)
    assert tok.item() == NINF and not torch.isnan(top_lp).any()
    assert top.tolist() == [[3, 1, 0, 2, 4]]                     # the finite ones, then the -inf entries by ascending id
    assert abs(top_lp[0, 0].item() - (1 - lse)) < 1e-12 and abs(top_lp[0, 1].item() + lse) < 1e-12 and top_lp[0, 2:].tolist() == [NINF] * 3
    # one finite logit: probability 1
    tok, top, top_lp = LR.logprobs_reference(torch.tensor([[NINF, NINF, -3.0]]), torch.tensor([2]), 2)
    assert tok.item() == 0.0 and top.tolist() == [[2, 0]] and top_lp.tolist() == [[0.0, NINF]]


def test_signed_zeros_are_equal():
    x = torch.tensor([[0.0, -0.0, -1.0, -0.0, 0.0, 1e-45]])
    _, top, top_lp = LR.logprobs_reference(x, torch.tensor([1]), 6)
    assert top.tolist() == [[5, 0, 1, 3, 4, 2]]                  # the denormal is above both zeros; the zeros by id
    assert top_lp[0, 1] == top_lp[0, 2] == top_lp[0, 3] == top_lp[0, 4]
    k = LR.order_key(torch.tensor([NINF, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, float("inf")]))
    assert k[3] == k[4] and bool((k[:3][1:] > k[:3][:-1]).all()) and k[2] < k[3] and bool((k[4:][1:] > k[4:][:-1]).all())


def test_n_zero_and_n_equal_v():
    x = _distinct(3, 17, seed=5)
    ids = torch.tensor([0, 16, 7])
    tok0, top0, lp0 = LR.logprobs_reference(x, ids, 0)
    assert top0.shape == (3, 0) and lp0.shape == (3, 0) and top0.dtype == torch.long
    tok, top, lp = LR.logprobs_reference(x, ids, 17)
    assert torch.equal(tok, tok0)
    assert torch.equal(top, torch.argsort(x, dim=1, descending=True))
    assert torch.allclose(torch.exp(lp).sum(1), torch.ones(3, dtype=torch.float64), atol=1e-12)      # the whole distribution
    tok1, top1, lp1 = LR.logprobs_reference(torch.tensor([[2.5]]), torch.tensor([0]), 1)              # V = 1
    assert tok1.item() == 0.0 and top1.tolist() == [[0]] and lp1.tolist() == [[0.0]]


def test_the_slices_are_the_kernels():
    assert [LR.slices(V) for V in (1, 2048, 2049, 4096, 4097, 131071, 131072, 151936, 152064)] == [1, 1, 2, 2, 3, 64, 64, 64, 64]


def test_the_bound_covers_fp32_and_is_not_vacuous():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 4096, generator=g) * torch.tensor([[0.05], [1.0], [5.0], [20.0]])
    ids = torch.tensor([0, 4095, 17, 2048])
    tok, top, top_lp = LR.logprobs_reference(x, ids, 16)
    ls32 = torch.log_softmax(x, dim=1)                           # an fp32 evaluation, in torch's order
    got_tok, got_top = ls32.gather(1, ids[:, None])[:, 0], ls32.gather(1, top)
    assert LR.check_against(x, ids, 16, got_tok, top, got_top) <= 1.0
    b = LR.logprob_bound(x, x.gather(1, top))
    assert b.shape == (4, 16) and float(b.max()) < 2e-5          # a few fp32 roundings of values up to ~100, not a tolerance
    # dropping one term of average size from Z moves every log-probability of the flat row (0.05) by ~1 / V: outside the bound
    assert 1.0 / 4096 > 10 * float(LR.logprob_bound(x[:1], x[:1, :1]).max())
    # a -inf value has bound 0
    y = x.clone()
    y[0, 3] = NINF
    assert float(LR.logprob_bound(y, y[:, 3:4])[0, 0]) == 0.0 and not torch.isnan(LR.logprob_bound(y, y[:, :8])).any()
