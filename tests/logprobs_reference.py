"""TEST INFRASTRUCTURE ONLY - the fp64 reference of the log-probabilities op (include/fvhd.h "LLM log-probabilities") with its exact
ordering rules, and the error bound of the kernel's fp32 arithmetic.  Plain torch, no GPU.  PINNING: tests/test_logprobs_reference.py.

    token_logprob[b] = x[b][id[b]] - lse[b],  lse = M + log sum_v exp(x[v] - M),  M = max x       (fp64 on the fp32 inputs)
    top_ids[b][0 .. n): descending x; equal values by ascending id; -0 == +0; -inf entries last (ascending id among themselves)
    a -inf logit: contributes 0, log-probability -inf
"""

import torch

U = 2.0 ** -24                 # unit roundoff of fp32: one rounded +, -, * is within U relative
ULP1 = 2.0 ** -23              # expf / logf of the device library: at most 1 ulp (HIP math API), i.e. within 2^-23 relative


def order_key(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> int64 keys with a > b <=> key(a) > key(b) and key(-0) == key(+0) (NaN excluded)"""
    x = x.float().contiguous()
    bits = x.view(torch.int32).long() & 0xFFFFFFFF
    bits = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
    neg = (bits & 0x80000000) != 0
    return torch.where(neg, 0xFFFFFFFF - bits, bits | 0x80000000)


def top_order(x: torch.Tensor, n: int) -> torch.Tensor:
    """the first n ids of every row of x [B, V] in the op's order (a stable descending sort of the keys keeps equal values by ascending id)"""
    B = x.shape[0]
    if n == 0:
        return torch.zeros((B, 0), dtype=torch.long)
    return torch.sort(order_key(x.cpu()), dim=1, descending=True, stable=True).indices[:, :n].contiguous()


def logprobs_reference(logits: torch.Tensor, ids: torch.Tensor, n: int):
    """logits fp32 [B, V], ids int64 [B], n in [0, V] -> (token_logprob fp64 [B], top_ids int64 [B, n], top_logprobs fp64 [B, n]) on the CPU"""
    x32 = logits.detach().float().cpu()
    ids = ids.detach().cpu().long()
    B, V = x32.shape
    assert 0 <= n <= V
    x = x32.double()
    M = x.max(1, keepdim=True).values
    lse = M + torch.log(torch.exp(x - M).sum(1, keepdim=True))
    lp = x - lse                                                  # -inf - finite = -inf
    top = top_order(x32, n)
    return lp.gather(1, ids[:, None])[:, 0], top, lp.gather(1, top)


def slices(V: int) -> int:
    """the kernel's slices per row (csrc/llm_logprobs.hip)"""
    return 64 if V >= 64 * 2048 else (V + 2047) // 2048


def logprob_bound(logits: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """|kernel - fp64| <= this, for the log-probability of the logit `values` [B, ...] (fp32 values of row b) under row b of logits [B, V]:

        bound = (1 + 2^-10) * ( d U  +  W U + 2 E + C U  +  E |log Z|  +  U |d + log Z| )

      d = M - value                       the kernel rounds (value - M) once
      W = sum_v t_v (M - x_v) / Z         t_v = exp(x_v - M), Z = sum t_v: a term's exponent is rounded once in its slice (x_v - m_s) and once in
                                          the merge (m_s - M); |x_v - m_s| + |m_s - M| = M - x_v, and an error e of an exponent is a relative error e
                                          of the term - weighted by the term's share of Z
      2 E                                 the two expf (slice, merge), 1 ulp each, E = 2^-23
      C = ceil(L / 256) + 14              roundings along the longest chain into Z: a thread adds ceil(L / 256) elements of its slice of
                                          L = ceil(V / S) (- 1 additions), 6 + 2 additions of the butterfly over 256 threads, the product
                                          sum_s * exp(m_s - M), 6 additions of the butterfly over the slices; the terms are >= 0, so each
                                          rounding is at most U relative to Z
      E |log Z|                           logf, 1 ulp; a relative error r of Z is an absolute error r of log Z (above)
      U |d + log Z|                       the final subtraction (value - M) - log Z
      1 + 2^-10                           the products of these first-order terms
    U = 2^-24.  A -inf value: the bound is 0 (the result must be -inf exactly)."""
    x = logits.detach().cpu().double()
    v = values.detach().cpu().double()
    B, V = x.shape
    M = x.max(1, keepdim=True).values
    t = torch.exp(x - M)
    Z = t.sum(1, keepdim=True)
    gap = torch.where(torch.isfinite(x), M - x, torch.zeros_like(x))
    W = (t * gap).sum(1, keepdim=True) / Z
    S = slices(V)
    L = (V + S - 1) // S
    C = (L + 255) // 256 + 14
    logZ = torch.log(Z)
    shape = (B,) + (1,) * (v.dim() - 1)
    W, logZ = W.reshape(shape), logZ.reshape(shape)
    d = M.reshape(shape) - v
    fin = torch.isfinite(v)
    d = torch.where(fin, d, torch.zeros_like(d))
    bound = (1 + 2.0 ** -10) * (d * U + W * U + 2 * ULP1 + C * U + ULP1 * logZ.abs() + U * (d + logZ).abs())
    return torch.where(fin, bound, torch.zeros_like(bound))


class Reference:
    """the reference and the bound of one (logits, ids), computed once for n_max and shared by the checks of every n <= n_max (the first n
    of the n_max ids are the n ids)"""

    def __init__(self, logits, ids, n_max):
        self.x = logits.detach().float().cpu()
        self.ids = ids.detach().cpu().long()
        self.n_max = n_max
        self.tok, self.top, self.top_lp = logprobs_reference(self.x, self.ids, n_max)
        self.tok_bound = logprob_bound(self.x, self.x.gather(1, self.ids[:, None])[:, 0])
        self.top_bound = logprob_bound(self.x, self.x.gather(1, self.top))

    def check(self, n, token_lp, top_ids, top_lp, what=""):
        """the op's outputs (any device) for n: ids exact, log-probabilities within the bound (-inf exact) -> the largest |err| / bound"""
        assert 0 <= n <= self.n_max
        worst = 0.0
        pairs = [(token_lp, self.tok, self.tok_bound, "token_logprob")]
        if n:
            assert torch.equal(top_ids.detach().cpu(), self.top[:, :n]), f"{what}: top_ids differ from the reference"
            pairs.append((top_lp, self.top_lp[:, :n], self.top_bound[:, :n], "top_logprobs"))
        for got, want, bound, name in pairs:
            got = got.detach().cpu().double()
            assert got.shape == want.shape, (what, name, got.shape, want.shape)
            fin = torch.isfinite(want)
            assert bool((got[~fin] == want[~fin]).all()), f"{what} {name}: a -inf entry is not -inf"
            assert bool(torch.isfinite(got[fin]).all()), f"{what} {name}: non-finite where the reference is finite"
            err = (got[fin] - want[fin]).abs()
            if err.numel():
                ratio = float((err / bound[fin]).max())
                worst = max(worst, ratio)
                assert bool((err <= bound[fin]).all()), f"{what} {name}: max |err| / bound = {ratio:.3g}"
        return worst


def check_against(logits, ids, n, token_lp, top_ids, top_lp, what=""):
    """one check of one n (`Reference.check`)"""
    return Reference(logits, ids, n).check(n, token_lp, top_ids, top_lp, what)
