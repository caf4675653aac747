"""TEST INFRASTRUCTURE ONLY - the fp64 reference of classifier-free guidance (include/fvhd.h "LLM classifier-free guidance") on fp32
inputs, and the error bound of the kernel's fp32 arithmetic (csrc/llm_guidance.hip).  Plain torch, no GPU.  PINNING:
tests/test_guidance_reference.py.

    logits fp32 [2 G, V]: row g the conditional sequence, row G + g the unconditional one; s the scale AS THE fp32 VALUE the library is given
    lc = log_softmax(x[g])   lu = log_softmax(x[G + g])   guided[g][v] = s * (lc[v] - lu[v]) + lu[v]        (fp64)

The kernel, in this order, every operation rounded once (no fused multiply-add):

    lc~ = (xc - Mc) - log Zc     lu~ = (xu - Mu) - log Zu     d~ = lc~ - lu~     p~ = s * d~     guided~ = p~ + lu~

with (M, log Z) of a row from the statistics launch, whose slices, chains and merge are those of the log-probabilities launch
(csrc/llm_logprobs.hip): S = min(64, ceil(V / 2048)) slices of L = ceil(V / S) elements, a thread adds ceil(L / 256) of them, a butterfly
over the 256 threads, a butterfly over the slices.  So |lc~ - lc| <= e_c and |lu~ - lu| <= e_u with e = `logprobs_reference.logprob_bound`
of the row and the value - the derivation there applies term for term - and

    |guided~ - guided| <= (1 + 2^-10) ( P + R1 + R2 + R3 )
      P  = |s| (e_c + e_u) + e_u                      the two log-softmax errors through s (lc - lu) + lu
      D  = |lc - lu| + e_c + e_u                      the largest |d~|
      R1 = |s| U D                                     the rounding of d~, scaled by s
      R2 = |s| U D                                     the rounding of the product
      R3 = U (|guided| + P + R1 + R2)                  the rounding of the sum
      1 + 2^-10                                        the products of these first-order terms
U = 2^-24.  Nothing here is measured."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprobs_reference as LR  # noqa: E402

U = LR.U
MAX_PROMPTS = 32               # G of one step (2 G <= 64 rows)


def slices(V: int) -> int:
    """the statistics launch's slices per row (csrc/llm_guidance.hip): those of the log-probabilities launch"""
    return LR.slices(V)


def apply_slices(V: int) -> int:
    """workgroups per pair of the apply launch: slices of 2048 ids"""
    return (V + 2047) // 2048


def fp32_scale(s) -> float:
    """the scale as the fp32 value the library receives"""
    return float(np.float32(s))


def log_softmax64(x32: torch.Tensor) -> torch.Tensor:
    x = x32.detach().float().cpu().double()
    M = x.max(-1, keepdim=True).values
    return x - (M + torch.log(torch.exp(x - M).sum(-1, keepdim=True)))


class Reference:
    """the log-softmax rows and their bounds of one logits [2 G, V], computed once and shared by the checks of every scale"""

    def __init__(self, logits: torch.Tensor):
        x = logits.detach().float().cpu()
        assert x.dim() == 2 and x.shape[0] % 2 == 0 and bool(torch.isfinite(x).all())
        G = x.shape[0] // 2
        self.lc, self.lu = log_softmax64(x[:G]), log_softmax64(x[G:])
        self.e_c, self.e_u = LR.logprob_bound(x[:G], x[:G]), LR.logprob_bound(x[G:], x[G:])

    def guided(self, s) -> torch.Tensor:
        return fp32_scale(s) * (self.lc - self.lu) + self.lu

    def bound(self, s) -> torch.Tensor:
        a = abs(fp32_scale(s))
        P = a * (self.e_c + self.e_u) + self.e_u
        D = (self.lc - self.lu).abs() + self.e_c + self.e_u
        R1 = a * U * D
        R2 = a * U * D
        R3 = U * (self.guided(s).abs() + P + R1 + R2)
        return (1 + 2.0 ** -10) * (P + R1 + R2 + R3)

    def check(self, s, got: torch.Tensor, what: str = "") -> float:
        """got [G, V] (any device, fp32 or fp64) under the bound, element-wise -> the largest |err| / bound"""
        want, bound = self.guided(s), self.bound(s)
        got = got.detach().cpu().double()
        assert got.shape == want.shape, (what, got.shape, want.shape)
        assert bool(torch.isfinite(got).all()), f"{what}: non-finite guided score"
        err = (got - want).abs()
        ratio = float((err / bound).max())
        assert bool((err <= bound).all()), f"{what}: max |err| / bound = {ratio:.3g}"
        return ratio


def guided_reference(logits: torch.Tensor, s) -> torch.Tensor:
    """logits fp32 [2 G, V] (finite) -> guided fp64 [G, V] on the CPU"""
    return Reference(logits).guided(s)


def guided_bound(logits: torch.Tensor, s) -> torch.Tensor:
    """|kernel - guided_reference| <= this, element-wise: fp64 [G, V] (the derivation in the module docstring)"""
    return Reference(logits).bound(s)


def check(logits: torch.Tensor, s, got: torch.Tensor, what: str = "") -> float:
    """one check of one scale (`Reference.check`)"""
    return Reference(logits).check(s, got, what)


def pair_batch(embeds, mask, neg_embeds, neg_mask):
    """the 2 G-row batch of a guided run, on the CPU or any device: both halves left-padded to the longer length, rows [0, G) the prompts and
    rows [G, 2 G) the negative prompts -> (embeds [2 G, T, H], mask [2 G, T]).  The library's own construction is
    `ml_fastvlm_amd.qwen2_decode.guidance_batch`; this is its independent restatement for the tests."""
    G, Tc, H = embeds.shape
    Tu = neg_embeds.shape[1]
    T = max(Tc, Tu)
    e = embeds.new_zeros((2 * G, T, H))
    m = mask.new_zeros((2 * G, T))
    e[:G, T - Tc:], m[:G, T - Tc:] = embeds, mask
    e[G:, T - Tu:], m[G:, T - Tu:] = neg_embeds, neg_mask
    return e, m
