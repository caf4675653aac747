"""TEST INFRASTRUCTURE ONLY - plain torch fp64 restatements of the vision tower's single operations (csrc/gemm.hip - with the two
epilogues the Qwen2 prefill adds to the same kernel family -, ffn_fused.hip, attention.hip, stem_head.hip, dwconv*.hip) on the bf16-rounded operands, written from oracle/fastvithd_oracle.py and the arithmetic
include/fvhd.h documents, not from the kernels; the per-element bounds of tests/test_gpu_tower_ops.py; the seeded input families of
those tests; and CPU models of the arithmetic a kernel is ALLOWED (bf16 operands, fp32 accumulation over the K tiles in order, the
polynomial GELUs, bf16 P over 64-key tiles with the online rescale, ONE rounding to the output type) that only serve to show that the
families leave room under their bound and that a planted fault does not.  The comparison / sentinel-guard helpers are those of
tests/llm_testlib.py.  Importing this module needs no GPU.

BOUNDS (per element; every rms is per row; nothing is pooled and no element is exempt).  u(T) is TWICE the worst case of one rounding
to T - 2^-7 bf16, 2^-10 f16 (+ 2^-24 absolute: its subnormal step), 2^-22 f32 - as the prefill tests state it:
  GEMM             |err| <= u(T) |want| + C_ACC f S (+ GELU7_ABS),  S = |A| @ |W|^T;  f = 1, |ls_n| (EPI_BIAS_LS_RESID) or GELU_SLOPE = 1.13
                   (EPI_BIAS_GELU: the accumulation error passes through the GELU, max |gelu'| = 1.129)
                   EPI_RESID (Qwen2 prefill: o_proj, down_proj): the form of EPI_BIAS_LS_RESID with ls = 1 and no bias
  GEMM, SwiGLU     |err| <= u(bf16) |want| + C_ACC (SILU_SLOPE S_gate |up| + |silu(gate)| S_up) + sig_rel(gate) |want|, want = silu(gate) up
                   [M, N / 2]; S_gate, S_up the |A| @ |W|^T sums of the two columns; SILU_SLOPE = 1.1 (max |silu'| = 1.0998); sig_rel(g) =
                   2^-20 + 2^-24 |g|, the fast sigmoid's fp32 chain (derived at sig_rel; four orders of magnitude below u)
  fused FFN        2^-7 |want| + |ls_n| sum_h ((e_phi |pre_mh| + u_hid |hid_mh|) + C_ACC (1.13 S1_mh + |hid_mh|)) |W2_nh|,  S1 = |A| @ |W1|^T
                   e_phi: 1.4e-3 (FFN_HALF, include/fvhd.h) / 2.33e-4 (FFN_BF16, csrc/fvhd_common.h);  u_hid: 2^-11 (f16) / 2^-8 (bf16)
  attention        2e-2 |want| + 2e-2 rms(row), a row = one (image, query, head) vector of 32 values: the project's budget
  layernorm        2^-7 |want| + C_LN (|x_c| + |mean|) rstd |w_c|
  SE head          u(T) |want| + GELU7_ABS + 1.13 (2^-22 + sqrt(T + C + RD) 2^-25 S_arg) |y|,  S_arg = |we| (|wr| mean|y| + |br|) + |be|: see se_head_bound
  depthwise        2^-7 |want| + (K K + 1) 2^-24 f (|x| * |w| + |b|) (+ GELU7_ABS), * = the same convolution: the worst case of K K + 1 fp32 terms

MEASURED (tests/test_tower_reference.py prints them; `python -m pytest tests/test_tower_reference.py -s`), over every family and every
(N, K) class the GPU tests use:
  GEMM, K = 32 .. 3136, fp32 sums of 32-wide K slabs in order: worst |acc32 - acc64| / S = 8.8e-8 -> C_ACC = 2^-22 = 2.4e-7 (2.7 times
        that); the whole model, rounded once, sits at 0.498 (bf16), 0.496 (f16), 0.26 (f32) of the bound; EPI_RESID 0.498, EPI_SWIGLU
        0.497 ("rc") and 0.494 (the integer pairing family, where it is also within one bf16 ulp element by element)
  layernorm, C = 4 .. 2048, two-pass fp32 statistics: worst error before the rounding / ((|x| + |mean|) rstd |w|) = 3.7e-7 (the
        large-mean family) -> C_LN = 2^-20 = 9.5e-7; the model sits at 0.498 of the bound
  fused FFN model 0.26 (FFN_HALF) / 0.19 (FFN_BF16); attention model 0.41 (qscale) and below; depthwise 0.497; SE head <= 0.5
  the polynomial GELUs against erf in fp64: degree 7 |Phi error| 3.304e-5, |gelu error| 1.320e-4 - csrc/fvhd_common.h said 3.3e-5 /
        1.3e-4, figures rounded DOWN to two digits: a finding, corrected there to 3.31e-5 / 1.33e-4; degree 5 2.330e-4 / 8.14e-4
        (documented 2.33e-4 / 8.2e-4); FFN_HALF 1.380e-3 (documented 1.4e-3).  A documented GELU error is the error of THAT polynomial,
        attained near x = -3: a model that evaluates the polynomial reaches 0.94 of a bound with a GELU term, by definition.  The margin
        of two is therefore shown with the exact GELU in the model (0.49), and the polynomial model only has to stay inside.
PINNING: tests/test_tower_reference.py checks every *_ref against oracle.fastvithd_oracle in fp32, every model against half its bound on
every family, and that the bound rejects ten planted faults (nine of them; the tenth provably cannot be seen in a bf16 output); for the
prefill's two epilogues (tests/test_gpu_prefill_gemm_ops.py) gemm_ref against transformers' Qwen2MLP in fp64, the model on both families,
and four more faults (gate / up swapped, gate j with up j + 1, the residual of the neighbouring 8 columns, a residual dropped on 16
columns), each rejected by the "rc" bound AND by the exact family."""
from __future__ import annotations

import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from ml_fastvlm_amd import _lib

# the comparison, the guards and the plumbing are those of the Qwen2 tests: re-exported for this module's users
from llm_testlib import SENT, check, close, close_pooled, guard_intact, guarded, ptr, row_scales, same_bits, stream, violations  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_LS_RESID = _lib.EPI_NONE, _lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_BIAS_LS_RESID
EPI_RESID, EPI_SWIGLU = _lib.EPI_RESID, _lib.EPI_SWIGLU          # the Qwen2 prefill's epilogues of the same kernel family

U = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -22}     # twice the worst case of one rounding
U_ABS = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24, torch.float32: 0.0}                # ... of a SUBNORMAL result (f16 below 6.1e-5: steps of 2^-24)
C_ACC = 2.0 ** -22             # fp32 accumulation, as a fraction of S (measured: see the docstring)
C_LN = 2.0 ** -20              # layernorm's fp32 statistics, as a fraction of (|x| + |mean|) rstd |w|
GELU_SLOPE = 1.13              # max |gelu'(x)| = 1.129 (at x = 1.41)
SILU_SLOPE = 1.1               # max |silu'(x)| = 1.0998 (at x = 2.4)
GELU7_ABS, PHI7 = 1.33e-4, 3.31e-5     # csrc/fvhd_common.h: the degree-7 fit every kernel but the fused FFN evaluates
GELU5_ABS, PHI5 = 8.2e-4, 2.33e-4     # csrc/fvhd_common.h: the degree-5 fit of the fused FFN's FFN_BF16 form
PHI_HALF = 1.4e-3                      # include/fvhd.h: |Phi error| of the FFN_HALF form
ATT_RTOL = ATT_RMS = 2e-2
KT = 64                        # key tile of attention_kernel
HD = 32                        # head_dim of the tower


def within(got, want, bound, what=""):
    """every element: |got - want| <= bound (a tensor of want's shape) -> (elements outside, worst err / bound)"""
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    got, want = got.double(), want.double()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - want).abs()
    ratio = torch.where(err > 0, err / bound.double().clamp_min(1e-300), torch.zeros_like(err))
    return int((err > bound).sum()), float(ratio.max()) if ratio.numel() else 0.0


def inside(got, want, bound, what):
    bad, worst = within(got, want, bound, what)
    assert bad == 0, f"{what}: {bad} of {want.numel()} elements outside the bound, worst err / bound {worst:.3g}"
    return worst


# ---- the GELUs --------------------------------------------------------------------------------------------------------------------------
def gelu64(x):
    """the erf GELU of the reference (nn.GELU() default) in fp64"""
    x = x.double()
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _poly(prefix, n):
    src = open(os.path.join(ROOT, "ml_fastvlm_amd", "csrc", "fvhd_common.h")).read()
    clamp = float(re.search(rf"#define {prefix}_CLAMP\s+([0-9.eE+-]+)f", src).group(1))
    return clamp, [float(re.search(rf"#define {prefix}_C{i}\s+([0-9.eE+-]+)f", src).group(1)) for i in range(n)]


def gelu_poly(x, degree=7):
    """gelu_erf of csrc/fvhd_common.h in fp32 with the header's own coefficients: Phi = 0.5 + xc Q(xc^2) -> (gelu, Phi)"""
    clamp, c = _poly("FVHD_GELU" if degree == 7 else "FVHD_GELU5", degree + 1)
    x = x.float()
    xc = x.clamp(-clamp, clamp)
    u = xc * xc
    q = torch.full_like(x, c[-1])
    for ck in reversed(c[:-1]):
        q = q * u + ck
    phi = xc * q + 0.5
    return x * phi, phi


def poly_contract(pre, acc_bound, dtype=torch.bfloat16):
    """where a kernel applies the degree-7 GELU, its output must ALSO be the documented polynomial of the fp64 pre-activation - without
    the GELU7_ABS allowance: -> (want, bound) = (x Phi7(x) in fp64, u(T) |want| + 1.13 acc_bound + |x| e_eval), acc_bound the error
    allowed on the pre-activation and e_eval the fp32 evaluation of Phi = 0.5 + xc Q(xc^2): Horner's worst case, 14 roundings of
    2^-24 on sum |c_k| u^k (the alternating terms reach 5 at |x| = 4, where Phi itself is ~1e-6), times |xc|, plus 2^-23 for the sum"""
    clamp, c = _poly("FVHD_GELU", 8)
    x = pre.double()
    xc = x.clamp(-clamp, clamp)
    u = xc * xc
    q, cond = torch.full_like(x, c[-1]), torch.full_like(x, abs(c[-1]))
    for ck in reversed(c[:-1]):
        q, cond = q * u + ck, cond * u + abs(ck)
    want = x * (xc * q + 0.5)
    e_eval = xc.abs() * 14 * 2.0 ** -24 * cond + 2.0 ** -23
    return want, U[dtype] * want.abs() + GELU_SLOPE * acc_bound + x.abs() * e_eval


def _half_constants():
    """gelu16_stage's constants, parsed from csrc/ffn_fused.hip in order of appearance: UMAX, c5 .. c0, 0.5"""
    src = open(os.path.join(ROOT, "ml_fastvlm_amd", "csrc", "ffn_fused.hip")).read()
    body = src[src.index("void gelu16_stage("):src.index("void gelu16_dispatch(")]
    bits = [int(b, 16) for b in re.findall(r"FFN_H2\(0x([0-9a-fA-F]{4})\)", body)]
    assert len(bits) == 8, bits
    vals = [np.array([b], dtype=np.uint16).view(np.float16)[0] for b in bits]
    return vals[0], vals[1:7], vals[7]


def _fma16(a, b, c):       # one rounding, like v_pk_fma_f16 (the product of two halves is exact in float64)
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float16)


def _rtz16(x):             # v_cvt_pkrtz_f16_f32: round toward zero, i.e. saturating at the largest finite half
    h = np.float16
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        y = x.astype(h)
    y = np.where(np.isinf(y), np.sign(x).astype(h) * h(65504), y).astype(h)
    too_big = np.abs(y.astype(np.float32)) > np.abs(x)
    return np.where(too_big, np.nextafter(y, h(0)), y).astype(h)


def gelu_half16(x_over_4):
    """x' = x / 4 (what the fused FFN's first GEMM delivers) -> (y' = gelu(x) / 4 as half, Phi as half): the instruction sequence of
    the FFN_HALF form, in numpy float16 with the kernel's own coefficient bit patterns"""
    h = np.float16
    umax, (c5, c4, c3, c2, c1, c0), half = _half_constants()
    x = _rtz16(x_over_4)
    u = np.minimum((x.astype(np.float64) ** 2).astype(h), umax)
    q = _fma16(np.full_like(u, c5), u, np.full_like(u, c4))
    for c in (c3, c2, c1, c0):
        q = _fma16(q, u, np.full_like(u, c))
    phi = np.clip(_fma16(x, q, np.full_like(u, half)).astype(np.float32), 0.0, 1.0).astype(h)      # the clamp modifier
    with np.errstate(over="ignore"):
        y = (x.astype(np.float32) * phi.astype(np.float32)).astype(h)
    return y, phi


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------------
def gemm_ref(A, W, bias=None, ls=None, resid=None, epi=EPI_NONE):
    """fvhd_op_gemm in fp64 on the operands as given (bf16 A, W, resid; fp32 bias, ls) -> (want, S = |A| @ |W|^T [M, N]); want is
    [M, N], for EPI_SWIGLU [M, N / 2]: silu(A.W^T[:, 2j]) * A.W^T[:, 2j + 1], the rows of W interleaved gate_j, up_j"""
    a, w = A.double(), W.double()
    y, S = a @ w.t(), a.abs() @ w.abs().t()
    if epi == EPI_SWIGLU:
        return F.silu(y[:, 0::2]) * y[:, 1::2], S
    if epi == EPI_RESID:
        return resid.double() + y, S
    if epi != EPI_NONE:
        y = y + bias.double()
    if epi == EPI_BIAS_GELU:
        y = gelu64(y)
    if epi == EPI_BIAS_LS_RESID:
        y = resid.double() + ls.double() * y
    return y, S


def sig_rel(gate):
    """relative error allowed to x * sigmoidf_fast(x) * up of csrc/fvhd_common.h, rcp(1 + exp2(x * -log2(e))) in fp32, as a function of
    the gate pre-activation: 2^-20 + 2^-24 |g|.  Derivation: the argument t = x * c is one fp32 product, |dt| <= 2^-24 |t| (c itself is
    off by 0.22 * 2^-24), and an absolute dt on exp2's argument is a relative ln 2 * dt on its value: 0.69 * 1.22 * 1.4427 * 2^-24 |g| =
    1.22 * 2^-24 |g| on e = exp(-g), which reaches the sigmoid times e / (1 + e) <= 1.  The terms without |g|: v_exp_f32 and v_rcp_f32
    one ulp each (2^-23; the guides of this project give no other figure for the two), the sum 1 + e (2^-24) and the two products
    x * s * up (2^-24 each): 7 * 2^-24.  2^-20 = 16 * 2^-24 holds those seven and the 0.22 * 2^-24 |g| left over up to |g| = 40; beyond
    that silu's own size, which S_gate >= |g| brings into the accumulation term, is orders of magnitude above either.  sig_rel stays
    four orders of magnitude below u(bf16) = 2^-7: it must never be what makes a comparison pass."""
    return 2.0 ** -20 + 2.0 ** -24 * gate.double().abs()


def gemm_bound(want, S, epi, dtype=torch.bfloat16, ls=None, pre=None):
    """pre: A . W^T in fp64 [M, N], needed by EPI_SWIGLU alone - the error of the gate's sum passes through silu (slope <= SILU_SLOPE)
    and is scaled by |up|, that of the up sum by |silu(gate)|, and the fast sigmoid adds sig_rel(gate) |want|"""
    if epi == EPI_SWIGLU:
        assert dtype == torch.bfloat16
        gate, up = pre[:, 0::2].double(), pre[:, 1::2].double()
        return U[dtype] * want.abs() + C_ACC * (SILU_SLOPE * S[:, 0::2] * up.abs() + F.silu(gate).abs() * S[:, 1::2]) + sig_rel(gate) * want.abs()
    f = ls.double().abs() if epi == EPI_BIAS_LS_RESID else (GELU_SLOPE if epi == EPI_BIAS_GELU else 1.0)
    return U[dtype] * want.abs() + U_ABS[dtype] + C_ACC * f * S + (GELU7_ABS if epi == EPI_BIAS_GELU else 0.0)


def one_ulp(got, want):
    """elements of the bf16 tensor `got` that are neither within one bf16 ulp of the bf16 tensor `want` (a distance of at most one
    between the bit patterns, so the same sign) nor zero where `want` is zero -> their number"""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.bfloat16, (got.shape, want.shape, got.dtype, want.dtype)
    gi, wi = got.contiguous().view(torch.int16).int(), want.contiguous().view(torch.int16).int()
    return int((~(((gi - wi).abs() <= 1) | ((got == 0) & (want == 0)))).sum())


def acc32(A, W, slab=32, fault=None):
    """A @ W^T with fp32 sums of `slab`-wide K slabs added in order (what an MFMA chain over the K tiles does).  fault: "skip_last_k"
    (the last 32-wide K tile is never added), "swap_k8" (A's 8-element K slots 1 and 2 change places in row 0 .. 15 of the first tile)"""
    a, w = A.float(), W.float()
    K = a.shape[1]
    if fault == "swap_k8":
        a = a.clone()
        a[:16, 8:16], a[:16, 16:24] = A.float()[:16, 16:24], A.float()[:16, 8:16]
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, K - (slab if fault == "skip_last_k" else 0), slab):
        acc += a[:, k0:k0 + slab] @ w[:, k0:k0 + slab].t()
    return acc


def sigmoid_fast32(x):
    """sigmoidf_fast of csrc/fvhd_common.h in fp32: 1 / (1 + exp2(x * -log2(e)))"""
    x = x.float()
    return 1.0 / (1.0 + torch.exp2(x * x.new_tensor(-1.4426950408889634)))


def gemm_model(A, W, bias=None, ls=None, resid=None, epi=EPI_NONE, dtype=torch.bfloat16, fault=None, group=0, erf=False):
    """the arithmetic a GEMM kernel is allowed: acc32, the epilogue in fp32 with the degree-7 GELU (erf: the exact one) or the fast
    sigmoid, one rounding.  fault: acc32's, or "bias16" (no bias on the 16-column group `group`), "ls_neighbour" (column n scaled by
    ls[n + 1]); EPI_SWIGLU: "swap_gate_up" (silu of the up column times the gate column), "pair_shift" (gate j with up j + 1 inside every
    group of 16 columns = 8 outputs, cyclically); EPI_RESID: "resid_neighbour8" (the residual of the other 8-column group of the same 16
    columns), "resid_dropped" (no residual on the 16-column group `group`)"""
    t = acc32(A, W, fault=fault)
    if epi == EPI_SWIGLU:
        gate, up = t[:, 0::2], t[:, 1::2]
        if fault == "swap_gate_up":
            gate, up = up, gate
        if fault == "pair_shift":
            up = up.reshape(up.shape[0], -1, 8).roll(-1, 2).reshape(up.shape)
        return (gate * sigmoid_fast32(gate) * up).to(dtype)
    if epi == EPI_RESID:
        r = resid.float().clone()
        if fault == "resid_neighbour8":
            r = r.reshape(r.shape[0], -1, 2, 8).flip(2).reshape(r.shape)
        if fault == "resid_dropped":
            r[:, 16 * group:16 * group + 16] = 0.0
        return (r + t).to(dtype)
    if epi != EPI_NONE:
        b = bias.float().clone()
        if fault == "bias16":
            b[16 * group:16 * group + 16] = 0.0
        t = t + b
    if epi == EPI_BIAS_GELU:
        t = gelu64(t).float() if erf else gelu_poly(t, 7)[0]
    if epi == EPI_BIAS_LS_RESID:
        l = ls.float().roll(-1) if fault == "ls_neighbour" else ls.float()
        t = resid.float() + l * t
    return t.to(dtype)


GATE_NNZ, GATE_MAX = 4, 36      # the pairing family of EPI_SWIGLU: non-zeros of a gate row of W, and the |gate sum| they allow (4 * 3 * 3)


def gemm_family(name, M, N, K, epi, seed, device="cpu"):
    """-> (A [M, K] bf16, W [N, K] bf16, bias fp32 [N] | None, ls fp32 [N] | None, resid bf16 [M, N] | None).
    "exact": integers |a|, |w|, |b| <= 3, ls a power of two, an integer residual - every partial sum stays below 2^24 up to K = 6144, so
      fp32 accumulation is exact in ANY order and the output must be the bits of bf16(fp64 result).  EPI_SWIGLU has no bit-exact form
      (the fast sigmoid): its "exact" is the integer PAIRING family - A and the up rows of W as above, every gate row of W with exactly
      GATE_NNZ non-zeros in +-3, so that |gate sum| <= GATE_MAX = 36 by construction (below the +-60 beyond which the fast sigmoid's
      exp nears the end of its fp32 range: test_dec_gemm_one_hot_exact) and both sums are exact in fp32; the output must then be
      bf16(silu(g) u) to ONE bf16 ulp or zero with it (tower_reference.one_ulp), element by element: the gate / up pairing and the
      [M, N / 2] column map, not an average over them.
    "rc" (rowscale x colscale): the rows of A carry row_scales 0.05 .. 20, the rows of W (= output columns) and ls each span 1e-5 .. 1
      (shuffled independently); bias and residual carry the scale of the term they are added to, so that no term hides another.
      EPI_SWIGLU: the gate rows and the up rows of W draw their column scales independently."""
    g = torch.Generator(device=device).manual_seed(seed)
    has_b, has_ls = epi in (EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_LS_RESID), epi == EPI_BIAS_LS_RESID
    has_r = has_ls or epi == EPI_RESID
    if name == "exact":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, device=device, generator=g).float()
        A, W = ri(-3, 3, M, K), ri(-3, 3, N, K)
        bias = ri(-3, 3, N) if has_b else None
        ls = 2.0 ** ri(-3, 1, N) if has_ls else None
        resid = ri(-8, 8, M, N) if has_r else None
        if epi == EPI_SWIGLU:
            keep = torch.rand(N // 2, K, device=device, generator=g).argsort(1)[:, :GATE_NNZ]          # GATE_NNZ distinct positions per gate row
            vals = ri(1, 3, N // 2, GATE_NNZ) * torch.where(torch.rand(N // 2, GATE_NNZ, device=device, generator=g) < 0.5, -1.0, 1.0)
            W[0::2] = torch.zeros(N // 2, K, device=device).scatter_(1, keep, vals)
            assert int((W[0::2] != 0).sum(1).min()) == int((W[0::2] != 0).sum(1).max()) == GATE_NNZ
            assert float((A.abs() @ W[0::2].abs().t()).max()) <= GATE_MAX
    else:
        assert name == "rc", name
        rn = lambda *s: torch.randn(*s, device=device, generator=g)
        span = lambda n: torch.logspace(-5.0, 0.0, n, device=device)[torch.randperm(n, device=device, generator=g)] if n > 1 else torch.ones(1, device=device)
        rows = row_scales(M, g, device)
        cols = torch.stack([span(N // 2), span(N // 2)], 1).reshape(N) if epi == EPI_SWIGLU else span(N)
        A, W = rn(M, K) * rows[:, None], rn(N, K) * K ** -0.5 * cols[:, None]
        bias = 0.3 * rn(N) * cols if has_b else None
        ls = span(N) if has_ls else None
        resid = rn(M, N) * rows[:, None] * ((ls * cols) if has_ls else cols)[None] if has_r else None
    b16 = lambda t: t.to(torch.bfloat16) if t is not None else None
    return b16(A), b16(W), bias, ls, b16(resid)


# ---- fused ConvFFN --------------------------------------------------------------------------------------------------------------------
def round_hidden(g, precision):
    """what the fused kernel keeps of the hidden activation (include/fvhd.h): f16 of gelu / 4, saturating (FFN_HALF), or bf16 of gelu"""
    if precision == _lib.FFN_HALF:
        return (g / 4.0).float().clamp(-65504.0, 65504.0).half().to(g.dtype) * 4.0
    return g.float().to(torch.bfloat16).to(g.dtype)


def ffn_ref(A, W1, b1, W2, b2, ls, X, precision):
    """X + ls * (hidden . W2^T + b2), hidden = round_hidden(gelu(A . W1^T + b1)) in fp64 -> (want, pre, hid)"""
    pre = A.double() @ W1.double().t() + b1.double()
    hid = round_hidden(gelu64(pre), precision)
    return X.double() + ls.double() * (hid @ W2.double().t() + b2.double()), pre, hid


def ffn_bound(want, pre, hid, A, W1, W2, ls, precision):
    e_phi, u_hid = (PHI_HALF, 2.0 ** -11) if precision == _lib.FFN_HALF else (PHI5, 2.0 ** -8)
    S1 = A.double().abs() @ W1.double().abs().t()
    per_h = e_phi * pre.abs() + u_hid * hid.abs() + C_ACC * (GELU_SLOPE * S1 + hid.abs())
    return 2.0 ** -7 * want.abs() + ls.double().abs() * (per_h @ W2.double().abs().t())


def ffn_model(A, W1, b1, W2, b2, ls, X, precision, fault=None):
    """the arithmetic the fused kernel is allowed: both GEMMs as acc32 (the second over the 32-unit hidden chunks), the polynomial GELU
    of the form, the hidden operand rounded once, the epilogue in fp32, one rounding to bf16.  fault "swap_hidden": hidden units 0 and 1
    change places in front of the second GEMM"""
    pre = acc32(A, W1) + b1.float()
    if precision == _lib.FFN_HALF:
        hid = 4.0 * torch.from_numpy(gelu_half16((pre / 4.0).numpy())[0].astype(np.float32))
    else:
        hid = gelu_poly(pre, 5)[0].to(torch.bfloat16).float()
    if fault == "swap_hidden":
        hid = hid.clone()
        hid[:, [0, 1]] = hid[:, [1, 0]]
    return (X.float() + ls.float() * (acc32(hid, W2) + b2.float())).to(torch.bfloat16)


def ffn_family(M, C, seed, device="cpu"):
    """rowscale: the rows of A carry row_scales 0.05 .. 20, ls spans 1e-5 .. 1 and X carries ls's scale (see gemm_family "rc")
    -> (A [M, C], W1 [4C, C], b1, W2 [C, 4C], b2, ls, X [M, C]); A, W1, W2, X bf16, the rest fp32"""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    rows = row_scales(M, g, device)
    ls = torch.logspace(-5.0, 0.0, C, device=device)[torch.randperm(C, device=device, generator=g)]
    A = rn(M, C) * rows[:, None] * 0.2                     # pre-activations of 0.01 .. 4 standard deviations: both GELU tails and the middle
    W1, W2 = rn(4 * C, C) * C ** -0.5, rn(C, 4 * C) * (4 * C) ** -0.5
    b1, b2 = 0.2 * rn(4 * C), 0.2 * rn(C)
    X = rn(M, C) * rows[:, None] * ls[None] * 0.2
    return A.to(torch.bfloat16), W1.to(torch.bfloat16), b1, W2.to(torch.bfloat16), b2, ls, X.to(torch.bfloat16)


# ---- attention ----------------------------------------------------------------------------------------------------------------------------
def split_qkv(qkv, B, N, C):
    """[B*N, 3C] -> q, k, v [B, nh, N, 32]"""
    return qkv.reshape(B, N, 3, C // HD, HD).permute(2, 0, 3, 1, 4).unbind(0)


def attention_ref(qkv, B, N, C):
    """the core of oracle.fastvithd_oracle.mhsa in fp64: softmax((q * 32^-0.5) k^T) v -> [B*N, C]"""
    q, k, v = split_qkv(qkv.double(), B, N, C)
    a = ((q * HD ** -0.5) @ k.transpose(-2, -1)).softmax(-1)
    return (a @ v).transpose(1, 2).reshape(B * N, C)


def attention_model(qkv, B, N, C, fault=None):
    """the arithmetic attention_kernel is allowed: 64-key tiles, fp32 scores, a running maximum with the rescale of the accumulators,
    P = exp2 rounded to bf16, the denominator summed from the ROUNDED P, fp32 accumulation, one rounding of O / l to bf16.
    fault: "unmasked" (the first key past N of the ragged tile - a clamped load, i.e. key N - 1 again - is not masked), "skip_64" (the
    first key of the second tile is never seen), "l_unrounded" (the denominator summed before the rounding of P)"""
    q, k, v = (t.float() for t in split_qkv(qkv, B, N, C))
    c = HD ** -0.5 * 1.4426950408889634
    m = torch.full(q.shape[:3], -1e30)
    l = torch.zeros(q.shape[:3])
    o = torch.zeros(q.shape)
    for t0 in range(0, N, KT):
        t1 = min(N, t0 + KT)
        kt, vt = k[:, :, t0:t1], v[:, :, t0:t1]
        if fault == "unmasked" and t1 == N and N % KT:
            kt, vt = torch.cat([kt, k[:, :, N - 1:N]], 2), torch.cat([vt, v[:, :, N - 1:N]], 2)
        s = q @ kt.transpose(-1, -2)
        if fault == "skip_64" and t0 == KT:
            s[..., 0] = -1e30
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.exp2((m - m_new) * c)
        p32 = torch.exp2(s * c - (m_new * c)[..., None])
        p = p32.to(torch.bfloat16).float()
        l = l * alpha + (p32 if fault == "l_unrounded" else p).sum(-1)
        o = o * alpha[..., None] + p @ vt
        m = m_new
    return (o / l[..., None]).to(torch.bfloat16).transpose(1, 2).reshape(B * N, C)


def attention_fp8_model(qkv, B, N, C):
    """the fp8 form's arithmetic as include/fvhd.h states it: Q, K, V rounded to OCP e4m3; per 64-key tile the online softmax with an
    fp32 running maximum, P = exp(s - running max) rounded to e4m3 before the PV product AND before the row sum -> [B*N, C] fp32"""
    f8 = lambda t: t.to(torch.float8_e4m3fn).float()
    q, k, v = (f8(t.float().cpu()) for t in split_qkv(qkv, B, N, C))
    scale = HD ** -0.5
    m = torch.full(q.shape[:3] + (1,), -1e30)
    l = torch.zeros(q.shape[:3] + (1,))
    o = torch.zeros(q.shape)
    for k0 in range(0, N, KT):
        s = q @ k[:, :, k0:k0 + KT].transpose(-2, -1)
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp((m - m_new) * scale)
        pr = f8(torch.exp((s - m_new) * scale))
        l = l * alpha + pr.sum(-1, keepdim=True)
        o = o * alpha + pr @ v[:, :, k0:k0 + KT]
        m = m_new
    return (o / l).transpose(1, 2).reshape(B * N, C)


ATT_FAMILIES = ("plain", "qscale", "ascending", "descending", "planted_first", "planted_last", "planted_ragged", "flat", "dominant")


def planted_key(name, N):
    """the winner's key: in the first tile, in the last FULL tile, in the last tile (the ragged one when N % 64 != 0)"""
    full = N // KT
    return {"planted_first": min(5, N - 1), "planted_last": min(max(full - 1, 0) * KT + 33, N - 1), "planted_ragged": N - 1 - (N - 1) % KT // 2,
            "dominant": N // 2}[name]


def attention_family(name, B, N, C, seed, device="cpu"):
    """-> qkv [B*N, 3C] bf16.  "plain": N(0, 1.5) as the first op tests; "qscale": the q rows carry row_scales 0.05 .. 20 (flat to
    one-hot softmax rows side by side), v of distinct scale per head; "ascending" / "descending": 40 logits along the keys (the running
    maximum moves in every tile / never after the first); "planted_*": one key 8 logits above the rest for every query (the others keep
    a visible share); "flat": q = 0, every score equal; "dominant": one key 60 logits above (P of every other key underflows to ~0)"""
    g = torch.Generator(device=device).manual_seed(seed)
    nh = C // HD
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    q, k, v = rn(B, N, nh, HD), rn(B, N, nh, HD), rn(B, N, nh, HD)
    if name == "plain":
        q, k, v = 1.5 * q, 1.5 * k, 1.5 * v
    elif name == "qscale":
        q = q * row_scales(B * N, g, device).view(B, N, 1, 1)
        v = v * (2.0 ** torch.arange(nh, device=device).remainder(5)).view(1, 1, nh, 1) * (1 + torch.arange(N, device=device).remainder(7) / 4.0).view(1, N, 1, 1)
    elif name == "flat":
        q = torch.zeros_like(q)
    else:
        u = torch.where(torch.rand(HD, device=device, generator=g) < 0.5, -1.0, 1.0)
        if name in ("ascending", "descending"):
            ramp = torch.arange(N, device=device, dtype=torch.float32) / max(N, 1)
            k = k + ((1.0 - ramp if name == "descending" else ramp) * 40.0 / math.sqrt(HD)).view(1, N, 1, 1) * u
        else:
            k[:, planted_key(name, N)] += (60.0 if name == "dominant" else 8.0) / math.sqrt(HD) * u
        q = q + u
    return torch.stack([q, k, v], 2).to(torch.bfloat16).reshape(B * N, 3 * C).contiguous()


def attention_violations(got, want, B, N, C):
    """the project's attention budget per (image, query, head) row of 32 values -> (elements outside, worst err / bound)"""
    return violations(got.reshape(B, N, C // HD, HD), want.reshape(B, N, C // HD, HD), ATT_RTOL, ATT_RMS)


# ---- layernorm ----------------------------------------------------------------------------------------------------------------------------
def layernorm_ref(x, w, b, eps=1e-5):
    """LayerNormChannel on NHWC rows x [M, C] in fp64 (biased variance) -> (want, mean [M, 1], rstd [M, 1])"""
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((x - mean).pow(2).mean(-1, keepdim=True) + eps)
    return (x - mean) * rstd * w.double() + b.double(), mean, rstd


def layernorm_bound(want, x, w, mean, rstd):
    return 2.0 ** -7 * want.abs() + C_LN * (x.double().abs() + mean.abs()) * rstd * w.double().abs()


def layernorm_model(x, w, b, eps=1e-5, fault=None):
    """two-pass fp32 statistics, one rounding.  fault "one_pass": the variance as E[x^2] - mean^2 in fp32"""
    x = x.float()
    C = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / C
    var = (x * x).sum(-1, keepdim=True) / C - mean * mean if fault == "one_pass" else (x - mean).pow(2).sum(-1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    return ((x - mean) * rstd * w.float() + b.float()).to(torch.bfloat16)


LN_FAMILIES = ("plain", "bigmean", "const", "wscale")


def layernorm_family(name, M, C, seed, device="cpu"):
    """-> (x [M, C] bf16, w, b fp32 [C]).  "bigmean": a row is m = 255 * 2^(k - 7) (all mantissa bits set) with 6 % of its elements one
    bf16 ulp below - the mean is ~1e3 times the spread, the largest ratio bf16 inputs allow - k = -2 .. 10 over the rows; "const": every
    row one value (row 0: zero), the output must be the bias; "wscale": |w| spans 1e-3 .. 10 with b at w's scale"""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    w, b = torch.rand(C, device=device, generator=g) + 0.5, 0.1 * rn(C)
    if name == "bigmean":
        ulp = 2.0 ** (torch.arange(M, device=device).remainder(13) - 2.0 - 7.0)[:, None]
        x = 255.0 * ulp - ulp * (torch.rand(M, C, device=device, generator=g) < 0.06)
    elif name == "const":
        x = (rn(M, 1) * row_scales(M, g, device)[:, None]).expand(M, C).clone()
        x[0] = 0.0
    else:
        x = 2.0 * rn(M, C) + 0.5
        if name == "wscale":
            w = torch.logspace(-3.0, 1.0, C, device=device)[torch.randperm(C, device=device, generator=g)] * torch.where(rn(C) < 0, -1.0, 1.0)
            b = 0.3 * rn(C) * w.abs()
    return x.to(torch.bfloat16), w, b


# ---- SE head ------------------------------------------------------------------------------------------------------------------------------
def se_head_ref(y, wr, br, we, be):
    """SEBlock + GELU of conv_exp on y [B, T, C] in fp64: gelu(y * sigmoid(we relu(wr mean_T(y) + br) + be)) ->
    (want, S_arg [B, 1, C]: the magnitude chain |we| (|wr| mean|y| + |br|) + |be| the fp32 noise of the sigmoid's argument scales with)"""
    y = y.double()
    s = torch.relu(y.mean(1) @ wr.double().t() + br.double())
    s = torch.sigmoid(s @ we.double().t() + be.double())[:, None]
    S_arg = (y.abs().mean(1) @ wr.double().abs().t() + br.double().abs()) @ we.double().abs().t() + be.double().abs()
    return gelu64(y * s), S_arg[:, None]


def se_head_bound(want, y, S_arg, dtype, RD):
    """one rounding + the GELU fit + the scale's fp32 chain times |y|, through the GELU.  The chain is three fp32 sums of T, C and RD
    terms (mean, reduce, expand): a random walk of n = T + C + RD roundings of at most 2^-24 S_arg each, taken at twice its expected
    size, 2 sqrt(n) 2^-24 S_arg, enters the sigmoid (slope <= 1/4); the sigmoid itself (v_exp_f32, v_rcp_f32: 1 ulp each) adds 2^-22"""
    B, T, C = y.shape
    c_chain = 2.0 * math.sqrt(T + C + RD) * 2.0 ** -24
    return U[dtype] * want.abs() + U_ABS[dtype] + GELU7_ABS + GELU_SLOPE * (2.0 ** -22 + 0.25 * c_chain * S_arg) * y.double().abs()


def se_head_family(B, T, C, RD, seed, device="cpu"):
    """pooled rows of distinct scale: image b's y carries a factor 4^-b, and the channels span 1e-2 .. 10"""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    ch = torch.logspace(-2.0, 1.0, C, device=device)[torch.randperm(C, device=device, generator=g)]
    y = (rn(B, T, C) + 0.5) * ch * (4.0 ** -torch.arange(B, device=device, dtype=torch.float32)).view(B, 1, 1)
    return y.to(torch.bfloat16), rn(RD, C) * C ** -0.5, 0.1 * rn(RD), rn(C, RD) * RD ** -0.5, 0.1 * rn(C)


# ---- depthwise convolutions -------------------------------------------------------------------------------------------------------------
def dwconv_ref(x, w, b, stride=1, gelu=False, bf16_taps=False):
    """x [B, Cin, H, W] (NCHW, bf16 values), w [Cout, 1, K, K], b [Cout] | None, padding K // 2, groups = Cin, in fp64; bf16_taps: the
    taps rounded to bf16 first (the matrix-core kernels) -> (want, S = conv(|x|, |w|) + |b|)"""
    w = (w.to(torch.bfloat16) if bf16_taps else w).double()
    K, cin = w.shape[-1], x.shape[1]
    y = F.conv2d(x.double(), w, None if b is None else b.double(), stride=stride, padding=K // 2, groups=cin)
    S = F.conv2d(x.double().abs(), w.abs(), None if b is None else b.double().abs(), stride=stride, padding=K // 2, groups=cin)
    return (gelu64(y) if gelu else y), S


def dwconv_bound(want, S, K, gelu=False, taps_rel=0.0):
    """accumulation: K * K taps + the bias in fp32 in any order - the worst case (K K + 1) 2^-24 S, no measurement needed for so few
    terms; taps_rel: the relative error of a tap the kernel documents beyond fp32 (2^-17 for the hi + lo bf16 split of the fused dw3x3)"""
    f = GELU_SLOPE if gelu else 1.0
    return 2.0 ** -7 * want.abs() + ((K * K + 1) * 2.0 ** -24 + taps_rel) * f * S + (GELU7_ABS if gelu else 0.0)


def dwconv_model(x, w, b, stride=1, gelu=False, bf16_taps=False, fault=None, erf=False):
    """fp32 convolution, the degree-7 GELU (erf: the exact one), one rounding.  fault = (channel, tap): that tap of that output channel is dropped"""
    w = (w.to(torch.bfloat16) if bf16_taps else w).float().clone()
    if fault is not None:
        w.view(w.shape[0], -1)[fault[0], fault[1]] = 0.0
    K = w.shape[-1]
    y = F.conv2d(x.float(), w, None if b is None else b.float(), stride=stride, padding=K // 2, groups=x.shape[1])
    return ((gelu64(y).float() if erf else gelu_poly(y, 7)[0]) if gelu else y).to(torch.bfloat16)


def dwconv_family(B, Cin, H, W, K, mult, seed, device="cpu"):
    """colscale: the channels span 1e-2 .. 10 in the input and, independently, in the taps (bias at the output's scale); a row of the
    comparison is one (image, channel) plane -> (x [B, Cin, H, W] bf16, w fp32 [Cout, 1, K, K], b fp32 [Cout])"""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    span = lambda n: torch.logspace(-2.0, 1.0, n, device=device)[torch.randperm(n, device=device, generator=g)]
    cx, cw = span(Cin), span(Cin * mult)
    x = rn(B, Cin, H, W) * cx.view(1, Cin, 1, 1)
    w = rn(Cin * mult, 1, K, K) / K * cw.view(-1, 1, 1, 1)
    b = 0.2 * rn(Cin * mult) * cw * cx.repeat_interleave(mult)
    return x.to(torch.bfloat16), w, b
