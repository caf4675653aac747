"""Element-wise tests of the GEMMs of the Qwen2 prefill (csrc/gemm.hip through fvhd_op_gemm with FVHD_EPI_RESID - o_proj, down_proj - and
FVHD_EPI_SWIGLU - gate|up -, fvhd_op_gemm_splitk, fvhd_op_gemm_splitk_norm, fvhd_op_gemm_qkv_rope) against the fp64 references of
tests/tower_reference.py (pinned on the CPU by tests/test_tower_reference.py) under that module's per-element bounds: the two epilogues
in EVERY kernel class of the family, as tests/test_gpu_tower_ops.py does for the tower's four.  The quantised prefills (e4m3, MXFP4)
dequantise into a bf16 scratch and call the same GEMMs.  Per case (tower_testlib.gemm_case): the class asserted with
fvhd_gemm_kernel_plan BEFORE the launch, a sentinel-guarded output (SwiGLU: [M, N / 2] in front of at least M guard rows), every input
keeps its bits, a second launch - in place for RESID, the prefill's form - gives the same bits, then the family's contract: "rc" (rows
0.05 .. 20 x columns 1e-5 .. 1, gate and up columns scaled independently) inside the per-element bound; "exact" the bits of bf16(fp64)
for RESID and, for SwiGLU, the integer pairing family to ONE bf16 ulp.  Where rows of a shape take another class the bits are equal.
The shapes are the smallest that reach each class on the 256 CUs of an MI355X (those of tests/test_gpu_tower_ops.py, whose
test_gemm_plan_thresholds guards them).  Each test prints its worst err / bound.

MEASURED: see profiles/prefill_gemm_ops_pytest.log (the run this table was filled from) - worst err / bound per family as printed,
beside the CPU model's ratio of tests/test_tower_reference.py:
  family                                                                     measured   CPU model
  EPI_RESID rc, v1 (NF 4 / 3 x BK 64 / 32), v1s, 256 x 128 (+ long K), 256 x 256, ping-pong   0.498      0.498
  EPI_SWIGLU rc, v1 NF 4 (EpiGrp 4, 16-byte stores)                           0.497      0.497
      v1 NF 3 (EpiGrp 1, the 4-byte stores no test reached before)            0.497      0.497
      v1s / 256 x 128, 256 x 256, ping-pong                                   0.497 / 0.498    0.497
  EPI_RESID exact, every class                                               19 cases, all the bits of bf16(fp64 result)
  EPI_SWIGLU pairing family, every class                                     18 cases, every element within one bf16 ulp (model: the same)
  SwiGLU planted gates +40 / 0 / -40 (v1 NF 4, v1 NF 3, v1s)                  0.483      0.483
  split-K rc (v1s and v1 partials, 1 / 2 / 4 slices), out                     0.498      (the GEMM's)
      norm_out against the fp64 norm of the rounded out, / (2^-7 |want|)      0.498      (half a bf16 ulp)
  split-K exact: the bits of bf16(fp64) and of the unsplit GEMM; NULL residual = zero residual, in place = out of place, _norm = the
      two launches: bit for bit.  q|k|v + rope, 9 edge cases: bit for bit the two launches, guards intact, every row written.
Every ratio sits at half a rounding, as the tower's epilogues do: nothing was found wrong in a kernel - not in the GRP == 1 SwiGLU path
of the 96-wide tile either.  Three libraries with a planted wrong result (gate j paired with up j + 1 in the 16-byte SwiGLU epilogue;
gate and up swapped in the 4-byte one; the residual of the neighbouring 8-column group) failed exactly the cases of the classes that
run the changed code (16, 5 and 15 of these tests).  ONE DEFECT in an argument check: fvhd_op_gemm launched EPI_RESID (and
EPI_BIAS_LS_RESID, and the bias epilogues) with a NULL residual / ls / bias, which the kernel then read on the device; it now refuses
them on the host (test_gemm_refusals, include/fvhd.h).  40 tests, 3.9 s.
"""
import os
import sys

import pytest
import torch

from ml_fastvlm_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefill_reference as PR  # noqa: E402
import tower_reference as R  # noqa: E402
import tower_testlib as T  # noqa: E402
from llm_testlib import lib  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu

DEV = T.DEV
BF16 = torch.bfloat16
RESID, SWIGLU = R.EPI_RESID, R.EPI_SWIGLU
P = _lib
NF3 = (P.GEMM_PLAN_V1_NF3_BK64, P.GEMM_PLAN_V1_NF3_BK32)
CASES = [(RESID, "exact"), (SWIGLU, "exact"), (RESID, "rc"), (SWIGLU, "rc")]


def _report(what, worst):
    print(f"{what}: worst err / bound over its rc cases {worst:.3f}")


# ---- RESID and SwiGLU in every kernel class ---------------------------------------------------------------------------------------------
def swiglu_epi_grp(plan):
    """EpiGrp<NF, EPI_SWIGLU, bf16> of csrc/gemm_layout.h by the plan code: the 96-wide tile (NF 3) has no group of four fragments and
    takes the identity W-tile fill with 4-byte stores (GRP 1); every other class stores 16 bytes from four fragments (GRP 4)"""
    return 1 if plan in NF3 else 4


@pytest.mark.parametrize("plan,M,N,K", T.V1_SHAPES)
def test_gemm_v1(lib, plan, M, N, K):
    assert swiglu_epi_grp(plan) == (1 if N % 128 and N % 96 == 0 else 4)       # the NF 3 entries are the only road to the GRP == 1 SwiGLU stores
    worst = max(w for epi, fam in CASES for w in [T.gemm_case(lib, plan, M, N, K, epi, fam)[1]] if w is not None)
    _report(f"v1 plan {plan} (SwiGLU EpiGrp {swiglu_epi_grp(plan)}) {M}x{N}x{K}", worst)


@pytest.mark.parametrize("M,N,K", [(128, 128, 128), (384, 256, 192), (640, 384, 320)])      # 2, 3 and 5 K tiles of 64: prologue only, ring not full, ring wraps
def test_gemm_v1s(lib, M, N, K):
    _report(f"v1s {M}x{N}x{K}", T.streaming(lib, P.GEMM_PLAN_V1S, M, N, K, CASES, other_rows=(M - 1,)))      # M - 1 rows: v1


@pytest.mark.parametrize("M,N,K,cases", [(8192, 2048, 128, CASES), (11008, 384, 3072, [(RESID, "exact"), (RESID, "rc")])])     # 512 tiles; the long-K rule (N % 256 != 0)
def test_gemm_256x128(lib, M, N, K, cases):
    _report(f"256x128 {M}x{N}x{K}", T.streaming(lib, P.GEMM_PLAN_256X128, M, N, K, cases))


def test_gemm_256x256(lib):
    _report("256x256 12800x2304x192", T.streaming(lib, P.GEMM_PLAN_256X256, 12800, 2304, 192, CASES))


@pytest.mark.parametrize("K", [3072, 3136])          # 48 and 49 K tiles of 64
def test_gemm_pingpong(lib, K):
    _report(f"ping-pong 8192x1024x{K}", T.streaming(lib, P.GEMM_PLAN_PINGPONG, 8192, 1024, K, CASES))


def test_gemm_128x192_is_the_gelu_epilogue_s_only(lib):
    for epi in (RESID, SWIGLU):
        assert T.plan(131072 + 40, 192, 192, epi) == P.GEMM_PLAN_V1_NF3_BK64


# ---- planted SwiGLU edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,M,N,K", [(P.GEMM_PLAN_V1_NF4_BK64, 257, 208, 64), (P.GEMM_PLAN_V1_NF3_BK32, 129, 96, 96), (P.GEMM_PLAN_V1S, 384, 256, 192)])
def test_swiglu_planted_gates(lib, plan, M, N, K):
    """gate pre-activations of exactly +40, 0 and -40: row m of A is one-hot at k = m % K with the power of two a_k = 2^(k % 4 - 1), and
    the gate row j of W holds s(j, k) 40 / a_k with s in {+1, 0, -1} (80, 40, 20, 10: exact in bf16), the up rows bf16 values of scales
    2^-6 .. 2^5 divided by a_k - every product and sum is exact.  At +40 the sigmoid is 1 - 4e-18: the output is bf16(40 u) to one ulp;
    at 0 it is zero and at -40 it is -1.7e-16 u, both inside the bound; nothing is NaN or infinite"""
    assert T.plan(M, N, K, SWIGLU) == plan
    g = torch.Generator(device=DEV).manual_seed(N + K)
    k_of = torch.arange(M, device=DEV) % K
    a = 2.0 ** (torch.arange(K, device=DEV) % 4 - 1.0)
    A = torch.zeros(M, K, device=DEV)
    A[torch.arange(M, device=DEV), k_of] = a[k_of]
    s = ((torch.arange(N // 2, device=DEV)[:, None] + torch.arange(K, device=DEV)[None]) % 3 - 1.0)
    W = torch.empty(N, K, device=DEV)
    W[0::2] = s * 40.0 / a
    up = torch.randn(N // 2, K, device=DEV, generator=g).to(BF16).float() * 2.0 ** (torch.arange(N // 2, device=DEV) % 12 - 6.0)[:, None]
    W[1::2] = up / a
    A, W = A.to(BF16), W.to(BF16)
    assert torch.equal(W[1::2].float() * a, up)
    out = T.gemm(lib, A, W, None, None, None, SWIGLU)
    assert T.bits(out, T.gemm(lib, A, W, None, None, None, SWIGLU))
    assert bool(torch.isfinite(out).all()), "NaN or infinity"
    pre = R.gemm_ref(A, W)[0]
    gate, u = pre[:, 0::2], pre[:, 1::2]
    assert torch.equal(gate, 40.0 * s[:, k_of].t().double()) and torch.equal(u, up[:, k_of].t().double())
    assert all(int((gate == v).sum()) >= M * N // 8 for v in (40.0, 0.0, -40.0))
    want, S = R.gemm_ref(A, W, epi=SWIGLU)
    worst = R.inside(out, want, R.gemm_bound(want, S, SWIGLU, BF16, pre=pre), f"planted gates, plan {plan}")
    hot = gate == 40.0
    assert R.one_ulp(out[hot], (40.0 * u[hot]).to(BF16)) == 0, "gate +40: not bf16(40 u) to one ulp"
    assert bool((out[gate == 0.0] == 0).all()), "gate 0: silu(0) u is zero"
    assert float(out[gate == -40.0].double().abs().max()) <= 1e-15 * float(u.abs().max())
    print(f"SwiGLU planted gates +40 / 0 / -40, plan {plan} {M}x{N}x{K}: worst err / bound {worst:.3f}")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _refused(lib, A, W, bias, ls, resid, epi, dtype, M, N, K):
    """the launch returns an error and leaves the sentinel-filled output as it was"""
    buf, out = T.guarded_out(M, N, dtype)
    e = lib.fvhd_op_gemm(T.st(), T.ptr(A), T.ptr(W), T.ptr(bias), T.ptr(ls), T.ptr(resid), T.ptr(out), M, N, K, epi, _lib.dtype_code(dtype))
    torch.cuda.synchronize()
    return e != 0 and T.guard_intact(buf, 0)


def test_gemm_refusals(lib):
    M, N, K = 129, 144, 64
    A, W, b, ls, r = R.gemm_family("rc", M, N, K, R.EPI_BIAS_LS_RESID, 1, device=DEV)
    refused = lambda A_, W_, b_, ls_, r_, epi, dtype=BF16: _refused(lib, A_, W_, b_, ls_, r_, epi, dtype, M, N, K)
    for dtype in (torch.float16, torch.float32):
        for epi in (RESID, SWIGLU):
            assert T.plan(M, N, K, epi, dtype) < 0, (epi, dtype)
            assert refused(A, W, None, None, r, epi, dtype), (epi, dtype)
    assert T.plan(M, N, K, RESID) >= 0 and T.plan(M, N, K, SWIGLU) >= 0
    # a NULL operand that the epilogue would read is refused on the host.  (Found by this test: fvhd_op_gemm used to launch the kernel,
    # which read the NULL residual on the device; include/fvhd.h now states the rule.)
    assert refused(A, W, None, None, None, RESID), "EPI_RESID with a NULL residual"
    assert refused(A, W, b, ls, None, R.EPI_BIAS_LS_RESID) and refused(A, W, b, None, r, R.EPI_BIAS_LS_RESID)
    assert refused(A, W, None, ls, r, R.EPI_BIAS_LS_RESID) and refused(A, W, None, None, None, R.EPI_BIAS)
    assert refused(None, W, None, None, r, RESID) and refused(A, None, None, None, r, RESID)
    # ... and the vectors an epilogue does not read may be NULL
    T.gemm(lib, A, W, None, None, r, RESID)
    T.gemm(lib, A, W, None, None, None, SWIGLU)
    T.gemm(lib, A, W, None, None, None, R.EPI_NONE)


# ---- split-K residual GEMMs of the prefill ----------------------------------------------------------------------------------------------
SPLITK_SHAPES = [(128, 128, 512, 2),       # partials on v1s
                 (77, 128, 2560, 4),       # partials on v1
                 (1, 640, 512, 2), (5, 640, 256, 1),       # the norm kernel's M % 4 (one wave per row, four rows per workgroup) and its second 512-column trip
                 (300, 1536, 512, 2), (7, 3584, 256, 1)]


@pytest.mark.parametrize("M,N,K,sp", SPLITK_SHAPES)
def test_gemm_splitk_and_its_norm(lib, M, N, K, sp):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    nw = 1.0 + 0.2 * torch.randn(N, device=DEV, generator=g)
    for family in ("exact", "rc"):
        A, W, _, _, r = R.gemm_family(family, M, N, K, RESID, 5, device=DEV)
        out = T.gemm_splitk(lib, A, W, r, sp)
        assert T.bits(out, T.gemm_splitk(lib, A, W, r, sp, inplace=True)), "in place differs from out of place"
        want, S = R.gemm_ref(A, W, None, None, r, RESID)
        what = f"split-K {M}x{N}x{K}/{sp} {family}"
        if family == "exact":
            assert torch.equal(out, want.to(BF16)), f"{what}: not the bits of the exact result"
            assert T.bits(out, T.gemm(lib, A, W, None, None, r, RESID)), f"{what}: other bits than the unsplit GEMM"
        else:
            print(f"{what}: worst err / bound {R.inside(out, want, R.gemm_bound(want, S, RESID), what):.3f}")
        assert T.bits(T.gemm_splitk(lib, A, W, None, sp), T.gemm_splitk(lib, A, W, torch.zeros_like(r), sp)), "NULL residual is not a zero residual"
        # ... with the RMSNorm of the finished rows: both outputs the bits of the two launches
        out_n, nout = T.gemm_splitk(lib, A, W, r, sp, norm_w=nw)
        assert T.bits(out_n, out), f"{what}: `out` of the _norm form differs"
        assert T.bits(nout, T.rmsnorm(lib, out, nw)), f"{what}: norm_out is not fvhd_op_rmsnorm of out"
        out_i, nout_i = T.gemm_splitk(lib, A, W, r, sp, inplace=True, norm_w=nw)
        assert T.bits(out_i, out) and T.bits(nout_i, nout), f"{what}: _norm in place differs"
        z, nz = T.gemm_splitk(lib, A, W, None, sp, norm_w=nw)
        z0, nz0 = T.gemm_splitk(lib, A, W, torch.zeros_like(r), sp, norm_w=nw)
        assert T.bits(z, z0) and T.bits(nz, nz0), "_norm: NULL residual is not a zero residual"
        nwant = PR.rmsnorm_ref(out, nw, 1e-6)
        print(f"{what}: norm_out worst err / (2^-7 |want|) {R.inside(nout, nwant, 2.0 ** -7 * nwant.abs(), what + ' norm_out'):.3f}")


def test_gemm_splitk_argument_errors_write_nothing(lib):
    M, N, K = 5, 640, 256
    A, W, _, _, r = R.gemm_family("rc", M, N, K, RESID, 5, device=DEV)
    nw = torch.ones(N, device=DEV)

    def refused(norm, n=N, k=K, sp=1, alias=False):
        buf, out = T.guarded_out(M, N)
        nbuf, nout = T.guarded_out(M, N)
        pbuf = torch.full((2 * M * N + 4096,), float("nan"), device=DEV)
        if norm:
            e = lib.fvhd_op_gemm_splitk_norm(T.st(), T.ptr(A), T.ptr(W), T.ptr(r), T.ptr(out), T.ptr(pbuf), M, n, k, sp, T.ptr(nw), T.ptr(out if alias else nout), 1e-6)
        else:
            e = lib.fvhd_op_gemm_splitk(T.st(), T.ptr(A), T.ptr(W), T.ptr(r), T.ptr(out), T.ptr(pbuf), M, n, k, sp)
        torch.cuda.synchronize()
        return e != 0 and T.guard_intact(buf, 0) and T.guard_intact(nbuf, 0) and bool(torch.isnan(pbuf).all())

    assert refused(True, alias=True), "norm_out == out"
    for norm in (False, True):
        assert refused(norm, n=N - 64), "N % 128 != 0"
        assert refused(norm, k=192, sp=2), "K % (64 * splits) != 0"
        assert refused(norm, k=K - 32), "K % 64 != 0"
        assert refused(norm, sp=0), "splits < 1"
    T.gemm_splitk(lib, A, W, r, 1)            # the same operands with the shape as it is: accepted


# ---- q|k|v projection with the rotary embedding in its epilogue: edges ----------------------------------------------------------------------
@pytest.mark.parametrize("K", [128, 192, 320])        # 2, 3 and 5 K tiles of 64 of the streaming 128 x 128 kernel
@pytest.mark.parametrize("M,Mp,B,T_", [(256, 256, 2, 128), (1, 128, 1, 1), (129, 256, 3, 43)])       # M == Mp, M == 1, M == Mp - 127
def test_gemm_qkv_rope_edges(lib, M, Mp, B, T_, K):
    """fvhd_op_gemm_qkv_rope against its contract - the bits of fvhd_op_gemm(EPI_BIAS) followed by fvhd_op_rope, each element-tested
    elsewhere (tests/test_gpu_tower_ops.py, tests/test_gpu_prefill_ops.py) - with the output and both caches sentinel-filled and
    guarded: every one of the Mp output rows is written, the padding rows M .. Mp - 1 projected and never rotated, every cache row of
    [B, nkv, T, hd] written and nothing behind them; the last real row sits at a position beyond the rotary table"""
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    nh, nkv, hd, theta = 2, 1, 64, 1e6
    width = (nh + 2 * nkv) * hd
    assert M == B * T_ and lib.fvhd_gemm_qkv_rope_supported(Mp, width, K, hd, nh, nkv) == 1
    g = torch.Generator(device=DEV).manual_seed(K + M)
    A = (torch.randn(Mp, K, device=DEV, generator=g) * R.row_scales(Mp, g, DEV)[:, None]).to(BF16)
    W = (torch.randn(width, K, device=DEV, generator=g) * K ** -0.5).to(BF16)
    bias = torch.randn(width, device=DEV, generator=g)
    Pn = max(T_, 8)
    pos = torch.stack([torch.randperm(T_, device=DEV, generator=g) for _ in range(B)]).reshape(M)
    pos[M - 1] = Pn + 500                                       # beyond the table: the phases are computed, not clamped
    table = rope_table(Pn, hd, theta, DEV)
    rows = B * nkv * T_

    def caches():
        (kb, k), (vb, v) = R.guarded(rows, hd, DEV), R.guarded(rows, hd, DEV)
        return kb, k, vb, v

    kb, kc, vb, vc = caches()
    obuf, got = T.guarded_out(Mp, width)
    with T.unchanged(A, W, bias, pos, table):
        T.check(lib.fvhd_op_gemm_qkv_rope(T.st(), T.ptr(A), T.ptr(W), T.ptr(bias), T.ptr(got), Mp, width, K, T.ptr(pos), T.ptr(table), T.ptr(kc), T.ptr(vc), M, T_, nh,
                                          nkv, hd, Pn, theta), "qkv + rope")
    assert T.guard_intact(obuf, Mp) and T.guard_intact(kb, rows) and T.guard_intact(vb, rows), "rows behind the output or behind a cache were written"
    for name, t in (("output", got), ("k cache", kc), ("v cache", vc)):
        assert not bool((t.view(torch.int16) == R.SENT).any()), f"{name}: elements left unwritten"
    assert T.plan(Mp, width, K, R.EPI_BIAS) == P.GEMM_PLAN_V1S
    proj = T.gemm(lib, A, W, bias, None, None, R.EPI_BIAS)
    ref = proj.clone()
    kb2, kc2, vb2, vc2 = caches()
    T.check(lib.fvhd_op_rope(T.st(), T.ptr(ref), T.ptr(pos), T.ptr(table), T.ptr(kc2), T.ptr(vc2), M, T_, nh, nkv, hd, Pn, theta), "rope")
    torch.cuda.synchronize()
    assert T.bits(got, ref), "fused epilogue differs from projection -> rope"
    assert T.bits(kc, kc2) and T.bits(vc, vc2), "KV cache"
    assert T.bits(got[M:], proj[M:]), "padding rows are the projection's, never rotated"
    assert T.bits(got[:, (nh + nkv) * hd:], proj[:, (nh + nkv) * hd:]), "the v heads are never rotated"
    assert not T.bits(got[M - 1:M, :(nh + nkv) * hd], proj[M - 1:M, :(nh + nkv) * hd]), "the row beyond the table is rotated"
    # the cache holds the rotated k heads and the v heads of the real rows, [B, nkv, T, hd]
    packed = got[:M].view(B, T_, nh + 2 * nkv, hd)
    assert T.bits(kc.view(B, nkv, T_, hd), packed[:, :, nh:nh + nkv].transpose(1, 2).contiguous())
    assert T.bits(vc.view(B, nkv, T_, hd), packed[:, :, nh + nkv:].transpose(1, 2).contiguous())
