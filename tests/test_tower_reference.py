"""The CPU pin of tests/tower_reference.py (no GPU): every *_ref agrees with the matching function of oracle/fastvithd_oracle.py in
fp32; the CPU model of the arithmetic each kernel is allowed stays at or below HALF the bound of tests/test_gpu_tower_ops.py on every
input family those tests use (so the reference alone, and a right kernel, sit inside with a margin of two); the same comparison rejects
the planted faults; and the small-row / small-channel faults pass the pooled bound of the first op tests - the hole this closes.

One of the ten planted faults, the softmax denominator summed BEFORE the rounding of P, cannot be rejected by any bound on a bf16
output: it moves an output by at most 2^-9 of its size (sum rb(p) / sum p - 1, every p off by at most 2^-9 relative), below the
output's own rounding and 1/10 of the project's attention budget.  test_fault_denominator_before_rounding_is_invisible states that."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from ml_fastvlm_amd import _lib
from oracle import fastvithd_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tower_reference as R  # noqa: E402

EPIS = (R.EPI_NONE, R.EPI_BIAS, R.EPI_BIAS_GELU, R.EPI_BIAS_LS_RESID)
# (N, K) of the GPU tests' GEMM classes (the rows are a sample: a ratio is a property of one element): the ragged N, the single-tile
# K, every K at which a streaming kernel's ring is in another state, the long K of the ping-pong kernel
GEMM_NK = [(16, 32), (48, 64), (80, 96), (144, 32), (208, 64), (272, 96), (1152, 64), (128, 128), (256, 192), (384, 320), (2304, 320), (192, 192),
           (1024, 3072), (1024, 3136), (384, 3072)]


def _fp32_close(a, b, tol=2e-5):
    a, b = a.double(), b.double()
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ---- agreement with the oracle -----------------------------------------------------------------------------------------------------
def test_refs_agree_with_the_oracle():
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = 3.0 * rn(4000)
    _fp32_close(R.gelu64(x), O.gelu(x))
    # gemm_ref's epilogues against torch's own linear / GELU
    A, W, b, ls, r = rn(9, 64), rn(48, 64) / 8, rn(48), torch.rand(48, generator=g), rn(9, 48)
    _fp32_close(R.gemm_ref(A, W, b, None, None, R.EPI_BIAS_GELU)[0], O.gelu(F.linear(A, W, b)))
    _fp32_close(R.gemm_ref(A, W, b, ls, r, R.EPI_BIAS_LS_RESID)[0], r + ls * F.linear(A, W, b))
    _fp32_close(R.gemm_ref(A, W, None, None, r, R.EPI_RESID)[0], r + F.linear(A, W))
    # layernorm_channel on NCHW
    M, C = 7, 96
    xx, w, bb = 2 * rn(M, C) + 0.5, torch.rand(C, generator=g) + 0.5, 0.1 * rn(C)
    _fp32_close(R.layernorm_ref(xx, w, bb)[0], O.layernorm_channel(xx.t().reshape(1, C, M, 1), w, bb)[0, :, :, 0].t())
    # mhsa: the oracle with qkv = proj = identity-like weights is its core.  qkv.weight = I makes F.linear the identity on [q | k | v]
    B, N, C = 2, 5, 64
    t = rn(B, N, C)
    p = {"m.qkv.weight": rn(3 * C, C) / 8, "m.proj.weight": torch.eye(C), "m.proj.bias": torch.zeros(C)}
    qkv = F.linear(t, p["m.qkv.weight"]).reshape(B * N, 3 * C)
    want = O.mhsa(t.transpose(1, 2).reshape(B, C, N, 1), p, "m").reshape(B, C, N).transpose(1, 2).reshape(B * N, C)
    _fp32_close(R.attention_ref(qkv, B, N, C), want)
    # convffn's MLP: dw7x7 = identity tap, BatchNorm = identity, so that the oracle computes fc2(gelu(fc1(x)))
    C, M = 96, 6
    A, W1, b1, W2, b2 = rn(M, C), rn(4 * C, C) / 10, 0.2 * rn(4 * C), rn(C, 4 * C) / 20, 0.2 * rn(C)
    dw = torch.zeros(C, 1, 7, 7)
    dw[:, 0, 3, 3] = 1.0
    p = {"f.conv.conv.weight": dw, "f.conv.bn.running_mean": torch.zeros(C), "f.conv.bn.running_var": torch.ones(C) - 1e-5,
         "f.conv.bn.weight": torch.ones(C), "f.conv.bn.bias": torch.zeros(C), "f.fc1.weight": W1.view(4 * C, C, 1, 1), "f.fc1.bias": b1,
         "f.fc2.weight": W2.view(C, 4 * C, 1, 1), "f.fc2.bias": b2}
    mlp = O.convffn(A.t().reshape(1, C, M, 1), p, "f")[0, :, :, 0].t()
    pre = A.double() @ W1.double().t() + b1.double()
    _fp32_close(R.gelu64(pre) @ W2.double().t() + b2.double(), mlp)
    want, pre2, hid = R.ffn_ref(A, W1, b1, W2, b2, torch.ones(C), torch.zeros(M, C), _lib.FFN_BF16)
    assert torch.equal(pre2, pre) and float((hid - R.gelu64(pre)).abs().max()) <= 2.0 ** -8 * float(hid.abs().max())
    # conv_exp: dwconv_ref (multiplier 2) + se_head_ref
    Cin, H = 32, 4
    x4, w3, b3 = rn(2, Cin, H, H), rn(2 * Cin, 1, 3, 3) / 3, 0.1 * rn(2 * Cin)
    wr, br, we, be = rn(8, 2 * Cin) / 8, 0.1 * rn(8), rn(2 * Cin, 8) / 3, 0.1 * rn(2 * Cin)
    p = {"c.reparam_conv.weight": w3, "c.reparam_conv.bias": b3, "c.se.reduce.weight": wr.view(8, -1, 1, 1), "c.se.reduce.bias": br,
         "c.se.expand.weight": we.view(-1, 8, 1, 1), "c.se.expand.bias": be}
    y = R.dwconv_ref(x4, w3, b3)[0]
    _fp32_close(y, F.conv2d(x4, w3, b3, padding=1, groups=Cin))
    got = R.se_head_ref(y.flatten(2).transpose(1, 2), wr, br, we, be)[0]
    _fp32_close(got, O.conv_exp(x4, p, "c").flatten(2).transpose(1, 2))


def test_documented_gelu_errors_cover_the_polynomials():
    """the e_phi / absolute GELU errors the bounds take from csrc/fvhd_common.h and include/fvhd.h against the polynomials themselves
    (fp32 Horner chains with the header's coefficients; the half-precision form with the kernel's bit patterns)"""
    x = torch.linspace(-9.0, 9.0, 720001)
    phi = 0.5 * (1.0 + torch.erf(x.double() * 0.7071067811865476))
    for deg, e_phi, e_abs in ((7, R.PHI7, R.GELU7_ABS), (5, R.PHI5, R.GELU5_ABS)):
        gp, pp = R.gelu_poly(x, deg)
        dphi, dg = float((pp.double() - phi).abs().max()), float((gp.double() - R.gelu64(x)).abs().max())
        print(f"degree {deg}: |Phi error| {dphi:.3e} (documented {e_phi}), |gelu error| {dg:.3e} (documented {e_abs})")
        assert dphi <= e_phi and dg <= e_abs
    y, ph = R.gelu_half16((x / 4.0).numpy())
    dphi = float((torch.from_numpy(ph.astype("float64")) - phi).abs().max())
    print(f"FFN_HALF: |Phi error| {dphi:.3e} (documented {R.PHI_HALF})")
    assert dphi <= R.PHI_HALF


# ---- the CPU models under half the bound ---------------------------------------------------------------------------------------------
def test_gemm_model_under_half_the_bound():
    worst_acc, worst = 0.0, {}
    for N, K in GEMM_NK:
        for epi in EPIS:
            A, W, b, ls, r = R.gemm_family("rc", 48, N, K, epi, seed=N + K + epi)
            want, S = R.gemm_ref(A, W, b, ls, r, epi)
            worst_acc = max(worst_acc, float(((R.acc32(A, W).double() - A.double() @ W.double().t()).abs() / S).max()))
            for dt in (torch.bfloat16,) + ((torch.float16, torch.float32) if epi == R.EPI_BIAS and K <= 96 else ()):
                bound = R.gemm_bound(want, S, epi, dt, ls)
                bad, ratio = R.within(R.gemm_model(A, W, b, ls, r, epi, dt, erf=True), want, bound)
                worst[(epi, dt)] = max(worst.get((epi, dt), 0.0), ratio)
                assert bad == 0 and ratio <= 0.5, (N, K, epi, dt, ratio)
                if epi == R.EPI_BIAS_GELU:                      # with the polynomial: GELU7_ABS is ITS error, attained near x = -3 - no margin of two there by definition
                    bad, ratio = R.within(R.gemm_model(A, W, b, ls, r, epi, dt), want, bound)
                    worst[("poly", dt)] = max(worst.get(("poly", dt), 0.0), ratio)
                    assert bad == 0, (N, K, epi, dt, ratio)
                    bad, ratio = R.within(R.gemm_model(A, W, b, ls, r, epi, dt), *R.poly_contract(R.gemm_ref(A, W, b, epi=R.EPI_BIAS)[0], R.C_ACC * S, dt))
                    worst[("vs poly", dt)] = max(worst.get(("vs poly", dt), 0.0), ratio)
                    assert bad == 0 and ratio <= 0.5, (N, K, "polynomial contract", ratio)
            if epi != R.EPI_BIAS_GELU:                          # the exact family: the model returns the bits of bf16(fp64 result)
                A, W, b, ls, r = R.gemm_family("exact", 48, N, K, epi, seed=7)
                assert torch.equal(R.gemm_model(A, W, b, ls, r, epi), R.gemm_ref(A, W, b, ls, r, epi)[0].to(torch.bfloat16)), (N, K, epi)
    print(f"gemm model: worst |acc32 - acc64| / S {worst_acc:.3e} (C_ACC {R.C_ACC:.3e}); worst err / bound " +
          ", ".join(f"epi {e} {str(d)[6:]} {v:.3f}" for (e, d), v in worst.items()))
    assert worst_acc <= 0.5 * R.C_ACC
    # the exact family's premise: partial sums below 2^24 up to K = 6144
    assert 9 * 6144 + 3 < 2 ** 24


def test_swiglu_ref_is_the_qwen2_mlp_front():
    """gemm_ref(EPI_SWIGLU) on W = rows interleaved gate_j, up_j is F.silu(gate_proj(x)) * up_proj(x) of transformers' Qwen2MLP in fp64"""
    from transformers import Qwen2Config
    from transformers.models.qwen2.modeling_qwen2 import Qwen2MLP
    torch.manual_seed(0)
    H, I, M = 64, 48, 9
    mlp = Qwen2MLP(Qwen2Config(hidden_size=H, intermediate_size=I)).double()
    x = torch.randn(M, H, dtype=torch.float64)
    W = torch.stack([mlp.gate_proj.weight, mlp.up_proj.weight], 1).reshape(2 * I, H).detach()      # row 2j = gate_j, row 2j + 1 = up_j
    assert torch.equal(W[0::2], mlp.gate_proj.weight) and torch.equal(W[1::2], mlp.up_proj.weight)       # de-interleaved: the module's own
    want, S = R.gemm_ref(x, W, epi=R.EPI_SWIGLU)
    with torch.no_grad():
        front = mlp.act_fn(mlp.gate_proj(x)) * mlp.up_proj(x)
        assert isinstance(mlp.act_fn, torch.nn.SiLU) or float((mlp.act_fn(x) - F.silu(x)).abs().max()) == 0.0
        assert want.shape == (M, I) and S.shape == (M, 2 * I)
        assert float((want - front).abs().max()) <= 1e-14 * float(front.abs().max())
        assert float((mlp.down_proj(want) - mlp(x)).abs().max()) <= 1e-13 * float(mlp(x).abs().max())


PREFILL_EPIS = (R.EPI_RESID, R.EPI_SWIGLU)


def _bound(A, W, ls, r, epi):
    want, S = R.gemm_ref(A, W, None, ls, r, epi)
    pre = A.double() @ W.double().t() if epi == R.EPI_SWIGLU else None
    return want, R.gemm_bound(want, S, epi, torch.bfloat16, ls, pre=pre), pre


def test_prefill_epilogue_models_under_half_the_bound():
    """EPI_RESID / EPI_SWIGLU: the fault-free model on "rc" at or below half its bound; on "exact" the bits of bf16(fp64) (RESID) and
    one bf16 ulp with the gate sums inside +-GATE_MAX (SwiGLU's pairing family) - and inside the rc bound there as well"""
    worst = {}
    for N, K in GEMM_NK:
        for epi in PREFILL_EPIS:
            for fam in ("rc", "exact"):
                A, W, b, ls, r = R.gemm_family(fam, 48, N, K, epi, seed=N + K + epi)
                assert b is None and ls is None and (r is None) == (epi == R.EPI_SWIGLU)
                want, bound, pre = _bound(A, W, ls, r, epi)
                assert want.shape == (48, N // 2 if epi == R.EPI_SWIGLU else N)
                got = R.gemm_model(A, W, b, ls, r, epi)
                bad, ratio = R.within(got, want, bound)
                worst[(epi, fam)] = max(worst.get((epi, fam), 0.0), ratio)
                assert bad == 0 and ratio <= 0.5, (N, K, epi, fam, ratio)
                if fam == "exact" and epi == R.EPI_RESID:
                    assert torch.equal(got, want.to(torch.bfloat16)), (N, K)
                elif fam == "exact":
                    assert float(pre[:, 0::2].abs().max()) <= R.GATE_MAX < 60 and R.one_ulp(got, want.to(torch.bfloat16)) == 0, (N, K)
                    assert float((R.acc32(A, W).double() - pre).abs().max()) == 0.0            # both sums exact in fp32
    print("prefill epilogues, model: worst err / bound " + ", ".join(f"epi {e} {f} {v:.3f}" for (e, f), v in worst.items()))
    assert float(R.sig_rel(torch.tensor(60.0))) < 1e-3 * R.U[torch.bfloat16]      # the fast sigmoid's allowance never carries a comparison


@pytest.mark.parametrize("precision", [_lib.FFN_HALF, _lib.FFN_BF16])
def test_ffn_model_under_half_the_bound(precision):
    worst = 0.0
    for C in (96, 192, 384):
        ops = R.ffn_family(48, C, seed=C)
        want, pre, hid = R.ffn_ref(*ops, precision)
        A, W1, b1, W2, b2, ls, X = ops
        bad, ratio = R.within(R.ffn_model(*ops, precision), want, R.ffn_bound(want, pre, hid, A, W1, W2, ls, precision))
        worst = max(worst, ratio)
        assert bad == 0 and ratio <= 0.5, (C, ratio)
    print(f"ffn model, precision {precision}: worst err / bound {worst:.3f}")


ATT_N = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]


def test_attention_model_under_half_the_bound():
    worst = {}
    for name in R.ATT_FAMILIES:
        for N in ATT_N + ([576] if name in ("qscale", "ascending") else []):
            B, C = (3, 96) if N % 2 else (1, 64)
            qkv = R.attention_family(name, B, N, C, seed=N)
            bad, ratio = R.attention_violations(R.attention_model(qkv, B, N, C), R.attention_ref(qkv, B, N, C), B, N, C)
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert bad == 0 and ratio <= 0.5, (name, N, ratio)
    print("attention model: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


LN_C = [4, 96, 252, 256, 260, 768, 1024, 1280, 1536, 1792, 2048]


def test_layernorm_model_under_half_the_bound():
    worst, worst_stat = {}, 0.0
    for name in R.LN_FAMILIES:
        for C in LN_C:
            x, w, b = R.layernorm_family(name, 37, C, seed=C)
            want, mean, rstd = R.layernorm_ref(x, w, b)
            bad, ratio = R.within(R.layernorm_model(x, w, b), want, R.layernorm_bound(want, x, w, mean, rstd))
            worst[name] = max(worst.get(name, 0.0), ratio)
            assert bad == 0 and ratio <= 0.5, (name, C, ratio)
            # the statistics alone (before the output rounding), as a fraction of (|x| + |mean|) rstd |w|: what C_LN covers
            xf = x.float()
            m32 = xf.sum(-1, keepdim=True) / C
            pre = (xf - m32) * (1.0 / torch.sqrt((xf - m32).pow(2).sum(-1, keepdim=True) / C + 1e-5)) * w + b
            scale = (x.double().abs() + mean.abs()) * rstd * w.double().abs()
            worst_stat = max(worst_stat, float(((pre.double() - want).abs() / scale.clamp_min(1e-300)).max()))
            if name == "const":                                   # the output is the bias, to within the bound
                assert R.within(R.layernorm_model(x, w, b), b.double().expand_as(want), R.layernorm_bound(want, x, w, mean, rstd))[0] == 0
    print(f"layernorm model: worst statistics error / scale {worst_stat:.3e} (C_LN {R.C_LN:.3e}); worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst_stat <= 0.5 * R.C_LN
    x, _, _ = R.layernorm_family("bigmean", 13, 768, seed=1)
    ratio = x.double().mean(-1).abs() / x.double().std(-1)
    assert float(ratio.min()) >= 700.0, ratio                 # "a mean 1e3 times the spread", as far as bf16 inputs allow


DW_CASES = [(3, 1, 1, 0, False), (7, 1, 1, 0, True), (7, 2, 2, 1, True), (3, 2, 1, 1, False)]      # K, stride, mult, gelu, bf16 taps


def test_dwconv_and_se_head_models_under_half_the_bound():
    for K, S, mult, gelu, bft in DW_CASES:
        x, w, b = R.dwconv_family(2, 64, 9, 20, K, mult, seed=K + S)
        want, Sc = R.dwconv_ref(x, w, b, S, gelu, bft)
        bad, ratio = R.within(R.dwconv_model(x, w, b, S, gelu, bft, erf=True), want, R.dwconv_bound(want, Sc, K, gelu))
        badp, ratiop = R.within(R.dwconv_model(x, w, b, S, gelu, bft), want, R.dwconv_bound(want, Sc, K, gelu))
        print(f"dwconv model K{K} S{S} m{mult} gelu{gelu}: worst err / bound {ratio:.3f} (with the polynomial GELU {ratiop:.3f})")
        assert bad == 0 and ratio <= 0.5 and badp == 0, (K, S, ratio, ratiop)
    for T in (1, 16, 256):
        y, wr, br, we, be = R.se_head_family(3, T, 256, 16, seed=T)
        want, S_arg = R.se_head_ref(y, wr, br, we, be)
        s32 = torch.sigmoid(torch.relu(y.float().mean(1) @ wr.t() + br) @ we.t() + be)[:, None]
        for dt in (torch.bfloat16, torch.float16, torch.float32):
            bound = R.se_head_bound(want, y, S_arg, dt, 16)
            bad, ratio = R.within(R.gelu64(y.float() * s32).float().to(dt), want, bound)
            assert bad == 0 and ratio <= 0.5, (T, dt, ratio)
            assert R.within(R.gelu_poly(y.float() * s32, 7)[0].to(dt), want, bound)[0] == 0


# ---- planted faults ----------------------------------------------------------------------------------------------------------------
def _rejected(got, want, bound):
    return R.within(got, want, bound)[0] > 0


def _passes_pooled(got, want):
    try:
        R.close_pooled(got, want.float())
    except AssertionError:
        return False
    return True


def test_gemm_faults_are_rejected_and_the_pooled_bound_lets_the_small_ones_pass():
    M, N, K = 32, 48, 64                                          # the smallest shape: one row tile, three 16-column groups, two K tiles
    for epi, fault in ((R.EPI_BIAS, "bias16"), (R.EPI_BIAS_LS_RESID, "ls_neighbour"), (R.EPI_NONE, "skip_last_k"), (R.EPI_NONE, "swap_k8"),
                       (R.EPI_BIAS_LS_RESID, "skip_last_k"), (R.EPI_BIAS_GELU, "swap_k8")):
        A, W, b, ls, r = R.gemm_family("rc", M, N, K, epi, seed=3)
        want, S = R.gemm_ref(A, W, b, ls, r, epi)
        bound = R.gemm_bound(want, S, epi, torch.bfloat16, ls)
        assert not _rejected(R.gemm_model(A, W, b, ls, r, epi), want, bound)
        # the bias fault on the 16-column group whose columns are the smallest
        group = int(W.float().abs().amax(1).view(N // 16, 16).amax(1).argmin())
        assert _rejected(R.gemm_model(A, W, b, ls, r, epi, fault=fault, group=group), want, bound), (epi, fault)
    # small channel: the missing bias of the smallest column group passes the pooled bound
    A, W, b, ls, r = R.gemm_family("rc", M, N, K, R.EPI_BIAS, seed=3)
    order = W.float().abs().amax(1).argsort()
    W, b = W[order], b[order]                                     # columns in ascending scale: group 0 is the smallest
    want, S = R.gemm_ref(A, W, b, None, None, R.EPI_BIAS)
    faulty = R.gemm_model(A, W, b, None, None, R.EPI_BIAS, fault="bias16", group=0)
    assert _rejected(faulty, want, R.gemm_bound(want, S, R.EPI_BIAS)) and _passes_pooled(faulty, want)
    # small row: the last of the 96 K tiles of a long-K shape (the ping-pong kernel's K) skipped in the rows of scale <= 0.1
    A, W, _, _, _ = R.gemm_family("rc", M, N, 3072, R.EPI_NONE, seed=3)
    want, S = R.gemm_ref(A, W)
    small = (A.float().abs().amax(1) <= 0.1 * 5.5)[:, None]      # |N(0, 1)| over 3072 draws stays below 5.5
    assert 1 <= int(small.sum()) <= M // 4
    faulty = torch.where(small, R.gemm_model(A, W, fault="skip_last_k"), R.gemm_model(A, W))
    assert _rejected(faulty, want, R.gemm_bound(want, S, R.EPI_NONE)) and _passes_pooled(faulty, want)


PREFILL_FAULTS = ((R.EPI_SWIGLU, "swap_gate_up"), (R.EPI_SWIGLU, "pair_shift"), (R.EPI_RESID, "resid_neighbour8"), (R.EPI_RESID, "resid_dropped"))


@pytest.mark.parametrize("epi,fault", PREFILL_FAULTS)
def test_prefill_epilogue_faults_are_rejected(epi, fault):
    """each fault of the prefill's epilogues fails the per-element bound on "rc" AND the exact family's check (bits for RESID, one ulp
    for SwiGLU's pairing family); the violation counts are asserted > 0 and printed.  ("resid_dropped" hits the 16-column group of the
    smallest columns: the next test shows that the pooled bound of the first op tests lets it pass.)"""
    M, N, K = 32, 48, 64
    A, W, b, ls, r = R.gemm_family("rc", M, N, K, epi, seed=3)
    want, bound, _ = _bound(A, W, ls, r, epi)
    group = int(W.float().abs().amax(1).view(N // 16, 16).amax(1).argmin())
    assert R.within(R.gemm_model(A, W, b, ls, r, epi), want, bound)[0] == 0
    faulty = R.gemm_model(A, W, b, ls, r, epi, fault=fault, group=group)
    n_rc = R.within(faulty, want, bound)[0]
    A, W, b, ls, r = R.gemm_family("exact", M, N, K, epi, seed=3)
    want16 = R.gemm_ref(A, W, b, ls, r, epi)[0].to(torch.bfloat16)
    good, faulty = R.gemm_model(A, W, b, ls, r, epi), R.gemm_model(A, W, b, ls, r, epi, fault=fault, group=group)
    if epi == R.EPI_RESID:
        assert torch.equal(good, want16)
        n_exact = int((faulty != want16).sum())
    else:
        assert R.one_ulp(good, want16) == 0
        n_exact = R.one_ulp(faulty, want16)
    print(f"epi {epi} fault {fault}: {n_rc} of {want.numel()} elements outside the rc bound, {n_exact} of {want16.numel()} fail the exact family")
    assert n_rc > 0 and n_exact > 0, (epi, fault, n_rc, n_exact)


def test_dropped_residual_of_small_columns_passes_the_pooled_bound():
    M, N, K = 32, 48, 64
    A, W, _, _, r = R.gemm_family("rc", M, N, K, R.EPI_RESID, seed=3)
    order = W.float().abs().amax(1).argsort()
    W, r = W[order], r[:, order].contiguous()                     # columns in ascending scale: group 0 is the smallest
    want, bound, _ = _bound(A, W, None, r, R.EPI_RESID)
    faulty = R.gemm_model(A, W, None, None, r, R.EPI_RESID, fault="resid_dropped", group=0)
    assert _rejected(faulty, want, bound) and _passes_pooled(faulty, want)


def test_ffn_fault_is_rejected():
    for precision in (_lib.FFN_HALF, _lib.FFN_BF16):
        ops = R.ffn_family(32, 96, seed=5)
        A, W1, b1, W2, b2, ls, X = ops
        want, pre, hid = R.ffn_ref(*ops, precision)
        bound = R.ffn_bound(want, pre, hid, A, W1, W2, ls, precision)
        assert not _rejected(R.ffn_model(*ops, precision), want, bound)
        assert _rejected(R.ffn_model(*ops, precision, fault="swap_hidden"), want, bound)


def test_attention_faults_are_rejected():
    for fault, name, N in (("unmasked", "qscale", 17), ("unmasked", "plain", 65), ("skip_64", "qscale", 65), ("skip_64", "planted_ragged", 65),
                           ("skip_64", "flat", 129)):
        B, C = 1, 64
        qkv = R.attention_family(name, B, N, C, seed=2)
        want = R.attention_ref(qkv, B, N, C)
        assert R.attention_violations(R.attention_model(qkv, B, N, C), want, B, N, C)[0] == 0
        assert R.attention_violations(R.attention_model(qkv, B, N, C, fault=fault), want, B, N, C)[0] > 0, (fault, name, N)


def test_fault_denominator_before_rounding_is_invisible():
    """sum p instead of sum rb(p) in the denominator: out changes by the factor sum rb(p) / sum p, within 2^-9 of one - less than the
    bf16 rounding of the output itself.  No bound on a bf16 output can reject it; the project's budget is ten times wider."""
    for name in R.ATT_FAMILIES:
        B, N, C = 1, 129, 64
        qkv = R.attention_family(name, B, N, C, seed=4)
        want = R.attention_ref(qkv, B, N, C)
        good, faulty = R.attention_model(qkv, B, N, C), R.attention_model(qkv, B, N, C, fault="l_unrounded")
        assert float(((faulty.double() - good.double()).abs() / good.double().abs().clamp_min(1e-30)).max()) <= 2.0 ** -7      # at most one bf16 ulp apart
        assert R.attention_violations(faulty, want, B, N, C)[0] == 0


def test_layernorm_fault_is_rejected_on_the_large_mean_family():
    x, w, b = R.layernorm_family("bigmean", 13, 768, seed=1)
    want, mean, rstd = R.layernorm_ref(x, w, b)
    bound = R.layernorm_bound(want, x, w, mean, rstd)
    assert not _rejected(R.layernorm_model(x, w, b), want, bound)
    assert _rejected(R.layernorm_model(x, w, b, fault="one_pass"), want, bound)
    xp, wp, bp = R.layernorm_family("plain", 13, 768, seed=1)      # on the old tests' input the one-pass variance is fine: the family is what sees it
    wantp, meanp, rstdp = R.layernorm_ref(xp, wp, bp)
    assert not _rejected(R.layernorm_model(xp, wp, bp, fault="one_pass"), wantp, R.layernorm_bound(wantp, xp, wp, meanp, rstdp))


def test_dwconv_fault_is_rejected_and_passes_the_pooled_bound():
    x, w, b = R.dwconv_family(1, 64, 9, 20, 7, 1, seed=8)
    want, S = R.dwconv_ref(x, w, b, bf16_taps=True)
    bound = R.dwconv_bound(want, S, 7)
    ch = int((want.abs().amax((0, 2, 3))).argmin())               # the channel of the smallest output
    faulty = R.dwconv_model(x, w, b, bf16_taps=True, fault=(ch, 24))      # its centre tap
    assert not _rejected(R.dwconv_model(x, w, b, bf16_taps=True), want, bound)
    assert _rejected(faulty, want, bound) and _passes_pooled(faulty, want)
