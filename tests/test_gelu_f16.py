"""The half-precision GELU of the fused ConvFFN (csrc/ffn_fused.hip: gelu16_stage), restated in numpy float16 with the kernel's own
coefficient bit patterns (parsed from the source, so the two cannot drift apart), against the exact erf GELU the reference uses
(nn.GELU() default, mci.py:870): the bounds DESIGN.md / include/fvhd.h / INTEGRATION.md state.  CPU only."""
import os
import sys

import numpy as np
import pytest
from scipy.special import erf

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tower_reference import _half_constants as _kernel_constants, gelu_half16  # noqa: E402  (the restatement, defined once for the tower tests)

h = np.float16


def test_constants_are_the_documented_ones():
    umax, coef, half = _kernel_constants()
    assert float(umax) == (3.5 / 4.0) ** 2 and float(half) == 0.5
    # c_k' = 4 * 16^k * FVHD_GELU5_Ck rounded to half, c0' one ulp up (exact saturation at +-3.5)
    c = [3.980601132e-01, -6.438287348e-02, 8.499878459e-03, -7.195603685e-04, 3.409395140e-05, -6.780236390e-07]
    want = [h(ck * 4 * 16.0 ** k) for k, ck in enumerate(c)]
    want[0] = np.nextafter(want[0], h(10))
    assert [float(v) for v in coef] == [float(v) for v in want[::-1]]


def test_phi_error_and_exact_tails():
    x = np.linspace(-8.0, 8.0, 400001).astype(np.float32)
    y, phi = gelu_half16(x / 4.0)
    ref = 0.5 * (1.0 + erf(x.astype(np.float64) / np.sqrt(2.0)))
    assert np.abs(phi.astype(np.float64) - ref).max() <= 1.4e-3                      # include/fvhd.h, DESIGN.md
    assert np.sqrt(np.mean((phi.astype(np.float64) - ref) ** 2)) <= 3e-4
    assert (phi[x >= 3.5] == 1).all() and (phi[x <= -3.51] == 0).all()               # gelu(x) = x from 3.5 on, 0 below -3.51, exactly
    assert (phi[(x <= -3.5) & (x > -3.51)] <= h(2.0 ** -13)).all()                   # (in between the half-precision sum leaves one ulp of 2^-13)
    big = np.array([10.0, 1e3, 2.6e5, 3e5, 1e30, -10.0, -1e3, -1e30], np.float32)
    yb, _ = gelu_half16(big / 4.0)
    assert np.isfinite(yb.astype(np.float32)).all()                                  # saturates, never inf / nan
    assert float(yb[3]) == 65504.0 and float(yb[4]) == 65504.0 and float(yb[2]) * 4 <= 2.6e5
    assert (yb[5:] == 0).all()


@pytest.mark.parametrize("sigma", [0.3, 1.0, 2.0, 4.0])
def test_hidden_activation_is_more_accurate_than_a_bf16_hidden_tensor(sigma):
    """the reason the change is a parity improvement and not a trade: rms error of the hidden activation over N(0, sigma) inputs"""
    rng = np.random.default_rng(int(sigma * 10))
    x = rng.normal(0.0, sigma, 200000).astype(np.float32)
    ref = 0.5 * x.astype(np.float64) * (1.0 + erf(x.astype(np.float64) / np.sqrt(2.0)))
    y, _ = gelu_half16(x / 4.0)
    err16 = np.sqrt(np.mean((4.0 * y.astype(np.float64) - ref) ** 2))
    u = ref.astype(np.float32).view(np.uint32)                                        # exact GELU rounded to bf16 (RNE): the best a bf16 tensor can do
    bf = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).view(np.float32)
    errbf = np.sqrt(np.mean((bf.astype(np.float64) - ref) ** 2))
    rms = np.sqrt(np.mean(ref ** 2))
    assert err16 / rms <= 1.1e-3
    assert err16 <= errbf, (err16, errbf)
