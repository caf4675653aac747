"""The Philox seeds of the selection cases of tests/test_gpu_beam_sample_ops.py (CPU only, no library): how its SELECTION_SEEDS table is re-derived.

    python tools/beam_sample_margins.py [--first 0 --tries 200]

For every case (V, G, K, keep, T) of the test: the fp64 reference (tests/beam_sample_reference.py) on the test's own inputs
(`inputs(V, G, K, 0)`, the settings of `selection_settings`), for Philox seeds first, first + 1, ...: the first seed at which every adjacent gap
among the reference's top keep + 1 keys a + g of every prompt (as many of them as the prompt has kept candidates) exceeds twice the derived bound on the device's key (`bound`) is printed - there
fp32 rounding cannot legitimately order the picks otherwise.  The test asserts the same about its inputs."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def margin(R, x, scores, G, K, keep, T, top_k, top_p, m, seed, n, fixed=None):
    """-> (the smallest adjacent gap among the top keep + 1 keys, the bound, the reference)"""
    if fixed is None:
        ref = R.reference(x, scores, G, K, keep, T, top_k, top_p, m, seed=seed, n=n, extra=1)
    else:                                                         # the same inputs under another seed: only the noise and the selection change
        ref = dict(fixed)
        ref["g"] = R.gumbel_noise(seed, G * K, n, x.shape[1])
        ref["scores"], ref["index"], ref["keys"] = R.select(ref["a"], ref["g"], ref["kept"], G, K, keep, 1)
    return R.smallest_gap(ref["keys"]), R.bound(ref, T)[0], ref


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--tries", type=int, default=200)
    a = ap.parse_args()
    import beam_sample_reference as R
    from test_gpu_beam_sample_ops import N_STEP, SHAPES, TEMPERATURES, selection_settings
    found = {}
    for V, G, K, keep in SHAPES:
        x, scores = R.inputs(V, G, K, 0)
        for T in TEMPERATURES:
            top_k, top_p, m = selection_settings(T, K, keep)
            fixed = None
            for seed in range(a.first, a.first + a.tries):
                gap, b, fixed = margin(R, x, scores, G, K, keep, T, top_k, top_p, m, seed, N_STEP, fixed)
                if gap > 2 * b:
                    found[(V, G, K, keep, T)] = seed
                    print(f"({V}, {G}, {K}, {keep}, {T}): {seed},   # smallest gap {gap:.3g} > 2 * {b:.3g}", flush=True)
                    break
            else:
                print(f"({V}, {G}, {K}, {keep}, {T}): no seed in [{a.first}, {a.first + a.tries})", flush=True)
    print(found)


if __name__ == "__main__":
    main()
