"""tests/warper_reference.py against transformers' own warpers (MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper
behind temperature / top-k / top-p), on the CPU: equal sets on float64 scores, without a tolerance; on fp32 scores the sets differ only
in tokens within the reference's margin of a threshold; and the two identities the device relies on.  Rows have no value ties where top-p
takes part (transformers' unstable sort splits tie groups)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warper_reference as W  # noqa: E402

VOCABS = [257, 2049, 65537]
KINDS = ["peaked", "gauss", "flat", "third_inf"]
SETTINGS, _args = W.SETTINGS, W.setting_args


def _row(kind, V, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "peaked":
        x = 3.0 * torch.randn(V, generator=g)
        x[torch.randperm(V, generator=g)[:8]] = 12.0 + 4.0 * torch.rand(8, generator=g)
    elif kind == "flat":
        x = 0.3 * torch.randn(V, generator=g)
    else:
        x = 2.0 * torch.randn(V, generator=g)
        if kind == "third_inf":
            x[torch.randperm(V, generator=g)[:V // 3]] = -math.inf
    return x


CASES = [(V, kind, name) for V in VOCABS for kind in KINDS for name in SETTINGS]


@pytest.mark.parametrize("V,kind,name", CASES)
def test_equals_transformers_on_float64_scores(V, kind, name):
    x = _row(kind, V, 31 * V + KINDS.index(kind))
    T, k, p, w = _args(SETTINGS[name])
    ref = W.warp_ref(x, T, k, p, **w)
    hf = W.oracle_kept(x, T, k, p, **w)
    assert torch.equal(ref["kept"], hf), (int(ref["kept"].sum()), int(hf.sum()), (ref["kept"] ^ hf).nonzero()[:8, 0].tolist())
    assert [s["name"] for s in ref["stages"]] == [n for n in W.STAGES if {"epsilon_cutoff": "eps", "eta_cutoff": "eta"}.get(n, n) in w]
    cs = [s["count"] for s in ref["stages"]]
    assert cs == sorted(cs, reverse=True) and ref["count"] == (cs[-1] if cs else ref["base"]["count"]) >= 1


@pytest.mark.parametrize("V,kind,name", CASES)
def test_differs_from_transformers_on_fp32_scores_only_inside_the_margins(V, kind, name):
    """a token the two disagree on lies, at some stage, closer to the threshold than transformers' own fp32 error reaches: in key space within
    1e-3 relative (its fp32 softmax / cumsum over V terms), or the stage's mass margin is below 1e-3"""
    x = _row(kind, V, 31 * V + KINDS.index(kind))
    T, k, p, w = _args(SETTINGS[name])
    ref = W.warp_ref(x, T, k, p, **w)
    diff = ref["kept"] ^ W.oracle_kept(x, T, k, p, dtype=torch.float32, **w)
    for i in diff.nonzero()[:, 0].tolist():
        near = False
        for st in ref["stages"]:
            if st["name"] == "typical_p":
                near |= abs(float(st["d"][i]) - st["threshold"]) <= 1e-3 * max(st["threshold"], 1.0) or st["mass"] <= 1e-3
            else:
                near |= st["threshold"] > 0 and abs(float(ref["x"][i]) - math.log(st["threshold"])) <= 1e-3
        assert near or ref["base"]["margin"] <= 1e-3, (i, float(ref["x"][i]), [(s["name"], s["threshold"], s["mass"]) for s in ref["stages"]])


@pytest.mark.parametrize("kind", KINDS)
def test_the_identities_the_device_relies_on(kind):
    """min_p without Z: e >= min_p <=> p >= min_p * p_max; typical_p without log Z: |-log p - H| = |(s - M) - A|"""
    x = _row(kind, 2049, 5)
    ref = W.warp_ref(x, 0.9, 40, 0.98, min_p=0.01, typical_p=0.9)
    K = ref["base"]["kept"]
    e, xs = ref["e"], ref["x"]
    Z = e[K].sum()
    pk = e / Z
    assert torch.equal((pk >= W.f32(0.01) * pk[K].max()) & K, ref["stages"][0]["kept"])
    K1 = ref["stages"][0]["kept"]
    Z1 = e[K1].sum()
    logp = xs - torch.log(Z1)
    H = -(e[K1] / Z1 * logp[K1]).sum()
    st = ref["stages"][1]
    assert torch.allclose((-logp - H).abs()[K1], st["d"][K1], rtol=0, atol=1e-12)
    assert abs(float(H) - (math.log(float(Z1)) - st["A"])) < 1e-12


def test_rules_at_the_edges():
    x = torch.tensor([1.0, 3.0, 3.0, -math.inf, 3.0, 0.5])
    r = W.warp_ref(x, 1.0, 0, 1.0, min_p=1.0)
    assert r["kept"].tolist() == [False, True, True, False, True, False] and r["counts"] == (3, 3, 3)
    one = torch.full((9,), -math.inf)
    one[4] = -3.0
    for w in SETTINGS.values():
        T, k, p, w = _args(w)
        r = W.warp_ref(one, T, k, p, **w)
        assert r["kept"].nonzero()[:, 0].tolist() == [4] and r["count"] == 1
    # a cutoff that removes every probability keeps the tokens tied at the maximum
    r = W.warp_ref(torch.tensor([0.0, 0.0, -0.1, -0.2]), 1.0, 0, 1.0, eps=0.9)
    assert r["kept"].tolist() == [True, True, False, False]


def test_place_gives_sound_margins():
    for kind in KINDS:
        x = _row(kind, 2049, 11)
        for name, st in SETTINGS.items():
            T, k, p, w = _args(st)
            placed = W.place(x, T, k, p, **{a: w.get(a) for a in ("min_p", "typical_p", "eps", "eta")})
            W.assert_margins(W.warp_ref(x, T, k, p, **placed), f"{kind} {name}")
