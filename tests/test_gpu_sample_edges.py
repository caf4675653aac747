"""The device sampler (csrc/llm_sample.hip) at its edges, against tests/decode_reference.py::sample_ref (fp64, pinned to transformers'
warpers on the CPU by tests/test_decode_reference.py): tied logits, -inf entries, vocabularies at the slice-count boundaries, top_k around V,
top_p between two value groups and 0, extreme temperatures, u at the ends of [0, 1).

Every row of every launch is checked, no row and no draw is skipped:
  * the info row: theta = the lowest kept value, the kept count, Z to rtol 1e-5, u;
  * the kept set {s >= theta, s > -inf} equals sample_ref's (top_p is placed mid-gap between two value groups, and the reference's
    distance to the nearest group boundary is asserted to be >= 1e-5);
  * the draw: with c_j the fp64 index-order CDF, the chosen id is a kept token whose interval [c_{j-1}, c_j] meets [u - 1e-5, u + 1e-5]
    (fp32 sums of up to 152064 terms against fp64).  So that this tolerance cannot hide a wrong draw, at least 75 % of every case's draws
    must have exactly ONE admissible token - a condition on the reference alone, asserted in _plan_case.  The settings are chosen for it
    (at V >= 65535 the whole-row settings run at T = 0.05); the only cases it is not asserted for are the named entries of EXEMPT;
  * the kept set against transformers' warpers on the same rows: HF is a subset of ours, the rest lies in the group at theta;
  * two launches give the same bits."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as R  # noqa: E402
import llm_testlib as L  # noqa: E402

pytestmark = pytest.mark.gpu

GAP = 1e-5
U_ENDS = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]
KINDS = ["grid", "grid_inf", "equal", "max3", "peaked", "flat", "one_finite", "signed_zero"]
TIED_KINDS = ["grid", "grid_inf", "equal", "max3", "peaked", "one_finite", "signed_zero"]      # a flat row has no group of >= 2e-5 mass


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import _lib
    return _lib.sampling_lib()


def _row(kind, V, seed):
    g = torch.Generator().manual_seed(seed)
    if kind in ("grid", "grid_inf"):
        x = torch.randint(-8, 9, (V,), generator=g).float() * 0.5
        if V >= 65535:                                            # a head of 2048 tokens on the grid in [-4, 4], the others 12 lower: still
            tail = torch.randperm(V, generator=g)[2048:]          # every value tied, but a tie group of ~120 tokens, not ~9000 of 1e-4 each
            x[tail] -= 12.0
        if kind == "grid_inf" and V >= 3:
            x[torch.randperm(V, generator=g)[:V // 3]] = -math.inf
    elif kind == "equal":
        x = torch.full((V,), 1.25)
    elif kind == "max3":
        x = 2.0 * torch.randn(V, generator=g)
        x[torch.randperm(V, generator=g)[:3]] = float(x.max()) + 1.5
    elif kind == "peaked":
        x = 3.0 * torch.randn(V, generator=g)
        if V > 8:
            x[torch.randperm(V, generator=g)[:8]] = 12.0 + 4.0 * torch.rand(8, generator=g)
    elif kind == "flat":
        x = 0.3 * torch.randn(V, generator=g)
    elif kind == "one_finite":
        x = torch.full((V,), -math.inf)
        x[int(torch.randint(0, V, (1,), generator=g))] = -3.0
    else:                                                         # signed zeros share one key: -0.0 == +0.0, tied at the row maximum
        x = -0.5 * torch.randint(1, 17, (V,), generator=g).float()
        top = torch.randperm(V, generator=g)[:max(min(V // 4, 512), 1)]
        x[top] = torch.tensor([-0.0, 0.0])[torch.randint(0, 2, (top.numel(),), generator=g)]
    return x


def _us(B, seed):
    """the 16 values of u per row: the ends of [0, 1), 0.5, and 12 seeded ones -> [16][B] fp32"""
    g = torch.Generator().manual_seed(seed)
    rnd = (torch.randint(0, 2 ** 24, (12, B), generator=g).float() * 2.0 ** -24)
    return torch.cat([torch.tensor(U_ENDS)[:, None].expand(4, B), rnd], 0).float()


# The named exceptions to "at least 75 % of a case's draws have exactly one admissible token": cases whose every kept token carries
# less than the 2e-5 window of the tolerance whatever the settings, so that no choice of top_k / temperature can pin the draw.  They
# are run and every draw is checked for admissibility; only the 75 % condition is not asserted.
EXEMPT = {
    "all-equal row, V >= 65535": "V tokens of mass 1 / V <= 1.6e-5 each; top_k keeps the whole tie group, temperature changes nothing",
    "T = 100 without top_k, V >= 65535": "a nearly uniform row: every token carries about 1 / V; the case is there for the kept count and Z",
}


def _plan_case(x, T, k, p, what, exempt=None, seed=0):
    """the reference side of one (T, k, p) setting, no GPU: -> (refs, u [16][B], admissible sets, fraction of draws with ONE admissible token).
    Asserts the case's design from the reference alone: top_p at least GAP away from a group boundary, and the 75 % condition unless the
    case is one of the named exceptions"""
    B, V = x.shape
    refs = [R.sample_ref(x[b], T, k, p) for b in range(B)]
    if p < 1.0:
        for b, r in enumerate(refs):
            assert r["margin"] >= GAP, f"{what}: row {b} has a group boundary within {r['margin']:.2g} of top_p (a case-design error)"
    us = _us(B, seed + V)
    adm = [[R.admissible_tokens(r, float(us[i, b])) for b, r in enumerate(refs)] for i in range(us.shape[0])]
    frac = sum(int(a.sum()) == 1 for row in adm for a in row) / (us.shape[0] * B)
    assert exempt is None or exempt in EXEMPT, exempt
    if exempt is None:
        assert frac >= 0.75, f"{what}: only {frac:.2f} of the draws have exactly one admissible token (a case-design error)"
    return refs, us, adm, frac


def _run_case(lib, x, T, k, p, what, exempt=None, seed=0):
    """x [B, V] on the CPU; one (T, k, p) setting over the 16 values of u; -> (refs, ids [16][B], fraction of draws with one admissible token)"""
    B, V = x.shape
    refs, us, adm, frac = _plan_case(x, T, k, p, what, exempt, seed)
    xd = x.cuda().contiguous()
    hf = L.oracle_scores(x, T, k, p) > -math.inf                    # transformers' warpers on the rows actually launched
    all_ids = []
    for i in range(us.shape[0]):
        ut = us[i].cuda().contiguous()
        ids, info = L.sample(lib, xd, T, k, p, u=ut)
        ids, info = ids.cpu(), info.cpu()
        if i == 0:
            ids2, info2 = L.sample(lib, xd, T, k, p, u=ut)
            assert torch.equal(ids, ids2.cpu()) and torch.equal(info.view(torch.int32), info2.cpu().view(torch.int32)), what + ": two launches differ"
        all_ids.append(ids)
        for b, r in enumerate(refs):
            w = f"{what} row {b} u={float(us[i, b])!r}"
            if i == 0:
                theta = float(info[b, 0])
                kept = (r["s"] >= theta) & (r["s"] > -math.inf)
                assert torch.equal(kept, r["kept"]), f"{w}: kept set differs: {int(kept.sum())} kept (theta {theta}), reference {r['count']} (theta {r['theta']})"
                assert theta == r["theta"] or (theta == -math.inf and r["count"] == int((r["s"] > -math.inf).sum())), (w, theta, r["theta"])
                # the relation to the warpers: HF is a subset of ours, and what we keep beyond it lies in the value group at theta
                assert bool((kept | ~hf[b]).all()), f"{w}: transformers keeps a token that the device does not"
                extra = kept & ~hf[b]
                assert bool((r["s"][extra] == r["theta"]).all()), f"{w}: kept beyond transformers' set outside the boundary group"
            assert int(info[b, 1]) == r["count"], f"{w}: kept count {int(info[b, 1])}, reference {r['count']}"
            assert abs(float(info[b, 2]) - r["Z"]) <= 1e-5 * r["Z"], f"{w}: Z {float(info[b, 2])}, reference {r['Z']}"
            assert float(info[b, 3]) == float(us[i, b]), w
            t = int(ids[b])
            assert 0 <= t < V and bool(adm[i][b][t]), (f"{w}: token {t} (kept {bool(r['kept'][t])}) is not admissible; admissible "
                                                       f"{adm[i][b].nonzero()[:8, 0].tolist()}")
    return refs, torch.stack(all_ids), frac


VOCABS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 65535, 65536, 65537, 152064]
LARGE = 65535


def _kinds(V):
    """the row kinds of the 75 % cases: at V >= 65535 without the all-equal row (a named exception, run on its own below)"""
    return KINDS if V < LARGE else [k for k in KINDS if k != "equal"]


def _settings(V):
    """(T, top_k, top_p) without a top_p boundary: top_k in {1, V - 1, V, V + 1}, top_p 0.  At V >= 65535 the settings that keep the whole
    row run at T = 0.05, where the mass sits in few enough tokens for the 1e-5 tolerance to leave one candidate"""
    wide = 1.0 if V < LARGE else 0.05
    ks = sorted({max(V - 1, 0), V, V + 1})
    return [(wide, 0, 1.0), (1.0, 0, 0.0), (0.7, 5, 1.0), (1.0, 1, 1.0), (1.0, 50, 1.0)] + [(wide, k, 1.0) for k in ks]


def _midgap(x, T, k, group):
    for gsel in range(group, -1, -1):                             # a group too light to resolve gives way to the next heavier one
        p, gap = R.top_p_midgap(x, T, k, gsel)
        if gap >= GAP:
            break
    assert gap >= GAP, (T, k, group, gap)
    return p


def _cases(name, V):
    """every (x [B, V], T, k, p, what, exempt) of test `name` - one generator, so that the cases' design can be checked without a GPU"""
    if name == "mixed":
        kinds = _kinds(V)
        x = torch.stack([_row(kinds[b % len(kinds)], V, 1000 + V + b) for b in range(16)])
        for T, k, p in _settings(V):
            yield x, T, k, p, f"V={V} T={T} k={k} p={p}", None
    elif name == "shuffles":
        base = _row("grid_inf", V, 2000 + V)
        g = torch.Generator().manual_seed(V)
        x = torch.stack([base[torch.randperm(V, generator=g)] for _ in range(16)])
        wide = 1.0 if V < LARGE else 0.05
        for T, k, group in [(wide, 0, 1), (wide, 0, 3), (0.7, 5, 0), (wide, max(V - 1, 0), 2), (0.2, 50, 1)]:
            p = _midgap(base, T, k, group)
            yield x, T, k, p, f"V={V} T={T} k={k} p={p:.6f}", None
    elif name == "single":
        wide = 1.0 if V < LARGE else 0.05
        for kind in _kinds(V):
            x = _row(kind, V, 3000 + V)[None]
            cases = list(_settings(V))
            if kind in TIED_KINDS:
                cases += [(T, k, _midgap(x[0], T, k, group)) for T, k, group in [(wide, 0, 1), (0.7, 5, 0), (wide, V + 1, 2)]]
            for T, k, p in cases:
                yield x, T, k, p, f"V={V} {kind} T={T} k={k} p={p:.6f}", None
    elif name == "equal_large":
        x = _row("equal", V, 7000 + V)[None].expand(16, V).contiguous()
        for T, k, p in [(1.0, 0, 1.0), (1.0, 1, 1.0), (0.05, V, 1.0), (1.0, 0, 0.0)]:
            yield x, T, k, p, f"V={V} all-equal T={T} k={k} p={p}", "all-equal row, V >= 65535"
    elif name == "extreme":
        kinds = _kinds(V)
        x = torch.stack([_row(kinds[b % len(kinds)], V, 5000 + V + b) * (4.0 if kinds[b % len(kinds)] in ("grid", "grid_inf", "signed_zero") else 1.0)
                         for b in range(16)])
        for k in (0, 50):
            yield x, 0.01, k, 1.0, f"V={V} T=0.01 k={k}", None
        for k in (0, 50, 1):
            yield x, 100.0, k, 1.0, f"V={V} T=100 k={k}", ("T = 100 without top_k, V >= 65535" if k == 0 and V >= LARGE else None)


@pytest.mark.parametrize("V", VOCABS)
def test_sixteen_rows_of_different_kinds(lib, V):
    """B = 16, every row another kind: settings without a top_p boundary (top_p 1 and 0: rows of different kinds do not share a gap)"""
    fr = [_run_case(lib, *c)[2] for c in _cases("mixed", V)]
    print(f"V={V} B=16 mixed kinds: single-token draw fraction {min(fr):.2f} .. {max(fr):.2f}")


@pytest.mark.parametrize("V", VOCABS)
def test_sixteen_shuffles_of_one_tied_row_top_p_mid_gap(lib, V):
    """B = 16 rows with the same multiset of values (so one mid-gap top_p serves them all) in 16 different orders: a 0.5 grid with a third
    of the row at -inf"""
    fr = [_run_case(lib, *c)[2] for c in _cases("shuffles", V)]
    print(f"V={V} B=16 shuffles: single-token draw fraction {min(fr):.2f} .. {max(fr):.2f}")


@pytest.mark.parametrize("V", VOCABS)
def test_single_rows_of_every_kind(lib, V):
    """B = 1, one launch per kind: top_k in {1, 50, V - 1, V, V + 1}, top_p 0, and top_p mid-gap below the first value groups"""
    fr = [_run_case(lib, *c)[2] for c in _cases("single", V)]
    print(f"V={V} B=1: single-token draw fraction {min(fr):.2f} .. {max(fr):.2f}")


@pytest.mark.parametrize("V", [v for v in VOCABS if v >= LARGE])
def test_all_equal_row_of_a_large_vocabulary(lib, V):
    """the named exception: kept set, count, Z and the admissibility of every draw are checked, the 75 % condition cannot hold"""
    fr = [_run_case(lib, *c)[2] for c in _cases("equal_large", V)]
    print(f"V={V} all-equal row: single-token draw fraction {min(fr):.2f} .. {max(fr):.2f} (exempt)")


@pytest.mark.parametrize("V", [3, 257, 4096, 152064])
def test_maximum_tied_three_ways_with_top_k_1(lib, V):
    """top_k = 1 keeps the whole group at the maximum: kept count 3, and over the sweep of u the draw lands on all three"""
    x = torch.stack([_row("max3", V, 4000 + V + b) for b in range(16)])
    refs, ids, _ = _run_case(lib, x, 1.0, 1, 1.0, f"V={V} max3 top_k=1")
    for b, r in enumerate(refs):
        top = r["kept"].nonzero()[:, 0].tolist()
        assert r["count"] == 3 and len(top) == 3
        assert sorted(set(ids[:, b].tolist())) == top, (b, top, ids[:, b].tolist())


@pytest.mark.parametrize("V", [2, 257, 2049, 65537, 152064])
def test_extreme_temperatures(lib, V):
    """T = 0.01: the grid rows step by 2.0, 200 after the division - everything below the top group is exactly 0 in fp32 (expf underflows
    below -104), so the draw is in the top group whatever u.  T = 100: a nearly uniform row - the kept count is exact and Z matches fp64 to
    1e-5 (asserted in _run_case)"""
    fired = 0
    for x, T, k, p, what, exempt in _cases("extreme", V):
        refs, ids, _ = _run_case(lib, x, T, k, p, what, exempt)
        if T != 0.01:
            continue
        for b, r in enumerate(refs):
            top = r["s"] == r["s"].max()
            rest = r["s"][~top & r["kept"]]
            if rest.numel() == 0 or float(rest.max()) <= float(r["s"].max()) - 104.0:
                fired += 1
                assert bool(top[ids[:, b]].all()), (b, "a token below the top group was drawn at T = 0.01")
    assert fired >= 4, f"the top-group check at T = 0.01 applied to {fired} rows only: the grid rows no longer underflow"


@pytest.mark.parametrize("V,T,k", [(V, T, k) for V in (2, 255, 4096, 65537, 152064) for T in (0.7, 1.0) for k in (0, 50)
                                   if (V, T, k) != (152064, 1.0, 0)])
def test_draws_on_peaked_rows_are_pinned_to_one_token(lib, V, T, k):
    """rows shaped like an LM's next-token distribution (V = 152064 at T = 1 without top-k is not generated: its tail's intervals are
    narrower than the tolerance; that vocabulary runs with top_k = 50 or T = 0.7)"""
    x = torch.stack([_row("peaked", V, 6000 + V + b) for b in range(16)])
    _, _, frac = _run_case(lib, x, T, k, 1.0, f"peaked V={V} T={T} k={k}")
    print(f"peaked V={V} T={T} k={k}: {frac:.2f} of the draws have exactly one admissible token")
