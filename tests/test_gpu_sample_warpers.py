"""The device sampler's warpers behind top-p (csrc/llm_sample.hip: min_p, typical_p, epsilon_cutoff, eta_cutoff) at the sampler's own edges,
through fvhd_op_dec_sample_warpers, against tests/warper_reference.py (fp64, pinned to transformers' warpers by test_warper_reference.py).
Built like test_gpu_sample_edges.py: its vocabularies (the slice-count boundaries), its row kinds plus a Gaussian row, its 16 values of u.

Every row of every launch is checked, no row and no draw is skipped:
  * every per-stage count of the info row (behind min_p, typical_p, epsilon_cutoff, and the final one) equals the reference's;
  * the final kept set, rebuilt from the info row's per-stage counts and the reference's keys (_rebuild), equals the reference's, and the
    lowest / highest kept s of the info row are that set's;
  * Z to rtol 1e-5; u;
  * the draw is admissible under the +-1e-5 window of test_gpu_sample_edges.py, and at least 75 % of a case's draws have exactly one
    admissible token - asserted on the reference alone in _plan, with that file's two named exemptions;
  * two launches give the same bits.
The settings of a case are placed mid-gap for its rows (warper_reference.place), and _plan asserts every row's margins (mass >= GAP, key
space >= 2 x the derived bound) before anything is launched.  The largest fraction of the key-space margin that the bound uses, and the
largest observed error of Z as a fraction of its bound, go to profiles/warpers_bound.log when FVHD_WRITE_PROFILES=1."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as R  # noqa: E402
import llm_testlib as L  # noqa: E402
import warper_reference as W  # noqa: E402

SETTINGS, _args = W.SETTINGS, W.setting_args                    # the nine settings: each warper alone, each behind top-k + top-p, all seven

pytestmark = pytest.mark.gpu

VOCABS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 65535, 65536, 65537, 152064]
LARGE = 65535
U_ENDS = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24]
KINDS = ["grid", "grid_inf", "equal", "max3", "peaked", "flat", "one_finite", "signed_zero", "gauss", "gauss_inf"]
EXEMPT = {
    "all-equal row, V >= 65535": "V tokens of mass 1 / V <= 1.6e-5 each: no setting can pin the draw (test_gpu_sample_edges.py)",
    "T = 100 without top_k, V >= 65535": "a nearly uniform row (test_gpu_sample_edges.py); not generated here",
}
STATS = dict(fraction=0.0, z=0.0, rows=0)


def _row(kind, V, seed):
    """test_gpu_sample_edges.py's row kinds, plus a Gaussian row and one with a third of it at -inf"""
    g = torch.Generator().manual_seed(seed)
    if kind in ("grid", "grid_inf"):
        x = torch.randint(-8, 9, (V,), generator=g).float() * 0.5
        if V >= LARGE:
            x[torch.randperm(V, generator=g)[2048:]] -= 12.0
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
    elif kind == "signed_zero":
        x = -0.5 * torch.randint(1, 17, (V,), generator=g).float()
        top = torch.randperm(V, generator=g)[:max(min(V // 4, 512), 1)]
        x[top] = torch.tensor([-0.0, 0.0])[torch.randint(0, 2, (top.numel(),), generator=g)]
    else:
        x = 2.0 * torch.randn(V, generator=g)
        if kind == "gauss_inf" and V >= 3:
            x[torch.randperm(V, generator=g)[:V // 3]] = -math.inf
    return x


def _us(B, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = (torch.randint(0, 2 ** 24, (12, B), generator=g).float() * 2.0 ** -24)
    return torch.cat([torch.tensor(U_ENDS)[:, None].expand(4, B), rnd], 0).float()


def _shuffled(ref, perm):
    """the reference of row[perm] from the reference of row: the sets and thresholds move with the tokens, the index-order CDF is rebuilt"""
    out = dict(ref)
    for key in ("s", "x", "e", "kept"):
        out[key] = ref[key][perm]
    out["base"] = dict(ref["base"], kept=ref["base"]["kept"][perm])
    out["stages"] = [dict(st, kept=st["kept"][perm], **({"d": st["d"][perm]} if "d" in st else {})) for st in ref["stages"]]
    pr = torch.where(out["kept"], out["e"], torch.zeros_like(out["e"]))
    out["cdf"] = pr.cumsum(0) / ref["Z"]
    return out


def _rebuild(r, info_row):
    """the kept set from the device's info row and the reference's keys: behind every stage that is on, the device's count of tokens with
    the smallest keys of the set before it (d for typical_p, -x for the e floors: the tokens tied at the maximum come first), a group of
    equal keys whole -> bool [V]"""
    counts = dict(min_p=info_row[5], typical_p=info_row[6], epsilon_cutoff=info_row[7], eta_cutoff=info_row[1])
    K = r["base"]["kept"].clone()
    for st in r["stages"]:
        key = st["d"] if st["name"] == "typical_p" else -r["x"]
        c = int(counts[st["name"]])
        if not 1 <= c <= int(K.sum()):
            return torch.zeros_like(K)
        K = K & (key <= key[K].sort().values[c - 1])
    return K


COLD = {"flat": 0.02, "signed_zero": 0.1}


def _setting(name, V, kind):
    """(T, k, p, nominal warpers) of SETTINGS[name]; at V >= 65535 the settings without top-k run at T <= 0.3 (a flat row, whose values spread
    by 0.3 only, and the signed-zero row with its 512-fold tied maximum colder still), where the mass sits in few enough tokens for the 1e-5
    window to leave one candidate (test_gpu_sample_edges.py runs its whole-row settings cold for the same reason)"""
    T, k, p, w = _args(SETTINGS[name])
    if V >= LARGE and k == 0:
        T = COLD.get(kind, 0.3)
    return T, k, p, w


def _plan(base, perms, name, what, exempt=None, kind=None, u_seed=0):
    """the reference side of one case, no GPU: rows = base[perm] for each perm (None: the base row itself) under SETTINGS[name] placed mid-gap
    for the base row -> (x [B, V], T, k, p, placed settings, refs, us [16][B], admissible sets, fraction).  Asserts the case's design."""
    V = base.numel()
    T, k, p, w = _setting(name, V, kind)
    placed = W.place(base, T, k, p, **{a: w.get(a) for a in ("min_p", "typical_p", "eps", "eta")})
    ref0 = W.warp_ref(base, T, k, p, **placed)
    W.assert_margins(ref0, what)
    refs = [ref0 if pm is None else _shuffled(ref0, pm) for pm in perms]
    x = torch.stack([base if pm is None else base[pm] for pm in perms])
    us = _us(len(perms), u_seed + V)
    adm = [[R.admissible_tokens(r, float(us[i, b])) for b, r in enumerate(refs)] for i in range(us.shape[0])]
    frac = sum(int(a.sum()) == 1 for row in adm for a in row) / (us.shape[0] * len(perms))
    assert exempt is None or exempt in EXEMPT, exempt
    if exempt is None:
        assert frac >= 0.75, f"{what}: only {frac:.2f} of the draws have exactly one admissible token (a case-design error)"
    return x, T, k, p, placed, refs, us, adm, frac


def _launch(lib, xd, T, k, p, placed, u=None, seq_rows=0, seq_row=0, n=0, seed=0):
    B, V = xd.shape
    ids = torch.full((B,), -1, device="cuda", dtype=torch.long)
    info = torch.zeros(B, 8, device="cuda")
    L.check(lib.fvhd_op_dec_sample_warpers(L.stream(), L.ptr(xd), B, V, float(T), int(k), float(p), placed["min_p"], placed["typical_p"], placed["eps"],
                                           placed["eta"], int(seed), int(seq_rows), int(seq_row), int(n), L.ptr(u), L.ptr(ids), L.ptr(info)),
            "fvhd_op_dec_sample_warpers")
    torch.cuda.synchronize()
    return ids.cpu(), info.cpu()


def _run(lib, plan, what):
    x, T, k, p, placed, refs, us, adm, frac = plan
    B, V = x.shape
    xd = x.cuda().contiguous()
    all_ids = []
    for i in range(us.shape[0]):
        ut = us[i].cuda().contiguous()
        ids, info = _launch(lib, xd, T, k, p, placed, u=ut)
        if i == 0:
            ids2, info2 = _launch(lib, xd, T, k, p, placed, u=ut)
            assert torch.equal(ids, ids2) and torch.equal(info.view(torch.int32), info2.view(torch.int32)), what + ": two launches differ"
        all_ids.append(ids)
        for b, r in enumerate(refs):
            w = f"{what} {placed} row {b} u={float(us[i, b])!r}"
            got = tuple(int(v) for v in info[b, 5:8].tolist())
            assert got == r["counts"], f"{w}: counts behind min_p / typical_p / epsilon_cutoff {got}, reference {r['counts']}"
            if i == 0:
                assert torch.equal(_rebuild(r, info[b]), r["kept"]), f"{w}: the set rebuilt from the info row's counts and the reference's keys differs"
            assert int(info[b, 1]) == r["count"], f"{w}: kept count {int(info[b, 1])}, reference {r['count']}"
            assert (float(info[b, 0]), float(info[b, 4])) == (r["lo"], r["hi"]), f"{w}: kept s in {info[b, 0]} .. {info[b, 4]}, reference {r['lo']} .. {r['hi']}"
            zerr = abs(float(info[b, 2]) - r["Z"]) / r["Z"]
            assert zerr <= 1e-5, f"{w}: Z {float(info[b, 2])}, reference {r['Z']}"
            assert float(info[b, 3]) == float(us[i, b]), w
            t = int(ids[b])
            assert 0 <= t < V and bool(adm[i][b][t]), f"{w}: token {t} (kept {bool(r['kept'][t])}) is not admissible; admissible {adm[i][b].nonzero()[:8, 0].tolist()}"
            STATS["z"] = max(STATS["z"], zerr / max(r["Ez"] + V * 2.0 ** -24, 1e-30))   # fp32 chunk sums of the draw: + one rounding per add
    STATS["fraction"] = max(STATS["fraction"], W.margin_fraction(refs[0]))
    STATS["rows"] += B
    return torch.stack(all_ids), frac


def _perms(V, B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(V, generator=g) for _ in range(B)]


SHUFFLE_KINDS = ["peaked", "grid_inf", "gauss_inf", "max3"]


def _cases(name, V):
    """every (base row, perms, setting name, what, exempt, kind) of test `name`: one generator, so the design is checked without a GPU too"""
    if name == "shuffles":                                         # B = 16 orders of one row, the kind changing with the setting
        for i, st in enumerate(SETTINGS):
            kind = SHUFFLE_KINDS[i % len(SHUFFLE_KINDS)]
            yield _row(kind, V, 100 + V + i), _perms(V, 16, V + i), st, f"V={V} B=16 {kind} [{st}]", None, kind
    elif name == "single":                                         # B = 1, every kind
        for j, kind in enumerate(KINDS):
            ex = "all-equal row, V >= 65535" if kind == "equal" and V >= LARGE else None
            for st in SETTINGS:
                yield _row(kind, V, 300 + V + j), [None], st, f"V={V} B=1 {kind} [{st}]", ex, kind
    elif name == "wide":                                           # B = 17 and 64: the row blocks of BMAX
        for B in (17, 64):
            for i, st in enumerate(SETTINGS):
                kind = SHUFFLE_KINDS[(i + 1) % len(SHUFFLE_KINDS)]
                yield _row(kind, V, 500 + V + i), _perms(V, B, V + B + i), st, f"V={V} B={B} {kind} [{st}]", None, kind


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import _lib
    return _lib.sampling_warpers_lib()


@pytest.fixture(scope="module", autouse=True)
def _bound_log():
    yield
    if os.environ.get("FVHD_WRITE_PROFILES") == "1" and STATS["rows"]:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "warpers_bound.log")
        with open(path, "w") as f:
            f.write(f"rows checked: {STATS['rows']}\n"
                    f"largest fraction of a row's key-space margin that the derived bound uses: {STATS['fraction']:.4f} (sound below {1 / W.SAFETY})\n"
                    f"largest observed |Z - Z_ref| / Z as a fraction of its bound (Ez + V 2^-24): {STATS['z']:.4f}\n")


@pytest.mark.parametrize("V", VOCABS)
def test_sixteen_shuffles_under_the_nine_settings(lib, V):
    fr = [_run(lib, _plan(b, pm, st, what, ex, kind), what)[1] for b, pm, st, what, ex, kind in _cases("shuffles", V)]
    print(f"V={V} B=16: single-token draw fraction {min(fr):.2f} .. {max(fr):.2f}")


@pytest.mark.parametrize("V", VOCABS)
def test_single_rows_of_every_kind(lib, V):
    fr = [_run(lib, _plan(b, pm, st, what, ex, kind), what)[1] for b, pm, st, what, ex, kind in _cases("single", V)]
    print(f"V={V} B=1: single-token draw fraction {min(fr):.2f} .. {max(fr):.2f}")


@pytest.mark.parametrize("V", [257, 2049, 65537])
def test_row_blocks_of_a_wide_batch(lib, V):
    fr = [_run(lib, _plan(b, pm, st, what, ex, kind), what)[1] for b, pm, st, what, ex, kind in _cases("wide", V)]
    print(f"V={V} B=17 / 64: single-token draw fraction {min(fr):.2f} .. {max(fr):.2f}")


@pytest.mark.parametrize("V", [3, 257, 4096, 152064])
def test_min_p_1_keeps_exactly_a_three_way_tied_maximum(lib, V):
    base = _row("max3", V, 4000 + V)
    x = torch.stack([base[pm] for pm in _perms(V, 16, V)])
    refs = [W.warp_ref(x[b], 1.0, 0, 1.0, min_p=1.0) for b in range(16)]
    placed = dict(W.OFF, min_p=1.0)
    us = _us(16, V)
    ids = []
    for i in range(16):
        got, info = _launch(lib, x.cuda(), 1.0, 0, 1.0, placed, u=us[i].cuda().contiguous())
        ids.append(got)
        assert info[:, 1].tolist() == [3.0] * 16 and info[:, 5:8].tolist() == [[3.0] * 3] * 16
    ids = torch.stack(ids)
    for b, r in enumerate(refs):
        top = r["kept"].nonzero()[:, 0].tolist()
        assert r["count"] == 3 and sorted(set(ids[:, b].tolist())) == top, (b, top, ids[:, b].tolist())


@pytest.mark.parametrize("V", [257, 2049, 65537])
def test_rows_of_one_sequence_equal_single_launches(lib, V):
    """seq_rows: row r of a T-row launch equals the B = 1 launch at n = n0 + r, bit for bit (Philox, no u_override)"""
    T_rows, n0, seed = 16, 37, 0x1234567811
    x = torch.stack([_row(KINDS[(r * 3) % len(KINDS)], V, 900 + V + r) for r in range(T_rows)]).cuda().contiguous()
    for name in ("typical_p behind top-k + top-p", "all seven"):
        T, k, p, w = _args(SETTINGS[name])
        placed = dict(W.OFF, **{a: W.f32(v) for a, v in w.items()})
        ids, info = _launch(lib, x, T, k, p, placed, seq_rows=1, seq_row=0, n=n0, seed=seed)
        for r in range(T_rows):
            i1, f1 = _launch(lib, x[r:r + 1].contiguous(), T, k, p, placed, n=n0 + r, seed=seed)
            assert int(ids[r]) == int(i1[0]) and torch.equal(info[r].view(torch.int32), f1[0].view(torch.int32)), (name, r, info[r], f1[0])


def test_the_off_values_are_the_plain_sampler(lib):
    """all four off: the ids and (theta -> lowest kept s, count, Z, u) of fvhd_op_dec_sample, bit for bit"""
    x = torch.stack([_row(KINDS[b % len(KINDS)], 2049, 70 + b) for b in range(16)]).cuda().contiguous()
    u = _us(16, 5)[7].cuda().contiguous()
    for T, k, p in [(1.0, 0, 1.0), (0.7, 50, 0.9)]:
        ids, info = _launch(lib, x, T, k, p, dict(W.OFF), u=u)
        ids0, info0 = L.sample(lib, x, T, k, p, u=u)
        assert torch.equal(ids, ids0.cpu()) and torch.equal(info[:, 1:4].contiguous().view(torch.int32), info0.cpu()[:, 1:4].contiguous().view(torch.int32))


def test_refusals(lib):
    x = torch.zeros(1, 8, device="cuda")
    for bad, word in [(dict(min_p=1.5), "min_p"), (dict(min_p=-0.1), "min_p"), (dict(typical_p=0.0), "typical_p"), (dict(typical_p=1.5), "typical_p"),
                      (dict(eps=1.0), "epsilon_cutoff"), (dict(eta=-1.0), "eta_cutoff"), (dict(eta=float("nan")), "eta_cutoff")]:
        with pytest.raises(Exception, match=word):
            _launch(lib, x, 1.0, 0, 1.0, dict(W.OFF, **bad))
