"""fp64 reference of the sampler's warpers behind top-p (csrc/llm_sample.hip; include/fvhd.h "LLM sampling"): min_p, typical_p,
epsilon_cutoff, eta_cutoff in transformers' order, each on the set K the earlier stages left.  Pinned to transformers' own warpers on
float64 scores by tests/test_warper_reference.py.

With s = fp32(logits) / fp32(T) (decode_reference.sample_ref), M = max s, x = s - M, e = exp(x), Z = sum of e over K, A = sum of e x over K / Z:
  min_p            keeps e >= min_p                         (p >= min_p p_max: Z cancels)
  typical_p = t    keeps the tokens of smallest d = |x - A| (= |-log p - H|: log Z cancels) until the mass reaches t Z: a group of equal d is
                   kept iff the mass of the groups before it is < t Z, the first group always
  epsilon_cutoff   keeps e >= eps Z, and the tokens tied at the largest s of K
  eta_cutoff       the same with eta = min(eps, sqrt(eps) exp(-H)), H = log Z - A

MARGINS.  A test may ask the device for the reference's kept set only where no token lies closer to a stage's threshold than the device's
own rounding can move it; every stage therefore reports
  mass   (typical_p) the smallest |mass before a group / Z - t| over the groups behind the first: the bound is the sampler tests' GAP = 1e-5;
  key    the distance of the threshold to the nearest token in key space - for the e floors (min_p, the cutoffs) in log space,
         |x_i - log floor|, a relative distance; for typical_p in d, the gap between d* and the nearest other value of d on either side
         (a token just inside d* matters as much as one just outside: if the two swap, the inner one is measured against the other's mass);
  bound  what `key` must exceed, derived from the kernel's order of operations (u = 2^-24, the fp32 unit roundoff):
    e_i = expf(fl(s_i - M)): the subtraction moves the exponent by <= |x| u, which is a relative |x| u on e; expf is within 2 ulp; with the
         fp32 rounding of the compared constant:                                       E(x) = (|x| + 4) u
    Z    a sum of trunc(e 2^40) words, exact in integers: relative                      Ez = sum p_i E(x_i) + N 2^-40 / Z
    A    sum of trunc(fl(e x) 2^40) / Z: absolute                                       Ea = sum p_i |x_i| (E(x_i) + u) + N 2^-40 / Z + |A| Ez
    min_p                      fl(e) against fp32 min_p:                                E(log min_p)
    epsilon_cutoff             fl(e) against fl(eps Z):                                 E(log floor) + Ez
    eta_cutoff                 and H = log Z - A in fp64 from those Z and A:            E(log floor) + 2 Ez + Ea
    typical_p                  d = |fl(fl(s - M) - fl(A))|, two tokens compared:        2 (u (|x| + |A| + d) + Ea) at x = the nearer token
  A case is sound when key >= 2 * bound (SAFETY) and mass >= GAP; `assert_margins` checks that on the reference alone."""
import math

import torch

import decode_reference as R

U = 2.0 ** -24
GAP = 1e-5
SAFETY = 2.0
OFF = dict(min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0)
STAGES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")
# the nine settings of the tests: each warper alone, each behind top-k + top-p, and all seven together (T 1, k 0, p 1 where not given)
SETTINGS = {
    "min_p": dict(min_p=0.05),
    "typical_p": dict(typical_p=0.9),
    "epsilon_cutoff": dict(eps=3e-4),
    "eta_cutoff": dict(eta=2e-3),
    "min_p behind top-k + top-p": dict(k=50, p=0.95, min_p=0.02),
    "typical_p behind top-k + top-p": dict(k=50, p=0.95, typical_p=0.8),
    "epsilon_cutoff behind top-k + top-p": dict(k=50, p=0.95, eps=1e-3),
    "eta_cutoff behind top-k + top-p": dict(k=50, p=0.95, eta=5e-3),
    "all seven": dict(T=0.8, k=60, p=0.97, min_p=0.001, typical_p=0.92, eps=1e-4, eta=1e-3),
}


def setting_args(st):
    """a SETTINGS entry -> (T, k, p, the warpers that are on)"""
    st = dict(st)
    return st.pop("T", 1.0), st.pop("k", 0), st.pop("p", 1.0), st


def f32(v):
    """the value the C ABI receives for a float argument"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _E(x):
    return (abs(x) + 4.0) * U


def _stats(x, e, K):
    """Z, A, and the error terms Ez, Ea of the set K"""
    ek, xk = e[K], x[K]
    Z = float(ek.sum())
    ex = ek * xk
    A = float(ex.sum()) / Z
    n = int(K.sum())
    p = ek / Z
    Ez = float((p * (xk.abs() + 4.0) * U).sum()) + n * 2.0 ** -40 / Z
    Ea = float((p * xk.abs() * ((xk.abs() + 4.0) * U + U)).sum()) + n * 2.0 ** -40 / Z + abs(A) * Ez
    return Z, A, Ez, Ea


def _floor_stage(name, x, e, s, K, floor, keep_top, bound_extra):
    """an e floor: keeps e >= floor (and with keep_top the tokens at the largest s of K)"""
    top = s == s[K].max() if keep_top else torch.zeros_like(K)
    kept = K & ((e >= floor) | top)
    if not bool(kept.any()):                                      # min_tokens_to_keep = 1 (min_p = 1 + rounding cannot do this: e_max = 1)
        kept = K & (s == s[K].max())
    near = K & ~top
    lf = math.log(floor) if floor > 0 else -math.inf
    key = float((x[near] - lf).abs().min()) if bool(near.any()) and floor > 0 else math.inf
    return dict(name=name, kept=kept, count=int(kept.sum()), Z=float(e[kept].sum()), threshold=floor, mass=math.inf, key=key,
                bound=_E(lf) + bound_extra if floor > 0 else 0.0)


def warp_ref(logits, T, k, p, min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0):
    """one row -> dict: s (fp32), x, e (fp64), `stages` = the list of the stages that are on, in order, each with name, kept (bool [V]), count, Z,
    threshold (the e floor, or d*), mass / key / bound (see the module text), typical_p also A and d; and of the final set: kept, count, Z,
    cdf (index order), lo / hi (lowest / highest kept s), counts = (behind min_p, behind typical_p, behind epsilon_cutoff)"""
    min_p, typical_p, eps, eta = f32(min_p), f32(typical_p), f32(eps), f32(eta)
    base = R.sample_ref(logits, T, k, f32(p))
    s = base["s"]
    sd = s.double()
    M = sd[sd > -math.inf].max()
    x = sd - M
    e = torch.exp(x)
    K = base["kept"].clone()
    stages = []
    if min_p > 0.0:
        stages.append(_floor_stage("min_p", x, e, sd, K, min_p, False, 0.0))
        K = stages[-1]["kept"]
    c_minp = int(K.sum())
    if typical_p < 1.0:
        Z, A, Ez, Ea = _stats(x, e, K)
        d = (x - A).abs()
        vals, inv = torch.unique(d[K], return_inverse=True)       # ascending
        mass = torch.zeros_like(vals).index_add_(0, inv, e[K])
        before = mass.cumsum(0) - mass
        keep_g = before < typical_p * Z
        keep_g[0] = True
        g = int(keep_g.nonzero().max())
        dstar = float(vals[g])
        kept = K & (d <= dstar)
        gaps = [float(vals[g + 1] - vals[g])] if g + 1 < vals.numel() else []
        gaps += [float(vals[g] - vals[g - 1])] if g > 0 else []
        xn = float(x[K][(d[K] - dstar).abs().argmin()].abs())
        stages.append(dict(name="typical_p", kept=kept, count=int(kept.sum()), Z=float(e[kept].sum()), threshold=dstar, A=A, d=d,
                           mass=float((before[1:] / Z - typical_p).abs().min()) if vals.numel() > 1 else math.inf,
                           key=min(gaps) if gaps else math.inf, bound=2.0 * (U * (xn + abs(A) + dstar) + Ea)))
        K = kept
    c_typ = int(K.sum())
    if eps > 0.0:
        Z, A, Ez, Ea = _stats(x, e, K)
        stages.append(_floor_stage("epsilon_cutoff", x, e, sd, K, eps * Z, True, Ez))
        K = stages[-1]["kept"]
    c_eps = int(K.sum())
    if eta > 0.0:
        Z, A, Ez, Ea = _stats(x, e, K)
        H = math.log(Z) - A
        stages.append(_floor_stage("eta_cutoff", x, e, sd, K, min(eta, math.sqrt(eta) * math.exp(-H)) * Z, True, 2.0 * Ez + Ea))
        stages[-1]["H"] = H
        K = stages[-1]["kept"]
    pr = torch.where(K, e, torch.zeros_like(e))
    Z = float(pr.sum())
    return dict(s=s, x=x, e=e, stages=stages, kept=K, count=int(K.sum()), Z=Z, cdf=pr.cumsum(0) / Z, lo=float(s[K].min()), hi=float(s[K].max()),
                counts=(c_minp, c_typ, c_eps), base=base, Ez=_stats(x, e, K)[2])


def assert_margins(ref, what=""):
    """the case-design condition, from the reference alone: no token within reach of a threshold (see the module text)"""
    if ref["base"]["margin"] < GAP:
        raise AssertionError(f"{what}: a top-p group boundary within {ref['base']['margin']:.2g} of top_p (a case-design error)")
    for st in ref["stages"]:
        if st["mass"] < GAP:
            raise AssertionError(f"{what}: {st['name']}: a group boundary within {st['mass']:.2g} of the mass threshold (a case-design error)")
        if st["key"] < SAFETY * st["bound"]:
            raise AssertionError(f"{what}: {st['name']}: a token within {st['key']:.3g} of the threshold in key space, the bound is "
                                 f"{SAFETY} * {st['bound']:.3g} (a case-design error)")


def margin_fraction(ref):
    """the largest bound / key over the stages of a row: how much of its key-space margin the derived bound uses (<= 1 / SAFETY when sound)"""
    return max([st["bound"] / st["key"] for st in ref["stages"] if st["key"] > 0 and st["key"] < math.inf] + [0.0])


# ---- settings placed mid-gap, so that a case has its margins by construction -------------------------------------------------------------
def _mid_floor(x, K, top_excluded, want_log):
    """log of an e floor half-way between two adjacent distinct values of x over K, the pair nearest to want_log among those whose gap is
    widest enough; -> log floor"""
    v = torch.unique(x[K & ~top_excluded]) if bool((K & ~top_excluded).any()) else torch.empty(0, dtype=torch.float64)
    if v.numel() < 2:
        return want_log
    mids, gaps = (v[1:] + v[:-1]) / 2, v[1:] - v[:-1]
    ok = gaps >= 64.0 * (mids.abs() + 64.0) * U                   # generous against every floor bound above
    if not bool(ok.any()):
        return want_log
    mids = mids[ok]
    return float(mids[(mids - want_log).abs().argmin()])


def place(logits, T, k, p, min_p=None, typical_p=None, eps=None, eta=None):
    """nominal settings (None = off) -> the four settings moved mid-gap for THIS row: each e floor half-way (in log space) between two
    adjacent values of the set it acts on, typical_p half-way through the mass of a group with clear neighbours in d; as fp32 values.
    The result still has to pass assert_margins: this only makes that likely."""
    out = dict(OFF)
    cur = lambda: warp_ref(logits, T, k, p, **out)                # noqa: E731
    if min_p is not None:
        r = cur()
        out["min_p"] = min(1.0, f32(math.exp(_mid_floor(r["x"], r["kept"], torch.zeros_like(r["kept"]), math.log(min_p)))))
    if typical_p is not None:
        r = cur()
        K, x, e = r["kept"], r["x"], r["e"]
        Z, A, Ez, Ea = _stats(x, e, K)
        d = (x - A).abs()
        vals, inv = torch.unique(d[K], return_inverse=True)
        mass = torch.zeros_like(vals).index_add_(0, inv, e[K]) / Z
        before = mass.cumsum(0) - mass
        gap = torch.full_like(vals, math.inf)
        if vals.numel() > 1:
            dv = vals[1:] - vals[:-1]
            gap[:-1] = dv
            gap[1:] = torch.minimum(gap[1:], dv)
        need = 8.0 * (U * (2.0 * x[K].abs().max() + 2.0 * abs(A)) + Ea)
        ok = (gap >= need) & (mass >= 4.0 * GAP)
        t = typical_p
        if bool(ok.any()):
            mid = (before + mass / 2)[ok]
            t = float(mid[(mid - typical_p).abs().argmin()])
        out["typical_p"] = min(f32(t), 1.0 - 2.0 ** -24)
    if eps is not None:
        r = cur()
        K = r["kept"]
        Z = float(r["e"][K].sum())
        top = r["s"].double() == r["s"].double()[K].max()
        out["eps"] = min(f32(math.exp(_mid_floor(r["x"], K, top, math.log(eps * Z))) / Z), 1.0 - 2.0 ** -24)
    if eta is not None:
        r = cur()
        K = r["kept"]
        Z, A, Ez, Ea = _stats(r["x"], r["e"], K)
        H = math.log(Z) - A
        top = r["s"].double() == r["s"].double()[K].max()
        want = min(eta, math.sqrt(eta) * math.exp(-H))
        et = math.exp(_mid_floor(r["x"], K, top, math.log(want * Z))) / Z          # the eta to reach; invert eta = min(eps, sqrt(eps) exp(-H))
        out["eta"] = min(f32(et if et <= math.exp(-2.0 * H) else (et * math.exp(H)) ** 2), 1.0 - 2.0 ** -24)
    return out


# ---- transformers' own warpers, for the pins --------------------------------------------------------------------------------------------
def oracle_kept(logits, T, k, p, min_p=0.0, typical_p=1.0, eps=0.0, eta=0.0, dtype=torch.float64):
    """transformers' seven warpers in _get_logits_processor's order on s = fp32(logits) / fp32(T) cast to `dtype` -> kept bool [V]"""
    from transformers.generation import logits_process as LP
    s = (logits.detach().float().cpu() / torch.tensor(float(T), dtype=torch.float32)).to(dtype)[None]
    if k > 0:
        s = LP.TopKLogitsWarper(int(k))(None, s)
    if p < 1.0:
        s = LP.TopPLogitsWarper(f32(p))(None, s)
    if min_p > 0.0:
        s = LP.MinPLogitsWarper(f32(min_p))(None, s)
    if typical_p < 1.0:
        s = LP.TypicalLogitsWarper(f32(typical_p))(None, s)
    if eps > 0.0:
        s = LP.EpsilonLogitsWarper(f32(eps))(None, s)
    if eta > 0.0:
        s = LP.EtaLogitsWarper(f32(eta), device="cpu")(None, s)
    return s[0] > -math.inf
