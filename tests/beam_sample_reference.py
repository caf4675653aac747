"""The fp64 reference of beam-search sampling (include/fvhd.h "LLM beam-search sampling"): the kept set behind temperature / top-k / top-p with
min_tokens_to_keep = m, the accumulated scores a, the Gumbel noise g from the Python Philox, and the selection of the `keep` kept
candidates with the largest a + g per prompt.  Plain torch on the device of its inputs, the Philox words from numpy on the CPU;
tests/test_beam_sample_reference.py pins it against transformers' own warpers and `_get_top_k_continuations`, the GPU tests compare the
kernels with it."""
import numpy as np
import torch

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10_np(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over numpy arrays of counters (uint64 holding 32-bit words; they broadcast) -> four uint64 arrays of 32-bit words"""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & _MASK for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    sh = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2            # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & _MASK, (p0 >> sh) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return c0, c1, c2, c3


def gumbel_words(seed: int, rows: int, n: int, V: int) -> np.ndarray:
    """uint64 [rows, V]: token v of row r takes word v & 3 of the counter (r, n, v >> 2, 1), key = the seed's two words"""
    assert V % 4 == 0
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = np.arange(rows, dtype=np.uint64)[:, None]
    q = np.arange(V // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10_np(r, np.uint64(n), q, np.uint64(1), seed, seed >> 32)
    return np.stack(w, axis=-1).reshape(rows, V)


def gumbel_uniform(words: np.ndarray) -> np.ndarray:
    """u = (2 (w >> 9) + 1) 2^-24: 24 significant bits, exact in fp32, inside (0, 1)"""
    return (2.0 * (words >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def gumbel_of_uniform(u: np.ndarray) -> np.ndarray:
    """g = -log(-log u) in fp64 (log1p near 1, where log u = log1p(u - 1) with u - 1 exact)"""
    u = np.asarray(u, dtype=np.float64)
    return -np.log(-np.where(u > 0.5, np.log1p(u - 1.0), np.log(u)))


def gumbel_noise(seed: int, rows: int, n: int, V: int, device="cpu") -> torch.Tensor:
    """fp64 [rows, V] on `device`: every candidate's g (the words from numpy; u and the logarithms in torch fp64 on the device)"""
    w = torch.from_numpy((gumbel_words(seed, rows, n, V) >> np.uint64(9)).astype(np.int64)).to(device)
    u = (2.0 * w.double() + 1.0) * 2.0 ** -24
    return -torch.log(-torch.where(u > 0.5, torch.log1p(u - 1.0), torch.log(u)))


def scaled_fp32(logits: torch.Tensor, temperature: float) -> torch.Tensor:
    """s = x / T as the device takes it: IEEE fp32 division by the fp32 temperature -> fp64 [rows, V] of fp32 values"""
    # on the host: there the division by a 0-dim tensor is the IEEE division (on the GPU torch may multiply by the reciprocal: one ulp)
    return (logits.float().cpu() / torch.tensor(temperature, dtype=torch.float32)).double().to(logits.device)


def kept_set(s: torch.Tensor, top_k: int, top_p: float, m: int):
    """s fp64 [rows, V] (the scaled logits; -inf = suppressed) -> (kept bool [rows, V], theta fp64 [rows]): the kept set is
    {s >= theta, s > -inf} with theta = max(theta_k', min(theta_p, v_m)) -
      theta_k' the max(top_k, m)-th largest s; off (-inf) at top_k = 0 and where max(top_k, m) >= V (it keeps everything);
      theta_p  the lowest s top-p keeps among the top-k survivors: a token stays when the normalised mass above it is < top_p, tokens of equal
               s as a group; off (-inf) at top_p = 1;
      v_m      the m-th largest s.
    theta is -inf where no filter binds."""
    R, V = s.shape
    dev = s.device
    neg = torch.full((R,), float("-inf"), dtype=torch.float64, device=dev)
    k = max(int(top_k), m) if top_k > 0 else 0
    if 0 < k < V:                                                 # only the top k matter: no full sort of a wide row
        desc = torch.topk(s, k, dim=-1).values
        theta_k = desc[:, k - 1].clone()
    else:
        desc = torch.sort(s, dim=-1, descending=True).values if top_p < 1.0 else torch.topk(s, m, dim=-1).values
        theta_k = neg.clone()
    v_m = desc[:, m - 1]
    theta_p = neg.clone()
    if top_p < 1.0:
        for r in range(R):
            row = desc[r][(desc[r] >= theta_k[r]) & (desc[r] > float("-inf"))]      # the top-k survivors, descending
            if row.numel() == 0:
                continue
            e = torch.exp(row - row[0])
            above = torch.cumsum(e, 0) - e                                           # the mass strictly before each token ...
            first = torch.cat((torch.ones(1, dtype=torch.bool, device=dev), row[1:] != row[:-1]))
            pos = torch.arange(row.numel(), device=dev)
            group = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), 0).values
            above = above[group]                                                     # ... of its group of equal s
            ok = (above < top_p * e.sum()) | (above == 0)
            theta_p[r] = row[ok][-1]
    theta = torch.maximum(theta_k, torch.minimum(theta_p, v_m)) if top_p < 1.0 else theta_k
    kept = (s >= theta[:, None]) & (s > float("-inf"))
    return kept, theta


def scores(logits: torch.Tensor, temperature: float, beam_scores: torch.Tensor) -> torch.Tensor:
    """a fp64 [rows, V] = log_softmax(x) / T + score of the row (T: the fp32 temperature)"""
    T = float(torch.tensor(temperature, dtype=torch.float32))
    return torch.log_softmax(logits.double(), dim=-1) / T + beam_scores.double().to(logits.device).reshape(-1, 1)


def select(a: torch.Tensor, g: torch.Tensor, kept: torch.Tensor, G: int, K: int, keep: int, extra: int = 0):
    """per prompt the keep (+ extra) kept candidates with the largest a + g, in descending a + g, equal keys by ascending flat index ->
    (a of the picks fp64 [G, n], flat indices k V + v int64 [G, n], keys a + g fp64 [G, n]); a slot that cannot be filled: (-inf, 0, -inf)"""
    V = a.shape[1]
    n = keep + extra
    key = torch.where(kept, a + g, torch.full_like(a, float("-inf"))).view(G, K * V)
    # the lower flat index first among equal keys: the n best values, then every candidate at or above the n-th in (-key, index) order
    nth = torch.topk(key, n, dim=-1).values[:, -1:]
    order = torch.zeros((G, n), dtype=torch.long, device=a.device)
    for g_ in range(G):
        cand = (key[g_] >= nth[g_]).nonzero().flatten()
        o = torch.sort(key[g_][cand], descending=True, stable=True).indices      # cand ascends: stable keeps the lower index first
        order[g_] = cand[o][:n]
    kk = torch.gather(key, 1, order)
    ok = torch.gather(kept.view(G, K * V), 1, order)
    av = torch.where(ok, torch.gather(a.view(G, K * V), 1, order), torch.full_like(kk, float("-inf")))
    return av, torch.where(ok, order, torch.zeros_like(order)), torch.where(ok, kk, torch.full_like(kk, float("-inf")))


def reference(logits, beam_scores, G, K, keep, temperature, top_k, top_p, m, seed=0, n=0, noise=None, extra=0):
    """the whole step on fp32 logits [G K, V] and scores [G, K] -> dict(a, g, s, logp, kept, theta, count, scores, index, keys)"""
    s = scaled_fp32(logits, temperature)
    kept, theta = kept_set(s, top_k, top_p, m)
    a = scores(logits, temperature, beam_scores)
    g = gumbel_noise(seed, G * K, n, logits.shape[1], logits.device) if noise is None else noise.double().to(logits.device)
    av, idx, keys = select(a, g, kept, G, K, keep, extra)
    return dict(a=a, g=g, s=s, kept=kept, theta=theta, count=kept.sum(-1), scores=av, index=idx, keys=keys,
                logp=torch.log_softmax(logits.double(), dim=-1))


# ---- the inputs of the GPU selection tests, their seeds (tools/beam_sample_margins.py) and the bound on a + g ---------------------------------
SCALES = (0.05, 1.0, 8.0)                                         # row r is N(0, 1) * SCALES[r % 3]: rows of very different scale side by side


def inputs(V: int, G: int, K: int, seed: int):
    """fp32 logits [G K, V] with about 1 % of -inf entries and beam scores [G, K] in (-2, 0], from the CPU generator"""
    g = torch.Generator().manual_seed(seed)
    rows = G * K
    x = torch.randn(rows, V, generator=g) * torch.tensor([SCALES[r % 3] for r in range(rows)])[:, None]
    x[torch.rand(rows, V, generator=g) < 0.01] = float("-inf")
    return x, -2.0 * torch.rand(G, K, generator=g)


def smallest_gap(keys: torch.Tensor) -> float:
    """the smallest adjacent gap among the finite keys of every prompt (keys [G, n] descending; a prompt with fewer than n kept candidates
    ends in -inf slots, which compete with nothing) -> inf when no prompt has two"""
    d = keys[:, :-1] - keys[:, 1:]
    d = d[torch.isfinite(keys[:, 1:])]
    return float(d.min()) if d.numel() else float("inf")


EPS = 2.0 ** -24                                                  # fp32 unit roundoff
ULPS_LOG = 3                                                      # the accuracy OpenCL asks of log (3 ulp; log1p: 2 ulp), which the device library's logf / log1pf meet
DELTA_L = 1.2e-5                                                  # |L_device - L|, see `bound`


def bound(ref: dict, temperature: float):
    """-> (bound on |device key - exact a + g|, bound on |device a - exact a|) over the reference's picks (keep + extra of them per prompt).
    From the kernel's order of operations, eps = 2^-24, magnitudes taken over those picks:
      g:   u is exact.  t = -log u by logf below 1/2 and by log1pf(u - 1) above (u - 1 exact), relative error <= 3 ulp = 3 * 2^-23 either
           way - plain logf(u) would have an ABSOLUTE error of an ulp of u near 1, which is a relative error of up to 1/2 in t = 2^-24.  g = -logf(t):
           the relative error of t moves g by 3 * 2^-23, its own rounding by 3 ulp(g):  dg <= 3 * 2^-23 (1 + |g|).
      L:   sum exp(x - M) over a row = per thread 16 terms in order, a 6-level shuffle tree, 4 waves, up to 64 slices each rescaled by
           expf(m_slice - M): <= 90 roundings, 5.4e-6 relative, + expf's own 2 ulp and its argument's rounding (|x - m| eps, the terms that
           count have |x - m| <= 20: 1.2e-6) ~ 8e-6 relative; logf: 3 ulp of L <= log 262144 = 12.5: 2.9e-6.  dL <= 1.2e-5.
      a:   ((x - M) - L) / T + score: the two subtractions round at <= |logp| eps each, dL enters undivided, the division rounds at
           |logp| / T eps, the addition at |a| eps:  da <= (dL + 3 eps |logp|) / T + eps |a|.
      key: the prompt's stage takes fl(a + g):  da + dg + eps |a + g|.  A row's stages take fl(fl(x / T) + g), which orders the row as a + g
           does up to  eps |s| + eps |s + g| + dg  (the row constant score - (M + L) / T drops out of a comparison within a row).
    A candidate outside the picks has larger magnitudes only as it lies further below them: its error grows by a few eps per unit of distance,
    so it cannot cross a gap of 2 * bound that the picks keep among themselves."""
    T = float(torch.tensor(temperature, dtype=torch.float32))
    idx, ok = ref["index"], torch.isfinite(ref["keys"])
    G = idx.shape[0]
    flat = lambda t: torch.gather(t.reshape(G, -1), 1, idx)[ok].abs().max().item()       # noqa: E731
    a, g, s = flat(ref["a"]), flat(ref["g"]), flat(ref["s"])
    sg, ag = flat(ref["s"] + ref["g"]), flat(ref["a"] + ref["g"])
    logp = flat(ref["logp"])
    dg = ULPS_LOG * 2.0 ** -23 * (1.0 + g)
    da = (DELTA_L + 3 * EPS * logp) / T + EPS * a
    return max(da + dg + EPS * ag, EPS * s + EPS * sg + dg), da
