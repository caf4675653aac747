"""TEST INFRASTRUCTURE ONLY - plain torch fp64 restatements of the prefill's single operations (csrc/llm.hip: RMSNorm, rotary embedding,
causal grouped-query attention) on the bf16-rounded operands, written from oracle/qwen2_oracle.py (itself pinned to `transformers`), not
from the kernels; a CPU model of the attention kernel's arithmetic (`flash_model`) that only serves to show that the inputs the GPU tests
use leave room under their bound; the input families of those tests; and the comparison / sentinel-guard helpers of tests/llm_testlib.py.

PINNING: tests/test_prefill_reference.py checks every *_ref here against oracle.qwen2_oracle in fp32 (<= 1e-5) and the headroom of every
input family under the GPU tests' bound (flash_model's err / bound <= 0.5, census <= 2^-7)."""
from __future__ import annotations

import math

import torch

from oracle import qwen2_oracle as Q

# the comparison (rms PER ROW) and sentinel-guard helpers, shared with the decode tests: re-exported for this module's two users
from llm_testlib import SENT, close as _close, guard_intact, guarded, same_bits, violations as _violations  # noqa: F401

KT = 64                        # key tile of llm_attention_kernel


# ---- the operations in fp64 --------------------------------------------------------------------------------------------------------------
def rmsnorm_ref(x, w, eps):
    """Qwen2RMSNorm as oracle.qwen2_oracle.rmsnorm states it, statistics and scaling in fp64"""
    return Q.rmsnorm(x.double(), w.double(), eps)


def rope_ref(qkv, pos, nh, nkv, hd, theta):
    """packed rows qkv [M, (nh + 2 nkv) * hd], pos int64 [M] -> fp64 [M, nh + 2 nkv, hd]: apply_rotary_pos_emb on the q and k heads, the v
    heads as they are.  cos / sin: oracle.qwen2_oracle.rope_cos_sin on the CPU (fp32 angles, as Qwen2RotaryEmbedding), the rotation in fp64"""
    M = qkv.shape[0]
    x = qkv.double().view(M, nh + 2 * nkv, hd)
    cos, sin = Q.rope_cos_sin(pos.view(1, M).cpu(), hd, theta)
    cos, sin = cos[0].double().to(qkv.device)[:, None], sin[0].double().to(qkv.device)[:, None]
    qk = x[:, :nh + nkv]
    return torch.cat([qk * cos + Q.rotate_half(qk) * sin, x[:, nh + nkv:]], 1)


def split_heads(qkv, B, T, nh, nkv, hd):
    """packed rows [B*T, (nh + 2 nkv) * hd] -> q [B, nh, T, hd], k, v [B, nkv, T, hd] (views)"""
    x = qkv.view(B, T, nh + 2 * nkv, hd)
    return x[:, :, :nh].transpose(1, 2), x[:, :, nh:nh + nkv].transpose(1, 2), x[:, :, nh + nkv:].transpose(1, 2)


def _allow(B, T, key_valid, device):
    allow = torch.tril(torch.ones(T, T, dtype=torch.bool, device=device))[None].expand(B, T, T)
    if key_valid is not None:
        allow = allow & (key_valid != 0)[:, None, :]
    return allow                                                   # [B, query, key]


def attention_ref(q, k, v, key_valid=None):
    """oracle.qwen2_oracle.attention in fp64: q [B, nh, T, hd], k / v [B, nkv, T, hd], key_valid [B, T] or None ->
    (out [B, T, nh, hd] fp64, empty [B, T] bool).  Key j is visible to query t iff j <= t and key_valid[b, j]; head h reads kv head
    h / (nh / nkv) (repeat_kv).  A query with no visible key (empty[b, t]) returns ZEROS - the library's contract for such rows."""
    B, nh, T, hd = q.shape
    rep = nh // k.shape[1]
    k, v = k.double().repeat_interleave(rep, 1), v.double().repeat_interleave(rep, 1)
    allow = _allow(B, T, key_valid, q.device)
    empty = ~allow.any(-1)
    s = (q.double() @ k.transpose(-1, -2)) * hd ** -0.5
    s = s.masked_fill(~allow[:, None], -math.inf)
    s = torch.where(empty[:, None, :, None], torch.zeros_like(s), s)          # placeholder scores: the row is zeroed below
    out = (torch.softmax(s, -1) @ v).transpose(1, 2)
    out = torch.where(empty[:, :, None, None], torch.zeros_like(out), out)
    return out, empty


def flash_model(q, k, v, key_valid=None):
    """A CPU model of llm_attention_kernel's ARITHMETIC (not a reference): 64-key tiles, fp32 scores, a running maximum with the
    rescale of the accumulators, P = exp2 rounded to bf16, the denominator summed from the ROUNDED P, fp32 accumulation, ONE rounding of
    O / l to bf16.  -> [B, T, nh, hd] bf16.  It shows that the inputs of the GPU tests leave room under their bound."""
    B, nh, T, hd = q.shape
    rep = nh // k.shape[1]
    qf = q.float()
    kf, vf = k.float().repeat_interleave(rep, 1), v.float().repeat_interleave(rep, 1)
    allow = _allow(B, T, key_valid, q.device)[:, None]
    c = hd ** -0.5 * 1.4426950408889634
    m = torch.full((B, nh, T), -1e30)
    l = torch.zeros(B, nh, T)
    o = torch.zeros(B, nh, T, hd)
    for t0 in range(0, T, KT):
        t1 = min(T, t0 + KT)
        s = qf @ kf[:, :, t0:t1].transpose(-1, -2)
        s = torch.where(allow[..., t0:t1], s, torch.full_like(s, -1e30))
        m_new = torch.maximum(m, s.amax(-1))
        m_ref = torch.where(m_new <= -1e29, torch.zeros_like(m_new), m_new)
        alpha = torch.where(m <= -1e29, torch.zeros_like(m), torch.exp2((m - m_ref) * c))
        p = torch.exp2(s * c - (m_ref * c)[..., None]).to(torch.bfloat16).float()
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p @ vf[:, :, t0:t1]
        m = m_new
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return (o * inv[..., None]).to(torch.bfloat16).transpose(1, 2)


# ---- the input families of tests/test_gpu_prefill_ops.py (and of the headroom check on the CPU) ------------------------------------------
ATT_RTOL = ATT_RMS = 2e-2      # the project's attention budget (P is rounded to bf16 for the PV MFMA), applied per (b, t, head) row
# family(): "plain", "qscale", "ascending", "descending", "planted", "holes", "left", "right", "census"


def planted_keys(T):
    """the planted winner's position per sequence: first tile, a middle tile, the diagonal tile of the last full-tile queries, the last
    query's own position"""
    nt = (T + KT - 1) // KT
    return [min(5, T - 1), min(KT * (nt // 2) + 33, T - 1), min(KT * (max(T - 2, 0) // KT) + 8, T - 1), T - 1]


def padding_counts(T):
    return [n for n in (1, 63, 64, 65, 128, 129, T - 1) if 0 < n < T]


def hole_masks(T, g, device):
    """[4, T] uint8: the whole key tile 64..127 invalid; half of all keys invalid at random; both; the tile 128..191 and key 0 invalid"""
    m = torch.ones(4, T, dtype=torch.uint8, device=device)
    m[0, 64:128] = 0
    m[1] = (torch.rand(T, device=device, generator=g) < 0.5).to(torch.uint8)
    m[2] = (torch.rand(T, device=device, generator=g) < 0.5).to(torch.uint8)
    m[2, 64:128] = 0
    m[3, 128:192] = 0
    m[3, 0] = 0
    return m


def family(name, B, T, nh, nkv, hd, seed, device="cpu", pad=None):
    """-> (qkv [B*T, (nh + 2 nkv) * hd] bf16 packed rows, key_valid uint8 [B, T] or None).  "planted" and "holes" need B = 4 (one form
    per sequence); pad: the padding count of every sequence of "left" / "right" (default: padding_counts(T) in turn)."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)
    q, k, v = rn(B, T, nh, hd), rn(B, T, nkv, hd), rn(B, T, nkv, hd)
    kvalid = None
    if name in ("qscale", "planted", "holes", "left", "right"):
        # q rows of distinct scale 0.05 .. 8 (at 8 the scores have std 8: a peaked softmax); v of distinct scale per kv head (x 4 each)
        # and per key (1 .. 2.5): a query head that read another kv head's values, or another key's, is far outside the bound
        n = B * T
        fac = torch.logspace(math.log10(0.05), math.log10(8.0), n, device=device) if n > 1 else torch.tensor([8.0], device=device)
        if name != "planted":
            q = q * fac[torch.randperm(n, device=device, generator=g)].view(B, T, 1, 1)
        v = v * (4.0 ** torch.arange(nkv, device=device)).view(1, 1, nkv, 1) * (1 + (torch.arange(T, device=device) % 7) / 4.0).view(1, T, 1, 1)
    if name in ("ascending", "descending", "planted"):
        u = torch.where(torch.rand(hd, device=device, generator=g) < 0.5, -1.0, 1.0)
        if name == "planted":                                     # key j 60 logits above the others for every query of the sequence
            assert B == 4
            for b, j in enumerate(planted_keys(T)):
                k[b, j] += 60.0 / math.sqrt(hd) * u
        else:                                                     # 40 logits along the sequence: ~10 per key tile at T = 257
            ramp = torch.arange(T, device=device, dtype=torch.float32) / T
            if name == "descending":
                ramp = 1.0 - ramp
            k = k + (ramp * 40.0 / math.sqrt(hd)).view(1, T, 1, 1) * u
        q = q + u
    if name == "holes":
        assert B == 4
        kvalid = hole_masks(T, g, device)
    if name in ("left", "right"):
        counts = list(pad) if pad is not None else padding_counts(T)
        kvalid = torch.ones(B, T, dtype=torch.uint8, device=device)
        for b in range(B):
            n = counts[b % len(counts)]
            if name == "left":
                kvalid[b, :n] = 0
            else:
                kvalid[b, T - n:] = 0
    if name == "census":                                          # q = 0: P = 1 for every visible key; v[j] = e_{j mod hd}
        q = torch.zeros_like(q)
        v = torch.zeros_like(v)
        j = torch.arange(T, device=device)
        v[:, j, :, j % hd] = 1.0
        kvalid = (torch.rand(B, T, device=device, generator=g) < 0.7).to(torch.uint8)
    qkv = torch.cat([q, k, v], 2).to(torch.bfloat16).reshape(B * T, (nh + 2 * nkv) * hd).contiguous()
    return qkv, kvalid
