"""TEST INFRASTRUCTURE ONLY - plain torch fp64 restatements of the decode step's operations (csrc/llm_decode.hip, csrc/llm_sample.hip),
written from the definition of the operation (transformers' Qwen2 modules and logits warpers), not from the kernels.

PINNING: tests/test_decode_reference.py checks every function here on the CPU against the installed `transformers` modules
(Qwen2DecoderLayer / Qwen2Attention with a DynamicCache in fp64, the Temperature / TopK / TopP warpers).  `act_dtype` is the one
rounding the bf16 reference model applies between two modules; the pin runs with act_dtype=None (no rounding: the same arithmetic as
the fp64 modules), the GPU tests with the default bf16."""
from __future__ import annotations

import math

import torch

from oracle import qwen2_oracle as Q


def _act(t, act_dtype):
    return t if act_dtype is None else t.to(act_dtype)


def normed_operand(x, norm_w, eps, act_dtype=torch.bfloat16):
    """Qwen2RMSNorm (statistics and scaling in fp32 whatever the module's dtype, as its forward does) with ONE rounding of the normed
    operand -> fp64; act_dtype None: no rounding, the weight applied in fp64 as an fp64 module does; norm_w None: x itself"""
    if norm_w is None:
        return x.double()
    if act_dtype is None:
        return Q.rmsnorm(x.float(), norm_w.double(), eps)
    return Q.rmsnorm(x.float(), norm_w.float(), eps).to(act_dtype).double()


def dec_gemm_ref(x, norm_w, eps, W, resid, epi, act_dtype=torch.bfloat16):
    """x [B, K], W [N, K] -> fp64.  epi "resid": resid + norm(x) @ W^T [B, N];  epi "swiglu": silu(gate) * up [B, N / 2] with the gate
    rows of W at 2 j and the up rows at 2 j + 1 (Qwen2MLP's act_fn(gate_proj(h)) * up_proj(h) on interleaved rows)"""
    acc = normed_operand(x, norm_w, eps, act_dtype) @ W.double().t()
    if epi == "resid":
        return acc if resid is None else resid.double() + acc
    assert epi == "swiglu", epi
    return torch.nn.functional.silu(acc[:, 0::2]) * acc[:, 1::2]


def dec_qkv_ref(x, norm_w, eps, W, bias, pos, nh, nkv, hd, theta, act_dtype=torch.bfloat16):
    """x [B, H], W [(nh + 2 nkv) * hd, H] = q | k | v rows, bias, pos [B] -> fp64 (q [B, nh, hd], k_new [B, nkv, hd], v_new [B, nkv, hd]):
    projection + bias, one rounding (the projections' outputs as the reference holds them), apply_rotary_pos_emb at position pos[b]"""
    B = x.shape[0]
    y = normed_operand(x, norm_w, eps, act_dtype) @ W.double().t() + bias.double()
    y = _act(y, act_dtype).double()
    q = y[:, :nh * hd].view(B, nh, 1, hd)
    k = y[:, nh * hd:(nh + nkv) * hd].view(B, nkv, 1, hd)
    v = y[:, (nh + nkv) * hd:].view(B, nkv, hd)
    cos, sin = Q.rope_cos_sin(pos.view(B, 1).cpu(), hd, theta)     # fp32 angles, as Qwen2RotaryEmbedding computes them
    q, k = Q.apply_rope(q, k, cos.to(x.device), sin.to(x.device))
    return q[:, :, 0], k[:, :, 0], v


def dec_attention_ref(q, kc, vc, key_valid, length):
    """q [B, nh * hd] or [B, nh, hd], caches [B, nkv, cap, hd], key_valid [B, cap] -> fp64 [B, nh * hd]: softmax(q . k hd^-0.5) . v over
    the keys j < length with key_valid[b, j] != 0 (repeat_kv: head h reads kv head h / (nh / nkv)); a row with no such key gives zeros"""
    B, nkv, cap, hd = kc.shape
    q = q.double().reshape(B, -1, hd)
    nh = q.shape[1]
    k = kc.double()[:, :, :length].repeat_interleave(nh // nkv, 1)
    v = vc.double()[:, :, :length].repeat_interleave(nh // nkv, 1)
    ok = key_valid[:, :length] != 0
    s = torch.einsum("bhd,bhkd->bhk", q, k) * hd ** -0.5
    s = s.masked_fill(~ok[:, None], -math.inf)
    none = ~ok.any(-1)
    s[none] = 0.0                                                   # placeholder scores: the row is zeroed below
    out = torch.einsum("bhk,bhkd->bhd", torch.softmax(s, -1), v)
    out[none] = 0.0
    return out.reshape(B, nh * hd)


def sample_ref(logits, T, k, p):
    """One row of logits [V] -> dict.  s = fp32(logits) / fp32(T) in IEEE fp32 (TemperatureLogitsWarper); then in fp64, by the value-threshold
    definition of the warpers: top-k (k > 0) keeps s >= the min(k, V)-th largest value; top-p (p < 1) keeps a group of equal values iff
    the normalised mass of the kept-so-far values strictly above it is < p, the top group always; -inf entries are never kept.
      s       fp32 [V]            kept   bool [V]               count  int
      theta   the lowest kept value (fp32, as a float)          Z      sum of exp(s - max s) over the kept set (fp64)
      cdf     fp64 [V]: the token-index-order cumulative probability over the kept set
      margin  the distance from p to the nearest `mass above a group` (inf when top-p is off or has one group): how far p is from a
              group boundary"""
    s = (logits.detach().float().cpu() / torch.tensor(float(T), dtype=torch.float32))
    sd = s.double()
    V = s.numel()
    kept = sd > -math.inf
    assert bool(kept.any()), "a row needs one finite logit"
    if k > 0:
        kth = sd.topk(min(int(k), V)).values[-1]
        kept &= sd >= kth
    smax = sd[kept].max()
    margin = math.inf
    if p < 1.0:
        vals, counts = torch.unique(sd[kept], return_counts=True)            # ascending
        mass = counts.double() * torch.exp(vals - smax)
        total = mass.sum()
        above = (mass.flip(0).cumsum(0) - mass.flip(0)).flip(0) / total      # normalised mass strictly above each group
        keep_g = above < p
        keep_g[-1] = True
        kept &= sd >= vals[keep_g].min()
        if vals.numel() > 1:
            margin = float((above[:-1] - p).abs().min())
    pr = torch.where(kept, torch.exp(sd - smax), torch.zeros_like(sd))
    Z = pr.sum()
    return dict(s=s, kept=kept, count=int(kept.sum()), theta=float(s[kept].min()), Z=float(Z), cdf=pr.cumsum(0) / Z, margin=margin)


def top_p_midgap(logits, T, k, group):
    """a top_p half-way between the masses above value groups `group` and `group + 1` (descending, 0 = the top group) of the top-k set:
    groups 0 .. group are kept.  -> (p, gap) with gap = half the mass of group `group`: the distance of p from both boundaries"""
    r = sample_ref(logits, T, k, 1.0)
    sd = r["s"].double()
    vals, counts = torch.unique(sd[r["kept"]], return_counts=True)
    vals, counts = vals.flip(0), counts.flip(0)
    mass = counts.double() * torch.exp(vals - vals[0])
    frac = mass / mass.sum()
    g = min(int(group), vals.numel() - 1)
    above = float(frac[:g].sum())
    return min(above + float(frac[g]) / 2, 1.0 - 2.0 ** -24), float(frac[g]) / 2


def admissible_tokens(ref, u, tol=1e-5):
    """kept tokens j whose CDF interval [c_{j-1}, c_j] meets [u - tol, u + tol] (the draw's inverse CDF in index order, fp32 sums against
    fp64) -> bool [V]"""
    cdf = ref["cdf"]
    lo = torch.cat([torch.zeros(1, dtype=torch.float64), cdf[:-1]])
    return ref["kept"] & (lo <= u + tol) & (cdf >= u - tol)
