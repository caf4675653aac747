"""tests/decode_reference.py pinned on the CPU to the installed `transformers`: the GEMM / q|k|v / attention restatements against the
pieces of a Qwen2DecoderLayer with a DynamicCache, all in fp64 (the same arithmetic: <= 1e-9 relative), and sample_ref's kept set
against TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper.

Ties: transformers' top-p sorts and cuts a group of equal values wherever the cumulative mass passes 1 - top_p; sample_ref keeps a group
whole.  So on tied rows  HF <= ours  and  ours \\ HF  lies inside the value group at the top-p boundary; top-k alone is equal.  top_p is
placed half-way between the masses above two consecutive groups and every case must have a gap >= 1e-5 of the mass to the boundary
(transformers' softmax is fp32) - a condition on the reference alone, asserted, no case skipped."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as R  # noqa: E402

GAP = 1e-5


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def tiny():
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(0)
    cfg = Qwen2Config(vocab_size=64, hidden_size=128, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, intermediate_size=256,
                      max_position_embeddings=512, rope_theta=1e6, rms_norm_eps=1e-6, attn_implementation="sdpa")     # eager rounds its softmax to fp32 even in an fp64 module
    m = Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m.double().requires_grad_(False), cfg


def test_gemm_epilogues_equal_the_mlp_and_o_proj(tiny):
    m, cfg = tiny
    layer = m.model.layers[0]
    g = torch.Generator().manual_seed(1)
    B, H, I = 5, cfg.hidden_size, cfg.intermediate_size
    x = torch.randn(B, H, generator=g, dtype=torch.float64) * torch.logspace(-1, 1, B, dtype=torch.float64)[:, None]
    Wgu = torch.stack([layer.mlp.gate_proj.weight, layer.mlp.up_proj.weight], 1).reshape(2 * I, H)        # gate rows 2 j, up rows 2 j + 1
    nw = layer.post_attention_layernorm.weight
    with torch.no_grad():
        h = layer.post_attention_layernorm(x)
        want_act = layer.mlp.act_fn(layer.mlp.gate_proj(h)) * layer.mlp.up_proj(h)
        want = x + layer.mlp(h)
        att = torch.randn(B, H, generator=g, dtype=torch.float64)
        want_o = x + layer.self_attn.o_proj(att)
    act = R.dec_gemm_ref(x, nw, cfg.rms_norm_eps, Wgu, None, "swiglu", act_dtype=None)
    assert _rel(act, want_act) <= 1e-9
    assert _rel(R.dec_gemm_ref(act, None, 0.0, layer.mlp.down_proj.weight, x, "resid", act_dtype=None), want) <= 1e-9
    assert _rel(R.dec_gemm_ref(att, None, 0.0, layer.self_attn.o_proj.weight, x, "resid", act_dtype=None), want_o) <= 1e-9
    # the one rounding: bf16 of the normed operand, nothing else
    r16 = R.dec_gemm_ref(x, nw, cfg.rms_norm_eps, Wgu, None, "swiglu")
    acc = R.Q.rmsnorm(x.float(), nw.float(), cfg.rms_norm_eps).to(torch.bfloat16).double() @ Wgu.t()
    assert torch.equal(r16, torch.nn.functional.silu(acc[:, 0::2]) * acc[:, 1::2])


@pytest.mark.parametrize("side", ["left", "right"])
def test_qkv_and_attention_equal_qwen2attention_with_a_cache(tiny, side):
    from transformers import DynamicCache
    m, cfg = tiny
    layer = m.model.layers[0]
    att = layer.self_attn
    nh, nkv, hd, H = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads, cfg.hidden_size
    g = torch.Generator().manual_seed(2)
    B, T = 3, 11
    mask = torch.ones(B, T, dtype=torch.long)
    for b in range(B):
        if b:
            if side == "left":
                mask[b, :2 * b] = 0
            else:
                mask[b, T - 2 * b:] = 0
    pos = (mask.cumsum(-1) - 1).masked_fill(mask == 0, 0)
    xs = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    xn = torch.randn(B, H, generator=g, dtype=torch.float64) * torch.tensor([0.1, 1.0, 7.0], dtype=torch.float64)[:, None]
    pos_new = pos[:, -1] + 1
    neg = torch.finfo(torch.float64).min
    cache = DynamicCache()
    with torch.no_grad():
        allow = torch.tril(torch.ones(T, T, dtype=torch.bool))[None, None] & mask.bool()[:, None, None, :]
        m4 = torch.zeros(B, 1, T, T, dtype=torch.float64).masked_fill(~allow, neg)
        att(layer.input_layernorm(xs), position_embeddings=m.model.rotary_emb(xs, pos), attention_mask=m4, past_key_values=cache)
        full = torch.cat([mask, torch.ones(B, 1, dtype=torch.long)], 1)
        m4 = torch.zeros(B, 1, 1, T + 1, dtype=torch.float64).masked_fill(~full.bool()[:, None, None, :], neg)
        want, _ = att(layer.input_layernorm(xn[:, None]), position_embeddings=m.model.rotary_emb(xn[:, None], pos_new[:, None]), attention_mask=m4,
                      past_key_values=cache)
    kc_hf, vc_hf = cache.layers[0].keys, cache.layers[0].values        # [B, nkv, T + 1, hd]
    W = torch.cat([att.q_proj.weight, att.k_proj.weight, att.v_proj.weight], 0)
    bias = torch.cat([att.q_proj.bias, att.k_proj.bias, att.v_proj.bias], 0)
    q, kn, vn = R.dec_qkv_ref(xn, layer.input_layernorm.weight, cfg.rms_norm_eps, W, bias, pos_new, nh, nkv, hd, 1e6, act_dtype=None)
    assert _rel(kn, kc_hf[:, :, T]) <= 1e-9 and _rel(vn, vc_hf[:, :, T]) <= 1e-9
    cap = T + 4                                                      # a cache with unused slots: garbage beyond `length` must not matter
    kc = torch.full((B, nkv, cap, hd), 1e3, dtype=torch.float64)
    vc = torch.full((B, nkv, cap, hd), -1e3, dtype=torch.float64)
    kc[:, :, :T], vc[:, :, :T] = kc_hf[:, :, :T], vc_hf[:, :, :T]
    kc[:, :, T], vc[:, :, T] = kn, vn
    valid = torch.ones(B, cap, dtype=torch.uint8)
    valid[:, :T + 1] = full.to(torch.uint8)
    a = R.dec_attention_ref(q, kc, vc, valid, T + 1)
    got = R.dec_gemm_ref(a, None, 0.0, att.o_proj.weight, None, "resid", act_dtype=None)
    assert _rel(got, want[:, 0]) <= 1e-9, _rel(got, want[:, 0])
    # a row without any valid key: zeros, the other rows unchanged
    valid[1] = 0
    a2 = R.dec_attention_ref(q, kc, vc, valid, T + 1)
    assert float(a2[1].abs().sum()) == 0.0 and torch.equal(a2[0], a[0]) and torch.equal(a2[2], a[2])


# ---- sample_ref against the warpers ---------------------------------------------------------------------------------------------------
def _hf_kept(logits, T, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = logits.detach().float().cpu().clone()[None]
    if T != 1.0:
        s = TemperatureLogitsWarper(T)(None, s)
    if k > 0:
        s = TopKLogitsWarper(k)(None, s)
    if p < 1.0:
        s = TopPLogitsWarper(p)(None, s)
    return s[0] > -math.inf


def _grid_row(V, seed, neg_inf):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-8, 9, (V,), generator=g).float() * 0.5     # a 0.5 grid: many exact ties
    if neg_inf and V >= 3:
        x[torch.randperm(V, generator=g)[:V // 3]] = -math.inf
    return x


def _midgap(x, T, k, group):
    """top_p mid-gap below value group `group`; a group too light to resolve (low temperature, a tiny vocabulary) gives way to the next
    heavier one - chosen from the reference alone, and the caller asserts the gap"""
    p, gap = R.top_p_midgap(x, T, k, group)
    while gap < GAP and group > 0:
        group -= 1
        p, gap = R.top_p_midgap(x, T, k, group)
    return p, gap


VOCABS = [1, 2, 17, 255, 257, 2049, 4096, 65535, 65536, 151936]


@pytest.mark.parametrize("V", VOCABS)
def test_sample_ref_tie_free_rows_equal_the_warpers(V):
    g = torch.Generator().manual_seed(V)
    cases = 0
    for kind in ("peaked", "flat") if V <= 4096 else ("peaked",):     # a flat row of a larger vocabulary has no token with 2e-5 of the mass
        # tie-free by construction: a shuffled jittered grid (random fp32 values of a large vocabulary collide)
        x = ((torch.randperm(V, generator=g).double() + 0.5 * torch.rand(V, generator=g, dtype=torch.float64)) / V * 2 - 1).float()
        x = x * (9.0 if kind == "peaked" else 1.0)
        if kind == "peaked" and V > 8:
            x[torch.randperm(V, generator=g)[:8]] = 12.0 + 4.0 * torch.rand(8, generator=g)
        assert x.unique().numel() == V
        for T in (0.2, 1.0, 1.5):
            for k in (0, 1, 5, max(V - 1, 1), V, V + 7):
                for group in (None, 0, 1, 3):
                    p, gap = (1.0, math.inf) if group is None else _midgap(x, T, k, group)
                    assert gap >= GAP, (kind, T, k, group, gap)
                    r = R.sample_ref(x, T, k, p)
                    assert r["margin"] >= GAP
                    assert torch.equal(r["kept"], _hf_kept(x, T, k, p)), (kind, T, k, p)
                    cases += 1
    assert cases == (2 if V <= 4096 else 1) * 3 * 6 * 4


@pytest.mark.parametrize("V", VOCABS)
def test_sample_ref_tied_rows_contain_the_warpers_set(V):
    cases = cut = 0
    for neg_inf in (False, True):
        x = _grid_row(V, V + neg_inf, neg_inf)
        for T in (0.2, 1.0, 1.5):
            for k in sorted({0, 1, 5, max(V - 1, 0), V, V + 7}):
                rk = R.sample_ref(x, T, k, 1.0)
                hf = _hf_kept(x, T, k, 1.0)
                finite = x > -math.inf
                assert torch.equal(rk["kept"], hf & finite), ("top-k alone", T, k)       # equal (HF's own -inf entries stay -inf)
                for group in (0, 1, 2):
                    p, gap = _midgap(x, T, k, group)
                    assert gap >= GAP, (V, T, k, group, gap)        # every generated case meets the condition: none is dropped
                    r = R.sample_ref(x, T, k, p)
                    assert r["margin"] >= GAP
                    hf = _hf_kept(x, T, k, p)
                    ours = r["kept"]
                    assert bool((ours | ~hf).all()), ("HF is not a subset", T, k, p)
                    extra = ours & ~hf
                    if bool(extra.any()):
                        cut += 1
                        assert bool((r["s"][extra] == r["theta"]).all()), ("extra tokens outside the boundary group", T, k, p)
                    cases += 1
    print(f"V={V}: {cases} tied cases, transformers cut a tie group in {cut}")
    assert cases == 2 * 3 * len({0, 1, 5, max(V - 1, 0), V, V + 7}) * 3


def test_sample_ref_definition_on_a_hand_made_row():
    x = torch.tensor([0.0, math.log(2.0), math.log(2.0), -math.inf, math.log(4.0)])          # masses 1, 2, 2, 0, 4 of 9
    r = R.sample_ref(x, 1.0, 0, 1.0)
    assert r["kept"].tolist() == [True, True, True, False, True] and r["count"] == 4 and abs(r["Z"] - 9 / 4) < 1e-6
    assert torch.allclose(r["cdf"], torch.tensor([1, 3, 5, 5, 9], dtype=torch.float64) / 9, atol=1e-7)
    assert R.sample_ref(x, 1.0, 2, 1.0)["kept"].tolist() == [False, True, True, False, True]  # the 2nd largest is tied: both kept
    assert R.sample_ref(x, 1.0, 0, 0.5)["kept"].tolist() == [False, True, True, False, True]  # mass above the tied group 4/9 < 0.5
    assert R.sample_ref(x, 1.0, 0, 0.4)["kept"].tolist() == [False, False, False, False, True]
    assert R.sample_ref(x, 1.0, 0, 0.0)["count"] == 1
    assert R.sample_ref(x, 1.0, 5, 1.0)["count"] == 4                                         # the k-th largest is -inf: never kept
    adm = R.admissible_tokens(r, 1 / 9)                                                       # u on the boundary of tokens 0 and 1
    assert adm.tolist() == [True, True, False, False, False]
