"""Qwen2 decode steps on the library's kernels (ml_fastvlm_amd/qwen2_decode.py, csrc/llm_decode.hip) against torch fp32 / transformers.

Oracle: transformers' Qwen2ForCausalLM in fp32 on the same bf16-rounded weights, continuing with its own cache.  Budgets: the single ops
within the prefill tests' rel-L2 1e-2; teacher-forced step logits within rel-L2 2e-2 (bf16 activations through the stack); greedy token
streams equal wherever the oracle's top-2 margin exceeds DELTA."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import (DELTA, GREEDY_SEEDS, lib, rel,  # noqa: E402,F401
                         agree as _agree, models as _models, prompt as _prompt, ptr as _p, stream as _st)

pytestmark = pytest.mark.gpu


def _norm_ref(x, w, eps=1e-6):
    xf = x.float()
    rstd = 1.0 / torch.sqrt((xf * xf).mean(-1, keepdim=True) + eps)
    return (xf * rstd * w).to(torch.bfloat16).float()


# ---- 1. the weight-streaming GEMM ---------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(896, 4864, False), (9728, 896, True), (1536, 8960, False), (3584, 18944, False), (37888, 3584, True), (896, 896, False)]


@pytest.mark.parametrize("B", [1, 3, 8, 16])
@pytest.mark.parametrize("N,K,swiglu", GEMM_SHAPES)
def test_dec_gemm_epilogues(lib, B, N, K, swiglu):
    from ml_fastvlm_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(N + K + B)
    x = torch.randn(B, K, device="cuda", generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
    nw = (1 + 0.1 * torch.randn(K, device="cuda", generator=g)).float() if swiglu else None
    resid = torch.randn(B, N, device="cuda", generator=g).to(torch.bfloat16)
    splits = 16
    part = torch.empty(splits * N * 16, device="cuda")
    cnt = torch.zeros((N + 63) // 64, device="cuda", dtype=torch.int32)
    epi = _lib.EPI_SWIGLU if swiglu else _lib.EPI_RESID
    outs = []
    for _ in range(2):
        out = torch.empty(B, N // 2 if swiglu else N, device="cuda", dtype=torch.bfloat16)
        _lib.check(lib.fvhd_op_dec_gemm(_st(), epi, _p(x), B, _p(nw), 1e-6, _p(W), N, K, _p(resid), _p(out), _p(part), _p(cnt), splits), "dec_gemm")
        outs.append(out)
    torch.cuda.synchronize()
    xa = _norm_ref(x, nw) if nw is not None else x.float()
    acc = xa @ W.float().t()
    want = (acc[:, 0::2] * torch.sigmoid(acc[:, 0::2]) * acc[:, 1::2]) if swiglu else resid.float() + acc
    assert rel(outs[0], want) <= 1e-2, rel(outs[0], want)
    assert torch.equal(outs[0], outs[1])                          # deterministic split-K
    assert int(cnt.abs().sum()) == 0                              # counters left zero for the next launch


# ---- 2. q|k|v + rope + cache append ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv,hd,H", [(14, 2, 64, 896), (12, 2, 128, 1536), (28, 4, 128, 3584)])
@pytest.mark.parametrize("B", [1, 3, 8, 16])
def test_dec_qkv_rope_cache(lib, nh, nkv, hd, H, B):
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    from transformers.models.qwen2.modeling_qwen2 import rotate_half
    g = torch.Generator(device="cuda").manual_seed(hd + B + H)
    N, cap, slot = (nh + 2 * nkv) * hd, 40, 17
    x = torch.randn(B, H, device="cuda", generator=g).to(torch.bfloat16)
    W = (torch.randn(N, H, device="cuda", generator=g) / H ** 0.5).to(torch.bfloat16)
    bias = 0.1 * torch.randn(N, device="cuda", generator=g)
    nw = (1 + 0.1 * torch.randn(H, device="cuda", generator=g)).float()
    pos = torch.arange(B, device="cuda", dtype=torch.long) * 421 + 5
    pos[-1] = 9000 if B > 1 else 5                                  # 9000: beyond the 8192-row table
    table = rope_table(8192, hd, 1e6, "cuda")
    kc = torch.zeros(B, nkv, cap, hd, device="cuda", dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    q = torch.empty(B, nh * hd, device="cuda", dtype=torch.bfloat16)
    length = torch.tensor([slot], device="cuda", dtype=torch.int32)
    part = torch.empty(16 * N * 16, device="cuda")
    cnt = torch.zeros((N + 63) // 64, device="cuda", dtype=torch.int32)
    _lib.check(lib.fvhd_op_dec_qkv(_st(), _p(x), B, H, _p(nw), 1e-6, _p(W), _p(bias), _p(q), _p(pos), _p(table), 8192, 1e6, _p(kc), _p(vc), cap,
                                   _p(length), nh, nkv, hd, _p(part), _p(cnt), 4), "dec_qkv")
    torch.cuda.synchronize()
    y = (_norm_ref(x, nw) @ W.float().t() + bias).to(torch.bfloat16).float()
    inv = 1.0 / (1e6 ** (torch.arange(0, hd, 2, device="cuda", dtype=torch.float32) / hd))
    ang = pos.float()[:, None] * inv[None]
    cos, sin = torch.cat([ang.cos()] * 2, -1)[:, None], torch.cat([ang.sin()] * 2, -1)[:, None]
    qh, kh, vh = y[:, :nh * hd].view(B, nh, hd), y[:, nh * hd:(nh + nkv) * hd].view(B, nkv, hd), y[:, (nh + nkv) * hd:].view(B, nkv, hd)
    qr, kr = qh * cos + rotate_half(qh) * sin, kh * cos + rotate_half(kh) * sin
    assert rel(q.view(B, nh, hd), qr) <= 1e-2
    assert rel(kc[:, :, slot], kr) <= 1e-2 and rel(vc[:, :, slot], vh) <= 1e-2
    others = torch.ones(cap, dtype=torch.bool)
    others[slot] = False
    assert kc[:, :, others].abs().sum() == 0 and vc[:, :, others].abs().sum() == 0


# ---- 3. single-query attention over the cache ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 12, 2), (128, 28, 4), (64, 4, 2)])
@pytest.mark.parametrize("length,cap", [(1, 64), (285, 300), (2049, 2050), (2050, 2050)])
@pytest.mark.parametrize("side", ["left", "right"])
def test_dec_attention(lib, hd, nh, nkv, length, cap, side):
    from ml_fastvlm_amd import _lib
    B = 3
    g = torch.Generator(device="cuda").manual_seed(hd * 7 + length + (side == "left"))
    q = torch.randn(B, nh * hd, device="cuda", generator=g).to(torch.bfloat16)
    kc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    vc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    mask = torch.zeros(B, cap, device="cuda", dtype=torch.uint8)
    for b in range(B):
        npad = min(b * 37, length - 1)
        if side == "left":
            mask[b, npad:length] = 1
        else:
            mask[b, :length - npad] = 1
    out = torch.empty(B, nh * hd, device="cuda", dtype=torch.bfloat16)
    ln = torch.tensor([length], device="cuda", dtype=torch.int32)
    splits = 9
    part = torch.empty(B * nh * splits * (hd + 2), device="cuda")
    cnt = torch.zeros(B * nh, device="cuda", dtype=torch.int32)
    res = []
    for _ in range(2):
        _lib.check(lib.fvhd_op_dec_attention(_st(), _p(q), _p(kc), _p(vc), _p(mask), _p(out), B, nh, nkv, hd, cap, _p(ln), _p(part), _p(cnt), splits),
                   "dec_attention")
        res.append(out.clone())
    torch.cuda.synchronize()
    rep = nh // nkv
    k = kc.float().repeat_interleave(rep, 1)[:, :, :length]
    v = vc.float().repeat_interleave(rep, 1)[:, :, :length]
    s = torch.einsum("bhd,bhkd->bhk", q.float().view(B, nh, hd), k) * hd ** -0.5
    s = s.masked_fill(mask[:, None, :length] == 0, float("-inf"))
    want = torch.einsum("bhk,bhkd->bhd", torch.softmax(s, -1), v).reshape(B, nh * hd)
    assert rel(res[0], want) <= 1e-2, rel(res[0], want)
    assert torch.equal(res[0], res[1])


# ---- 4. lm_head + argmax -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 16])
def test_dec_lm_argmax_full_vocab_ties(lib, B):
    from ml_fastvlm_amd import _lib
    V, H = 151936, 896
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, H, device="cuda", generator=g).to(torch.bfloat16)
    W = (torch.randn(V, H, device="cuda", generator=g) / H ** 0.5).to(torch.bfloat16)
    nw = torch.ones(H, device="cuda")
    # planted ties: row 0's winner is copied to a higher and a lower index - the lowest copy must win
    xa = _norm_ref(x, nw)
    best = int((xa[0] @ W.float().t()).argmax())
    W[151000] = W[best]
    W[7] = W[best]
    lg = torch.empty(B, V, device="cuda")
    ids = torch.empty(B, device="cuda", dtype=torch.long)
    nblk = (V // 16 + 3) // 4
    sv = torch.empty(nblk * 16, device="cuda")
    si = torch.empty(nblk * 16, device="cuda", dtype=torch.int32)
    _lib.check(lib.fvhd_op_dec_lm_argmax(_st(), _p(x), B, _p(nw), 1e-6, _p(W), V, H, _p(lg), _p(ids), _p(sv), _p(si)), "lm_argmax")
    torch.cuda.synchronize()
    assert torch.equal(ids, lg.argmax(-1))
    assert int(ids[0]) == min(7, best)
    assert rel(lg, xa @ W.float().t()) <= 1e-2


# ---- model-level tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["0.5B", "1.5B", "7B"])
def test_teacher_forced_steps(name):
    from transformers import DynamicCache
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator, generation_position_ids
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, ref = _models(name)
    B, T, steps = 2, 24, 32
    e, mask = _prompt(ref, B, T, "left")
    gen = Qwen2Generator.from_hf(m16, B, T + steps + 4)
    pos = generation_position_ids(mask, B, T)
    with torch.no_grad():
        lg, ids = gen.start(e.to(torch.bfloat16), mask, pos)
        cache = DynamicCache()
        out = ref(inputs_embeds=e, attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True)
        want = out.logits[:, -1]
        errs = [rel(lg, want)]
        am, p = mask, pos
        emb_ref = ref.get_input_embeddings()
        fed_seq = []
        for _ in range(steps):
            tok = want.argmax(-1)
            fed_seq.append(tok)
            lg, _ = gen.step(tok.contiguous())
            am = torch.cat([am, torch.ones(B, 1, device="cuda", dtype=am.dtype)], 1)
            p = p[:, -1:] + 1
            out = ref(inputs_embeds=emb_ref(tok)[:, None], attention_mask=am, position_ids=p, past_key_values=out.past_key_values, use_cache=True)
            want = out.logits[:, -1]
            errs.append(rel(lg, want))
    print(name, "step rel-L2 max", max(errs))
    assert max(errs) <= 2e-2, errs
    # start + k steps ~ ONE prefill over the longer sequence (no padding: the same positions either way)
    k = 6
    gen2 = Qwen2Generator(gen.pre, B, T + k + 1, embed_tokens=None if m16.config.tie_word_embeddings else m16.get_input_embeddings().weight,
                          tie_word_embeddings=m16.config.tie_word_embeddings)
    ones = torch.ones(B, T, device="cuda", dtype=torch.long)
    with torch.no_grad():
        gen2.start(e.to(torch.bfloat16), ones)
        for i in range(k):
            lg, _ = gen2.step(fed_seq[i].contiguous())
        emb = m16.get_input_embeddings()(torch.stack(fed_seq[:k], 1))
        long = torch.cat([e.to(torch.bfloat16), emb], 1)
        pre = gen.pre(long, torch.ones(B, T + k, device="cuda", dtype=torch.long))
    assert rel(lg, pre) <= 1e-2, rel(lg, pre)
    assert isinstance(gen.pre, Qwen2Prefill)


@pytest.mark.parametrize("side", ["left", "right"])
def test_greedy_equals_transformers_generate(side):
    """B = 3: our greedy tokens equal transformers' greedy generate exactly; then with an EOS list that every row emits, both stop at
    the step where the last row finishes and pad the finished rows"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _models("0.5B", seed=1)
    B, T, new = 3, 20, 12
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    for seed in GREEDY_SEEDS[side]:
        e, mask = _prompt(ref, B, T, side, seed=seed)
        with torch.no_grad():
            r = ref.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                             output_scores=True, return_dict_in_generate=True)
            got = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
        top = torch.stack(r.scores, 1).float().topk(2, -1).values
        assert (top[..., 0] - top[..., 1]).min().item() > DELTA          # the seed's precondition (oracle only)
        assert torch.equal(got.cpu(), r.sequences.cpu()), (got.tolist(), r.sequences.tolist())
        # EOS: one token of every row (rows 0 / 1 / 2 at steps 2 / 4 / 6) -> every sequence finishes, the output ends at the last finish
        eos = [int(r.sequences[b, 2 + 2 * b]) for b in range(B)]
        with torch.no_grad():
            r2 = ref.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=eos, pad_token_id=7,
                              output_scores=True, return_dict_in_generate=True)
            got2 = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, eos_token_id=eos, pad_token_id=7, poll_every=4)
        assert r2.sequences.shape[1] < new
        assert got2.shape == r2.sequences.shape and torch.equal(got2.cpu(), r2.sequences.cpu()), (got2.tolist(), r2.sequences.tolist())


def test_graph_replay_bit_identical_and_overflow():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _models("0.5B", seed=3)
    B, T, N = 2, 16, 12
    e, mask = _prompt(ref, B, T, "left", seed=4)
    e = e.to(torch.bfloat16)
    gen = Qwen2Generator.from_hf(m16, B, T + N)
    eager_ids, eager_lg = [], []
    with torch.no_grad():
        gen.start(e, mask)
        for _ in range(N):
            lg, ids = gen.step()
            eager_ids.append(ids.clone())
            eager_lg.append(lg.clone())
        gen.start(e, mask)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                lg, ids = gen.step()
        torch.cuda.current_stream().wait_stream(s)
        for i in range(N):
            g.replay()
            assert torch.equal(ids, eager_ids[i]) and torch.equal(lg, eager_lg[i]), i
        assert gen.cache_state() == (T + N, 0)
        g.replay()                                                # past the capacity: nothing written, the error is sticky
        torch.cuda.synchronize()
        assert gen.cache_state() == (T + N, 1)
        assert torch.equal(ids, eager_ids[-1])
        with pytest.raises(_lib.FvhdError, match="capacity"):
            gen.step()


def test_generate_end_to_end_standin():
    """ml_fastvlm_amd.generate on a stand-in LLaVA model: Qwen2ForCausalLM + our tower / projector + a prepare_inputs_labels_for_multimodal
    that calls multimodal_splice, against the same stand-in driven through transformers' generate(inputs_embeds=...)."""
    from types import MethodType, SimpleNamespace
    import ml_fastvlm_amd as fv
    from ml_fastvlm_amd import splice as S
    from ml_fastvlm_amd import synth
    m16, ref = _models("0.5B", seed=5)
    res, hidden = 256, 896
    tower = fv.MobileCLIPVisionTower(f"mobileclip_l_{res}", SimpleNamespace(unfreeze_mm_vision_tower=False))
    tower.vision_tower.model.load_state_dict(synth.synthetic_state_dict(1234, "mild"), strict=True)
    proj = fv.build_vision_projector(SimpleNamespace(mm_projector_type="mlp2x_gelu", mm_hidden_size=3072, hidden_size=hidden))
    proj.load_state_dict(synth.synthetic_projector_state_dict(hidden, 1234), strict=True)
    tower, proj = tower.to("cuda", torch.bfloat16), proj.to("cuda", torch.bfloat16)

    def prepare(self, input_ids, position_ids, attention_mask, past_key_values, labels, images, image_sizes=None):
        feats = fv.encode_images(tower, proj, images)
        o = S.multimodal_splice(input_ids, position_ids, attention_mask, labels, feats, self.get_input_embeddings().weight, "right", None)
        return o[0], o[1], o[2], past_key_values, o[4], o[5]

    m16.prepare_inputs_labels_for_multimodal = MethodType(prepare, m16)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(10, 4000, (2, 12), generator=g)
    ids[:, 3] = -200                                              # IMAGE_TOKEN_INDEX
    mask = torch.ones_like(ids)
    mask[1, 9:] = 0
    ids, mask = ids.cuda(), mask.cuda()
    images = synth.synthetic_images(2, res, seed=0).to("cuda", torch.bfloat16)
    new = 16
    with torch.no_grad():
        got = fv.generate(m16, ids, images=images, attention_mask=mask, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
        _, pos, am, _, emb, _ = prepare(m16, ids, None, mask, None, None, images)
        r = ref.generate(inputs_embeds=emb.float(), attention_mask=am, position_ids=pos, max_new_tokens=new, do_sample=False, eos_token_id=None,
                         pad_token_id=0, output_scores=True, return_dict_in_generate=True)
    n = _agree(got, r.sequences, r.scores)
    print("end to end: steps compared per row", n)
    assert got.shape == r.sequences.shape and sum(n) >= 4, n
    if min(n) == new:
        assert torch.equal(got, r.sequences)
    with pytest.raises(NotImplementedError, match="num_beams"):
        fv.generate(m16, ids, images=images, attention_mask=mask, num_beams=2)


def test_untied_model_needs_its_embedding_table():
    """the decode never guesses its input embedding: an untied model without model.embed_tokens.weight, and a context whose tie flag is
    unknown, are refused at start(); with the table (or the flag of a tied model) the same contexts decode"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, ref = _models("7B", seed=6)
    e, mask = _prompt(ref, 2, 8, "left", seed=7)
    e = e.to(torch.bfloat16)
    pre = Qwen2Prefill.from_hf(m16)
    assert pre.tie_word_embeddings is False
    gen = Qwen2Generator(pre, 2, 16)                               # the documented constructor form, no embed_tokens
    with pytest.raises(_lib.FvhdError, match="embed_tokens"):
        gen.start(e, mask)
    gen = Qwen2Generator(pre, 2, 16, embed_tokens=m16.get_input_embeddings().weight)
    gen.start(e, mask)
    _, ids = gen.step()
    assert ids.shape == (2,)
    # a context built by hand: nothing says whether lm_head is the embedding table
    cfg = m16.config
    raw = Qwen2Prefill(0, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads, 128, cfg.intermediate_size,
                       cfg.vocab_size)
    raw.load_state_dict(m16.state_dict())
    gen = Qwen2Generator(raw, 2, 16)
    with pytest.raises(_lib.FvhdError, match="unknown"):
        gen.start(e, mask)
    gen = Qwen2Generator(raw, 2, 16, tie_word_embeddings=True)   # the caller's explicit statement is taken
    gen.start(e, mask)
