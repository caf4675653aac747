"""Qwen2 prefill and decode on MXFP4 weights (`weights="mxfp4"`, include/fvhd.h "LLM 4-bit weights"), end to end.

Reference: the library's own bf16 path.  `gen4 = from_hf(model, weights="mxfp4")` against `gen16 = from_hf(the same model holding the
dequantised matrices)`: dequantised MXFP4 values are bf16 values and quantise to themselves as values, the 4-bit decode kernels feed the
MFMAs the operands the bf16 kernels read from such a matrix, the prefill dequantises into a bf16 scratch, and the decode's plans depend
on N, K and the CU count only - so EVERY comparison with gen16 below is bit for bit, no tolerance.  (The bf16 path is tested against fp32 /
transformers in tests/test_gpu_decode.py and the others.)  The decode cache has no read-back: K / V are compared where the library hands
them out (the prefill's return_kv) and through the logits of every later step, which read every appended row; the q|k|v op's cache slot
is compared directly in tests/test_gpu_w4_ops.py.
One independent check: teacher-forced logits against the fp32 exact-weight oracle, rel-L2 <= 2e-2 (the bound of tests/test_gpu_decode.py
and tests/test_gpu_decode_w8.py)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
import w4_testlib as W  # noqa: E402

pytestmark = pytest.mark.gpu

W4 = W.W4
NAMES = ["0.5B", "7B"]                                           # tied / untied
CAP = 64


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module", params=NAMES)
def pair(request):
    """(name, model with dequantised matrices, fp32 oracle, gen4, gen16) at batch 40, made once per width"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = W.models(request.param, seed=3)
    gen4 = Qwen2Generator.from_hf(m16, 40, CAP, weights=W4)
    gen16 = Qwen2Generator.from_hf(m16, 40, CAP)
    assert gen4.pre.weight_format == W4 and gen16.pre.weight_format == "bf16"
    return request.param, m16, ref, gen4, gen16


def _prompt(ref, B, T, seed):
    e, mask = L.wide_prompt(ref, B, T, seed=seed)
    return e.to(torch.bfloat16), mask


def test_prefill_logits_and_kv(pair):
    _, _, ref, gen4, gen16 = pair
    e, mask = _prompt(ref, 3, 20, 1)
    a = gen4.pre(e, mask, None, return_kv=True)
    b = gen16.pre(e, mask, None, return_kv=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert bool(torch.isfinite(x.float()).all()) and _same(x, y)


@pytest.mark.parametrize("B", [2, 40])
def test_start_and_greedy_steps(pair, B):
    _, _, ref, gen4, gen16 = pair
    e, mask = _prompt(ref, B, 20, 2)
    with torch.no_grad():
        (l4, i4), (l16, i16) = gen4.start(e, mask), gen16.start(e, mask)
        assert _same(l4, l16) and _same(i4, i16)
        for step in range(9):                                     # (the row step 8 appended is read by step 9)
            (l4, i4), (l16, i16) = gen4.step(), gen16.step()
            assert bool(torch.isfinite(l4).all()) and _same(l4, l16) and _same(i4, i16), step
        assert gen4.cache_state() == gen16.cache_state() == (29, 0)


def test_graph_replay_equals_eager(pair):
    _, _, ref, gen4, _ = pair
    B, T, N = 2, 16, 8
    e, mask = _prompt(ref, B, T, 4)
    eager = []
    with torch.no_grad():
        gen4.start(e, mask)
        for _ in range(N):
            lg, ids = gen4.step()
            eager.append((lg.clone(), ids.clone()))
        gen4.start(e, mask)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                lg, ids = gen4.step()
        torch.cuda.current_stream().wait_stream(s)
        for i in range(N):
            g.replay()
            assert _same(lg, eager[i][0]) and _same(ids, eager[i][1]), i
        assert gen4.cache_state() == (T + N, 0)


def test_verify_step(pair):
    _, _, ref, gen4, gen16 = pair
    e, mask = _prompt(ref, 1, 18, 5)
    drafts = torch.tensor([5, 17, 4000, 33, 900], device="cuda")
    outs = []
    with torch.no_grad():
        for gen in (gen4, gen16):
            gen.spec_reserve(6)
            gen.start(e, mask)
            lg, ids, emitted = gen.verify(drafts)
            torch.cuda.synchronize()
            outs.append((lg.clone(), ids.clone(), emitted.clone()))
    for a, b in zip(*outs):
        assert _same(a, b)


def test_extend_then_step(pair):
    _, _, ref, gen4, gen16 = pair
    e, mask = _prompt(ref, 2, 16, 6)
    chunk, cmask = _prompt(ref, 2, 7, 7)
    outs = []
    with torch.no_grad():
        for gen in (gen4, gen16):
            gen.start(e, mask)
            lg, ids = gen.extend(chunk, cmask)
            a = (lg.clone(), ids.clone())
            lg, ids = gen.step()
            outs.append(a + (lg.clone(), ids.clone()))
            assert gen.cache_state() == (24, 0)
    for a, b in zip(*outs):
        assert _same(a, b)


def test_score(pair):
    _, m16, ref, gen4, gen16 = pair
    e, mask = _prompt(ref, 2, 24, 8)
    g = torch.Generator(device="cuda").manual_seed(9)
    labels = torch.randint(0, m16.config.vocab_size, (2, 24), device="cuda", generator=g)
    with torch.no_grad():
        a = gen4.pre.score(e, labels, mask)
        b = gen16.pre.score(e, labels, mask)
        for x, y in zip(a, b):
            assert bool(torch.isfinite(x).all()) and _same(x, y)
        gen4.start(e, mask)
        gen16.start(e, mask)
        for x, y in zip(gen4.score_last(labels), gen16.score_last(labels)):
            assert _same(x, y)


def test_sample_step_with_a_fixed_seed(pair):
    _, _, ref, gen4, gen16 = pair
    e, mask = _prompt(ref, 2, 16, 10)
    outs = []
    with torch.no_grad():
        for gen in (gen4, gen16):
            gen.set_sampling(True, temperature=0.8, top_k=40, top_p=0.95, seed=11)
            try:
                _, i0 = gen.start(e, mask)
                i0 = i0.clone()
                lg, i1 = gen.step()
                outs.append((i0, lg.clone(), i1.clone()))
            finally:
                gen.set_sampling(False)
    for a, b in zip(*outs):
        assert _same(a, b)


@pytest.mark.parametrize("B", [2, 40])
def test_teacher_forced_steps_against_the_fp32_oracle(pair, B):
    """the independent check: rel-L2 <= 2e-2 of every step's logits against transformers in fp32 on exactly the weights the library holds"""
    from transformers import DynamicCache
    from ml_fastvlm_amd.qwen2_decode import generation_position_ids
    name, _, ref, gen4, _ = pair
    T, steps = 24, 16
    e, mask = L.prompt(ref, min(B, 4), T, "left", seed=0, draw_on="cpu")
    if B > 4:
        e, mask = e.repeat(B // 4, 1, 1), mask.repeat(B // 4, 1)
    pos = generation_position_ids(mask, B, T)
    with torch.no_grad():
        lg, _ = gen4.start(e.to(torch.bfloat16), mask, pos)
        out = ref(inputs_embeds=e, attention_mask=mask, position_ids=pos, past_key_values=DynamicCache(), use_cache=True)
        want = out.logits[:, -1]
        errs = [L.rel(lg, want)]
        am, p = mask, pos
        emb_ref = ref.get_input_embeddings()
        for _ in range(steps):
            tok = want.argmax(-1)
            lg, _ = gen4.step(tok.contiguous())
            am = torch.cat([am, torch.ones(B, 1, device="cuda", dtype=am.dtype)], 1)
            p = p[:, -1:] + 1
            out = ref(inputs_embeds=emb_ref(tok)[:, None], attention_mask=am, position_ids=p, past_key_values=out.past_key_values, use_cache=True)
            want = out.logits[:, -1]
            errs.append(L.rel(lg, want))
    print(name, "B", B, "mxfp4 step rel-L2 max", max(errs))
    assert max(errs) <= 2e-2, errs


@pytest.mark.parametrize("name", NAMES)
def test_packed_layouts_read_back(name):
    """after set_tensor_device in mxfp4 mode the packed q|k|v, interleaved gate|up and lm_head matrices (and the others) read back, in plain
    order, as quantize_blocks_mxfp4 of the SOURCE tensors (codes are compared from the same source, never across a requantisation); the
    host path (fvhd_llm_set_tensor) packs the same bytes"""
    from ml_fastvlm_amd import _lib, quantize_blocks_mxfp4
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, _ = L.models(name, seed=8, layers=1)
    ctxs = [Qwen2Prefill.from_hf(m16, weights=W4)]
    if name == "0.5B":                                            # (the host path moves every matrix through the CPU: the small width only)
        ctxs.append(Qwen2Prefill.from_hf(m16.to("cpu"), device="cuda", weights=W4))
        m16 = m16.to("cuda")
    blk = m16.model.layers[0]
    a, mlp = blk.self_attn, blk.mlp
    # the torch recipe on the device (tests/test_gpu_w4_ops.py: the bytes it gives on the CPU)
    q = [quantize_blocks_mxfp4(t.detach()) for t in (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight)]
    gu = [quantize_blocks_mxfp4(t.detach()) for t in (mlp.gate_proj.weight, mlp.up_proj.weight)]
    want = {
        _lib.MAT_QKV: tuple(torch.cat([t[i] for t in q], 0) for i in (0, 1)),
        _lib.MAT_O: quantize_blocks_mxfp4(a.o_proj.weight.detach()),
        _lib.MAT_GATE_UP: tuple(torch.stack([t[i] for t in gu], 1).reshape(-1, gu[0][i].shape[1]) for i in (0, 1)),
        _lib.MAT_DOWN: quantize_blocks_mxfp4(mlp.down_proj.weight.detach()),
        _lib.MAT_LM_HEAD: quantize_blocks_mxfp4(m16.lm_head.weight.detach()),
    }
    for which, (wc, ws) in want.items():
        for ctx in ctxs:
            codes, scales = ctx.packed_mxfp4(0, which)
            assert torch.equal(scales, ws), which
            assert torch.equal(codes, wc), which
    bf = Qwen2Prefill.from_hf(m16)
    with pytest.raises(_lib.FvhdError, match="MXFP4"):
        bf.packed_mxfp4(0, _lib.MAT_QKV)


@pytest.mark.parametrize("name,layers", [("0.5B", 2), ("7B", 2)])
def test_footprint(name, layers):
    """weight_bytes: per matrix N K / 2 code bytes + N K / 32 scale bytes, plus the unquantised vectors, to the byte.  And the device holds
    no bf16 copy: building the context takes the packed bytes plus the stated dequantisation scratch (2 bytes x the largest matrix),
    within the slack of test_footprint_e4m3."""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, _ = L.models(name, seed=9, layers=layers)
    cfg = m16.config
    bf = Qwen2Prefill.from_hf(m16)
    bf_bytes = bf.weight_bytes
    bf.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    q4 = Qwen2Prefill.from_hf(m16, weights=W4)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    H, I, V, nh, nkv = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.num_attention_heads, cfg.num_key_value_heads
    hd = H // nh
    qkvw = (nh + 2 * nkv) * hd
    mats = [(qkvw, H), (H, nh * hd), (2 * I, H), (H, I)]
    want = layers * (sum(n * k // 2 + n * k // 32 for n, k in mats) + 4 * (H + qkvw + H)) + 4 * H + V * H // 2 + V * H // 32
    print(name, "weight bytes bf16", bf_bytes, "mxfp4", q4.weight_bytes, "ratio", q4.weight_bytes / bf_bytes)
    assert q4.weight_bytes == want
    scratch = 2 * H * max(2 * I, V, qkvw)
    held = free0 - free1
    print(name, "device bytes taken by the mxfp4 context", held, "packed + scratch", q4.weight_bytes + scratch)
    assert held <= q4.weight_bytes + scratch + (64 << 20), (held, q4.weight_bytes, scratch)
    assert held < q4.weight_bytes + scratch + bf_bytes // 2
    e = (0.5 * torch.randn(1, 16, H, device="cuda")).to(torch.bfloat16)
    assert bool(torch.isfinite(q4(e)).all())


def test_refusals():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    lib = _lib.w4_lib()
    # the format after a tensor
    pre = Qwen2Prefill(0, 896, 1, 14, 2, 64, 4864, 4096)
    w = torch.ones(896)
    shape = (C.c_int64 * 1)(896)
    _lib.check(lib.fvhd_llm_set_weight_format(pre._h, _lib.W_MXFP4), "set_weight_format")
    _lib.check(lib.fvhd_llm_set_weight_format(pre._h, _lib.W_BF16), "set_weight_format")      # nothing set yet: still free to choose
    _lib.check(lib.fvhd_llm_set_tensor(pre._h, b"model.norm.weight", C.c_void_p(w.data_ptr()), _lib.F32, shape, 1), "set_tensor")
    assert lib.fvhd_llm_set_weight_format(pre._h, _lib.W_MXFP4) != 0 and b"already set" in lib.fvhd_last_error()
    assert lib.fvhd_llm_set_weight_format(pre._h, 7) != 0
    # odd widths, with a message naming 128
    odd = Qwen2Prefill(0, 64, 1, 1, 1, 64, 64, 64)
    assert lib.fvhd_llm_set_weight_format(odd._h, _lib.W_MXFP4) != 0 and b"128" in lib.fvhd_last_error() and b"MXFP4" in lib.fvhd_last_error()
    # an untied model without its embedding table
    m16, ref = L.models("7B", seed=6)
    e, mask = _prompt(ref, 2, 8, 7)
    p4 = Qwen2Prefill.from_hf(m16, weights=W4)
    gen = Qwen2Generator(p4, 2, 16)
    with pytest.raises(_lib.FvhdError, match="embed_tokens"):
        gen.start(e, mask)
    with pytest.raises(ValueError, match="mxfp4"):
        Qwen2Generator.from_hf(m16, 2, 16, prefill=p4)            # a bf16 generator on an mxfp4 context: an error, not a repack
    with pytest.raises(_lib.FvhdError, match="bf16 weights|e4m3"):
        p4.packed_e4m3(0, _lib.MAT_QKV)
