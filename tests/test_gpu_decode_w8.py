"""Qwen2 prefill and decode steps on e4m3 weights (`weights="fp8_e4m3"`, include/fvhd.h version 504) against torch fp32 / transformers.

Oracle: the models of tests/test_gpu_decode.py (tests/llm_testlib.py::models) with ONE change, quantised=True - every 2-D weight of the
decoder stack and lm_head (for a tied model that is the embedding table too) is replaced by its dequantised value,
`quantize_rows_e4m3` codes * scale, before the bf16 and fp32 copies are
made.  Those values are exact in bf16 and quantise to themselves, so the fp32 oracle holds exactly the weights the library computes with:
what is left is the bf16 arithmetic of the steps, and the budgets are those of the bf16 tests (teacher-forced logits rel-L2 2e-2, greedy
tokens equal where the oracle's top-2 margin exceeds DELTA)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402

pytestmark = pytest.mark.gpu

W8 = "fp8_e4m3"


def _models(name, seed=0, quantised=True, layers=None):
    return L.models(name, seed=seed, quantised=quantised, layers=layers)


def _prompt(ref, B, T, side, seed=0):
    """drawn on the CPU (the seeds below were chosen there)"""
    return L.prompt(ref, B, T, side, seed=seed, draw_on="cpu")


def _teacher_forced(gen, ref, e, mask, steps):
    """start + `steps` steps fed the oracle's argmax -> the rel-L2 of every step's logits against the oracle's"""
    from transformers import DynamicCache
    from ml_fastvlm_amd.qwen2_decode import generation_position_ids
    B, T = mask.shape
    pos = generation_position_ids(mask, B, T)
    with torch.no_grad():
        lg, _ = gen.start(e.to(torch.bfloat16), mask, pos)
        out = ref(inputs_embeds=e, attention_mask=mask, position_ids=pos, past_key_values=DynamicCache(), use_cache=True)
        want = out.logits[:, -1]
        errs = [L.rel(lg, want)]
        am, p = mask, pos
        emb_ref = ref.get_input_embeddings()
        for _ in range(steps):
            tok = want.argmax(-1)
            lg, _ = gen.step(tok.contiguous())
            am = torch.cat([am, torch.ones(B, 1, device="cuda", dtype=am.dtype)], 1)
            p = p[:, -1:] + 1
            out = ref(inputs_embeds=emb_ref(tok)[:, None], attention_mask=am, position_ids=p, past_key_values=out.past_key_values, use_cache=True)
            want = out.logits[:, -1]
            errs.append(L.rel(lg, want))
    return errs


@pytest.mark.parametrize("name,B", [("0.5B", 2), ("1.5B", 2), ("7B", 2), ("0.5B", 40)])
def test_teacher_forced_steps_e4m3(name, B):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16q, ref = _models(name)
    T, steps = 24, 32
    e, mask = _prompt(ref, min(B, 4), T, "left")
    if B > 4:                                                     # 40 rows: the four padded prompts in turn
        e, mask = e.repeat(B // 4, 1, 1), mask.repeat(B // 4, 1)
    gen = Qwen2Generator.from_hf(m16q, B, T + steps + 4, weights=W8)
    assert gen.pre.weight_format == W8
    errs = _teacher_forced(gen, ref, e, mask, steps)
    print(name, "B", B, "e4m3 step rel-L2 max", max(errs))
    assert max(errs) <= 2e-2, errs


# prompt seeds (of `_prompt`, model seed 1, quantised) where the fp32 oracle's top-2 margin exceeds 2 * DELTA at EVERY step of every row for
# 12 new tokens (the first two of seeds 0, 1, 2, ... each) - chosen from the oracle alone (on the CPU), as GREEDY_SEEDS of
# tests/llm_testlib.py was
GREEDY_SEEDS = {"left": [198, 271], "right": [158, 440]}


@pytest.mark.parametrize("side", ["left", "right"])
def test_greedy_equals_transformers_generate_e4m3(side):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16q, ref = _models("0.5B", seed=1)
    B, T, new = 3, 20, 12
    gen = Qwen2Generator.from_hf(m16q, B, T + new, weights=W8)
    assert len(GREEDY_SEEDS[side]) >= 2
    for seed in GREEDY_SEEDS[side]:
        e, mask = _prompt(ref, B, T, side, seed=seed)
        with torch.no_grad():
            r = ref.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                             output_scores=True, return_dict_in_generate=True)
            got = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
            eager = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, eos_token_id=None, pad_token_id=0, graph=False)
        top = torch.stack(r.scores, 1).float().topk(2, -1).values
        assert (top[..., 0] - top[..., 1]).min().item() > L.DELTA          # the seed's precondition (oracle only)
        assert torch.equal(got.cpu(), r.sequences.cpu()), (got.tolist(), r.sequences.tolist())
        assert torch.equal(got, eager)


def test_graph_replay_bit_identical_and_sampling_repeats_e4m3():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16q, ref = _models("0.5B", seed=3)
    B, T, N = 2, 16, 12
    e, mask = _prompt(ref, B, T, "left", seed=4)
    e = e.to(torch.bfloat16)
    gen = Qwen2Generator.from_hf(m16q, B, T + N, weights=W8)
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
        a = gen.sample(e, mask, None, max_new_tokens=N, temperature=0.8, top_k=40, top_p=0.95, seed=11)
        b = gen.sample(e, mask, None, max_new_tokens=N, temperature=0.8, top_k=40, top_p=0.95, seed=11)
        c = gen.sample(e, mask, None, max_new_tokens=N, temperature=0.8, top_k=40, top_p=0.95, seed=11, graph=False)
        d = gen.sample(e, mask, None, max_new_tokens=N, temperature=0.8, top_k=40, top_p=0.95, seed=12)
    assert torch.equal(a, b) and torch.equal(a, c)
    assert not torch.equal(a, d)                                  # 24 draws at temperature 0.8: another seed gives other tokens


def test_batch_invariance_e4m3():
    """40 copies of one prompt: rows in all three batch tiles have the bits of row 0, at every step (start and 12 steps)"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16q, ref = _models("0.5B", seed=2)
    B, T, steps = 40, 20, 12
    e1, m1 = _prompt(ref, 2, T, "left", seed=5)
    e, mask = e1[1:2].expand(B, -1, -1).contiguous().to(torch.bfloat16), m1[1:2].expand(B, -1).contiguous()
    gen = Qwen2Generator.from_hf(m16q, B, T + steps, weights=W8)
    with torch.no_grad():
        lg, ids = gen.start(e, mask)
        for step in range(steps + 1):
            assert bool(torch.isfinite(lg).all())
            assert bool((lg == lg[0]).all()) and bool((ids == ids[0]).all()), step
            if step < steps:
                lg, ids = gen.step()


def test_tied_model_embeds_through_the_dequantised_lm_head_rows():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16q, ref = _models("0.5B", seed=6)
    e, mask = _prompt(ref, 2, 8, "left", seed=7)
    e = e.to(torch.bfloat16)
    tok = torch.tensor([5, 4000], device="cuda")
    pre = Qwen2Prefill.from_hf(m16q, weights=W8)
    tied = Qwen2Generator(pre, 2, 16)                             # no table: dec_embed_w8_kernel on the lm_head codes
    with torch.no_grad():
        tied.start(e, mask)
        a, _ = tied.step(tok)
        a = a.clone()
    # the same context given the table explicitly (a bf16 row gather): lm_head codes * scale ARE the module's bf16 rows
    pre2 = Qwen2Prefill.from_hf(m16q, weights=W8)
    table = Qwen2Generator(pre2, 2, 16, embed_tokens=m16q.get_input_embeddings().weight)
    with torch.no_grad():
        table.start(e, mask)
        b, _ = table.step(tok)
    assert torch.equal(a, b)


def test_untied_model_needs_its_embedding_table_e4m3():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16q, ref = _models("7B", seed=6)
    e, mask = _prompt(ref, 2, 8, "left", seed=7)
    e = e.to(torch.bfloat16)
    pre = Qwen2Prefill.from_hf(m16q, weights=W8)
    gen = Qwen2Generator(pre, 2, 16)
    with pytest.raises(_lib.FvhdError, match="embed_tokens"):
        gen.start(e, mask)
    gen = Qwen2Generator.from_hf(m16q, 2, 16, prefill=pre, weights=W8)           # the bf16 table of the module
    gen.start(e, mask)
    _, ids = gen.step()
    assert ids.shape == (2,)
    with pytest.raises(ValueError, match="fp8_e4m3"):
        Qwen2Generator.from_hf(m16q, 2, 16, prefill=pre)          # a bf16 generator on an e4m3 context: an error, not a repack


def test_weight_format_after_a_tensor_is_refused_by_the_library():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    lib = _lib.w8_lib()
    pre = Qwen2Prefill(0, 896, 1, 14, 2, 64, 4864, 4096)
    w = torch.ones(896)
    shape = (C.c_int64 * 1)(896)
    _lib.check(lib.fvhd_llm_set_weight_format(pre._h, _lib.W_E4M3), "set_weight_format")
    _lib.check(lib.fvhd_llm_set_weight_format(pre._h, _lib.W_BF16), "set_weight_format")      # nothing set yet: still free to choose
    _lib.check(lib.fvhd_llm_set_tensor(pre._h, b"model.norm.weight", C.c_void_p(w.data_ptr()), _lib.F32, shape, 1), "set_tensor")
    assert lib.fvhd_llm_set_weight_format(pre._h, _lib.W_E4M3) != 0
    assert b"already set" in lib.fvhd_last_error()
    assert lib.fvhd_llm_set_weight_format(pre._h, 7) != 0
    odd = Qwen2Prefill(0, 64, 1, 1, 1, 64, 64, 64)                # hidden 64: fine for the bf16 prefill, not a multiple of 128
    assert lib.fvhd_llm_set_weight_format(odd._h, _lib.W_E4M3) != 0 and b"128" in lib.fvhd_last_error()


@pytest.mark.parametrize("name", ["0.5B", "7B"])
def test_packed_layouts_read_back(name):
    """after set_tensor_device in e4m3 mode the packed q|k|v and interleaved gate|up matrices (and the others) read back, in [N, K] order,
    as quantize_rows_e4m3 of the packed bf16 matrix; the host path (fvhd_llm_set_tensor) packs the same bytes"""
    from ml_fastvlm_amd import _lib, quantize_rows_e4m3
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, _ = _models(name, seed=8, quantised=False)
    pre = Qwen2Prefill.from_hf(m16, weights=W8)
    host = Qwen2Prefill.from_hf(m16.to("cpu"), device="cuda", weights=W8)
    m16 = m16.to("cuda")
    for layer, blk in enumerate(m16.model.layers):
        a, mlp = blk.self_attn, blk.mlp
        packed = {
            _lib.MAT_QKV: torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0),
            _lib.MAT_O: a.o_proj.weight,
            _lib.MAT_GATE_UP: torch.stack([mlp.gate_proj.weight, mlp.up_proj.weight], 1).reshape(-1, mlp.gate_proj.weight.shape[1]),
            _lib.MAT_DOWN: mlp.down_proj.weight,
        }
        for which, w in packed.items():
            want_codes, want_scale = quantize_rows_e4m3(w.detach().cpu())         # the recipe on the CPU: the reference
            for ctx in (pre, host):
                codes, scale = ctx.packed_e4m3(layer, which)
                assert torch.equal(scale.cpu(), want_scale), (layer, which)
                assert torch.equal(codes.view(torch.uint8).cpu(), want_codes.view(torch.uint8)), (layer, which)
    want_codes, want_scale = quantize_rows_e4m3(m16.lm_head.weight.detach().cpu())
    codes, scale = pre.packed_e4m3(0, _lib.MAT_LM_HEAD)
    assert torch.equal(scale.cpu(), want_scale) and torch.equal(codes.view(torch.uint8).cpu(), want_codes.view(torch.uint8))
    bf = Qwen2Prefill.from_hf(m16)
    with pytest.raises(_lib.FvhdError, match="bf16 weights"):
        bf.packed_e4m3(0, _lib.MAT_QKV)


@pytest.mark.parametrize("name,layers", [("0.5B", 2), ("7B", 2)])
def test_footprint_e4m3(name, layers):
    """weight_bytes: 1 byte per matrix element instead of 2, plus 4 bytes per output row and the unquantised vectors - at these shapes
    (rows of 896 .. 18944 elements) <= 0.5 + 4 / 896 / 2 + the vectors' share < 0.52 of the bf16 context's.  And the device holds no second
    bf16 copy: building the e4m3 context takes the packed bytes plus the stated dequantisation scratch (2 bytes x the largest matrix)."""
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    m16, _ = _models(name, seed=9, quantised=False, layers=layers)
    cfg = m16.config
    bf = Qwen2Prefill.from_hf(m16)
    bf_bytes = bf.weight_bytes
    bf.close()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]          # the device's own count: the library's allocations and torch's segments alike
    q8 = Qwen2Prefill.from_hf(m16, weights=W8)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert q8.weight_format == W8 and bf.weight_format == "bf16"
    print(name, "weight bytes bf16", bf_bytes, "e4m3", q8.weight_bytes, "ratio", q8.weight_bytes / bf_bytes)
    assert q8.weight_bytes <= 0.52 * bf_bytes
    H, I, V = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size
    scratch = 2 * H * max(2 * I, V, (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * (H // cfg.num_attention_heads))
    held = free0 - free1
    print(name, "device bytes taken by the e4m3 context", held, "packed + scratch", q8.weight_bytes + scratch)
    assert held <= q8.weight_bytes + scratch + (64 << 20), (held, q8.weight_bytes, scratch)
    assert held < q8.weight_bytes + scratch + bf_bytes // 2       # far from a bf16 copy of the matrices on top
    # the prefill of such a context agrees with the bf16 context's on dequantised weights (tests above); here: it runs and is finite
    e = (0.5 * torch.randn(1, 16, H, device="cuda")).to(torch.bfloat16)
    assert bool(torch.isfinite(q8(e)).all())
