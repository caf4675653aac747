"""Qwen2 decode steps at cache sizes where the attention splits its key axis (csrc/llm_step.hip att_plan: capacity > 64 and a grid that
does not fill the chip): prompts of 285 and 600 tokens in a cache of 2304 positions, left padding longer than a key slice.  Every case
first asserts, from att_plan's rule restated here, that it runs with more than one key slice - so the in-launch combine across slices,
the len_add = 1 call form, the attention's counter offset and the scratch sizing of fvhd_llm_cache_reserve are what is measured.

Oracle: transformers' Qwen2ForCausalLM in fp32 on the same bf16-rounded weights (tests/llm_testlib.py::models).  Budget: the step
budget of test_teacher_forced_steps, rel-L2 <= 2e-2 of the step logits, applied PER ROW.  The stock bf16 transformers model is measured
against the same oracle on the same inputs and printed beside ours.

Measured on an MI355X (per-row maximum over the prefill and 8 steps; ours / stock bf16):
  0.5B  T=285  B=1 7.1e-3 / 1.5e-2   B=8, 16 8.3e-3 / 1.5e-2        0.5B  T=600  B=1 6.7e-3 / 1.8e-2   B=8, 16 7.9e-3 / 2.0e-2
  7B    T=285  B=1 9.7e-3 / 7.3e-2                                  7B    T=600  B=1 1.0e-2 / 1.6e-1
so the 2e-2 budget holds per row at these lengths with a factor of two to spare, and no case needed the stock model's number."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 2304


def _att_slices(cap, heads):
    """att_plan (csrc/llm_step.hip), restated: -> (slices, keys per slice)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    want = (2 * ncu + heads - 1) // heads
    s = max(1, min(want, (cap + 63) // 64, 32))
    chunk = ((cap + s - 1) // s + 63) // 64 * 64
    return (cap + chunk - 1) // chunk, chunk


def _assert_split(m16, reserved_batch, cap=CAP):
    S, chunk = _att_slices(cap, reserved_batch * m16.config.num_attention_heads)
    assert S > 1, f"the attention of this case runs in one slice (capacity {cap}, batch {reserved_batch}): it does not test the key split"
    return S, chunk


def _long_prompt(ref, B, T, seed=0):
    """prompt's embeddings with row b left-padded by 97 * b positions (capped below T): more than one key slice from row 2 on"""
    e, mask = L.prompt(ref, B, T, "left", seed=seed)
    mask[:] = 1
    for b in range(B):
        mask[b, :min(97 * b, T - 1)] = 0
    return e, mask


def _row_rel(a, b):
    a, b = a.float(), b.float()
    return (a - b).norm(dim=-1) / b.norm(dim=-1).clamp_min(1e-30)


def _forced_steps(gen, m16, ref, e, mask, steps):
    """teacher-forced steps (the oracle's greedy tokens are fed to all three) -> (ours, stock bf16) per-row rel-L2 maxima [B], fed tokens"""
    from transformers import DynamicCache
    from ml_fastvlm_amd.qwen2_decode import generation_position_ids
    B, T = mask.shape
    pos = generation_position_ids(mask, B, T)
    with torch.no_grad():
        lg, _ = gen.start(e.to(torch.bfloat16), mask, pos)
        out = ref(inputs_embeds=e, attention_mask=mask, position_ids=pos, past_key_values=DynamicCache(), use_cache=True)
        o16 = m16(inputs_embeds=e.to(torch.bfloat16), attention_mask=mask, position_ids=pos, past_key_values=DynamicCache(), use_cache=True)
        want = out.logits[:, -1]
        ours, stock = _row_rel(lg, want), _row_rel(o16.logits[:, -1], want)
        am, p, fed = mask, pos, []
        for _ in range(steps):
            tok = want.argmax(-1)
            fed.append(tok)
            lg, _ = gen.step(tok.contiguous())
            am = torch.cat([am, torch.ones(B, 1, device="cuda", dtype=am.dtype)], 1)
            p = p[:, -1:] + 1
            out = ref(inputs_embeds=ref.get_input_embeddings()(tok)[:, None], attention_mask=am, position_ids=p, past_key_values=out.past_key_values,
                      use_cache=True)
            o16 = m16(inputs_embeds=m16.get_input_embeddings()(tok)[:, None], attention_mask=am, position_ids=p, past_key_values=o16.past_key_values,
                      use_cache=True)
            want = out.logits[:, -1]
            ours, stock = torch.maximum(ours, _row_rel(lg, want)), torch.maximum(stock, _row_rel(o16.logits[:, -1], want))
    return ours, stock, fed


@pytest.mark.parametrize("name,B,T", [("0.5B", 1, 285), ("0.5B", 8, 285), ("0.5B", 16, 285), ("0.5B", 1, 600), ("0.5B", 8, 600), ("0.5B", 16, 600),
                                      ("7B", 1, 285), ("7B", 1, 600)])
def test_teacher_forced_steps_in_the_split_regime(name, B, T):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = L.models(name)
    S, chunk = _assert_split(m16, B)
    e, mask = _long_prompt(ref, B, T)
    gen = Qwen2Generator.from_hf(m16, B, CAP)
    ours, stock, _ = _forced_steps(gen, m16, ref, e, mask, 8)
    print(f"{name} B={B} T={T} capacity={CAP} slices={S} x {chunk}: per-row step rel-L2 max ours {ours.max().item():.3e}, stock bf16 {stock.max().item():.3e}")
    assert ours.max().item() <= 2e-2, (ours.tolist(), stock.tolist())


def test_start_plus_steps_equals_one_long_prefill():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = L.models("0.5B")
    B, T, k = 2, 285, 6
    _assert_split(m16, B)
    e, _ = L.prompt(ref, B, T, "left")
    ones = torch.ones(B, T, device="cuda", dtype=torch.long)
    gen = Qwen2Generator.from_hf(m16, B, CAP)
    _, _, fed = _forced_steps(gen, m16, ref, e, ones, k)
    with torch.no_grad():
        gen.start(e.to(torch.bfloat16), ones)
        for i in range(k):
            lg, _ = gen.step(fed[i].contiguous())
        long = torch.cat([e.to(torch.bfloat16), m16.get_input_embeddings()(torch.stack(fed[:k], 1))], 1)
        pre = gen.pre(long, torch.ones(B, T + k, device="cuda", dtype=torch.long))
    r = _row_rel(lg, pre)
    assert r.max().item() <= 1e-2, r.tolist()


def test_started_batch_smaller_than_the_reserved_one_after_a_full_generation():
    """reserved 8, a B = 8 generation fills every cache row, then 3 rows start: within the budget, and bit-identical to the same three rows
    on a freshly reserved batch-8 generator - the unused rows' stale keys, mask bytes and positions must not matter.  (Not compared with a
    batch-3 reservation: att_plan sizes its slices by the reserved batch.)"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = L.models("0.5B", seed=2)
    _assert_split(m16, 8)
    e8, mask8 = _long_prompt(ref, 8, 600, seed=1)
    e3, mask3 = _long_prompt(ref, 3, 285, seed=2)
    used = Qwen2Generator.from_hf(m16, 8, CAP)
    used.greedy(e8.to(torch.bfloat16), mask8, None, max_new_tokens=10, pad_token_id=0)
    fresh = Qwen2Generator.from_hf(m16, 8, CAP)
    ours, stock, fed = _forced_steps(used, m16, ref, e3, mask3, 6)
    print(f"3 of 8 rows after a full generation: per-row step rel-L2 max ours {ours.max().item():.3e}, stock bf16 {stock.max().item():.3e}")
    assert ours.max().item() <= 2e-2, ours.tolist()
    logs = []
    with torch.no_grad():
        for gen in (used, fresh):
            log = []
            lg, ids = gen.start(e3.to(torch.bfloat16), mask3)
            log.append((lg.clone(), ids.clone()))
            for t in fed:
                lg, ids = gen.step(t.contiguous())
                log.append((lg.clone(), ids.clone()))
            logs.append(log)
    for i, ((la, ia), (lb, ib)) in enumerate(zip(*logs)):
        assert torch.equal(la, lb) and torch.equal(ia, ib), f"step {i}: stale rows changed the result"


def test_restart_with_a_shorter_prompt():
    """start(600 tokens) + 8 steps, then start(285 tokens) on the same generator: the following steps are bit-identical to a fresh
    generator's - stale cache rows and mask bytes beyond the new length are not read"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = L.models("0.5B", seed=3)
    B = 4
    _assert_split(m16, B)
    e6, mask6 = _long_prompt(ref, B, 600, seed=3)
    e2, mask2 = _long_prompt(ref, B, 285, seed=4)
    used, fresh = Qwen2Generator.from_hf(m16, B, CAP), Qwen2Generator.from_hf(m16, B, CAP)
    logs = []
    with torch.no_grad():
        used.start(e6.to(torch.bfloat16), mask6)
        for _ in range(8):
            used.step()
        for gen in (used, fresh):
            log = []
            lg, ids = gen.start(e2.to(torch.bfloat16), mask2)
            log.append((lg.clone(), ids.clone()))
            for _ in range(8):
                lg, ids = gen.step()
                log.append((lg.clone(), ids.clone()))
            logs.append(log)
    for i, ((la, ia), (lb, ib)) in enumerate(zip(*logs)):
        assert torch.equal(la, lb) and torch.equal(ia, ib), f"step {i} after the restart differs from a fresh generator's"
    assert used.cache_state() == (285 + 8, 0)


def test_graph_replay_bit_identical_in_the_split_regime():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = L.models("0.5B", seed=3)
    B, T, N = 3, 285, 16
    _assert_split(m16, B)
    e, mask = _long_prompt(ref, B, T, seed=4)
    e = e.to(torch.bfloat16)
    gen = Qwen2Generator.from_hf(m16, B, CAP)
    eager = []
    with torch.no_grad():
        gen.start(e, mask)
        for _ in range(N):
            lg, ids = gen.step()
            eager.append((lg.clone(), ids.clone()))
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
            assert torch.equal(ids, eager[i][1]) and torch.equal(lg, eager[i][0]), i
    assert gen.cache_state() == (T + N, 0)


LONG_GREEDY_SEED = 13      # the first prompt seed of 0, 1, 2, .. (model seed 1) that meets the precondition asserted below, found on an MI355X


def test_greedy_equals_transformers_generate_on_a_long_prompt():
    """T = 285, B = 3, 12 new tokens under the agree rule of tests/llm_testlib.py.  The prompt seed is one for which the fp32 oracle keeps a top-2
    margin > 2 * L.DELTA for the first 8 steps of every row (asserted from the oracle's scores alone), so at least 24 tokens are compared"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = L.models("0.5B", seed=1)
    B, T, new = 3, 285, 12
    _assert_split(m16, B)
    e, mask = _long_prompt(ref, B, T, seed=LONG_GREEDY_SEED)
    with torch.no_grad():
        r = ref.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                         output_scores=True, return_dict_in_generate=True)
    top = torch.stack(r.scores, 1).float().topk(2, -1).values
    assert (top[:, :8, 0] - top[:, :8, 1]).min().item() > 2 * L.DELTA          # the seed's precondition (oracle only)
    gen = Qwen2Generator.from_hf(m16, B, CAP)
    with torch.no_grad():
        got = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
    n = L.agree(got, r.sequences, r.scores)
    print(f"long-prompt greedy: steps compared per row {n}")
    assert min(n) >= 8 and sum(n) >= 24, n
