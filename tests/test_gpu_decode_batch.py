"""Decode steps of 17 .. 64 sequences (csrc/llm_decode.hip batch tiles, include/fvhd.h version 503) against tests/decode_reference.py,
the fp32 oracle and transformers' generate - with the helpers of tests/llm_testlib.py and the shapes and tolerances of test_gpu_decode.py /
test_gpu_decode_ops.py / test_gpu_sample*.py for the same operations (the arithmetic per row is the 16-row kernel's, so no new tolerance):

  single ops       |got - want| <= 1e-2 |want| + 1e-2 rms(want_row), rms per batch row (fp32 logits: 2e-3)
  step logits      rel-L2 <= 2e-2 against the fp32 oracle
  greedy tokens    equal to transformers' where the oracle's top-2 margin exceeds DELTA at every step (asserted on the oracle)

and bit for bit: a B-row launch equals the same op on rows [0, 16), [16, 32), .. with the same `splits` - a batch tile IS the 16-row
kernel's arithmetic - and copies of a prompt in different batch tiles give identical step logits."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as R  # noqa: E402
from llm_testlib import (DELTA, GREEDY_SEEDS, SENT, lib, rel,  # noqa: E402,F401
                         agree as _agree, blocks as _blocks, close_by_batch_row as _close, dec_attention as _attention, dec_gemm as _gemm,
                         dec_lm_argmax as _lm, guard_intact as _guard_intact, guarded_rows as _guarded, models as _models, nb as _nb,
                         padded_mask, plan_splits as _plan_splits, prompt as _prompt, ptr as _p, row_scales as _row_scales, stream as _st,
                         wide_prompt as _wide_prompt)

pytestmark = pytest.mark.gpu

GAP = 1e-5            # a draw closer than this to a CDF / group boundary is not pinned by the reference (test_gpu_sample_edges.py)
WIDE = [17, 24, 32, 33, 48, 63, 64]


# ---- 1. the weight-streaming GEMM ---------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(80, 256), (896, 4864), (9728, 896), (3584, 18944), (37888, 3584)]


@pytest.mark.parametrize("epi", ["resid", "swiglu"])
@pytest.mark.parametrize("N,K", GEMM_SHAPES)
def test_dec_gemm_wide_elementwise_and_bits_by_rows(lib, N, K, epi):
    worst = 0.0
    for B in WIDE:
        g = torch.Generator(device="cuda").manual_seed(N + K + B)
        x = (torch.randn(B, K, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
        W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(torch.bfloat16)
        nw = (1 + 0.3 * torch.randn(K, device="cuda", generator=g)).float()
        resid = (torch.randn(B, N, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
        for norm in (nw, None):
            want = R.dec_gemm_ref(x, norm, 1e-6, W, resid, epi)
            for splits in sorted({1, 3, _plan_splits(N, K)}):
                what = f"N={N} K={K} B={B} {epi} norm={norm is not None} splits={splits}"
                got = _gemm(lib, epi, x, norm, W, resid, splits)
                worst = max(worst, _close(got, want, what))
                by_rows = torch.cat([_gemm(lib, epi, x[a:b], norm, W, resid[a:b], splits) for a, b in _blocks(B)])
                assert torch.equal(got.view(torch.int16), by_rows.view(torch.int16)), what + ": differs from the 16-row launches"
    print(f"dec_gemm wide N={N} K={K} {epi}: worst err / bound {worst:.3f}")


# ---- 2. q|k|v + rope + cache append ---------------------------------------------------------------------------------------------------
QKV_SHAPES = [(14, 2, 64, 896), (12, 2, 128, 1536), (28, 4, 128, 3584)]


def _qkv(lib, x, nw, W, bias, pos, table, P, nh, nkv, hd, cap, slot, splits, rows):
    """one launch on `rows` cache rows (>= B) -> (q [B, nh * hd], k cache, v cache as int16)"""
    from ml_fastvlm_amd import _lib
    B, H = x.shape
    N = W.shape[0]
    kc = torch.full((rows, nkv, cap, hd), SENT, device="cuda", dtype=torch.int16)
    vc = torch.full((rows, nkv, cap, hd), SENT + 1, device="cuda", dtype=torch.int16)
    qbuf, q = _guarded(nh * hd, B)
    length = torch.tensor([slot], device="cuda", dtype=torch.int32)
    part = torch.empty(splits * N * 16 * _nb(B), device="cuda") if splits > 1 else None
    cnt = torch.zeros((N // 16 + 3) // 4, device="cuda", dtype=torch.int32) if splits > 1 else None
    _lib.check(lib.fvhd_op_dec_qkv(_st(), _p(x), B, H, _p(nw), 1e-6, _p(W), _p(bias), _p(q), _p(pos), _p(table), P, 1e6, _p(kc), _p(vc), cap,
                                   _p(length), nh, nkv, hd, _p(part), _p(cnt), splits), "dec_qkv")
    torch.cuda.synchronize()
    assert _guard_intact(qbuf, B * nh * hd) and (cnt is None or int(cnt.abs().sum()) == 0)
    return q.clone(), kc, vc


@pytest.mark.parametrize("nh,nkv,hd,H", QKV_SHAPES)
@pytest.mark.parametrize("B", [17, 40, 64])
def test_dec_qkv_wide(lib, nh, nkv, hd, H, B):
    from ml_fastvlm_amd.qwen2_prefill import rope_table
    g = torch.Generator(device="cuda").manual_seed(hd + B + H)
    N, cap, P, slot = (nh + 2 * nkv) * hd, 40, 8192, 17
    x = (torch.randn(B, H, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
    W = (torch.randn(N, H, device="cuda", generator=g) / H ** 0.5).to(torch.bfloat16)
    bias = 0.1 * torch.randn(N, device="cuda", generator=g)
    nw = (1 + 0.3 * torch.randn(H, device="cuda", generator=g)).float()
    pos = torch.arange(B, device="cuda", dtype=torch.long) * 121 + 5
    pos[0] = 0
    pos[-1] = 9000                                                # beyond the table: computed on the fly
    table = rope_table(P, hd, 1e6, "cuda")
    qw, kw, vw = R.dec_qkv_ref(x, nw, 1e-6, W, bias, pos, nh, nkv, hd, 1e6)
    worst = 0.0
    for splits in (1, 4, _plan_splits(N, H)):
        what = f"B={B} splits={splits}"
        q, kc, vc = _qkv(lib, x, nw, W, bias, pos, table, P, nh, nkv, hd, cap, slot, splits, rows=B + 2)
        worst = max(worst, _close(q.view(B, nh, hd), qw, "q " + what))
        worst = max(worst, _close(kc.view(torch.bfloat16)[:B, :, slot], kw, "k " + what))
        worst = max(worst, _close(vc.view(torch.bfloat16)[:B, :, slot], vw, "v " + what))
        others = torch.ones(cap, dtype=torch.bool, device="cuda")
        others[slot] = False
        assert bool((kc[:, :, others] == SENT).all()) and bool((vc[:, :, others] == SENT + 1).all()), "cache written outside the slot: " + what
        assert bool((kc[B:] == SENT).all()) and bool((vc[B:] == SENT + 1).all()), "cache rows >= B written: " + what
        for a, b in _blocks(B):                                   # bit for bit the 16-row launches
            q1, k1, v1 = _qkv(lib, x[a:b], nw, W, bias, pos[a:b].contiguous(), table, P, nh, nkv, hd, cap, slot, splits, rows=b - a)
            assert torch.equal(q[a:b].view(torch.int16), q1.view(torch.int16)), (what, a)
            assert torch.equal(kc[a:b], k1) and torch.equal(vc[a:b], v1), (what, a)
    print(f"dec_qkv wide nh={nh} hd={hd} H={H} B={B}: worst err / bound {worst:.3f}")


# ---- 3. single-query attention over the cache ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,nkv", [(64, 14, 2), (128, 28, 4)])
@pytest.mark.parametrize("length,cap", [(1, 64), (285, 300), (2049, 2050)])
@pytest.mark.parametrize("B", [40, 64])
def test_dec_attention_wide(lib, hd, nh, nkv, length, cap, B):
    g = torch.Generator(device="cuda").manual_seed(hd * 7 + length + B)
    q = (torch.randn(B, nh * hd, device="cuda", generator=g) * torch.linspace(0.5, 2.0, B, device="cuda")[:, None]).to(torch.bfloat16)
    kc = torch.randn(B, nkv, cap, hd, device="cuda", generator=g).to(torch.bfloat16)
    vc = (torch.randn(B, nkv, cap, hd, device="cuda", generator=g) * _row_scales(B, g)[:, None, None, None]).to(torch.bfloat16)
    worst = 0.0
    for side in ("left", "right"):
        mask = padded_mask(B, cap, length, side, wrap=13)          # row b: b % 13 + 1 steps of padded keys
        want = R.dec_attention_ref(q, kc, vc, mask, length)
        for splits in (1, 9):
            got = _attention(lib, q, kc, vc, mask, length, splits)
            worst = max(worst, _close(got, want, f"{side} length={length} cap={cap} B={B} splits={splits}"))
            assert torch.equal(got, _attention(lib, q, kc, vc, mask, length, splits))
    print(f"dec_attention wide hd={hd} nh={nh} length={length} B={B}: worst err / bound {worst:.3f}")


# ---- 4. lm_head + argmax -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,H", [(151936, 896), (4112, 896), (152064, 3584)])
@pytest.mark.parametrize("B", [17, 64])
def test_dec_lm_argmax_wide_and_ties(lib, V, H, B):
    g = torch.Generator(device="cuda").manual_seed(V + H + B)
    x = (torch.randn(B, H, device="cuda", generator=g) * _row_scales(B, g)[:, None]).to(torch.bfloat16)
    W = (torch.randn(V, H, device="cuda", generator=g) / H ** 0.5).to(torch.bfloat16)
    nw = (1 + 0.3 * torch.randn(H, device="cuda", generator=g)).float()
    xa = R.normed_operand(x, nw, 1e-6)
    want = torch.cat([xa @ W[i:i + 32768].double().t() for i in range(0, V, 32768)], 1)
    lg, ids = _lm(lib, x, nw, W)
    _close(lg, want, f"logits V={V} H={H} B={B}", rtol=2e-3, atol_rms=2e-3)
    assert torch.equal(ids, lg.argmax(-1))
    _, ids2 = _lm(lib, x, nw, W, logits=False)
    assert torch.equal(ids, ids2)
    # planted ties for rows of different batch tiles: the row's winning weight row moved to index pairs inside a lane, across waves,
    # across workgroups and in the ragged tail - the lowest index must win, in every tile
    pairs = [(1, 2), (645, 661), (700, 3000), (0, 2000), (V - 40, V - 1), (V - 2, V - 1)]
    for r in sorted({0, 16, B - 1}):
        best = int(ids[r])
        wrow, keep_best = W[best].clone(), W[best].clone()
        W[best] = 0
        for lo, hi in pairs:
            keep = W[[lo, hi]].clone()
            W[lo], W[hi] = wrow, wrow
            lg2, got = _lm(lib, x, nw, W)
            assert float(lg2[r, lo]) == float(lg2[r, hi]) == float(lg2[r].max()), (r, lo, hi)
            assert int(got[r]) == lo, (r, lo, hi, int(got[r]))
            assert torch.equal(got, lg2.argmax(-1))               # torch.argmax: the lowest index on ties
            _, got2 = _lm(lib, x, nw, W, logits=False)
            assert torch.equal(got, got2)
            W[[lo, hi]] = keep
        W[best] = keep_best


# ---- model-level tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["0.5B", "7B"])
def test_teacher_forced_steps_wide(name):
    from transformers import DynamicCache
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator, generation_position_ids
    m16, ref = _models(name)
    B, T, steps = 40, 24, 16
    e, mask = _wide_prompt(ref, B, T)
    gen = Qwen2Generator.from_hf(m16, 48, T + steps + 4)
    pos = generation_position_ids(mask, B, T)
    with torch.no_grad():
        lg, ids = gen.start(e.to(torch.bfloat16), mask, pos)
        out = ref(inputs_embeds=e, attention_mask=mask, position_ids=pos, past_key_values=DynamicCache(), use_cache=True)
        want = out.logits[:, -1]
        errs = [rel(lg, want)]
        am, p = mask, pos
        emb_ref = ref.get_input_embeddings()
        for _ in range(steps):
            tok = want.argmax(-1)
            lg, _ = gen.step(tok.contiguous())
            am = torch.cat([am, torch.ones(B, 1, device="cuda", dtype=am.dtype)], 1)
            p = p[:, -1:] + 1
            out = ref(inputs_embeds=emb_ref(tok)[:, None], attention_mask=am, position_ids=p, past_key_values=out.past_key_values, use_cache=True)
            want = out.logits[:, -1]
            errs.append(rel(lg, want))
            worst_row = max(rel(lg[b], want[b]) for b in range(B))
            assert worst_row <= 2e-2, worst_row                   # no row hides behind the pooled norm
    print(name, "B = 40 step rel-L2 max", max(errs))
    assert max(errs) <= 2e-2, errs
    # three copies of 16 distinct prompts: rows b, b + 16, b + 32 sit in three batch tiles and must agree bit for bit at every step
    e3, mask3 = _wide_prompt(ref, 48, T, seed=1, distinct=16)
    with torch.no_grad():
        lg, ids = gen.start(e3.to(torch.bfloat16), mask3)
        for i in range(steps):
            assert torch.equal(ids[:16], ids[16:32]) and torch.equal(ids[:16], ids[32:])
            lg, ids = gen.step(ids.clone())
            assert torch.equal(lg[:16], lg[16:32]) and torch.equal(lg[:16], lg[32:48]), f"step {i}: the copies differ between batch tiles"
            assert len({tuple(r) for r in lg[:16, :8].tolist()}) == 16                   # the 16 prompts themselves are distinct


@pytest.mark.parametrize("B", [48, 33])
@pytest.mark.parametrize("side", ["left", "right"])
def test_greedy_equals_transformers_generate_wide(side, B):
    """the three rows of the 16-row test, interleaved (row i = prompt i % 3) so that every 16-row tile holds all three and the last tile of
    33 holds one row: equal to transformers' greedy generate token for token, also with an EOS list that every row emits"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _models("0.5B", seed=1)
    T, new = 20, 12
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    idx = torch.arange(B, device="cuda") % 3
    for seed in GREEDY_SEEDS[side]:
        e3, mask3 = _prompt(ref, 3, T, side, seed=seed)
        e, mask = e3[idx].contiguous(), mask3[idx].contiguous()
        with torch.no_grad():
            r = ref.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                             output_scores=True, return_dict_in_generate=True)
            got = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, eos_token_id=None, pad_token_id=0)
        top = torch.stack(r.scores, 1).float().topk(2, -1).values
        assert (top[..., 0] - top[..., 1]).min().item() > DELTA          # the seed's precondition (oracle only)
        assert got.shape == (B, new) and torch.equal(got.cpu(), r.sequences.cpu()), (got.tolist(), r.sequences.tolist())
        eos = [int(r.sequences[b, 2 + 2 * b]) for b in range(3)]
        with torch.no_grad():
            r2 = ref.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=eos, pad_token_id=7,
                              output_scores=True, return_dict_in_generate=True)
            got2 = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, eos_token_id=eos, pad_token_id=7, poll_every=4)
        assert r2.sequences.shape[1] < new
        assert got2.shape == r2.sequences.shape and torch.equal(got2.cpu(), r2.sequences.cpu()), (got2.tolist(), r2.sequences.tolist())


def test_sampling_wide():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator, philox_uniform
    m16, ref = _models("0.5B", seed=1)
    B, T, new = 40, 20, 12
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    e, mask = _wide_prompt(ref, B, T, seed=2)
    e = e.to(torch.bfloat16)
    # top_k = 1 equals greedy on every row (precondition on our logits: no tie at the row max)
    g = gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0)
    with torch.no_grad():
        lg, _ = gen.start(e, mask)
        for i in range(new):
            top = lg.topk(2, -1).values
            assert bool((top[:, 0] > top[:, 1]).all()), i
            if i + 1 < new:
                lg, _ = gen.step(g[:, i].contiguous())
    s = gen.sample(e, mask, None, max_new_tokens=new, temperature=1.0, top_k=1, top_p=1.0, seed=99, pad_token_id=0)
    assert torch.equal(s, g), (s.tolist(), g.tolist())
    s = gen.sample(e, mask, None, max_new_tokens=new, temperature=0.3, top_k=1, top_p=0.5, seed=5, pad_token_id=0, graph=False)
    assert torch.equal(s, g)
    # predict.py's settings (temperature 0.2, transformers' default top_k = 50, no top_p), a fixed seed: eager equals graph replay
    Tm, k, p = 0.2, 50, 1.0
    kw = dict(max_new_tokens=new, temperature=Tm, top_k=k, top_p=p, pad_token_id=0)
    a = gen.sample(e, mask, None, seed=11, graph=True, **kw)
    b = gen.sample(e, mask, None, seed=11, graph=False, **kw)
    assert a.shape == (B, new) and torch.equal(a, b), (a.tolist(), b.tolist())
    assert gen.cache_state() == (T + new - 1, 0)
    # one step's chosen ids against the reference draw: row r's u is Philox with counter (r, n, 0, 0), r the GLOBAL row.  The step's logits
    # do not depend on the seed (the fed tokens are given), so the seed is picked on the CPU, from the reference alone, such that at most
    # 10 % of the rows have u within GAP of a CDF boundary (those rows are not pinned by the reference and are skipped)
    fed = g[:, 0].contiguous()
    n = T + 1                                                     # the cache length when the step's token is chosen
    with torch.no_grad():
        gen.set_sampling(False)
        gen.start(e, mask)
        lg0 = gen.step(fed)[0].clone().cpu()
    refs = [R.sample_ref(lg0[r], Tm, k, p) for r in range(B)]

    def plan(seed):
        picks, skipped = [], 0
        for r in range(B):
            u = philox_uniform(seed, r, n)
            adm = R.admissible_tokens(refs[r], u, tol=GAP)
            if int(adm.sum()) != 1 or refs[r]["margin"] < GAP:
                picks.append(None)
                skipped += 1
            else:
                picks.append(int((refs[r]["kept"] & (refs[r]["cdf"] > u)).nonzero()[0, 0]))
                assert bool(adm[picks[-1]])
        return picks, skipped

    seed = next(sd for sd in range(1, 200) if plan(sd)[1] <= B // 10)
    picks, skipped = plan(seed)
    assert skipped <= B // 10
    with torch.no_grad():
        gen.set_sampling(True, Tm, k, p, seed)
        try:
            gen.start(e, mask)
            lg1, ids = gen.step(fed)
            lg1, ids = lg1.cpu(), ids.cpu()
        finally:
            gen.set_sampling(False)
    assert torch.equal(lg0, lg1)
    checked = 0
    for r in range(B):
        if picks[r] is not None:
            assert int(ids[r]) == picks[r], (r, int(ids[r]), picks[r])
            checked += 1
    print(f"sampling B = 40: seed {seed}, {checked} rows pinned by the reference, {skipped} skipped")
    assert checked >= 36 and any(picks[r] is not None for r in range(16, B))
    # the draws of rows >= 16 are their own, not those of rows 0 .. 15 (a sampler that took the row within its block of 16 would repeat u)
    assert len({philox_uniform(seed, r, n) for r in range(B)}) == B


def test_graph_replay_bit_identical_and_overflow_wide():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _models("0.5B", seed=3)
    B, T, N = 64, 16, 12
    e, mask = _wide_prompt(ref, B, T, seed=4)
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


def test_library_generate_standin_32_rows():
    """test_gpu_decode.py's stand-in LLaVA model (Qwen2ForCausalLM + our tower / projector + multimodal_splice) with 32 images in one
    `_make_library_generate`-patched generate call: it stays on the library and agrees with transformers up to each row's first near-tie"""
    from types import MethodType, SimpleNamespace
    import ml_fastvlm_amd as fv
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd import splice as S
    from ml_fastvlm_amd import synth
    m16, ref = _models("0.5B", seed=5)
    res, hidden, B = 256, 896, 32
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
    ids = torch.randint(10, 4000, (B, 12), generator=g)
    ids[:, 3] = -200                                              # IMAGE_TOKEN_INDEX
    mask = torch.ones_like(ids)
    for b in range(B):
        if b % 4:
            mask[b, 12 - (b % 4):] = 0
    ids, mask = ids.cuda(), mask.cuda()
    images = synth.synthetic_images(B, res, seed=0).to("cuda", torch.bfloat16)
    new = 16

    def never(self, *a, **kw):
        raise AssertionError("the call was left to the reference's generate")

    generate = builder._make_library_generate(never)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with torch.no_grad():
            got = generate(m16, ids, images=images, attention_mask=mask, max_new_tokens=new, do_sample=False, pad_token_id=0, use_cache=True)
    assert not [x for x in w if "stays on the reference" in str(x.message)], [str(x.message) for x in w]
    with torch.no_grad():
        _, pos, am, _, emb, _ = prepare(m16, ids, None, mask, None, None, images)
        r = ref.generate(inputs_embeds=emb.float(), attention_mask=am, position_ids=pos, max_new_tokens=new, do_sample=False, eos_token_id=None,
                         pad_token_id=0, output_scores=True, return_dict_in_generate=True)
    assert got.shape[0] == B and got.shape == r.sequences.shape
    n = _agree(got, r.sequences, r.scores)
    print("32-row stand-in: steps compared per row", n)
    assert sum(n) >= 4, n
    if min(n) == new:
        assert torch.equal(got, r.sequences)
