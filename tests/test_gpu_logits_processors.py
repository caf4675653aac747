"""Logits processors inside the decode step (csrc/llm_logits.hip, include/fvhd.h version 506, Qwen2Generator.set_logits_processors,
builder._make_library_generate(logits_processors=True)): the kernel against transformers' own processors bit for bit, the step against an
exact oracle built from its own raw logits, graph replay, the effects on real output, stock transformers' generate, and "off is off"."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import llm_testlib as L  # noqa: E402
from llm_testlib import lib  # noqa: E402,F401
from logits_testlib import hf_chain  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3                                                             # no_repeat_ngram_size of the op cases: g below covers n - 1 and n
G = [0, 1, N - 1, N, 255, 256, 257, 700]                          # history lengths around the workgroup's stride of 256
CAP = 704
VARIANTS = ("distinct", "one token", "8 tokens")
SETTINGS = ("penalty", "ngram", "min_new", "suppress", "all")    # every processor alone, and all together


def _bits(t):
    return t.contiguous().view(torch.int32)


def _history(variant, B, V, g, gen):
    """int32 [B, CAP] on the CPU: the first g entries are the row's history, the rest valid tokens that must never be read"""
    h = torch.empty(B, CAP, dtype=torch.int64)
    for b in range(B):
        if variant == "distinct":
            row = torch.randperm(V, generator=gen)[:CAP]
        elif variant == "one token":
            row = torch.full((CAP,), (V - 1 - b) % V)
        else:                                                     # heavy duplicates, the vocabulary's first and last ids among them
            pool = torch.cat([torch.tensor([0, V - 1, 31, 32]), torch.randint(0, V, (4,), generator=gen)])
            row = pool[torch.randint(0, 8, (CAP,), generator=gen)]
        h[b] = row
    h[:, g:] = (h[:, g:] + 17) % V                                # past the history: other tokens
    return h.to(torch.int32)


def _settings(V, h, g):
    """name -> (p, n, m, eos, suppress): every processor alone and all together; m = 256 bans the EOS ids for g < 256 only; the lists hold
    the vocabulary's ends and tokens of the history"""
    in_hist = [int(h[0, 0]), int(h[-1, max(g - 1, 0)])]
    eos = sorted({V - 1, in_hist[0], 5})
    sup = sorted({0, V - 2, in_hist[1], 64, 65})
    return {"penalty": (1.3, 0, 0, None, None), "ngram": (1.0, N, 0, None, None), "min_new": (1.0, 0, 256, eos, None),
            "suppress": (1.0, 0, 0, None, sup), "all": (0.8, N, 256, eos, sup)}


def _run_op(lib, logits, hist, g, p, n, m, eos, sup):
    import ctypes as C
    B, V = logits.shape
    e = (C.c_int32 * max(1, len(eos or [])))(*(eos or []))
    s = (C.c_int32 * max(1, len(sup or [])))(*(sup or []))
    L.check(lib.fvhd_op_dec_logits_process(L.stream(), L.ptr(logits), B, V, L.ptr(hist), hist.shape[1], g, p, n, m, C.cast(e, C.c_void_p), len(eos or []),
                                           C.cast(s, C.c_void_p), len(sup or [])), "fvhd_op_dec_logits_process")


@pytest.mark.parametrize("V", [1001, 4096, 151936])
@pytest.mark.parametrize("B", [1, 17, 64])
def test_the_op_equals_transformers_bit_for_bit(lib, B, V):
    gen = torch.Generator().manual_seed(B * 7 + V)
    raw = 4.0 * torch.randn(B, V, generator=gen)
    raw[:, ::97] = 0.0
    raw[:, 1::89] = -math.inf
    raw[:, 2::83] = -0.0
    raw_d = raw.cuda()
    full = B * V <= 300000                                        # the whole cross product where a case is cheap; a covering subset above
    done = 0
    for gi, g in enumerate(G):
        for vi, variant in enumerate(VARIANTS):
            # above the size limit, per g: all processors on one variant, one processor alone on another - both rotate with g
            names = [n for si, n in enumerate(SETTINGS) if full or (n == "all" and vi == gi % 3) or (si == gi % 4 and vi == (gi + 1) % 3)]
            if not names:
                continue
            h = _history(variant, B, V, g, gen)
            h_d = h.cuda()
            settings = _settings(V, h, g)
            for name in names:
                p, n, m, eos, sup = settings[name]
                want = hf_chain(h[:, :g].long(), raw, p, n, m, eos, sup)
                runs = []
                for _ in range(2):
                    x = raw_d.clone()
                    _run_op(lib, x, h_d, g, p, n, m, eos, sup)
                    runs.append(x)
                torch.cuda.synchronize()
                what = (B, V, g, variant, name)
                assert torch.equal(_bits(runs[0]), _bits(runs[1])), what           # run to run
                assert torch.equal(_bits(runs[0]), _bits(want.cuda())), what       # the whole rows: edited and untouched logits alike
                assert torch.equal(h_d.cpu(), h), what                             # the caller's history is read only
                done += 1
    assert done == (120 if full else 16)


# ---- the step --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return L.models("0.5B", seed=1)


def _prompt_for(ref, B, T):
    if B <= 3:
        e, mask = L.prompt(ref, B, T, "left", seed=5, draw_on="cpu")
    else:
        e, mask = L.wide_prompt(ref, B, T, seed=5)
    return e.to(torch.bfloat16), mask


@pytest.mark.parametrize("B", [3, 17])
def test_the_step_equals_its_raw_logits_processed_by_transformers(small, B):
    """N eager steps with processors on and logits=True; the same fed tokens with processors off give the raw logits (the step is
    deterministic), and transformers' processors on those must give the processed logits bit for bit - no margin involved"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = small
    T, steps = 20, 12
    e, mask = _prompt_for(ref, B, T)
    gen = Qwen2Generator.from_hf(m16, B, T + steps + 1)
    with torch.no_grad():
        lg, _ = gen.start(e, mask)
        first_raw = L.lowest_argmax(lg).tolist()
    cfg = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=4, eos_token_id=[7, first_raw[-1] ^ 1],
               suppress_tokens=sorted(set(first_raw)))           # the raw choice of every row: the first token has to change
    gen.set_logits_processors(**cfg)
    try:
        fed, got, chosen = [], [], []
        with torch.no_grad():
            lg, ids = gen.start(e, mask)
            got.append(lg.clone())
            chosen.append(ids.clone())
            for i in range(steps):
                fed.append(chosen[-1].clone())
                lg, ids = gen.step(fed[-1] if B == 3 else None)   # both sources of the fed token: the caller's ids, the previous choice
                got.append(lg.clone())
                chosen.append(ids.clone())
        assert gen.cache_state() == (T + steps, 0)
    finally:
        gen.set_logits_processors()
    raw = []
    with torch.no_grad():
        lg, _ = gen.start(e, mask)
        raw.append(lg.clone())
        for i in range(steps):
            lg, _ = gen.step(fed[i])
            raw.append(lg.clone())
    torch.cuda.synchronize()
    assert all(int(chosen[0][b]) != first_raw[b] for b in range(B))              # fvhd_llm_start applies them
    kw = dict(p=1.3, n=2, m=4, eos=cfg["eos_token_id"], suppress=cfg["suppress_tokens"])
    for i in range(steps + 1):
        hist = torch.stack(fed[:i], 1).cpu() if i else torch.zeros(B, 0, dtype=torch.long)
        want = hf_chain(hist, raw[i].cpu(), **kw)
        assert torch.equal(_bits(got[i].cpu()), _bits(want)), i
        assert torch.equal(chosen[i].cpu(), L.lowest_argmax(want)), i
    assert any(not torch.equal(_bits(got[i]), _bits(raw[i])) for i in range(1, steps + 1))


ALL = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=5, suppress_tokens=[3, 9, 4000])


def test_graph_replay_equals_eager_and_a_new_start_resets_the_history(small):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = small
    B, T, new = 3, 20, 14
    e, mask = _prompt_for(ref, B, T)
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    plain = gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0)
    eos = [int(plain[0, 2]), int(plain[1, 3])]
    kw = dict(max_new_tokens=new, eos_token_id=eos, pad_token_id=0, **ALL)
    a = gen.greedy(e, mask, None, graph=True, **kw)
    b = gen.greedy(e, mask, None, graph=False, **kw)
    c = gen.greedy(e, mask, None, graph=True, **kw)              # a second run: the history and the bitmap start empty again
    assert torch.equal(a, b) and torch.equal(a, c), (a.tolist(), b.tolist(), c.tolist())
    assert not torch.equal(a[:, :plain.shape[1]], plain[:, :a.shape[1]])
    skw = dict(kw, temperature=0.8, top_k=40, top_p=0.95, seed=21)
    sa = gen.sample(e, mask, None, graph=True, **skw)
    sb = gen.sample(e, mask, None, graph=False, **skw)
    sc = gen.sample(e, mask, None, graph=True, **skw)
    assert torch.equal(sa, sb) and torch.equal(sa, sc), (sa.tolist(), sb.tolist())
    assert gen._processors is None and torch.equal(gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0), plain)


def test_sampling_17_rows_appends_once_per_step(small):
    """above 16 rows the sampler runs in blocks of 16: the one processors launch over all rows comes first.  Every row's sampled tokens
    respect the bans, eager = graph"""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = small
    B, T, new = 17, 20, 10
    e, mask = _prompt_for(ref, B, T)
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    kw = dict(max_new_tokens=new, temperature=1.0, top_k=0, top_p=1.0, seed=5, no_repeat_ngram_size=1, suppress_tokens=[0, 1, 2])
    a = gen.sample(e, mask, None, graph=True, **kw)
    b = gen.sample(e, mask, None, graph=False, **kw)
    assert torch.equal(a, b)
    for row in a.tolist():
        assert len(set(row)) == new and not set(row) & {0, 1, 2}, row            # n = 1: no token twice


def test_the_effects_show_on_real_output(small):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = small
    B, T, new = 3, 20, 24
    e, mask = _prompt_for(ref, B, T)
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    out = gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0, no_repeat_ngram_size=2)
    assert out.shape == (B, new)
    for row in out.tolist():                                      # no EOS: every row is unfinished to the end
        bigrams = list(zip(row, row[1:]))
        assert len(set(bigrams)) == len(bigrams), row
    plain = gen.greedy(e, mask, None, max_new_tokens=8, pad_token_id=0)
    eos = sorted(set(plain[:, 1].tolist()))                       # the unprocessed greedy token of step 1, of every row
    pad = next(t for t in range(10) if t not in eos)
    stopped = gen.greedy(e, mask, None, max_new_tokens=12, eos_token_id=eos, pad_token_id=pad)
    assert stopped.shape[1] <= 2                                  # without the processor every row ends there
    held = gen.greedy(e, mask, None, max_new_tokens=12, eos_token_id=eos, pad_token_id=pad, min_new_tokens=6)
    assert held.shape[1] >= 6 and not torch.isin(held[:, :6].cpu(), torch.tensor(eos)).any(), held.tolist()


# prompt seeds (of `prompt` drawn on the CPU, model seed 1, B = 3, T = 20) chosen with the fp32 oracle alone: under
# repetition_penalty = 1.3 and no_repeat_ngram_size = 3 the top-2 gap of transformers' processed scores stays above DELTA for at least 10
# tokens of every row (147, 159: all 12; 537: 11; 164: 10), and no compared gap lies within a quarter of DELTA of it
PROCESSOR_SEEDS = {"left": [147, 537], "right": [159, 164]}


def test_greedy_with_processors_against_stock_transformers(small):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = small
    B, T, new = 3, 20, 12
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    compared = []
    for side, seeds in PROCESSOR_SEEDS.items():
        for seed in seeds:
            e, mask = L.prompt(ref, B, T, side, seed=seed, draw_on="cpu")
            with torch.no_grad():
                r = ref.generate(inputs_embeds=e, attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0,
                                 repetition_penalty=1.3, no_repeat_ngram_size=3, output_scores=True, return_dict_in_generate=True)
                got = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, pad_token_id=0, repetition_penalty=1.3,
                                 no_repeat_ngram_size=3)
            n = L.agree(got, r.sequences, r.scores)
            print(f"processors vs transformers, {side} seed {seed}: tokens compared per row {n}")
            compared.append(min(n))
    assert sum(c >= 8 for c in compared) >= 3, compared


def test_off_is_off(small):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = small
    B, T, new = 3, 20, 8
    e, mask = _prompt_for(ref, B, T)
    never = Qwen2Generator.from_hf(m16, B, T + new)
    want_tokens = never.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0)
    with torch.no_grad():
        lg, ids = never.start(e, mask)
        want = [lg.clone(), ids.clone()]
        for _ in range(3):
            lg, ids = never.step()
            want += [lg.clone(), ids.clone()]
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    gen.set_logits_processors(repetition_penalty=1.5, no_repeat_ngram_size=1, suppress_tokens=[int(want_tokens[0, 0])])
    assert not torch.equal(gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0), want_tokens)
    gen.set_logits_processors()
    assert torch.equal(gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0), want_tokens)
    with torch.no_grad():
        lg, ids = gen.start(e, mask)
        got = [lg.clone(), ids.clone()]
        for _ in range(3):
            lg, ids = gen.step()
            got += [lg.clone(), ids.clone()]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # processors set after a start without them: the step has no history and says so
    from ml_fastvlm_amd import _lib
    gen.set_logits_processors(no_repeat_ngram_size=2)
    try:
        with pytest.raises(_lib.FvhdError, match="before fvhd_llm_start"):
            gen.step()
        with pytest.raises(ValueError, match="beam search"):
            gen.beam_search(e, mask, None, num_beams=2, max_new_tokens=2)
    finally:
        gen.set_logits_processors()


def test_the_patched_generate_runs_the_processors_on_the_library(small):
    """builder._make_library_generate(logits_processors=True) on the stand-in of test_gpu_sample's test_library_generate_on_a_standin:
    generate(repetition_penalty=..., no_repeat_ngram_size=...) equals Qwen2Generator.greedy with the same settings"""
    from transformers import Qwen2ForCausalLM
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd import splice as S

    class StandIn(Qwen2ForCausalLM):
        def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images, image_sizes=None):
            o = S.multimodal_splice(input_ids, position_ids, attention_mask, labels, images, self.get_input_embeddings().weight, "right", None)
            return o[0], o[1], o[2], past_key_values, o[4], o[5]

    m16, _ = small
    model = StandIn(m16.config).eval()
    model.load_state_dict(m16.state_dict())
    model = model.to("cuda", torch.bfloat16)
    orig = StandIn.generate
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(10, 4000, (2, 12), generator=g)
    ids[:, 3] = -200                                              # IMAGE_TOKEN_INDEX
    ids = ids.cuda()
    feats = (0.5 * torch.randn(2, 16, 896, generator=g)).to("cuda", torch.bfloat16)
    call = dict(images=feats, image_sizes=[(256, 256)] * 2, do_sample=False, num_beams=1, max_new_tokens=10, use_cache=True, pad_token_id=0,
                repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[11, 12])
    try:
        StandIn.generate = builder._make_library_generate(orig, logits_processors=True)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("error")                        # no fallback warning: the library took the call
            got = model.generate(ids, **call)
        plain = model.generate(ids, **dict(call, repetition_penalty=1.0, no_repeat_ngram_size=0, suppress_tokens=None))
    finally:
        StandIn.generate = orig
    _, pos, mask, _, embeds, _ = model.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, feats, image_sizes=call["image_sizes"])
    gen = builder.generator_context(model, 2, embeds.shape[1] + 10)
    want = gen.greedy(embeds, mask, pos, max_new_tokens=10, pad_token_id=0, repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[11, 12])
    assert got.shape == (2, 10) and torch.equal(got, want) and not torch.equal(got, plain)
