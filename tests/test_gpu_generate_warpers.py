"""The sampling warpers min_p / typical_p / epsilon_cutoff / eta_cutoff through Qwen2Generator (.sample, .lookup_sample, the step calls) and
builder._make_library_generate, on the small models of llm_testlib.

Oracles: tests/warper_reference.py (fp64, pinned to transformers' warpers) on the fp32 transformers model's teacher-forced logits for the
kept set; and, for the exact checks, on the scores the step itself returns - start() / step() hand back the fp32 logits the sampler read
(behind guidance, the processors and the constraint, which test_gpu_step_chain.py compares with chain_reference bit for bit), the Python
Philox of qwen2_decode gives the step's u, and the chosen id must be admissible for warp_ref's index-order CDF under the sampler tests'
+-1e-5 window."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_reference as R  # noqa: E402
import llm_testlib as L  # noqa: E402
import warper_reference as W  # noqa: E402

pytestmark = pytest.mark.gpu

# the small models' logits spread by about 0.6 only: at temperature 0.2 the top-50 set holds probabilities from 1e-3 to 0.2, and these
# settings each remove a part of it
TEMP = 0.2
ALL = dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=1e-2, eta_cutoff=5e-2)
EACH = [dict(min_p=0.1), dict(typical_p=0.8), dict(epsilon_cutoff=2e-2), dict(eta_cutoff=0.1)]


def _ref_kw(w):
    return dict(min_p=w.get("min_p", 0.0), typical_p=w.get("typical_p", 1.0), eps=w.get("epsilon_cutoff", 0.0), eta=w.get("eta_cutoff", 0.0))


def _gen(seed, B, cap):
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    _lib.sampling_warpers_lib()                                   # a library without the feature fails here, by name
    m16, ref = L.models("0.5B", seed=seed)
    return Qwen2Generator.from_hf(m16, B, cap), m16, ref


def _oracle_steps(ref, e, mask, toks):
    """the fp32 model's logits [B, V] (CPU) in front of every token of toks [B, n], teacher-forced"""
    from transformers import DynamicCache
    from ml_fastvlm_amd.qwen2_decode import generation_position_ids
    B, T = mask.shape
    pos = generation_position_ids(mask, B, T)
    out = []
    with torch.no_grad():
        o = ref(inputs_embeds=e, attention_mask=mask, position_ids=pos, past_key_values=DynamicCache(), use_cache=True)
        am, ps = mask, pos
        for i in range(toks.shape[1]):
            out.append(o.logits[:, -1].float().cpu())
            am = torch.cat([am, torch.ones(B, 1, device=am.device, dtype=am.dtype)], 1)
            ps = ps[:, -1:] + 1
            o = ref(inputs_embeds=ref.get_input_embeddings()(toks[:, i])[:, None], attention_mask=am, position_ids=ps,
                    past_key_values=o.past_key_values, use_cache=True)
    return out


def _distance(r, t, lg, Tm):
    """how far token t, outside the oracle's kept set r, lies from the nearest threshold that removed it, in units of s: the top-k / top-p
    boundary value, an e floor (in log space), or typical_p's d*"""
    x = float(r["x"][t])
    best = abs(float(r["s"][t]) - r["base"]["theta"])
    for st in r["stages"]:
        if st["name"] == "typical_p":
            best = min(best, abs(float(st["d"][t]) - st["threshold"]))
        elif st["threshold"] > 0:
            best = min(best, abs(x - math.log(st["threshold"])))
    return best


def _stepwise(gen, e, mask, steps, T, k, p, w, seed, rows=None, pos=None):
    """start + `steps` decode steps under sampling with the warpers w; every chosen id is checked against warp_ref on the scores the step
    returned, with the step's own u -> (tokens [B, steps + 1], the number of draws with exactly one admissible token)"""
    from ml_fastvlm_amd.qwen2_decode import philox_uniform
    B, P = mask.shape
    rows = B if rows is None else rows
    gen.set_sampling(True, T, k, p, seed, **w)
    toks, single = [], 0
    try:
        with torch.no_grad():
            lg, ids = gen.start(e, mask, pos)
            for i in range(steps + 1):
                torch.cuda.synchronize()
                lgc, idc = lg[:rows].float().cpu().clone(), ids[:rows].cpu().clone()
                for b in range(rows):
                    r = W.warp_ref(lgc[b], T, k, p, **_ref_kw(w))
                    adm = R.admissible_tokens(r, philox_uniform(seed, b, P + i))
                    t = int(idc[b])
                    assert bool(adm[t]), (i, b, t, bool(r["kept"][t]), r["count"], adm.nonzero()[:6, 0].tolist())
                    single += int(adm.sum()) == 1
                toks.append(ids.clone())
                if i < steps:
                    lg, ids = gen.step()
    finally:
        gen.set_sampling(False)
    return torch.stack(toks, 1), single


def test_min_p_1_equals_greedy():
    gen, m16, ref = _gen(1, 3, 32)
    B, T, new = 3, 20, 12
    e, mask = L.prompt(ref, B, T, "left", seed=2)
    g = gen.greedy(e.to(torch.bfloat16), mask, None, max_new_tokens=new, pad_token_id=0)
    for i, lg in enumerate(_oracle_steps(ref, e, mask, g)):        # the fp32 oracle: no step's maximum is tied
        top = lg.topk(2, -1).values
        assert bool((top[:, 0] > top[:, 1]).all()), i
    with torch.no_grad():                                         # nor are our own logits'
        lg, _ = gen.start(e.to(torch.bfloat16), mask)
        for i in range(new):
            top = lg.topk(2, -1).values
            assert bool((top[:, 0] > top[:, 1]).all()), i
            if i + 1 < new:
                lg, _ = gen.step(g[:, i].contiguous())
    for graph in (True, False):
        s = gen.sample(e.to(torch.bfloat16), mask, None, max_new_tokens=new, temperature=0.9, top_k=0, top_p=1.0, seed=7, pad_token_id=0, graph=graph, min_p=1.0)
        assert torch.equal(s, g), (graph, s.tolist(), g.tolist())


@pytest.mark.parametrize("w", EACH + [ALL], ids=lambda w: "+".join(w))
def test_teacher_forced_sampled_tokens_lie_in_the_oracle_kept_set(w):
    gen, m16, ref = _gen(6, 3, 48)
    B, T, new = 3, 24, 16
    Tm, k, p = TEMP, 50, 0.95
    e, mask = L.prompt(ref, B, T, "left", seed=7)
    toks = gen.sample(e.to(torch.bfloat16), mask, None, max_new_tokens=new, temperature=Tm, top_k=k, top_p=p, seed=3, **w)
    assert toks.shape == (B, new)
    plain = gen.sample(e.to(torch.bfloat16), mask, None, max_new_tokens=new, temperature=Tm, top_k=k, top_p=p, seed=3)
    inside = total = smaller = 0
    outside = []
    for i, lg in enumerate(_oracle_steps(ref, e, mask, toks)):
        for b in range(B):
            r = W.warp_ref(lg[b], Tm, k, p, **_ref_kw(w))
            total += 1
            inside += bool(r["kept"][int(toks[b, i])])
            smaller += r["count"] < r["base"]["count"]
            if not bool(r["kept"][int(toks[b, i])]):
                outside.append(_distance(r, int(toks[b, i]), lg[b], Tm))
    print(f"{w}: sampled tokens inside the oracle's kept set: {inside} of {total}; the warpers removed tokens in {smaller} steps; "
          f"differs from the plain sample: {not torch.equal(toks, plain)}")
    # The device's bf16 model against the fp32 oracle: their logits differ by up to ~DELTA / 10 (llm_testlib.DELTA), DELTA / (10 T) in s, so a
    # token near a threshold may fall on the other side; the existing sampler test allows 10 % of the tokens for that.  Every such token must
    # lie within REACH of a threshold of some stage, where REACH = DELTA / T in s (ten times the logits' error) covers the shift of the
    # token itself and, for the statistics (A, log Z, H), the same shift of every other token.
    assert inside >= 0.9 * total and smaller >= 0.5 * total       # the case exercises the warpers: they cut the set in most steps
    assert all(d <= L.DELTA / Tm for d in outside), outside


def test_eager_graph_and_a_second_run_give_equal_tokens():
    gen, m16, ref = _gen(3, 2, 40)
    e, mask = L.prompt(ref, 2, 16, "left", seed=4)
    e = e.to(torch.bfloat16)
    kw = dict(max_new_tokens=14, temperature=TEMP, top_k=50, top_p=0.98, seed=11, **ALL)
    a = gen.sample(e, mask, None, graph=True, **kw)
    b = gen.sample(e, mask, None, graph=False, **kw)
    c = gen.sample(e, mask, None, graph=True, **kw)
    assert torch.equal(a, b) and torch.equal(a, c), (a.tolist(), b.tolist(), c.tolist())
    d = gen.sample(e, mask, None, graph=True, **dict(kw, seed=12))
    assert not torch.equal(a, d)


@pytest.mark.parametrize("w", [dict(typical_p=0.8), ALL], ids=lambda w: "+".join(w))
def test_lookup_sample_equals_sample(w):
    gen, m16, ref = _gen(5, 1, 96)
    e, mask = L.prompt(ref, 1, 20, "left", seed=9)
    e = e.to(torch.bfloat16)
    kw = dict(max_new_tokens=24, temperature=TEMP, top_k=40, top_p=0.95, seed=21, **w)
    s = gen.sample(e, mask, None, **kw)
    lk, stats = gen.lookup_sample(e, mask, None, prompt_lookup_num_tokens=7, return_stats=True, **kw)
    assert torch.equal(lk, s), (lk.tolist(), s.tolist(), stats)
    plain = gen.sample(e, mask, None, **dict(kw, **{k: None for k in w}))
    assert torch.equal(gen.lookup_sample(e, mask, None, prompt_lookup_num_tokens=7, **dict(kw, **{k: None for k in w})), plain)   # restored: off again


def test_off_values_give_the_plain_sample():
    gen, m16, ref = _gen(8, 2, 40)
    e, mask = L.prompt(ref, 2, 16, "right", seed=9)
    e = e.to(torch.bfloat16)
    kw = dict(max_new_tokens=12, temperature=TEMP, top_k=50, top_p=0.9, seed=5)
    plain = gen.sample(e, mask, None, **kw)
    assert torch.equal(gen.sample(e, mask, None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, **kw), plain)
    on = gen.sample(e, mask, None, min_p=0.5, **kw)
    assert torch.equal(gen.sample(e, mask, None, **kw), plain)    # a run that set them has put them back
    assert on.shape == plain.shape and not torch.equal(on, plain)


def test_seventeen_rows_step_by_step():
    gen, m16, ref = _gen(4, 17, 40)
    e, mask = L.wide_prompt(ref, 17, 18, seed=3)
    toks, single = _stepwise(gen, e.to(torch.bfloat16), mask, 5, TEMP, 50, 0.95, ALL, seed=77)
    assert single >= 0.75 * toks.numel(), single
    s = gen.sample(e.to(torch.bfloat16), mask, None, max_new_tokens=6, temperature=TEMP, top_k=50, top_p=0.95, seed=77, **ALL)
    assert torch.equal(s, toks)


def test_behind_the_processors():
    gen, m16, ref = _gen(2, 3, 48)
    e, mask = L.prompt(ref, 3, 20, "left", seed=5)
    gen.set_logits_processors(repetition_penalty=1.3, no_repeat_ngram_size=2, suppress_tokens=[5, 17, 900])
    try:
        toks, single = _stepwise(gen, e.to(torch.bfloat16), mask, 10, TEMP, 50, 0.95, ALL, seed=13)
    finally:
        gen.set_logits_processors()
    assert single >= 0.75 * toks.numel() and not bool(torch.isin(toks, torch.tensor([5, 17, 900], device=toks.device)).any())


def test_behind_a_constraint():
    gen, m16, ref = _gen(2, 3, 48)
    e, mask = L.prompt(ref, 3, 20, "left", seed=6)
    aut = L.make_automaton(seed=1, vocab=4096, sizes=L.AUTOMATON_WIDE)
    gen.set_constraint(aut, None)
    try:
        toks, single = _stepwise(gen, e.to(torch.bfloat16), mask, 8, TEMP, 0, 1.0, ALL, seed=14)
    finally:
        gen.set_constraint(None)
    assert single >= 0.75 * toks.numel(), single


def test_behind_guidance():
    gen, m16, ref = _gen(2, 6, 48)
    from ml_fastvlm_amd.qwen2_decode import guidance_batch
    x, m, pos = guidance_batch(*L.guidance_inputs(m16, 3, seed=2)[:2], None, *L.guidance_inputs(m16, 3, seed=2)[2:], None)
    gen.set_guidance(1.5)
    try:
        toks, single = _stepwise(gen, x, m, 8, TEMP, 50, 0.95, ALL, seed=15, rows=3, pos=pos)
    finally:
        gen.set_guidance(1.0)
    assert bool((toks[:3] == toks[3:]).all())                     # row G + g is fed the token of row g
    assert single >= 0.75 * toks[:3].numel(), single


def test_library_generate_takes_min_p_under_the_flag_only():
    from transformers import Qwen2ForCausalLM
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator

    class StandIn(Qwen2ForCausalLM):
        @torch.no_grad()
        def generate(self, inputs=None, images=None, image_sizes=None, **kwargs):
            position_ids = kwargs.pop("position_ids", None)
            attention_mask = kwargs.pop("attention_mask", None)
            return super().generate(position_ids=position_ids, attention_mask=attention_mask, inputs_embeds=self.get_input_embeddings()(inputs), **kwargs)

    m16, _ = L.models("0.5B", seed=10)
    model = StandIn(m16.config).eval()
    model.load_state_dict(m16.state_dict())
    model = model.to("cuda", torch.bfloat16)
    orig = StandIn.generate
    ids = torch.randint(10, 4000, (2, 12), generator=torch.Generator().manual_seed(0)).cuda()
    calls = []
    real = Qwen2Generator.sample

    def spy(self, *a, **kw):
        calls.append(kw)
        return real(self, *a, **kw)

    Qwen2Generator.sample = spy
    try:
        kw = dict(do_sample=True, temperature=0.7, top_p=None, num_beams=1, max_new_tokens=8, use_cache=True, min_p=0.1)
        StandIn.generate = builder._make_library_generate(orig, sampling_warpers=True)
        torch.manual_seed(0)
        a = model.generate(ids, **kw)
        torch.manual_seed(0)
        b = model.generate(ids, **kw)
        assert len(calls) == 2 and calls[0]["min_p"] == pytest.approx(0.1) and torch.equal(a, b) and a.shape[0] == 2
        StandIn.generate = builder._make_library_generate(orig)
        with pytest.warns(UserWarning, match="stays on the reference \\(min_p=0.1\\)"):
            model.generate(ids, **kw)
        assert len(calls) == 2
    finally:
        Qwen2Generator.sample = real
        StandIn.generate = orig
