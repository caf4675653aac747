"""Token sampling on the device (csrc/llm_sample.hip, Qwen2Generator.sample, builder._make_library_generate).

Oracle: transformers' own TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper on the same fp32 logits for the kept set, an fp64
inverse CDF in token-index order for the draw, the Python Philox of qwen2_decode for the random numbers, and the fp32 transformers model
for the teacher-forced steps."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import DELTA, models as _models, oracle_scores as _oracle_scores, prompt as _prompt, sample as _sample  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from ml_fastvlm_amd import _lib
    return _lib.sampling_lib()


def _near_top_p(logits, T, k, p, tol=1e-5):
    """rows whose fp64 descending cumulative mass (over the top-k set) lies within tol of top_p at some token"""
    s = (logits.cpu() / T).double()
    if k > 0:
        kth = s.topk(min(k, s.shape[1]), -1).values[:, -1:]
        s = s.masked_fill(s < kth, -math.inf)
    pr = torch.softmax(s, -1).sort(-1, descending=True).values
    before = pr.cumsum(-1) - pr
    return ((before - p).abs() < tol).any(-1) if p < 1.0 else torch.zeros(s.shape[0], dtype=torch.bool, device=s.device)


def _rows(B, V, kind, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, V, device="cuda", generator=g)
    if kind == "peaked":                                          # a few dominant tokens over a wide tail (an LM's next-token shape)
        x = 3.0 * x
        top = torch.randint(0, V, (B, 8), device="cuda", generator=g)
        x.scatter_(1, top, 12.0 + 4.0 * torch.rand(B, 8, device="cuda", generator=g))
    else:                                                         # flat: a narrow spread, a large kept set
        x = 0.3 * x
    return x.contiguous()


# ---- 1. Philox on the device -----------------------------------------------------------------------------------------------------------
def test_philox_uniform_bit_exact(lib):
    from ml_fastvlm_amd.qwen2_decode import philox_uniform
    B, V = 16, 1001
    x = _rows(B, V, "flat", 1)
    for seed in (0, 0x0123456789ABCDEF, 2 ** 64 - 1):
        for n in (0, 1, 285, 4097, 2 ** 31 - 1):
            _, info = _sample(lib, x, 1.0, 0, 1.0, seed=seed, n=n)
            want = torch.tensor([philox_uniform(seed, b, n) for b in range(B)], dtype=torch.float32)
            assert torch.equal(info[:, 3].cpu(), want), (seed, n)


# ---- 2. the kept set against transformers' warpers --------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [151936, 152064, 4096, 1001])
@pytest.mark.parametrize("B", [1, 5, 16])
def test_kept_set_equals_transformers(lib, B, V):
    compared = total = 0
    for kind in ("peaked", "flat"):
        x = _rows(B, V, kind, V + B + (kind == "flat"))
        for T in (0.2, 0.7, 1.0, 1.5):
            for k in (0, 1, 50, 1000):
                for p in (1.0, 0.95, 0.5, 0.0):
                    ids, info = _sample(lib, x, T, k, p, seed=7, n=3)
                    ref = _oracle_scores(x, T, k, p)
                    kept_ref = ref > -math.inf
                    ids, info = ids.cpu(), info.cpu()
                    s = x.cpu() / T
                    kept = s >= info[:, 0:1]
                    skip = _near_top_p(x, T, k, p)
                    for b in range(B):
                        total += 1
                        if bool(skip[b]):
                            assert abs(int(kept[b].sum()) - int(kept_ref[b].sum())) <= 1
                            continue
                        compared += 1
                        assert torch.equal(kept[b], kept_ref[b]), (kind, T, k, p, b, int(kept[b].sum()), int(kept_ref[b].sum()))
                        assert int(info[b, 1]) == int(kept_ref[b].sum())
                        assert bool(kept_ref[b, ids[b]]), (kind, T, k, p, b)
    print(f"B={B} V={V}: rows compared {compared} of {total}")
    assert compared > total // 2          # flat rows of a large vocabulary step by < 1e-5 of mass per token: their top-p rows are excluded


# ---- 3. the draw given u: fp64 inverse CDF in index order ----------------------------------------------------------------------------
@pytest.mark.parametrize("T,k,p", [(0.2, 50, 1.0), (0.7, 50, 0.95), (1.0, 0, 0.95), (1.5, 1000, 0.5), (1.0, 0, 1.0)])
def test_draw_given_u_is_the_index_order_inverse_cdf(lib, T, k, p):
    B, V = 16, 151936
    x = _rows(B, V, "peaked" if T < 1.0 else "flat", 11)
    _, info = _sample(lib, x, T, k, p)
    s = x.cpu() / T
    kept = s >= info.cpu()[:, 0:1]
    near = _near_top_p(x, T, k, p)
    oracle = _oracle_scores(x, T, k, p) > -math.inf
    assert torch.equal(kept[~near], oracle[~near])                 # the oracle's kept set wherever the top-p boundary is not within 1e-5
    s = s.double()
    pr = torch.where(kept, torch.exp(s - s.max(-1, keepdim=True).values), torch.zeros_like(s))
    cdf = pr.cumsum(-1) / pr.sum(-1, keepdim=True)
    g = torch.Generator().manual_seed(int(T * 10) + k)
    u, want = [], []
    for b in range(B):
        width = torch.diff(cdf[b], prepend=torch.zeros(1, dtype=torch.float64))
        cand = (width > 1e-5).nonzero()[:, 0]                    # tokens with enough mass for an fp32 u mid-interval
        j = int(cand[torch.randint(0, cand.numel(), (1,), generator=g)])
        lo = float(cdf[b, j - 1]) if j > 0 else 0.0
        u.append((lo + float(cdf[b, j])) / 2)
        want.append(j)
    ut = torch.tensor(u, device="cuda", dtype=torch.float32)
    ids, info = _sample(lib, x, T, k, p, u=ut)
    assert ids.cpu().tolist() == want
    assert torch.equal(info[:, 3], ut)
    z = pr.sum(-1)
    assert torch.allclose(info[:, 2].double().cpu(), z, rtol=1e-5)


# ---- 4. the distribution ---------------------------------------------------------------------------------------------------------------
def test_distribution_chi_square(lib):
    B, V, T, k, N = 16, 151936, 0.7, 50, 512
    row = _rows(1, V, "peaked", 5)
    x = row.expand(B, V).contiguous()
    ids = []
    for n in range(N):
        got, _ = _sample(lib, x, T, k, 1.0, seed=1234, n=n)
        ids.append(got)
    ids = torch.stack(ids).flatten().cpu()
    ids2 = torch.stack([_sample(lib, x, T, k, 1.0, seed=1234, n=n)[0] for n in range(4)]).flatten().cpu()
    assert torch.equal(ids2, ids[:4 * B])                         # deterministic for the fixed seed
    kept = (_oracle_scores(row, T, k, 1.0) > -math.inf)[0]
    assert bool(kept[ids].all())
    s = (row[0].cpu() / T).double()
    prob = torch.softmax(s.masked_fill(~kept, -math.inf), -1)
    idx = kept.nonzero()[:, 0]
    exp = prob[idx] * ids.numel()
    obs = torch.bincount(ids, minlength=V)[idx].double()
    order = exp.argsort(descending=True)
    exp, obs = exp[order], obs[order]
    big = exp >= 5                                                # sparse categories merged into one
    e = torch.cat([exp[big], exp[~big].sum()[None]]) if (~big).any() else exp[big]
    o = torch.cat([obs[big], obs[~big].sum()[None]]) if (~big).any() else obs[big]
    stat = float(((o - e) ** 2 / e).sum())
    df = e.numel() - 1
    pval = float(torch.special.gammaincc(torch.tensor(df / 2, dtype=torch.float64), torch.tensor(stat / 2, dtype=torch.float64)))
    print(f"chi-square {stat:.1f} on {df} degrees of freedom: p = {pval:.4f}")
    assert pval >= 1e-4


# ---- model-level tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
def test_top_k_1_equals_greedy(side):
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _models("0.5B", seed=1)
    B, T, new = 3, 20, 12
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    e, mask = _prompt(ref, B, T, side, seed=2)
    e = e.to(torch.bfloat16)
    g = gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0)
    with torch.no_grad():                                         # precondition on our logits: no tie at the row max
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


def test_reproducible_eager_and_graph_and_overflow():
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _models("0.5B", seed=3)
    B, T, N = 2, 16, 12
    e, mask = _prompt(ref, B, T, "left", seed=4)
    e = e.to(torch.bfloat16)
    gen = Qwen2Generator.from_hf(m16, B, T + N)
    kw = dict(max_new_tokens=N + 1, temperature=1.0, top_k=0, top_p=1.0)
    a = gen.sample(e, mask, None, seed=11, graph=True, **kw)
    b = gen.sample(e, mask, None, seed=11, graph=False, **kw)
    c = gen.sample(e, mask, None, seed=12, graph=True, **kw)
    assert torch.equal(a, b), (a.tolist(), b.tolist())
    assert not torch.equal(a, c)
    torch.manual_seed(0)
    d1 = gen.sample(e, mask, None, **kw)
    torch.manual_seed(0)
    d2 = gen.sample(e, mask, None, **kw)
    assert torch.equal(d1, d2)
    assert gen.cache_state() == (T + N, 0)
    # capacity: the step past it writes nothing and the error is sticky, as in greedy
    gen.set_sampling(True, 1.0, 0, 1.0, 11)
    with torch.no_grad():
        gen.start(e, mask, logits=False)
        for _ in range(N):
            gen.step(logits=False)
        assert gen.cache_state() == (T + N, 0)
        gen.step(logits=False)
        assert gen.cache_state() == (T + N, 1)
        with pytest.raises(_lib.FvhdError, match="capacity"):
            gen.step()
    gen.set_sampling(False)


def test_teacher_forced_sampled_tokens_lie_in_the_oracle_kept_set():
    from transformers import DynamicCache
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator, generation_position_ids
    m16, ref = _models("0.5B", seed=6)
    B, T, new = 3, 24, 24
    Tm, k, p = 0.7, 50, 0.9
    e, mask = _prompt(ref, B, T, "left", seed=7)
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    toks = gen.sample(e.to(torch.bfloat16), mask, None, max_new_tokens=new, temperature=Tm, top_k=k, top_p=p, seed=3)
    assert toks.shape == (B, new)
    pos = generation_position_ids(mask, B, T)
    checked = total = 0
    with torch.no_grad():
        out = ref(inputs_embeds=e, attention_mask=mask, position_ids=pos, past_key_values=DynamicCache(), use_cache=True)
        am, ps = mask, pos
        for i in range(new):
            lg = out.logits[:, -1].float().cpu()
            kept = _oracle_scores(lg, Tm, k, p) > -math.inf
            s = lg / Tm
            pr = torch.softmax(s.masked_fill(s < s.topk(k, -1).values[:, -1:], -math.inf).double(), -1)
            for b in range(B):
                total += 1
                t = int(toks[b, i])
                if bool(kept[b, t]):
                    checked += 1
                    continue
                # outside the oracle's set: only where a boundary is within the logits' error - the top-k boundary within DELTA, or the
                # top-p boundary within the mass that such an error moves
                lkept = lg[b][kept[b]].min()
                before = float(pr[b][pr[b] > pr[b, t]].sum())
                assert float(lkept - lg[b, t]) <= DELTA or before < p + 0.05, (i, b, t)
            am = torch.cat([am, torch.ones(B, 1, device="cuda", dtype=am.dtype)], 1)
            ps = ps[:, -1:] + 1
            out = ref(inputs_embeds=ref.get_input_embeddings()(toks[:, i])[:, None], attention_mask=am, position_ids=ps,
                      past_key_values=out.past_key_values, use_cache=True)
    print(f"sampled tokens inside the oracle's kept set: {checked} of {total}")
    assert checked >= 0.9 * total


def test_greedy_after_sample_is_unchanged():
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    m16, ref = _models("0.5B", seed=8)
    B, T, new = 2, 16, 10
    e, mask = _prompt(ref, B, T, "right", seed=9)
    e = e.to(torch.bfloat16)
    g1 = Qwen2Generator.from_hf(m16, B, T + new).greedy(e, mask, None, max_new_tokens=new, pad_token_id=0)
    gen = Qwen2Generator.from_hf(m16, B, T + new)
    gen.sample(e, mask, None, max_new_tokens=new, temperature=1.0, top_k=0, seed=1)
    gen.set_sampling(True, 1.0, 0, 1.0, 2)                         # even with sampling left on, greedy sets its own mode
    g2 = gen.greedy(e, mask, None, max_new_tokens=new, pad_token_id=0)
    assert torch.equal(g1, g2)


def test_library_generate_on_a_standin():
    """builder._make_library_generate on a stand-in of LlavaQwen2ForCausalLM (written here): predict.py's exact generate() arguments run on
    the library (Qwen2Generator.sample), torch.manual_seed repeats a run, beam search falls back to the original generate"""
    from transformers import Qwen2ForCausalLM
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd import splice as S
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator

    class StandIn(Qwen2ForCausalLM):
        def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images, image_sizes=None):
            o = S.multimodal_splice(input_ids, position_ids, attention_mask, labels, images, self.get_input_embeddings().weight, "right", None)
            return o[0], o[1], o[2], past_key_values, o[4], o[5]

        @torch.no_grad()
        def generate(self, inputs=None, images=None, image_sizes=None, **kwargs):
            position_ids = kwargs.pop("position_ids", None)
            attention_mask = kwargs.pop("attention_mask", None)
            if "inputs_embeds" in kwargs:
                raise NotImplementedError("`inputs_embeds` is not supported")
            if images is not None:
                (inputs, position_ids, attention_mask, _, inputs_embeds, _) = self.prepare_inputs_labels_for_multimodal(
                    inputs, position_ids, attention_mask, None, None, images, image_sizes=image_sizes)
            else:
                inputs_embeds = self.get_input_embeddings()(inputs)
            return super().generate(position_ids=position_ids, attention_mask=attention_mask, inputs_embeds=inputs_embeds, **kwargs)

    m16, _ = _models("0.5B", seed=10)
    model = StandIn(m16.config).eval()
    model.load_state_dict(m16.state_dict())
    model = model.to("cuda", torch.bfloat16)
    orig = StandIn.generate
    StandIn.generate = builder._make_library_generate(orig)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(10, 4000, (2, 12), generator=g)
    ids[:, 3] = -200                                              # IMAGE_TOKEN_INDEX
    ids = ids.cuda()
    feats = (0.5 * torch.randn(2, 16, 896, generator=g)).to("cuda", torch.bfloat16)
    calls = []
    real = Qwen2Generator.sample

    def spy(self, *a, **kw):
        calls.append(kw)
        return real(self, *a, **kw)

    Qwen2Generator.sample = spy
    try:
        predict = dict(images=feats, image_sizes=[(256, 256)] * 2, do_sample=True, temperature=0.2, top_p=None, num_beams=1,
                       max_new_tokens=8, use_cache=True)
        torch.manual_seed(1)
        r1 = model.generate(ids, **predict)
        assert len(calls) == 1 and calls[0]["temperature"] == pytest.approx(0.2) and calls[0]["top_k"] == 50 and calls[0]["top_p"] == 1.0
        assert r1.shape == (2, 8) and r1.device.type == "cuda"
        torch.manual_seed(1)
        r2 = model.generate(ids, **predict)
        assert torch.equal(r1, r2)
        beams = dict(predict, do_sample=False, temperature=None, num_beams=2, pad_token_id=0)
        with pytest.warns(UserWarning, match="num_beams"):
            got = model.generate(ids, **beams)
        assert len(calls) == 2
        want = orig(model, ids, **beams)
        assert torch.equal(got, want)
    finally:
        Qwen2Generator.sample = real
        StandIn.generate = orig
