"""Verify steps and prompt-lookup decoding under sampling, and the log-probabilities of a lookup generation (Qwen2Generator.verify with
set_verify_sampling, lookup_sample, lookup_greedy / lookup_sample(logprobs=n)) against the sequential runs of the same library: row t of
a verify step draws with the Philox counter of the plain step at its position on logits with that step's bits, so everything here is
compared under torch.equal - no tolerance."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from llm_testlib import models as _models, prompt as _prompt, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

P, NEW, CAP = 37, 21, 96          # prompt length, new tokens of a run, cache capacity (prompt + new + 15 drafts and room)
SETTINGS = {"predict": (0.2, 50, 1.0), "k40p95": (0.9, 40, 0.95), "hot": (1.5, 0, 1.0)}      # temperature, top_k, top_p
SEEDS = [11, 0x5DEECE66D1234567]
_gens, _prompts, _sampled = {}, {}, {}


def _gen(weights="bf16", twin=False):
    """per weight format, built once: (model, generator of one sequence); twin: a second generator with a context of its own"""
    key = (weights, twin)
    if key not in _gens:
        from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
        if "model" not in _gens:
            _gens["model"] = _models("0.5B", seed=1, layers=2)
        m16, _ = _gens["model"]
        _gens[key] = Qwen2Generator.from_hf(m16, 1, CAP, weights=weights)
    return _gens[key]


def _inputs(side):
    """one prompt with three padded positions on `side`"""
    if side not in _prompts:
        _, ref = _gens.get("model") or _gens.setdefault("model", _models("0.5B", seed=1, layers=2))
        e, mask = _prompt(ref, 2, P, side, seed=14)
        _prompts[side] = (e[1:2].to(torch.bfloat16).contiguous(), mask[1:2].contiguous())
    return _prompts[side]


def _sample(side, setting, seed, weights="bf16"):
    """the sequential run, computed once and left unchanged: NEW tokens of `sample` [NEW]"""
    key = (side, setting, seed, weights)
    if key not in _sampled:
        e, mask = _inputs(side)
        T_, k, p = SETTINGS[setting]
        with torch.no_grad():
            tok = _gen(weights).sample(e, mask, None, max_new_tokens=NEW, temperature=T_, top_k=k, top_p=p, seed=seed, pad_token_id=0)
        assert tok.shape == (1, NEW)
        _sampled[key] = tok[0].clone()
    return _sampled[key]


def _predict_steps(look, tokens, K, max_ngram):
    """the verify steps a lookup generation that must emit `tokens` takes: each step drafts what the drafting rule
    (`prompt_lookup.propose`) finds in the lookup ids + the tokens so far, keeps the drafts that ARE the next tokens, and emits one more"""
    from ml_fastvlm_amd.prompt_lookup import propose
    want = tokens.tolist()
    buf = ([] if look is None else look.reshape(-1).tolist()) + want[:1]
    done, steps = 1, 0
    while done < len(want):
        drafts = propose(buf, max_ngram, K)
        kept = 0
        while kept < K and done + kept < len(want) and drafts[kept] == want[done + kept]:
            kept += 1
        emitted = min(kept + 1, len(want) - done)
        buf += want[done:done + emitted]
        done += emitted
        steps += 1
    return steps


def _prompt_ids(V):
    """stand-in input_ids of the prompt: random ids around an image placeholder"""
    rnd = torch.randint(0, V, (50,), generator=torch.Generator().manual_seed(3)).cuda()
    return torch.cat([rnd[:20], torch.tensor([-200], device="cuda"), rnd[20:]])[None]


# ---- the verify step under sampling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 8, 16])
def test_verify_under_sampling_is_the_teacher_forced_twin(T):
    gen, twin = _gen(), _gen(twin=True)
    e, mask = _inputs("left")
    T_, k, p = SETTINGS["k40p95"]
    seed, V = SEEDS[0], gen.pre.vocab
    tok = _sample("left", "k40p95", seed)                        # the twin's own tokens: drafts taken from them are right
    gen.spec_reserve(16)
    cases = {"all accepted": T - 1, "first rejected": 0}
    if T > 2:
        cases["rejected at a middle j"] = (T - 1) // 2
    try:
        for what, j in cases.items():                            # j: the first wrong draft (T - 1: none)
            drafts = tok[1:T].clone()
            if j < T - 1:
                drafts[j] = (drafts[j] + 1) % V
            with torch.no_grad():
                # the twin: plain sampled steps fed the last token, then the drafts
                twin.set_sampling(True, T_, k, p, seed)
                first = twin.start(e, mask)[1].clone()           # (the returned ids are the generator's buffer: the steps overwrite it)
                feeds = torch.cat([first, drafts])
                want_lg, want_ids = [], []
                for t in range(T):
                    lg, ids = twin.step(feeds[t:t + 1].contiguous())
                    want_lg.append(lg[0].clone())
                    want_ids.append(ids[0].clone())
                want_ids = torch.stack(want_ids)
                n = 0
                while n < T - 1 and int(drafts[n]) == int(want_ids[n]):
                    n += 1
                assert n == j, (what, n, j)                      # the drafts are right up to j, by construction of the test
                # the twin's state after `emitted` steps: a restart, the accepted feeds, then the step that feeds the last emitted token
                twin.start(e, mask)
                for t in range(n + 1):
                    twin.step(feeds[t:t + 1].contiguous())
                assert twin.cache_state() == (P + n + 1, 0)
                next_lg, next_ids = twin.step()
                next_lg, next_ids = next_lg[0].clone(), next_ids.clone()
                # the verify step
                gen.set_sampling(True, T_, k, p, seed)
                gen.set_verify_sampling(True)
                _, ids0 = gen.start(e, mask)
                assert torch.equal(ids0, first)
                lg, ids, emitted = gen.verify(drafts)
                assert torch.equal(ids, want_ids), (what, T, ids.tolist(), want_ids.tolist())
                for t in range(T):
                    assert same_bits(lg[t], want_lg[t]), (what, T, t)
                assert int(emitted) == 1 + n, (what, T, int(emitted), n)
                assert gen.cache_state() == (P + n + 1, 0)
                lg1, ids1 = gen.step()
                assert same_bits(lg1[0], next_lg) and torch.equal(ids1, next_ids), (what, T)
    finally:
        gen.set_verify_sampling(False)
        gen.set_sampling(False)
        twin.set_sampling(False)


# ---- lookup_sample is sample ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_lookup_sample_equals_sample(setting, seed, graph, side):
    gen = _gen()
    e, mask = _inputs(side)
    T_, k, p = SETTINGS[setting]
    tok = _sample(side, setting, seed)
    kw = dict(max_new_tokens=NEW, temperature=T_, top_k=k, top_p=p, seed=seed, prompt_lookup_num_tokens=7, max_matching_ngram_size=2, graph=graph,
              poll_every=3, return_stats=True, pad_token_id=0)
    for look, oracle in ((_prompt_ids(gen.pre.vocab), False), (tok[None], True)):
        with torch.no_grad():
            got, st = gen.lookup_sample(e, mask, None, lookup_ids=look, **kw)
        print(setting, hex(seed), "graph" if graph else "eager", side, "oracle lookup ids" if oracle else "prompt ids", st)
        assert got.shape == (1, NEW) and torch.equal(got[0], tok), (got.tolist(), tok.tolist())
        assert st["tokens"] == NEW and st["steps"] == _predict_steps(look, tok, 7, 2), (st, _predict_steps(look, tok, 7, 2))
        if oracle:                                               # the drafts are the future: some must have been accepted
            assert st["steps"] < st["tokens"] - 1, st
    assert gen.cache_state()[1] == 0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_eos_and_the_token_limit(graph):
    gen = _gen()
    e, mask = _inputs("left")
    T_, k, p = SETTINGS["k40p95"]
    seed = SEEDS[1]
    tok = _sample("left", "k40p95", seed)
    kw = dict(temperature=T_, top_k=k, top_p=p, seed=seed, pad_token_id=0)
    mid = NEW // 2
    eos = int(tok[mid])
    with torch.no_grad():
        want = gen.sample(e, mask, None, max_new_tokens=NEW, eos_token_id=eos, graph=graph, **kw)
        assert want.shape[1] <= mid + 1 and int(want[0, -1]) == eos
        for look in (None, tok[None]):
            got = gen.lookup_sample(e, mask, None, lookup_ids=look, max_new_tokens=NEW, prompt_lookup_num_tokens=4, eos_token_id=eos, graph=graph,
                                    poll_every=2, **kw)
            assert torch.equal(got, want), (got.tolist(), want.tolist())
        for limit in (1, 3):
            got, st = gen.lookup_sample(e, mask, None, lookup_ids=tok[None], max_new_tokens=limit, prompt_lookup_num_tokens=15, graph=graph,
                                        return_stats=True, **kw)
            assert torch.equal(got[0], tok[:limit]) and st["tokens"] == limit and st["steps"] <= limit - 1, (limit, got.tolist(), st)
    assert gen.cache_state()[1] == 0


@pytest.mark.parametrize("weights", ["fp8_e4m3", "mxfp4"])
def test_weight_formats(weights):
    gen = _gen(weights)
    e, mask = _inputs("left")
    T_, k, p = SETTINGS["predict"]
    tok = _sample("left", "predict", SEEDS[0], weights)
    with torch.no_grad():
        got, st = gen.lookup_sample(e, mask, None, lookup_ids=tok[None], max_new_tokens=NEW, temperature=T_, top_k=k, top_p=p, seed=SEEDS[0],
                                    pad_token_id=0, return_stats=True)
    assert torch.equal(got[0], tok) and st["steps"] == _predict_steps(tok[None], tok, 7, 2) < NEW - 1, st


# ---- log-probabilities of a lookup generation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("n", [0, 5, 16])
@pytest.mark.parametrize("how", ["greedy", "sample"])
def test_logprobs_of_a_lookup_generation(how, n, graph):
    gen = _gen()
    e, mask = _inputs("left")
    T_, k, p = SETTINGS["k40p95"]
    skw = dict(temperature=T_, top_k=k, top_p=p, seed=SEEDS[0]) if how == "sample" else {}
    plain, lookup = (gen.sample, gen.lookup_sample) if how == "sample" else (gen.greedy, gen.lookup_greedy)
    with torch.no_grad():
        want_tok, want = plain(e, mask, None, max_new_tokens=NEW, pad_token_id=0, logprobs=n, graph=graph, **skw)
        got_tok, got, st = lookup(e, mask, None, lookup_ids=want_tok, max_new_tokens=NEW, pad_token_id=0, logprobs=n, graph=graph, poll_every=3,
                                  return_stats=True, **skw)
    assert st["steps"] < st["tokens"] - 1, st                    # steps that emitted several tokens took part
    m = got_tok.shape[1]
    assert m == NEW and torch.equal(got_tok, want_tok[:, :m])
    for name in ("token_logprobs", "top_ids", "top_logprobs"):
        a, b = getattr(got, name), getattr(want, name)[:, :m]
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (how, n, name, a, b)
    assert bool(torch.isfinite(got.token_logprobs).all()) and got.top_ids.shape == (1, NEW, n)


# ---- the public entry points -------------------------------------------------------------------------------------------------------------------
def test_generate_and_the_patched_generate_take_the_lookup():
    """ml_fastvlm_amd.generate(prompt_lookup_num_tokens=K, logprobs=n) returns what generate(logprobs=n) returns, and
    builder._make_library_generate(prompt_lookup=True) - what install_into_llava(generate=True, prompt_lookup=True) installs - runs
    transformers' own keyword on the library, greedy and sampled, with the tokens of the call without it"""
    import warnings

    import ml_fastvlm_amd
    from transformers import Qwen2ForCausalLM
    from ml_fastvlm_amd import builder
    from ml_fastvlm_amd import splice as S

    class StandIn(Qwen2ForCausalLM):
        def prepare_inputs_labels_for_multimodal(self, input_ids, position_ids, attention_mask, past_key_values, labels, images, image_sizes=None):
            o = S.multimodal_splice(input_ids, position_ids, attention_mask, labels, images, self.get_input_embeddings().weight, "right", None)
            return o[0], o[1], o[2], past_key_values, o[4], o[5]

    _gen()
    m16, _ = _gens["model"]
    model = StandIn(m16.config).eval()
    model.load_state_dict(m16.state_dict())
    model = model.to("cuda", torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(10, 4000, (1, 12), generator=g)
    ids[:, 3] = -200                                              # IMAGE_TOKEN_INDEX
    ids = ids.cuda()
    feats = (0.5 * torch.randn(1, 16, 896, generator=g)).to("cuda", torch.bfloat16)
    img = dict(images=feats, image_sizes=[(256, 256)])
    want_tok, want = ml_fastvlm_amd.generate(model, ids, max_new_tokens=NEW, pad_token_id=0, logprobs=5, **img)
    got_tok, got = ml_fastvlm_amd.generate(model, ids, max_new_tokens=NEW, pad_token_id=0, logprobs=5, prompt_lookup_num_tokens=7, **img)
    assert torch.equal(got_tok, want_tok) and all(torch.equal(a, b) for a, b in zip(got, want))
    orig = StandIn.generate
    call = dict(num_beams=1, max_new_tokens=NEW, use_cache=True, pad_token_id=0, **img)
    try:
        StandIn.generate = builder._make_library_generate(orig, prompt_lookup=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                        # no fallback warning: the library took every call
            for kw in (dict(do_sample=False), dict(do_sample=True, temperature=0.2, top_p=None)):
                torch.manual_seed(5)                              # (the sampled call draws its seed from torch's CPU generator)
                plain = model.generate(ids, **call, **kw)
                torch.manual_seed(5)
                got = model.generate(ids, **call, **kw, prompt_lookup_num_tokens=7, max_matching_ngram_size=3)
                assert got.shape == (1, NEW) and torch.equal(got, plain), (kw, got.tolist(), plain.tolist())
                assert kw["do_sample"] or torch.equal(got, want_tok)
    finally:
        StandIn.generate = orig


# ---- the opt-in is restored ------------------------------------------------------------------------------------------------------------------
def test_the_opt_in_ends_with_the_run():
    from ml_fastvlm_amd import _lib
    gen = _gen()
    e, mask = _inputs("left")
    tok = _sample("left", "predict", SEEDS[0])
    T_, k, p = SETTINGS["predict"]
    with torch.no_grad():
        gen.lookup_sample(e, mask, None, lookup_ids=tok[None], max_new_tokens=NEW, temperature=T_, top_k=k, top_p=p, seed=SEEDS[0], pad_token_id=0)
        gen.spec_reserve(8)
        gen.set_sampling(True, T_, k, p, SEEDS[0])
        try:
            gen.start(e, mask)
            with pytest.raises(_lib.FvhdError, match="sampling is on"):
                gen.verify(tok[1:4].contiguous())
        finally:
            gen.set_sampling(False)
        gen.start(e, mask)                                       # and greedy verification is what it was
        _, ids, emitted = gen.verify(tok[1:4].contiguous())
        assert 1 <= int(emitted) <= 4 and gen.cache_state() == (P + int(emitted), 0)
