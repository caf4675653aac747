"""Decode-step time of the Qwen2 LLM on one MI355X: the library's steps (`ml_fastvlm_amd.qwen2_decode.Qwen2Generator`) replayed as one
captured graph and called eagerly, against the stock `transformers` decode loop continuing from the same prefill cache.

    python tools/decode_bench.py [--hidden 896 1536 3584] [--batch 1 8 16 32 64] [--prompt 285] [--new 128] [--repeats 3] [--no-stock]
    python tools/decode_bench.py --sample [--hidden 896] [--batch 1 8]
    python tools/decode_bench.py --trace-steps 16 --hidden 3584 --batch 64      (eager steps only: the program of a kernel trace)
    python tools/decode_bench.py --weights fp8_e4m3 ...                         (the packed matrices as e4m3 codes + row scales)
    python tools/decode_bench.py --weights mxfp4 ...                            (as MXFP4: e2m1 codes + one scale byte per 32 elements)
    python tools/decode_bench.py --num-beams 4 --hidden 896 3584 --batch 1 16   (beam search: --batch prompts x K beams per step)
    python tools/decode_bench.py --processors --hidden 896 --batch 1 64         (logits processors on against off, greedy and sampled)
    python tools/decode_bench.py --num-beams 4 --processors --hidden 896 3584 --batch 1 16   (the beam step under repetition_penalty 1.2, no_repeat_ngram_size 3)
    python tools/decode_bench.py --num-beams 4 --constraint --hidden 896 3584 --batch 1 16   (the beam step under a token automaton; both flags combine)
    python tools/decode_bench.py --lookup --hidden 896 3584 --rows 4 8 16       (prompt-lookup decoding: the verify step at one sequence)
    python tools/decode_bench.py --lookup --trace-steps 16 --hidden 896 --rows 8    (eager verify steps only: the program of a kernel trace)
    python tools/decode_bench.py --logprobs 0 5 16 --hidden 896 3584 --batch 1 64   (log-probabilities of the chosen tokens inside the step)
    python tools/decode_bench.py --constraint --hidden 896 3584 --batch 1 64        (constrained decoding: a token automaton masks the logits)
    python tools/decode_bench.py --lookup-sample 7 --hidden 896 3584 --repeats 3    (the lookup step under sampling and with log-probabilities)
    python tools/decode_bench.py --warpers --hidden 896 3584 --batch 1 64           (min_p / typical_p / epsilon_cutoff / eta_cutoff in the sampled step)

--batch takes up to 64 sequences per step (more than 16 need a library of version 503).  --repeats times the graph replay that many
times (`graph_ms_per_token` is their median, `graph_ms_per_token_runs` all of them); --no-stock leaves the stock transformers loop (and
the eager library step) out - above 16 sequences it only measures transformers.  A width's model is built and packed once for all batches.

--sample times the sampled step (`Qwen2Generator.set_sampling`, csrc/llm_sample.hip) next to the greedy one, both by graph replay at
vocab 151936, with predict.py's settings (temperature 0.2, top_k 50: transformers' default) and a flat one (temperature 1.0, top_k 0,
top_p 0.95); greedy is timed before and after the sampled settings and averaged.

--num-beams K times one beam-search step (`Qwen2Generator.beam_search`'s: cache reorder, decode step with logits, top continuations,
bookkeeping) by graph replay over a whole search of --new tokens, and - each captured and replayed on its own, on the state the search
left - its parts: the plain step on the same rows, the reorder (with the search's last parent map, and with the worst one: every row
moves), the top-K launches and the torch bookkeeping; then the stock `transformers` beam search on the same prompts.

--processors times the step with all four logits processors on (`Qwen2Generator.set_logits_processors`, csrc/llm_logits.hip:
repetition_penalty 1.2, no_repeat_ngram_size 3, min_new_tokens 8 with two EOS ids, three suppressed ids) against the same build's step
with none, greedy and sampled (predict.py's settings), each by graph replay over --new tokens, measured twice in alternation and averaged.
The addition is split by differences of whole steps: logits store = greedy with logits_out - greedy; process launch = sampled on - sampled
off (the sampler stores its logits and chooses the same way either way); argmax from the logits = greedy on - greedy with logits_out -
process launch.

--lookup times the verify step of prompt-lookup decoding (`Qwen2Generator.verify / lookup_greedy`, csrc/llm_spec.hip) at one sequence, by
graph replay, for --rows 4 8 16 rows per step: the plain step at B = 1 and at B = rows (the yardstick: the same GEMMs, attention over
`rows` caches instead of one), the verify step with every draft WRONG (a fixed draft id the recorded greedy run never emits: one token
per step) and with every draft RIGHT (drafts from the recorded greedy run: `rows` tokens per step), the whole lookup step (draft +
verify + accept) with the recorded run as lookup ids (drafts right wherever the run's 2-grams are unique: `accepted_per_step` says how
many were), and the draft and accept launches replayed alone.  Derived: tokens per second at full acceptance and the break-even
acceptance per draft (t_verify / t_plain(1) - 1) / (rows - 1), t_verify = the slower of the two verify runs.  Random weights
emit noise-like tokens: no acceptance rate on real text is claimed here.

--logprobs N ... times the captured greedy step with the log-probabilities of the chosen tokens (`Qwen2Generator.set_logprobs` / `.logprobs`,
csrc/llm_logprobs.hip) for every top-n named, against the same build's step without them and against the composition the library allowed
before inside the same graph: `step(logits=True)` + torch.log_softmax + gather + topk(n) (n = 0: no topk).  Every case by graph replay over
--new tokens at vocab 151936, measured twice (the second time in reverse order) and averaged; `off` twice more at the ends, so that its
four runs show the run-to-run spread the additions are read against.

--constraint times the captured greedy step with a token automaton on (`Qwen2Generator.set_constraint`, csrc/llm_constrain.hip) for two
kinds of state - sparse (4 edges) and dense (every other id: vocab / 2 edges), each one state that leads back to itself - against the same
build's step without it and against torch doing the same job inside the same captured step from dense [states, vocab] tables:
`state = nxt[state, fed]; logits.masked_fill_(~allowed[state], -inf); fed = logits.argmax(-1)` behind `step(fed, logits=True)` (a baseline
written for the measurement).  Every case by graph replay over --new tokens, measured twice (the second time in reverse order) and averaged;
`off` twice more at the ends, so that its four runs show the run-to-run spread the additions are read against.

--lookup-sample K times the whole lookup step (draft + verify of K + 1 rows + accept; `Qwen2Generator.lookup_greedy / lookup_sample`) by
graph replay under greedy selection and under sampling (predict.py's settings: the T-row sampler in place of the argmax reduce), each
without and with log-probabilities (--logprobs N, default 5: the logits rows kept, the logprobs launch at B = K + 1, the copy behind the
accept), next to the plain step the same four ways; every case once per round (--repeats), the rounds in alternating order, medians
reported.  No lookup ids are given, so on random weights a step emits one token but for chance matches (`accepted_per_step`).  Derived: the
accepted drafts per step at which the lookup step breaks even with the plain one, t_lookup / t_plain - 1.

--guidance: the step under classifier-free guidance (`Qwen2Generator.set_guidance`, csrc/llm_guidance.hip) for G prompts (--batch) = 2 G rows
against the same build's plain step at B = 2 G and against the stock loop's two eager forwards per token (`measure_guidance`); --out FILE
also writes the result line to a file.

Full layer counts, random bf16 weights (`tools/ttft.py: build_llm`).  Prints ONE JSON line: per (width, batch) the ms per token of each
path, the bytes a step must read (packed weights + the KV cache at the mean length) and their fraction of 8 TB/s."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _ms_per(fn, n, dev):
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / n


@torch.no_grad()
def measure(llm, pre, batch: int, prompt: int, new: int, dev, repeats: int = 1, stock: bool = True, trace_steps: int = 0, weights: str = "bf16") -> dict:
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import kv_to_dynamic_cache
    cfg = llm.config
    hidden = cfg.hidden_size
    gen = Qwen2Generator.from_hf(llm, batch, prompt + new + 4, prefill=pre, weights=weights)
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(batch, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(batch, prompt, device=dev, dtype=torch.long)
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "batch": batch, "prompt": prompt, "new_tokens": new, "weights": weights}
    if trace_steps:                                         # a kernel trace's program: the prefill and `trace_steps` eager steps, nothing else
        gen.start(emb, mask, logits=False)
        for _ in range(trace_steps):
            gen.step(logits=False)
        torch.cuda.synchronize(dev)
        res["trace_steps"] = trace_steps
        return res
    # graph replay of one captured step
    gen.start(emb, mask, logits=False)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            gen.step(logits=False)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph.replay()
    runs = []
    for _ in range(max(1, repeats)):
        gen.start(emb, mask, logits=False)
        runs.append(round(_ms_per(graph.replay, new, dev), 4))
        assert gen.cache_state() == (prompt + new, 0)
    res["graph_ms_per_token"] = sorted(runs)[len(runs) // 2]
    res["graph_ms_per_token_runs"] = runs
    nkv, hd = cfg.num_key_value_heads, hidden // cfg.num_attention_heads
    wbytes = step_weight_bytes(cfg, weights)
    kvbytes = cfg.num_hidden_layers * batch * nkv * (prompt + new / 2) * hd * 2 * 2
    res["weight_bytes_per_token"] = int(wbytes)
    res["kv_bytes_per_token"] = int(kvbytes)
    res["fraction_of_8TBps_graph"] = round((wbytes + kvbytes) / (res["graph_ms_per_token"] * 1e-3) / 8e12, 3)
    if not stock:
        return res
    gen.start(emb, mask, logits=False)
    res["eager_ms_per_token"] = round(_ms_per(lambda: gen.step(logits=False), new, dev), 4)
    # the stock transformers loop (eager module calls, DynamicCache) continuing from the same prefill's cache
    logits, k, v = pre(emb, mask, None, return_kv=True)
    cache = kv_to_dynamic_cache(k, v)
    state = {"tok": logits.argmax(-1), "mask": mask, "pos": torch.full((batch, 1), prompt - 1, device=dev, dtype=torch.long)}

    def hf_step():
        state["mask"] = torch.cat([state["mask"], torch.ones(batch, 1, device=dev, dtype=torch.long)], 1)
        state["pos"] = state["pos"] + 1
        out = llm(input_ids=state["tok"][:, None], attention_mask=state["mask"], position_ids=state["pos"], past_key_values=cache, use_cache=True)
        state["tok"] = out.logits[:, -1].argmax(-1)

    for _ in range(3):                                      # lazy initialisation of the stock path stays out of the timing
        hf_step()
    res["stock_transformers_ms_per_token"] = round(_ms_per(hf_step, new, dev), 4)
    res["speedup_graph_vs_stock"] = round(res["stock_transformers_ms_per_token"] / res["graph_ms_per_token"], 2)
    return res


def measure_width(hidden: int, batches, prompt: int, new: int, dev, weights: str = "bf16", **kw) -> list:
    """every batch of one width on ONE model and ONE packed copy of its weights"""
    from tools.ttft import build_llm
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    llm = build_llm(hidden, dev)
    pre = Qwen2Prefill.from_hf(llm, weights=weights)        # ("bf16" asks nothing new of the library: a build before 504 still measures)
    rows = []
    for b in batches:
        rows.append(measure(llm, pre, b, prompt, new, dev, weights=weights, **kw))
        torch.cuda.empty_cache()
    del pre, llm
    torch.cuda.empty_cache()
    return rows


WARPER_SETTINGS = {"min_p": dict(min_p=0.05), "typical_p": dict(typical_p=0.9), "epsilon_cutoff": dict(epsilon_cutoff=3e-4),
                   "eta_cutoff": dict(eta_cutoff=2e-3), "all_four": dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=2e-3)}


@torch.no_grad()
def measure_warpers(llm, pre, batch: int, prompt: int, new: int, dev, repeats: int = 3) -> dict:
    """the sampled step (predict.py's settings) plain - `repeats` runs, whose spread the additions are read against; on a library built
    before the warpers that is all - then with each warper alone and all four, and torch doing all four from step(logits=True) inside the
    same captured graph (transformers' warpers restated in plain torch, and torch.multinomial: a baseline written for the measurement)"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    hidden = llm.config.hidden_size
    gen = Qwen2Generator(pre, batch, prompt + new + 4, embed_tokens=None if llm.config.tie_word_embeddings else llm.get_input_embeddings().weight,
                         tie_word_embeddings=bool(llm.config.tie_word_embeddings))
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(batch, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(batch, prompt, device=dev, dtype=torch.long)
    st = SAMPLE_SETTINGS["predict_py"]
    res = {"hidden": hidden, "layers": llm.config.num_hidden_layers, "batch": batch, "vocab": llm.config.vocab_size, "prompt": prompt,
           "new_tokens": new, "settings": st, "warpers": WARPER_SETTINGS}

    def graph_ms(warpers, torch_job=False):
        gen.set_sampling(True, seed=1, **st, **(warpers or {}))
        gen.start(emb, mask, logits=False)
        fed = torch.zeros(batch, device=dev, dtype=torch.long)

        a4, NEG = WARPER_SETTINGS["all_four"], float("-inf")

        def entropy_of(s):                                  # -(p log p) summed over the kept tokens (0 * -inf counts as 0: transformers' nansum)
            logp = torch.log_softmax(s, -1)
            return logp, -torch.nan_to_num(logp.exp() * logp, nan=0.0).sum(-1, keepdim=True)

        def torch_step():
            # transformers' warpers restated in plain torch without a host synchronisation (its EtaLogitsWarper builds a validated
            # torch.distributions.Categorical per call, which reads a flag back and cannot be captured)
            lg, _ = gen.step(fed, logits=True)
            s = lg / st["temperature"]
            s = s.masked_fill(s < s.topk(st["top_k"], -1).values[..., -1:], NEG)
            p = torch.softmax(s, -1)
            s = s.masked_fill(p < a4["min_p"] * p.amax(-1, keepdim=True), NEG)
            logp, ent = entropy_of(s)
            key, idx = torch.sort((-logp - ent).abs(), -1)
            cum = s.gather(-1, idx).softmax(-1).cumsum(-1)
            last = (cum < a4["typical_p"]).sum(-1, keepdim=True).clamp(max=s.shape[-1] - 1)
            drop = key > key.gather(-1, last)
            drop[..., :1] = False
            s = s.masked_fill(drop.scatter(-1, idx, drop), NEG)
            p = torch.softmax(s, -1)
            s = s.masked_fill((p < a4["epsilon_cutoff"]) & (s < s.amax(-1, keepdim=True)), NEG)
            logp, ent = entropy_of(s)
            eta = (math.sqrt(a4["eta_cutoff"]) * torch.exp(-ent)).clamp(max=a4["eta_cutoff"])
            s = s.masked_fill((logp.exp() < eta) & (s < s.amax(-1, keepdim=True)), NEG)
            p = torch.softmax(s, -1)
            if torch_job == "multinomial":
                fed.copy_(torch.multinomial(p, 1)[:, 0])
            else:                                           # the same draw as torch.multinomial makes it: argmax of p / Exp(1)
                fed.copy_((p / torch.empty_like(p).exponential_()).argmax(-1))

        one = torch_step if torch_job else (lambda: gen.step(logits=False))
        if torch_job:
            one()                                           # lazy initialisation stays out of the capture
            gen.start(emb, mask, logits=False)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                one()
        torch.cuda.current_stream(dev).wait_stream(side)
        graph.replay()
        gen.start(emb, mask, logits=False)
        ms = _ms_per(graph.replay, new, dev)
        assert gen.cache_state() == (prompt + new, 0)
        return ms

    plain = [graph_ms(None) for _ in range(max(repeats, 3))]
    res["plain_sample_graph_ms_per_token_runs"] = [round(x, 4) for x in plain]
    res["plain_sample_graph_ms_per_token"] = round(sorted(plain)[len(plain) // 2], 4)
    res["plain_spread_us"] = round(1000 * (max(plain) - min(plain)), 1)
    if _lib.has("sampling_warpers"):
        for name, w in WARPER_SETTINGS.items():
            ms = graph_ms(w)
            res[f"{name}_graph_ms_per_token"] = round(ms, 4)
            res[f"{name}_added_us_per_token"] = round(1000 * (ms - res["plain_sample_graph_ms_per_token"]), 1)
        for draw in ("multinomial", "exponential_argmax"):  # the second only if a capture refuses the first
            try:
                ms = graph_ms(None, torch_job=draw)
            except Exception as e:
                res[f"torch_all_four_{draw}_error"] = f"{type(e).__name__}: {str(e)[:200]}"
                continue
            res["torch_all_four_draw"] = draw
            res["torch_all_four_graph_ms_per_token"] = round(ms, 4)
            res["torch_all_four_added_us_per_token"] = round(1000 * (ms - res["plain_sample_graph_ms_per_token"]), 1)
            break
    gen.set_sampling(False)
    del gen
    torch.cuda.empty_cache()
    return res


SAMPLE_SETTINGS = {"predict_py": dict(temperature=0.2, top_k=50, top_p=1.0), "flat": dict(temperature=1.0, top_k=0, top_p=0.95)}


@torch.no_grad()
def measure_sample(hidden: int, batch: int, prompt: int, new: int, dev) -> dict:
    from tools.ttft import build_llm
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    llm = build_llm(hidden, dev)
    gen = Qwen2Generator.from_hf(llm, batch, prompt + new + 4)
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(batch, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(batch, prompt, device=dev, dtype=torch.long)
    res = {"hidden": hidden, "layers": llm.config.num_hidden_layers, "batch": batch, "vocab": llm.config.vocab_size, "prompt": prompt,
           "new_tokens": new}

    def graph_ms(settings):
        if settings is None:
            gen.set_sampling(False)
        else:
            gen.set_sampling(True, seed=1, **settings)
        gen.start(emb, mask, logits=False)
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                gen.step(logits=False)
        torch.cuda.current_stream(dev).wait_stream(side)
        graph.replay()
        gen.start(emb, mask, logits=False)
        ms = _ms_per(graph.replay, new, dev)
        assert gen.cache_state() == (prompt + new, 0)
        return ms

    greedy = [graph_ms(None)]
    for name, st in SAMPLE_SETTINGS.items():
        res[f"{name}_settings"] = st
        res[f"{name}_graph_ms_per_token"] = round(graph_ms(st), 4)
    greedy.append(graph_ms(None))
    gen.set_sampling(False)
    res["greedy_graph_ms_per_token"] = round(sum(greedy) / 2, 4)
    res["greedy_graph_ms_per_token_runs"] = [round(x, 4) for x in greedy]
    for name in SAMPLE_SETTINGS:
        res[f"{name}_added_us_per_token"] = round(1000 * (res[f"{name}_graph_ms_per_token"] - res["greedy_graph_ms_per_token"]), 1)
    del gen, llm
    torch.cuda.empty_cache()
    return res


PROCESSORS = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8, eos_token_id=[151645, 151643], suppress_tokens=[0, 1, 2])


@torch.no_grad()
def measure_processors(llm, pre, batch: int, prompt: int, new: int, dev) -> dict:
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    cfg = llm.config
    hidden = cfg.hidden_size
    gen = Qwen2Generator.from_hf(llm, batch, prompt + new + 4, prefill=pre)
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(batch, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(batch, prompt, device=dev, dtype=torch.long)
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "batch": batch, "vocab": cfg.vocab_size, "prompt": prompt, "new_tokens": new,
           "processors": PROCESSORS, "sampling": SAMPLE_SETTINGS["predict_py"]}

    def graph_ms(sample, proc, logits):
        gen.set_sampling(bool(sample), seed=1, **(SAMPLE_SETTINGS["predict_py"] if sample else {}))
        gen.set_logits_processors(**(PROCESSORS if proc else {}))
        gen.start(emb, mask, logits=False)
        graph = _graph_of(lambda: gen.step(logits=logits), dev)
        graph.replay()
        gen.start(emb, mask, logits=False)
        ms = _ms_per(graph.replay, new, dev)
        assert gen.cache_state() == (prompt + new, 0)
        return ms

    cases = {"greedy_off": (False, False, False), "greedy_off_logits_out": (False, False, True), "greedy_on": (False, True, False),
             "sample_off": (True, False, False), "sample_on": (True, True, False)}
    runs = {k: [] for k in cases}
    for order in (list(cases), list(cases)[::-1]):              # twice, the second time in reverse order
        for k in order:
            runs[k].append(graph_ms(*cases[k]))
    gen.set_sampling(False)
    gen.set_logits_processors()
    for k, v in runs.items():
        res[f"{k}_ms_per_token"] = round(sum(v) / len(v), 4)
        res[f"{k}_ms_per_token_runs"] = [round(x, 4) for x in v]
    us = lambda a, b: round(1000 * (res[f"{a}_ms_per_token"] - res[f"{b}_ms_per_token"]), 1)      # noqa: E731
    res["greedy_added_us_per_token"] = us("greedy_on", "greedy_off")
    res["sample_added_us_per_token"] = us("sample_on", "sample_off")
    res["logits_store_us"] = us("greedy_off_logits_out", "greedy_off")
    res["process_launch_us"] = res["sample_added_us_per_token"]
    res["argmax_from_logits_us"] = round(us("greedy_on", "greedy_off_logits_out") - res["process_launch_us"], 1)
    del gen
    return res


@torch.no_grad()
def measure_logprobs(llm, pre, batch: int, prompt: int, new: int, dev, ns) -> dict:
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    cfg = llm.config
    hidden = cfg.hidden_size
    gen = Qwen2Generator.from_hf(llm, batch, prompt + new + 4, prefill=pre)
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(batch, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(batch, prompt, device=dev, dtype=torch.long)
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "batch": batch, "vocab": cfg.vocab_size, "prompt": prompt, "new_tokens": new,
           "top_n": list(ns)}
    gen._set_greedy()
    tok = torch.zeros((batch,), device=dev)
    top_i = {n: torch.zeros((batch, n), device=dev, dtype=torch.long) for n in ns}
    top_v = {n: torch.zeros((batch, n), device=dev) for n in ns}

    def lib_step(n):
        gen.step(logits=False)
        gen.logprobs(n, tok, top_i[n] if n else None, top_v[n] if n else None)

    def torch_step(n):                                      # what the library allowed before: the logits out, three torch ops
        lg, ids = gen.step(logits=True)
        ls = torch.log_softmax(lg, dim=-1)
        tok.copy_(ls.gather(1, ids[:, None])[:, 0])
        if n:
            v, i = torch.topk(ls, n, dim=-1)
            top_v[n].copy_(v)
            top_i[n].copy_(i)

    def graph_ms(kind, n):
        gen.set_logprobs(kind == "lib")
        gen.start(emb, mask, logits=False)
        fn = {"off": lambda: gen.step(logits=False), "lib": lambda: lib_step(n), "torch": lambda: torch_step(n)}[kind]
        graph = _graph_of(fn, dev)
        graph.replay()
        gen.start(emb, mask, logits=False)
        ms = _ms_per(graph.replay, new, dev)
        assert gen.cache_state() == (prompt + new, 0)
        return ms

    cases = {"off": ("off", 0)}
    for n in ns:
        cases[f"logprobs_{n}"] = ("lib", n)
        cases[f"torch_{n}"] = ("torch", n)
    runs = {k: [] for k in cases}
    runs["off"].append(graph_ms("off", 0))
    for order in (list(cases), list(cases)[::-1]):              # twice, the second time in reverse order
        for k in order:
            runs[k].append(graph_ms(*cases[k]))
    runs["off"].append(graph_ms("off", 0))
    gen.set_logprobs(False)
    for k, v in runs.items():
        res[f"{k}_ms_per_token"] = round(sum(v) / len(v), 4)
        res[f"{k}_ms_per_token_runs"] = [round(x, 4) for x in v]
    res["off_spread_us"] = round(1000 * (max(runs["off"]) - min(runs["off"])), 1)
    for n in ns:
        for kind in ("logprobs", "torch"):
            res[f"{kind}_{n}_added_us_per_token"] = round(1000 * (res[f"{kind}_{n}_ms_per_token"] - res["off_ms_per_token"]), 1)
    del gen
    return res


@torch.no_grad()
def measure_constraint(llm, pre, batch: int, prompt: int, new: int, dev) -> dict:
    from ml_fastvlm_amd.constraints import TokenAutomaton
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    cfg = llm.config
    hidden, V = cfg.hidden_size, cfg.vocab_size
    gen = Qwen2Generator.from_hf(llm, batch, prompt + new + 4, prefill=pre)
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(batch, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(batch, prompt, device=dev, dtype=torch.long)
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "batch": batch, "vocab": V, "prompt": prompt, "new_tokens": new}
    gen._set_greedy()
    ids = {"sparse": [5, V // 3, V // 2 + 1, V - 2], "dense": list(range(0, V, 2))}
    res["edges"] = {k: len(v) for k, v in ids.items()}
    allowed_ids = {k: set(v) for k, v in ids.items()}
    autos = {k: TokenAutomaton([0, len(v)], v, [0] * len(v), V) for k, v in ids.items()}      # one state that leads back to itself
    state = torch.zeros((batch,), device=dev, dtype=torch.long)
    fed = torch.zeros((batch,), device=dev, dtype=torch.long)
    dense = {}
    for k, a in autos.items():                              # the torch baseline's tables: allowed bool [S, V], nxt int64 [S, V] (-1 = FREE is not reached)
        dense[k] = (a.mask([0]).to(dev), torch.zeros((1, V), device=dev, dtype=torch.long))

    def torch_step(kind):
        allowed, nxt = dense[kind]
        lg, _ = gen.step(fed, logits=True)
        state.copy_(nxt[state, fed])
        lg.masked_fill_(~allowed[state], float("-inf"))
        fed.copy_(lg.argmax(-1))

    def graph_ms(how, kind):
        gen.set_constraint(autos[kind] if how == "lib" else None)
        _, first = gen.start(emb, mask, logits=False)
        state.zero_()
        fed.copy_(torch.full_like(first, ids[kind][0]) if how == "torch" else first)
        fn = {"off": lambda: gen.step(logits=False), "lib": lambda: gen.step(logits=False), "torch": lambda: torch_step(kind)}[how]
        graph = _graph_of(fn, dev)
        graph.replay()
        _, first = gen.start(emb, mask, logits=False)
        state.zero_()
        fed.copy_(torch.full_like(first, ids[kind][0]) if how == "torch" else first)
        ms = _ms_per(graph.replay, new, dev)
        assert gen.cache_state() == (prompt + new, 0)
        if how == "lib":
            st, fl = gen.constraint_state()
            assert st.tolist() == [0] * batch and fl.tolist() == [0] * batch
        if how != "off":
            chosen = (fed if how == "torch" else gen._ids[:batch]).tolist()
            assert all(t in allowed_ids[kind] for t in chosen)
        return ms

    cases = {"off": ("off", "sparse")}
    for kind in ids:
        cases[f"constraint_{kind}"] = ("lib", kind)
        cases[f"torch_{kind}"] = ("torch", kind)
    runs = {k: [] for k in cases}
    runs["off"].append(graph_ms("off", "sparse"))
    for order in (list(cases), list(cases)[::-1]):              # twice, the second time in reverse order
        for k in order:
            runs[k].append(graph_ms(*cases[k]))
    runs["off"].append(graph_ms("off", "sparse"))
    gen.set_constraint()
    for k, v in runs.items():
        res[f"{k}_ms_per_token"] = round(sum(v) / len(v), 4)
        res[f"{k}_ms_per_token_runs"] = [round(x, 4) for x in v]
    res["off_spread_us"] = round(1000 * (max(runs["off"]) - min(runs["off"])), 1)
    for kind in ids:
        for how in ("constraint", "torch"):
            res[f"{how}_{kind}_added_us_per_token"] = round(1000 * (res[f"{how}_{kind}_ms_per_token"] - res["off_ms_per_token"]), 1)
    del gen
    return res


@torch.no_grad()
def measure_lookup(llm, pre, rows_list, prompt: int, new: int, dev, repeats: int = 1, weights: str = "bf16", trace_steps: int = 0) -> dict:
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    cfg = llm.config
    hidden, V = cfg.hidden_size, cfg.vocab_size
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "vocab": V, "prompt": prompt, "new_tokens": new, "weights": weights, "rows": {}}
    g0 = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(1, prompt, hidden, device=dev, generator=g0)).to(torch.bfloat16)
    mask = torch.ones(1, prompt, device=dev, dtype=torch.long)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731

    def plain(batch):                                       # the plain step at `batch` rows, as `measure` times it
        gen = Qwen2Generator.from_hf(llm, batch, prompt + new + 20, prefill=pre, weights=weights)
        e, m = emb.expand(batch, -1, -1).contiguous(), mask.expand(batch, -1).contiguous()
        gen.start(e, m, logits=False)
        graph = _graph_of(lambda: gen.step(logits=False), dev)
        graph.replay()
        runs = []
        for _ in range(max(1, repeats)):
            gen.start(e, m, logits=False)
            runs.append(round(_ms_per(graph.replay, new, dev), 4))
            assert gen.cache_state() == (prompt + new, 0)
        del gen
        return runs

    if trace_steps:                                         # a kernel trace's program: the prefill and eager verify steps (every draft wrong) at rows_list[0]
        gen = Qwen2Generator.from_hf(llm, 1, prompt + new + 20, prefill=pre, weights=weights)
        gen.spec_reserve(rows_list[0])
        drafts = torch.zeros((rows_list[0] - 1,), device=dev, dtype=torch.long)
        gen.start(emb, mask, logits=False)
        for _ in range(trace_steps):
            gen.verify(drafts, logits=False)
        torch.cuda.synchronize(dev)
        res["trace_steps"], res["trace_rows"] = trace_steps, rows_list[0]
        return res
    yard = {T: plain(T) for T in rows_list}
    res["plain_ms_runs"] = plain(1)
    res["plain_ms"] = med(res["plain_ms_runs"])
    gen = Qwen2Generator.from_hf(llm, 1, prompt + new + 20, prefill=pre, weights=weights)      # the cache the verify steps run on: made last
    rec = gen.greedy(emb, mask, None, max_new_tokens=new, pad_token_id=0)[0]                   # the recorded greedy run
    wrong = next(t for t in range(V) if t not in set(rec.tolist()))
    lib = _lib.lookup_lib()
    for T in rows_list:
        r = {"plain_at_B_rows_ms_runs": yard[T], "plain_at_B_rows_ms": med(yard[T])}
        gen.spec_reserve(16, new)
        # every draft wrong: one token per step, `new - 1` steps
        drafts = torch.full((T - 1,), wrong, device=dev, dtype=torch.long)
        gen.start(emb, mask, logits=False)
        graph = _graph_of(lambda: gen.verify(drafts, logits=False), dev)
        runs = []
        for _ in range(max(1, repeats)):
            gen.start(emb, mask, logits=False)
            runs.append(round(_ms_per(graph.replay, new - 1, dev), 4))
            assert gen.cache_state() == (prompt + new - 1, 0)
        r["verify_all_wrong_ms_runs"], r["verify_all_wrong_ms"] = runs, med(runs)
        # every draft right: drafts taken from the recorded run, T tokens per step.  The drafts of step k are row k of a table, copied
        # into the fixed draft buffer by two small torch kernels inside the graph (index_select + counter); those two are replayed alone
        # and their time is subtracted
        nst = (new - 1) // T
        table = torch.stack([rec[k * T + 1:(k + 1) * T] for k in range(nst)]).contiguous()
        idx = torch.zeros(1, device=dev, dtype=torch.long)

        def feed():
            torch.index_select(table, 0, idx, out=drafts.view(1, T - 1))
            idx.add_(1)

        def right_step():
            feed()
            gen.verify(drafts, logits=False)

        gen.start(emb, mask, logits=False)
        graph, feed_graph = _graph_of(right_step, dev), _graph_of(feed, dev)
        runs, feeds = [], []
        for _ in range(max(1, repeats)):
            idx.zero_()
            feeds.append(_ms_per(feed_graph.replay, nst, dev))
            gen.start(emb, mask, logits=False)
            idx.zero_()
            runs.append(round(_ms_per(graph.replay, nst, dev) - feeds[-1], 4))
            assert gen.cache_state() == (prompt + nst * T, 0), "a draft from the recorded run was rejected"
        r["verify_all_right_ms_runs"], r["verify_all_right_ms"], r["draft_feed_us"] = runs, med(runs), round(1000 * med(feeds), 1)
        # the whole lookup step (draft + verify + accept) with the recorded run as lookup ids: drafts right wherever its 2-grams are
        # unique.  An untimed run counts the steps; the timed run replays exactly that many, with no host poll inside the interval
        def begin():
            gen.start(emb, mask, logits=False)
            _lib.check(lib.fvhd_llm_lookup_begin(gen.pre._h, _lib.ptr(rec), new, C.cast(eos, C.c_void_p), 0, new, _lib.ptr(out), _lib.stream_ptr(dev)), "begin")

        out = torch.zeros((new,), device=dev, dtype=torch.long)
        eos = (C.c_int32 * 1)()
        begin()
        graph = _graph_of(lambda: _lib.check(lib.fvhd_llm_lookup_step(gen.pre._h, T, 2, _lib.stream_ptr(dev)), "step"), dev)
        while True:
            graph.replay()
            written, finished, steps, _tok = gen.lookup_state()
            if finished or written >= new:
                break
        assert torch.equal(out, rec), "the lookup run's tokens differ from the greedy run's"
        runs = []
        for _ in range(max(1, repeats)):
            begin()
            runs.append(round(_ms_per(graph.replay, steps, dev), 4))
            assert gen.lookup_state()[:3] == (new, True, steps) and torch.equal(out, rec)
        r["lookup_steps"], r["accepted_per_step"] = steps, round((new - 1) / max(steps, 1) - 1, 3)
        r["lookup_step_ms_runs"], r["lookup_step_ms"] = runs, med(runs)
        r["tokens_per_s_at_measured_acceptance"] = round((new - 1) / (r["lookup_steps"] * r["lookup_step_ms"] * 1e-3), 1)
        r["tokens_per_s_at_full_acceptance"] = round(T / (r["verify_all_right_ms"] * 1e-3), 1)
        t_verify = max(r["verify_all_wrong_ms"], r["verify_all_right_ms"])
        r["break_even_acceptance_per_draft"] = round((t_verify / res["plain_ms"] - 1) / (T - 1), 4)
        r["verify_over_plain_at_B_rows_ms"] = round(t_verify - r["plain_at_B_rows_ms"], 4)
        res["rows"][str(T)] = r
    # the draft and accept launches replayed alone (the single ops on buffers of the run's sizes)
    seq = torch.cat([rec, rec]).to(torch.int32).contiguous()
    ln = torch.tensor([seq.numel()], device=dev, dtype=torch.int32)
    dr = torch.zeros(16, device=dev, dtype=torch.long)
    ids = torch.arange(16, device=dev, dtype=torch.long)
    last, pos = torch.zeros(1, device=dev, dtype=torch.long), torch.zeros(1, device=dev, dtype=torch.long)
    length = torch.zeros(1, device=dev, dtype=torch.int32)
    kvalid = torch.zeros(64, device=dev, dtype=torch.uint8)
    def alone():
        length.zero_()
        _lib.check(lib.fvhd_op_dec_lookup_draft(_lib.stream_ptr(dev), _lib.ptr(seq), _lib.ptr(ln), 2, 15, _lib.ptr(dr)), "draft")
        _lib.check(lib.fvhd_op_dec_lookup_accept(_lib.stream_ptr(dev), _lib.ptr(dr), _lib.ptr(ids), 16, None, None, 0, None, 0, None, _lib.ptr(last), _lib.ptr(pos),
                                                 _lib.ptr(length), _lib.ptr(kvalid), 64), "accept")

    graph = _graph_of(alone, dev)
    graph.replay()
    zero = _graph_of(lambda: length.zero_(), dev)
    res["draft_and_accept_alone_us"] = round(1000 * (_ms_per(graph.replay, 200, dev) - _ms_per(zero.replay, 200, dev)), 1)
    del gen
    return res


@torch.no_grad()
def measure_lookup_sample(llm, pre, K: int, prompt: int, new: int, dev, repeats: int = 3, lp_n: int = 5) -> dict:
    """the lookup step (draft + verify + accept, K drafts) by graph replay under greedy and under sampling (predict.py's settings), each
    without and with log-probabilities, next to the plain step the same ways; no lookup ids, so on random weights nearly every step emits
    one token (`accepted_per_step` says how many more) - the step's COST, not a speed-up"""
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    cfg = llm.config
    hidden, V, T = cfg.hidden_size, cfg.vocab_size, K + 1
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "vocab": V, "prompt": prompt, "new_tokens": new, "drafts": K,
           "sampling": SAMPLE_SETTINGS["predict_py"], "logprobs": lp_n}
    g0 = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(1, prompt, hidden, device=dev, generator=g0)).to(torch.bfloat16)
    mask = torch.ones(1, prompt, device=dev, dtype=torch.long)
    gen = Qwen2Generator.from_hf(llm, 1, prompt + new + T + 4, prefill=pre)
    lib = _lib.lookup_sample_lib()
    tok, top_i, top_v = torch.zeros((1,), device=dev), torch.zeros((1, lp_n), device=dev, dtype=torch.long), torch.zeros((1, lp_n), device=dev)
    out = torch.zeros((new,), device=dev, dtype=torch.long)
    o_tok, o_ids, o_top = torch.zeros((new,), device=dev), torch.zeros((new, lp_n), device=dev, dtype=torch.long), torch.zeros((new, lp_n), device=dev)
    eos = (C.c_int32 * 1)()

    def settings(sample, lp):
        gen.set_sampling(bool(sample), seed=1, **(SAMPLE_SETTINGS["predict_py"] if sample else {}))
        gen.set_verify_sampling(bool(sample))
        gen.set_logprobs(bool(lp))

    def plain_ms(sample, lp):
        settings(sample, lp)

        def step():
            gen.step(logits=False)
            if lp:
                gen.logprobs(lp_n, tok, top_i, top_v)

        gen.start(emb, mask, logits=False)
        graph = _graph_of(step, dev)
        graph.replay()
        gen.start(emb, mask, logits=False)
        ms = _ms_per(graph.replay, new, dev)
        assert gen.cache_state() == (prompt + new, 0)
        return ms, 0

    def lookup_ms(sample, lp):
        settings(sample, lp)
        gen.spec_reserve(T, 0)

        def begin():
            gen.start(emb, mask, logits=False)
            _lib.check(lib.fvhd_llm_lookup_begin(gen.pre._h, None, 0, C.cast(eos, C.c_void_p), 0, new, _lib.ptr(out), _lib.stream_ptr(dev)), "begin")
            if lp:
                _lib.check(lib.fvhd_llm_lookup_logprobs(gen.pre._h, lp_n, _lib.ptr(o_tok), _lib.ptr(o_ids), _lib.ptr(o_top), _lib.stream_ptr(dev)), "logprobs")

        begin()
        graph = _graph_of(lambda: _lib.check(lib.fvhd_llm_lookup_step(gen.pre._h, T, 2, _lib.stream_ptr(dev)), "step"), dev)
        while True:                                         # an untimed run counts the steps; the timed run replays exactly that many
            graph.replay()
            written, finished, steps, _tok = gen.lookup_state()
            if finished or written >= new:
                break
        begin()
        ms = _ms_per(graph.replay, steps, dev)
        assert gen.lookup_state()[:3] == (new, True, steps) and gen.cache_state()[1] == 0
        return ms, steps

    cases = {"plain_greedy": (plain_ms, False, False), "plain_sample": (plain_ms, True, False), "plain_greedy_logprobs": (plain_ms, False, True),
             "plain_sample_logprobs": (plain_ms, True, True), "lookup_greedy": (lookup_ms, False, False), "lookup_sample": (lookup_ms, True, False),
             "lookup_greedy_logprobs": (lookup_ms, False, True), "lookup_sample_logprobs": (lookup_ms, True, True)}
    runs, steps = {k: [] for k in cases}, {}
    for rep in range(max(1, repeats)):                      # every case once per round, the rounds in alternating order
        for k in (list(cases) if rep % 2 == 0 else list(cases)[::-1]):
            fn, sample, lp = cases[k]
            ms, st = fn(sample, lp)
            runs[k].append(round(ms, 4))
            steps[k] = st
    settings(False, False)
    med = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
    for k, v in runs.items():
        res[f"{k}_step_ms"], res[f"{k}_step_ms_runs"] = med(v), v
        if k.startswith("lookup"):
            res[f"{k}_steps"], res[f"{k}_accepted_per_step"] = steps[k], round((new - 1) / max(steps[k], 1) - 1, 3)
    res["rows_sampler_over_argmax_finish_us"] = round(1000 * (res["lookup_sample_step_ms"] - res["lookup_greedy_step_ms"]), 1)
    res["lookup_logprobs_added_us"] = {k: round(1000 * (res[f"lookup_{k}_logprobs_step_ms"] - res[f"lookup_{k}_step_ms"]), 1) for k in ("greedy", "sample")}
    # a lookup step that accepts a drafts emits 1 + a tokens: it breaks even with the plain step at a = t_lookup / t_plain - 1
    for k in ("greedy", "sample"):
        res[f"break_even_accepted_per_step_{k}"] = round(res[f"lookup_{k}_step_ms"] / res[f"plain_{k}_step_ms"] - 1, 3)
        res[f"break_even_accepted_per_step_{k}_logprobs"] = round(res[f"lookup_{k}_logprobs_step_ms"] / res[f"plain_{k}_logprobs_step_ms"] - 1, 3)
    del gen
    return res


@torch.no_grad()
def measure_guidance(llm, pre, G: int, prompt: int, new: int, dev, repeats: int = 3, scale: float = 1.5) -> dict:
    """--guidance: the step under classifier-free guidance for G prompts (2 G rows: the two guidance launches, the choice on G rows, the mirror
    launch) against the same build's plain step at B = 2 G (guidance off: launch for launch the step without the feature), graph replay, the
    two in alternating rounds, medians; and the stock transformers loop doing what generate(guidance_scale=...) does per token - one eager
    forward of the G conditional rows, a second one of the G unconditional rows on its own cache, and the processor's combination."""
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import kv_to_dynamic_cache
    cfg = llm.config
    hidden, B = cfg.hidden_size, 2 * G
    gen = Qwen2Generator.from_hf(llm, B, prompt + new + 4, prefill=pre)
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(B, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(B, prompt, device=dev, dtype=torch.long)
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "prompts": G, "rows": B, "prompt": prompt, "new_tokens": new, "guidance_scale": scale}
    graphs = {}
    for name, s in (("plain", 1.0), ("guided", scale)):
        gen.set_guidance(s)
        gen.start(emb, mask, logits=False)
        graphs[name] = _graph_of(lambda: gen.step(logits=False), dev)
    runs = {"plain": [], "guided": []}
    for r in range(max(1, repeats)):
        for name in (("plain", "guided") if r % 2 == 0 else ("guided", "plain")):
            gen.set_guidance(scale if name == "guided" else 1.0)
            gen.start(emb, mask, logits=False)
            runs[name].append(round(_ms_per(graphs[name].replay, new, dev), 4))
            assert gen.cache_state() == (prompt + new, 0)
    gen.set_guidance()
    for name in runs:
        res[f"{name}_2G_rows_graph_ms_per_token"] = sorted(runs[name])[len(runs[name]) // 2]
        res[f"{name}_2G_rows_graph_ms_per_token_runs"] = runs[name]
    res["guidance_adds_ms_per_token"] = round(res["guided_2G_rows_graph_ms_per_token"] - res["plain_2G_rows_graph_ms_per_token"], 4)
    # the stock loop: two eager forwards per token on two caches, then the processor's arithmetic
    state = []
    for half in (slice(0, G), slice(G, B)):
        logits, k, v = pre(emb[half], mask[half], None, return_kv=True)
        state.append({"cache": kv_to_dynamic_cache(k, v), "logits": logits})
    st = {"tok": state[0]["logits"].argmax(-1), "mask": mask[:G], "pos": torch.full((G, 1), prompt - 1, device=dev, dtype=torch.long)}

    def hf_step():
        st["mask"] = torch.cat([st["mask"], torch.ones(G, 1, device=dev, dtype=torch.long)], 1)
        st["pos"] = st["pos"] + 1
        lc, lu = (torch.nn.functional.log_softmax(
            llm(input_ids=st["tok"][:, None], attention_mask=st["mask"], position_ids=st["pos"], past_key_values=h["cache"], use_cache=True).logits[:, -1].float(),
            dim=-1) for h in state)
        st["tok"] = (scale * (lc - lu) + lu).argmax(-1)

    for _ in range(3):
        hf_step()
    res["stock_transformers_guidance_ms_per_token"] = round(_ms_per(hf_step, new, dev), 4)
    res["speedup_guided_graph_vs_stock"] = round(res["stock_transformers_guidance_ms_per_token"] / res["guided_2G_rows_graph_ms_per_token"], 2)
    return res


def _graph_of(fn, dev):
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    return graph


BEAM_PROCESSORS = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)      # --num-beams with --processors: the usual caption settings


@torch.no_grad()
def measure_beam(llm, pre, groups: int, K: int, prompt: int, new: int, dev, repeats: int = 1, stock: bool = True, weights: str = "bf16",
                 do_sample: bool = False, processors: bool = False, constraint: bool = False) -> dict:
    """do_sample: beam-search SAMPLING at predict.py's settings (temperature 0.2, top_k 50, top_p off): `beam_sample_topk` in place of
    `beam_topk` in the step, and the stock loop run with do_sample=True.  processors: the step under BEAM_PROCESSORS
    (`Qwen2Generator.set_beam_scoring` + `set_logits_processors`: the rows normalised, the processors' launch, the histories carried by the
    reorder, the top-K on the rows as they are), and the stock loop with the same settings.  constraint: the step under a one-state automaton that
    allows every other id (`set_beam_scoring` + `set_constraint`: the states carried by the reorder); the stock loop is then left out (its
    `prefix_allowed_tokens_fn` is a host callback per row per step)"""
    from ml_fastvlm_amd.beam import BeamSearchState
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    cfg = llm.config
    hidden, rows, V = cfg.hidden_size, groups * K, cfg.vocab_size
    gen = Qwen2Generator.from_hf(llm, rows, prompt + new + 4, prefill=pre, weights=weights)
    g = torch.Generator(device=dev).manual_seed(0)
    emb = (0.5 * torch.randn(groups, prompt, hidden, device=dev, generator=g)).to(torch.bfloat16)
    mask = torch.ones(groups, prompt, device=dev, dtype=torch.long)
    res = {"hidden": hidden, "layers": cfg.num_hidden_layers, "prompts": groups, "num_beams": K, "rows": rows, "vocab": V, "prompt": prompt,
           "new_tokens": new, "weights": weights, "do_sample": do_sample}
    gen.beam_reserve()
    gen._set_greedy()
    if processors:
        res["processors"] = BEAM_PROCESSORS
        gen.set_beam_scoring(True)
        gen.set_logits_processors(**BEAM_PROCESSORS)
    if constraint:
        from ml_fastvlm_amd.constraints import TokenAutomaton
        ids = list(range(0, V, 2))
        res["constraint_edges"] = len(ids)
        gen.set_beam_scoring(True)
        gen.set_constraint(TokenAutomaton([0, len(ids)], ids, [0] * len(ids), V))
        stock = False
    processors = processors or constraint                   # (from here on: "the step is the processed one")
    keep = 2 * K
    topk = gen.beam_topk
    if do_sample:
        res.update(temperature=0.2, top_k=50, top_p=1.0, min_keep=2)
        gen.beam_sample_reserve()

        def topk(*a):
            gen.beam_sample_topk(*a, temperature=0.2, top_k=50, top_p=1.0, min_keep=2, seed=1)
    cand_s = torch.zeros((groups, keep), device=dev)
    cand_i = torch.zeros((groups, keep), device=dev, dtype=torch.long)
    expand = torch.arange(rows, device=dev) // K
    box = {}

    def begin():                                            # Qwen2Generator.beam_search up to its first update; the state tensors keep their addresses
        st = box.get("state")
        fresh = BeamSearchState(groups, K, V, new, device=dev)
        if st is None:
            st = box["state"] = fresh
        else:
            for name, t in vars(fresh).items():
                if isinstance(t, torch.Tensor):
                    getattr(st, name).copy_(t)
        lg, _ = gen.start(emb, mask, logits=True)
        gen._logits[:rows].copy_(lg.repeat_interleave(K, dim=0))
        gen.cache_gather(expand, groups)
        topk(gen._logits[:rows], st.running_beam_scores, keep, cand_s, cand_i)
        st.update(cand_s, cand_i)
        return st

    st = begin()

    def one_step():
        gen.cache_gather(st.parent, rows)
        lg, _ = gen.step(st.fed_ids, logits=True)
        topk(lg, st.running_beam_scores, keep, cand_s, cand_i)
        st.update(cand_s, cand_i)

    full = _graph_of(one_step, dev)
    runs, moved = [], []
    for _ in range(max(1, repeats)):
        begin()
        runs.append(round(_ms_per(full.replay, new - 1, dev), 4))
        assert gen.cache_state() == (prompt + new - 1, 0) and st.finished()
    res["beam_step_ms"] = sorted(runs)[len(runs) // 2]
    res["beam_step_ms_runs"] = runs
    # the parts, each replayed on its own (the cache length is reset first: a step past the capacity would do nothing)
    begin()
    for _ in range(new // 2):
        full.replay()
    torch.cuda.synchronize(dev)
    parent = st.parent.clone()
    res["rows_moved_at_mid_search"] = int((parent != torch.arange(rows, device=dev)).sum())
    worst = torch.roll(torch.arange(rows, device=dev), 1)
    src = parent.clone()
    # under `processors` the step is not the plain one: with logits it holds the normalisation and the processors' launch, without them the
    # processors' launch alone - named for what they are, and no "added over the plain step" is derived (the plain run of the same build has it)
    step = "processed_step" if processors else "plain_step"
    parts = {f"{step}_with_logits": lambda: gen.step(st.fed_ids, logits=True), step: lambda: gen.step(st.fed_ids, logits=False),
             "topk": lambda: topk(gen._logits[:rows], st.running_beam_scores, keep, cand_s, cand_i),
             "bookkeeping": lambda: st.update(cand_s, cand_i), "gather": lambda: gen.cache_gather(src, rows)}
    for name, fn in parts.items():
        graph = _graph_of(fn, dev)
        for tag, m in ((("_mid_search_map", parent), ("_every_row_moves", worst), ("_identity", torch.arange(rows, device=dev))) if name == "gather" else (("", None),)):
            begin()
            if name == "gather":
                for _ in range(new // 2):                   # the cache at its mean length
                    full.replay()
                src.copy_(m)
            res[f"{name}{tag}_ms"] = round(_ms_per(graph.replay, new - 1 if name.startswith(step) else new // 2, dev), 4)
    if not processors:
        res["added_ms_over_plain_step"] = round(res["beam_step_ms"] - res["plain_step_ms"], 4)
    nkv, hd = cfg.num_key_value_heads, hidden // cfg.num_attention_heads
    res["logits_bytes"] = rows * V * 4
    res["kv_bytes_moved_twice_if_every_row_moves"] = int(2 * 2 * cfg.num_hidden_layers * rows * nkv * (prompt + new / 2) * hd * 2)
    if stock:
        ref_kw = dict(inputs_embeds=emb, attention_mask=mask, num_beams=K, max_new_tokens=new, do_sample=False, eos_token_id=None, pad_token_id=0)
        if do_sample:
            ref_kw.update(do_sample=True, temperature=0.2, top_k=50, top_p=1.0)
        if "processors" in res:
            ref_kw.update(BEAM_PROCESSORS)
        llm.generation_config.eos_token_id = None           # (random weights: no early end)
        llm.generate(**dict(ref_kw, max_new_tokens=4))      # lazy initialisation stays out of the timing
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        llm.generate(**dict(ref_kw, max_new_tokens=1))
        b.record()
        torch.cuda.synchronize(dev)
        first = a.elapsed_time(b)
        a.record()
        llm.generate(**ref_kw)
        b.record()
        torch.cuda.synchronize(dev)
        res["stock_transformers_beam_ms_per_step"] = round((a.elapsed_time(b) - first) / (new - 1), 4)
        res["speedup_beam_step_vs_stock"] = round(res["stock_transformers_beam_ms_per_step"] / res["beam_step_ms"], 2)
    if processors:
        gen.set_logits_processors()
        gen.set_constraint()
        gen.set_beam_scoring(False)
    del gen
    return res


def step_weight_bytes(cfg, weights: str) -> int:
    """bytes of the packed matrices one decode step streams (every layer's q|k|v, o, gate|up, down and lm_head)"""
    I, H, nh, nkv, V = cfg.intermediate_size, cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads, cfg.vocab_size
    hd = H // nh
    elems = cfg.num_hidden_layers * ((nh + 2 * nkv) * hd * H + H * nh * hd + 3 * I * H) + V * H
    if weights == "fp8_e4m3":                               # one byte per element + one fp32 scale per output row
        return elems + 4 * (cfg.num_hidden_layers * ((nh + 2 * nkv) * hd + 2 * H + 2 * I) + V)
    if weights == "mxfp4":                                  # half a byte per element + one scale byte per 32 elements
        return elems // 2 + elems // 32
    return elems * 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="+", default=[896, 1536, 3584])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--prompt", type=int, default=285)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--sample", action="store_true", help="the sampled step against the greedy one (default widths: 896 only)")
    ap.add_argument("--repeats", type=int, default=1, help="time the graph replay this many times")
    ap.add_argument("--no-stock", action="store_true", help="leave out the stock transformers loop and the eager library step")
    ap.add_argument("--weights", choices=["bf16", "fp8_e4m3", "mxfp4"], default="bf16",
                    help="storage of the packed LLM matrices (fp8_e4m3 needs a library of version 504, mxfp4 one built with the 4-bit entry points)")
    ap.add_argument("--trace-steps", type=int, default=0, help="run only the prefill and this many eager steps (for a kernel trace)")
    ap.add_argument("--processors", action="store_true", help="the step with all four logits processors on against off (needs a library of version 506)")
    ap.add_argument("--beam-sample", action="store_true", help="with --num-beams: beam-search sampling (do_sample=True, temperature 0.2, top_k 50) instead of the greedy search")
    ap.add_argument("--num-beams", type=int, default=0, help="time beam search with this many beams per prompt (--batch = prompts; needs a library of version 505)")
    ap.add_argument("--lookup", action="store_true", help="the verify step of prompt-lookup decoding at one sequence (needs a library of version 507)")
    ap.add_argument("--rows", type=int, nargs="+", default=[4, 8, 16], help="--lookup: rows per verify step")
    ap.add_argument("--logprobs", type=int, nargs="+", default=None, metavar="N",
                    help="the step with the chosen tokens' log-probabilities and top-N alternatives, for every N named, against off and against torch ops")
    ap.add_argument("--constraint", action="store_true",
                    help="the step with a token automaton on (a sparse and a dense state) against off and against torch doing the same from dense tables")
    ap.add_argument("--lookup-sample", type=int, default=0, metavar="K",
                    help="the lookup step with K drafts under greedy and under sampling, without and with --logprobs N (default 5), beside the plain step")
    ap.add_argument("--guidance", action="store_true",
                    help="the step under classifier-free guidance (--batch = prompts G, 2 G rows) against the plain step at B = 2 G and the stock loop's two forwards")
    ap.add_argument("--warpers", action="store_true",
                    help="the sampled step with min_p / typical_p / epsilon_cutoff / eta_cutoff, each and all, against the plain sampled step and torch")
    ap.add_argument("--out", default=None, help="--guidance / --warpers: also write the JSON result to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.warpers:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in (a.hidden if "--hidden" in sys.argv else [896, 3584]):
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm)
            for b in a.batch:
                rows.append(measure_warpers(llm, pre, b, a.prompt, a.new, dev, repeats=max(a.repeats, 3)))
                torch.cuda.empty_cache()
            del pre, llm
            torch.cuda.empty_cache()
        line = json.dumps({"tool": "decode_bench", "mode": "warpers", "device": torch.cuda.get_device_name(dev),
                           "library_version": _lib.sampling_lib().fvhd_version(), "has_warpers": _lib.has("sampling_warpers"), "results": rows})
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    if a.guidance:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in (a.hidden if "--hidden" in sys.argv else [896, 3584]):
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm)
            for b in a.batch:
                rows.append(measure_guidance(llm, pre, b, a.prompt, a.new, dev, repeats=max(a.repeats, 3)))
                torch.cuda.empty_cache()
            del pre, llm
            torch.cuda.empty_cache()
        line = json.dumps({"tool": "decode_bench", "mode": "guidance", "device": torch.cuda.get_device_name(dev),
                           "library_version": _lib.guidance_lib().fvhd_version(), "results": rows})
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    if a.lookup_sample:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in (a.hidden if "--hidden" in sys.argv else [896, 3584]):
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm)
            rows.append(measure_lookup_sample(llm, pre, a.lookup_sample, a.prompt, a.new, dev, repeats=a.repeats, lp_n=(a.logprobs or [5])[0]))
            del pre, llm
            torch.cuda.empty_cache()
        print(json.dumps({"tool": "decode_bench", "mode": "lookup_sample", "device": torch.cuda.get_device_name(dev),
                          "library_version": _lib.lookup_sample_lib().fvhd_version(), "results": rows}))
        return
    if a.constraint and not a.num_beams:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in (a.hidden if "--hidden" in sys.argv else [896, 3584]):
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm)
            for b in a.batch:
                rows.append(measure_constraint(llm, pre, b, a.prompt, a.new, dev))
                torch.cuda.empty_cache()
            del pre, llm
            torch.cuda.empty_cache()
        print(json.dumps({"tool": "decode_bench", "mode": "constraint", "device": torch.cuda.get_device_name(dev),
                          "library_version": _lib.constraint_lib().fvhd_version(), "results": rows}))
        return
    if a.logprobs is not None:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in (a.hidden if "--hidden" in sys.argv else [896, 3584]):
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm)
            for b in a.batch:
                rows.append(measure_logprobs(llm, pre, b, a.prompt, a.new, dev, a.logprobs))
                torch.cuda.empty_cache()
            del pre, llm
            torch.cuda.empty_cache()
        print(json.dumps({"tool": "decode_bench", "mode": "logprobs", "device": torch.cuda.get_device_name(dev),
                          "library_version": _lib.logprobs_lib().fvhd_version(), "results": rows}))
        return
    if a.lookup:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in (a.hidden if "--hidden" in sys.argv else [896, 3584]):
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm, weights=a.weights)
            rows.append(measure_lookup(llm, pre, a.rows, a.prompt, a.new, dev, repeats=a.repeats, weights=a.weights, trace_steps=a.trace_steps))
            del pre, llm
            torch.cuda.empty_cache()
        print(json.dumps({"tool": "decode_bench", "mode": "lookup", "device": torch.cuda.get_device_name(dev),
                          "library_version": _lib.lookup_lib().fvhd_version(), "results": rows}))
        return
    if a.num_beams:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in a.hidden:
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm, weights=a.weights)
            for b in a.batch:
                rows.append(measure_beam(llm, pre, b, a.num_beams, a.prompt, a.new, dev, repeats=a.repeats, stock=not a.no_stock, weights=a.weights, do_sample=a.beam_sample,
                                         processors=a.processors, constraint=a.constraint))
                torch.cuda.empty_cache()
            del pre, llm
            torch.cuda.empty_cache()
        print(json.dumps({"tool": "decode_bench", "mode": "beam", "device": torch.cuda.get_device_name(dev), "library_version": _lib.beam_lib().fvhd_version(),
                          "results": rows}))
        return
    if a.processors:
        from tools.ttft import build_llm
        from ml_fastvlm_amd import _lib
        from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
        rows = []
        for h in (a.hidden if "--hidden" in sys.argv else [896]):
            llm = build_llm(h, dev)
            pre = Qwen2Prefill.from_hf(llm)
            for b in a.batch:
                rows.append(measure_processors(llm, pre, b, a.prompt, a.new, dev))
                torch.cuda.empty_cache()
            del pre, llm
            torch.cuda.empty_cache()
        print(json.dumps({"tool": "decode_bench", "mode": "processors", "device": torch.cuda.get_device_name(dev),
                          "library_version": _lib.processors_lib().fvhd_version(), "results": rows}))
        return
    if a.sample:
        hidden = a.hidden if "--hidden" in sys.argv else [896]
        rows = [measure_sample(h, b, a.prompt, a.new, dev) for h in hidden for b in a.batch]
        print(json.dumps({"tool": "decode_bench", "mode": "sample", "device": torch.cuda.get_device_name(dev), "results": rows}))
        return
    from ml_fastvlm_amd import _lib
    rows = [r for h in a.hidden for r in measure_width(h, a.batch, a.prompt, a.new, dev, repeats=a.repeats, stock=not a.no_stock,
                                                       trace_steps=a.trace_steps, weights=a.weights)]
    print(json.dumps({"tool": "decode_bench", "device": torch.cuda.get_device_name(dev), "library_version": _lib.load().fvhd_version(),
                      "results": rows}))


if __name__ == "__main__":
    main()
