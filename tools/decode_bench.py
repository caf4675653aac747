"""Decode-step time of the Qwen2 LLM on one MI355X: the library's steps (`ml_fastvlm_amd.qwen2_decode.Qwen2Generator`) replayed as one
captured graph and called eagerly, against the stock `transformers` decode loop continuing from the same prefill cache.

    python tools/decode_bench.py [--hidden 896 1536 3584] [--batch 1 8 16 32 64] [--prompt 285] [--new 128] [--repeats 3] [--no-stock]
    python tools/decode_bench.py --sample [--hidden 896] [--batch 1 8]
    python tools/decode_bench.py --trace-steps 16 --hidden 3584 --batch 64      (eager steps only: the program of a kernel trace)
    python tools/decode_bench.py --weights fp8_e4m3 ...                         (the packed matrices as e4m3 codes + row scales)

--batch takes up to 64 sequences per step (more than 16 need a library of version 503).  --repeats times the graph replay that many
times (`graph_ms_per_token` is their median, `graph_ms_per_token_runs` all of them); --no-stock leaves the stock transformers loop (and
the eager library step) out - above 16 sequences it only measures transformers.  A width's model is built and packed once for all batches.

--sample times the sampled step (`Qwen2Generator.set_sampling`, csrc/llm_sample.hip) next to the greedy one, both by graph replay at
vocab 151936, with predict.py's settings (temperature 0.2, top_k 50: transformers' default) and a flat one (temperature 1.0, top_k 0,
top_p 0.95); greedy is timed before and after the sampled settings and averaged.

Full layer counts, random bf16 weights (`tools/ttft.py: build_llm`).  Prints ONE JSON line: per (width, batch) the ms per token of each
path, the bytes a step must read (packed weights + the KV cache at the mean length) and their fraction of 8 TB/s."""
from __future__ import annotations

import argparse
import json
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
    I, H, nh, nkv, hd, V = cfg.intermediate_size, hidden, cfg.num_attention_heads, cfg.num_key_value_heads, hidden // cfg.num_attention_heads, cfg.vocab_size
    wbytes = cfg.num_hidden_layers * ((nh + 2 * nkv) * hd * H + H * nh * hd + 3 * I * H) * 2 + V * H * 2
    if weights == "fp8_e4m3":                               # one byte per element + one fp32 scale per output row
        wbytes = wbytes // 2 + 4 * (cfg.num_hidden_layers * ((nh + 2 * nkv) * hd + 2 * H + 2 * I) + V)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, nargs="+", default=[896, 1536, 3584])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--prompt", type=int, default=285)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--sample", action="store_true", help="the sampled step against the greedy one (default widths: 896 only)")
    ap.add_argument("--repeats", type=int, default=1, help="time the graph replay this many times")
    ap.add_argument("--no-stock", action="store_true", help="leave out the stock transformers loop and the eager library step")
    ap.add_argument("--weights", choices=["bf16", "fp8_e4m3"], default="bf16", help="storage of the packed LLM matrices (fp8_e4m3 needs a library of version 504)")
    ap.add_argument("--trace-steps", type=int, default=0, help="run only the prefill and this many eager steps (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
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
