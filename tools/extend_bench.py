"""What does a later turn cost?  `Qwen2Generator.extend` of a chunk of T tokens onto a cache of P tokens, next to the only way a library
before version 509 reaches the same state: `start` on all P + T tokens.

    python tools/extend_bench.py all --parent-lib /path/to/the/parent/libfvhd.so --out profiles/r14_extend_bench.json

`all` measures in the manner of tools/decode_bench.py's A/B runs: fresh processes, alternating (parent library: start(P + T); this
library: extend(T | P)), three rounds, the median of the three per-process medians; every process builds the full-depth model of one
width (tools/ttft.py build_llm: random weights, the real shapes), times every (batch, P, T) of that width and prints one JSON line.
Inside a process one call is timed with events around it (extend: a start(P) before every timed call, outside the timing), 20 calls,
the median.  The attention kernel alone (`fvhd_op_attention_extend`) is timed per launch at (P, T) = (2000, 16): few queries on a long past,
the shape whose keys a split across workgroups would spread (not implemented: DESIGN 4.3 "Extend")."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(285, 32), (285, 285)]             # (P, T): a short follow-up question, a turn as long as the first prompt
BATCHES = [1, 8]
WIDTHS = [896, 3584]
CALLS = 20


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def one(hidden: int, mode: str) -> dict:
    import torch
    from tools.ttft import build_llm
    from ml_fastvlm_amd import _lib
    from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
    from ml_fastvlm_amd.qwen2_prefill import Qwen2Prefill
    dev = torch.device("cuda:0")
    with torch.no_grad():
        llm = build_llm(hidden, dev)
        pre = Qwen2Prefill.from_hf(llm)
        res = {"hidden": hidden, "layers": llm.config.num_hidden_layers, "mode": mode, "library_version": _lib.load().fvhd_version(), "ms": {}}
        for B in BATCHES:
            gen = Qwen2Generator.from_hf(llm, B, max(p + t for p, t in SHAPES) + 4, prefill=pre)
            for P, T in SHAPES:
                g = torch.Generator(device=dev).manual_seed(P + T + B)
                emb = (0.5 * torch.randn(B, P + T, hidden, device=dev, generator=g)).to(torch.bfloat16)
                past, chunk = emb[:, :P].contiguous(), emb[:, P:].contiguous()
                times = []
                for i in range(CALLS + 3):
                    if mode == "extend":
                        gen.start(past, logits=False)
                    torch.cuda.synchronize(dev)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    if mode == "extend":
                        gen.extend(chunk, logits=False)
                    else:
                        gen.start(emb, logits=False)
                    b.record()
                    torch.cuda.synchronize(dev)
                    if i >= 3:                                  # the first calls grow the workspace and load the kernels
                        times.append(a.elapsed_time(b))
                assert gen.cache_state() == (P + T, 0)
                res["ms"][f"B{B}_P{P}_T{T}"] = round(_median(times), 4)
    return res


def attention(P: int, T: int) -> dict:
    """per-launch time of the attention over the cache alone, at the 0.5B and 7B head shapes, one row"""
    import torch
    from ml_fastvlm_amd import _lib
    lib = _lib.extend_lib()
    dev = torch.device("cuda:0")
    out = {}
    for name, (hd, nh, nkv) in {"0.5B": (64, 14, 2), "7B": (128, 28, 4)}.items():
        g = torch.Generator(device=dev).manual_seed(hd)
        cap = P + T
        rows = torch.randn(T, (nh + 2 * nkv) * hd, device=dev, generator=g).to(torch.bfloat16)
        kc = torch.randn(1, nkv, cap, hd, device=dev, generator=g).to(torch.bfloat16)
        vc = torch.randn(1, nkv, cap, hd, device=dev, generator=g).to(torch.bfloat16)
        mask = torch.ones(1, cap, device=dev, dtype=torch.uint8)
        res = torch.empty(T, nh * hd, device=dev, dtype=torch.bfloat16)
        past = torch.tensor([P], device=dev, dtype=torch.int32)
        st = _lib.stream_ptr(dev)

        def launch():
            _lib.check(lib.fvhd_op_attention_extend(st, _lib.ptr(rows), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(mask), _lib.ptr(res), 1, T, nh, nkv, hd, cap,
                                                    _lib.ptr(past)), "fvhd_op_attention_extend")
        for _ in range(10):
            launch()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 200
        a.record()
        for _ in range(n):
            launch()
        b.record()
        torch.cuda.synchronize(dev)
        out[name] = {"head_dim": hd, "n_heads": nh, "n_kv_heads": nkv, "us_per_launch": round(a.elapsed_time(b) / n * 1e3, 2)}
    return {"past": P, "chunk": T, "batch": 1, "back_to_back_launches": 200, "shapes": out}


def _child(args, lib=None) -> dict:
    env = dict(os.environ)
    if lib:
        env["FVHD_LIB"] = lib
    else:
        env.pop("FVHD_LIB", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{args} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def everything(parent_lib: str, rounds: int = 3) -> dict:
    runs = {h: {"start_parent": [], "extend": []} for h in WIDTHS}
    for _ in range(rounds):                                     # alternating fresh processes
        for h in WIDTHS:
            runs[h]["start_parent"].append(_child(["one", "--hidden", str(h), "--mode", "start"], parent_lib))
            runs[h]["extend"].append(_child(["one", "--hidden", str(h), "--mode", "extend"]))
    rows = []
    for h in WIDTHS:
        for key in runs[h]["extend"][0]["ms"]:
            s = [r["ms"][key] for r in runs[h]["start_parent"]]
            e = [r["ms"][key] for r in runs[h]["extend"]]
            B, P, T = (int(x[1:]) for x in key.split("_"))
            rows.append({"hidden": h, "layers": runs[h]["extend"][0]["layers"], "batch": B, "past": P, "chunk": T,
                         "parent_start_ms": _median(s), "parent_start_ms_runs": s, "extend_ms": _median(e), "extend_ms_runs": e,
                         "parent_library_version": runs[h]["start_parent"][0]["library_version"],
                         "library_version": runs[h]["extend"][0]["library_version"]})
    return {"what": "extend(T | P) on this library against start(P + T) on the parent commit's library; ms per call, median of three fresh "
                    "processes (each the median of 20 calls), processes alternating",
            "rows": rows, "attention_past": _child(["attention", "--past", "2000", "--chunk", "16"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["one", "attention", "all"])
    ap.add_argument("--hidden", type=int, default=896)
    ap.add_argument("--mode", choices=["extend", "start"], default="extend")
    ap.add_argument("--past", type=int, default=2000)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "one":
        res = one(a.hidden, a.mode)
    elif a.what == "attention":
        res = attention(a.past, a.chunk)
    else:
        if not a.parent_lib or not os.path.exists(a.parent_lib):
            raise SystemExit("all: --parent-lib must name the parent commit's libfvhd.so (build it from a checkout of the parent)")
        res = everything(os.path.abspath(a.parent_lib))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
