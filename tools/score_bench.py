"""What does scoring every position cost?  The fused op (`fvhd_op_lm_score`: lm_head, log-softmax and the pick of the target in one kernel,
no [rows, vocab] tensor) next to what a user of the library could do before it: `fvhd_op_gemm` into fp32 logits [rows, vocab], then
`torch.logsumexp` and `gather`.

    python tools/score_bench.py all --out profiles/r15_score_bench.json

Shapes: the benchmark's prefill rows (8 x 317) at the 0.5B head (V = 151 936, K = 896) and the 7B head (V = 152 064, K = 3584); xn and W are
seeded random bf16 (the time of a GEMM does not depend on the values), targets random ids.
`all` measures in the manner of tools/extend_bench.py: fresh processes, alternating (unfused, fused), three rounds, the median of the three
per-process medians with every per-process median listed (the spread).  Inside a process one call is timed with events around it, 20 calls
after 3 warm-up calls, the median.  Peak extra memory: `torch.cuda.max_memory_allocated` over the timed calls minus what was allocated
before them (the operands) - the logits and torch's temporaries on one side, the scratch and the two [rows] outputs on the other.  Each
process also checks its result against the other path's arithmetic at 64 rows (fp64 from the fp32 logits)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8 * 317, 151936, 896), (8 * 317, 152064, 3584)]        # (rows, V, K)
CALLS, WARMUP = 20, 3


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def one(shape: int, path: str) -> dict:
    import torch
    from ml_fastvlm_amd import _lib
    lib = _lib.score_lib()
    dev = torch.device("cuda:0")
    M, V, K = SHAPES[shape]
    g = torch.Generator(device=dev).manual_seed(V + K)
    x = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    W = (torch.randn(V, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
    tg = torch.randint(0, V, (M,), device=dev, generator=g)
    st = _lib.stream_ptr(dev)
    nbytes = lib.fvhd_lm_score_scratch_bytes(M, V, K)

    def fused(x=x, tg=tg):
        m = x.shape[0]
        scratch = torch.empty(lib.fvhd_lm_score_scratch_bytes(m, V, K) // 4, device=dev)
        lp, lse = torch.empty(m, device=dev), torch.empty(m, device=dev)
        _lib.check(lib.fvhd_op_lm_score(st, _lib.ptr(x), _lib.ptr(W), _lib.ptr(tg), m, V, K, _lib.ptr(lp), _lib.ptr(lse), _lib.ptr(scratch), scratch.numel() * 4),
                   "fvhd_op_lm_score")
        return lp, lse

    def unfused(x=x, tg=tg):
        m = x.shape[0]
        z = torch.empty(m, V, device=dev, dtype=torch.float32)
        _lib.check(lib.fvhd_op_gemm(st, _lib.ptr(x), _lib.ptr(W), None, None, None, _lib.ptr(z), m, V, K, _lib.EPI_NONE, _lib.F32), "fvhd_op_gemm")
        lse = torch.logsumexp(z, -1)
        return z.gather(1, tg[:, None])[:, 0] - lse, lse

    # the two paths compute the same thing (64 rows; fp64 from the unfused path's fp32 logits)
    a, b = fused(x[:64], tg[:64]), unfused(x[:64], tg[:64])
    torch.cuda.synchronize(dev)
    assert float((a[0].double() - b[0].double()).abs().max()) < 1e-2 and float((a[1].double() - b[1].double()).abs().max()) < 1e-2
    del a, b
    call = fused if path == "fused" else unfused
    for _ in range(WARMUP):
        call()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize(dev)
        times.append(e0.elapsed_time(e1))
        del out
    peak = torch.cuda.max_memory_allocated(dev) - base
    flops = 2.0 * M * V * K
    ms = _median(times)
    return {"path": path, "rows": M, "vocab": V, "hidden": K, "segments": lib.fvhd_lm_score_plan(M, V, K), "scratch_bytes": int(nbytes), "ms": round(ms, 4),
            "ms_min": round(min(times), 4), "ms_max": round(max(times), 4), "peak_extra_bytes": int(peak), "tflops": round(flops / ms / 1e9, 1)}


def _child(args) -> dict:
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, cwd=ROOT, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{args} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def everything(rounds: int = 3) -> dict:
    rows = []
    for i, (M, V, K) in enumerate(SHAPES):
        runs = {"unfused": [], "fused": []}
        for _ in range(rounds):                                   # alternating fresh processes
            for path in ("unfused", "fused"):
                runs[path].append(_child(["one", "--shape", str(i), "--path", path]))
                print(json.dumps(runs[path][-1]), file=sys.stderr, flush=True)
        row = {"rows": M, "vocab": V, "hidden": K, "segments": runs["fused"][0]["segments"]}
        for path in ("unfused", "fused"):
            ms = [r["ms"] for r in runs[path]]
            row[path] = {"ms": _median(ms), "ms_runs": ms, "ms_min_call": min(r["ms_min"] for r in runs[path]), "ms_max_call": max(r["ms_max"] for r in runs[path]),
                         "peak_extra_bytes": max(r["peak_extra_bytes"] for r in runs[path]), "tflops": _median([r["tflops"] for r in runs[path]])}
        row["fused_over_unfused"] = round(row["fused"]["ms"] / row["unfused"]["ms"], 3)
        rows.append(row)
    return {"what": "fvhd_op_lm_score (fused) against fvhd_op_gemm to fp32 [rows, vocab] + torch.logsumexp + gather (unfused); ms per call on one "
                    "MI355X, median of three fresh processes (each the median of 20 calls after 3 warm-up calls), processes alternating; "
                    "ms_runs: the per-process medians; peak_extra_bytes: torch's peak allocation over the timed calls beyond the operands",
            "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["one", "all"])
    ap.add_argument("--shape", type=int, default=0, choices=range(len(SHAPES)))
    ap.add_argument("--path", choices=["fused", "unfused"], default="fused")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = one(a.shape, a.path) if a.what == "one" else everything()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
