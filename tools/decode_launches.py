#!/usr/bin/env python3
"""Does another build of the library enqueue the same launches?  The ordered (kernel, grid, block) list of the decode step's features,
from a rocprofv3 kernel trace (no counters in the same run), to be diffed between two builds.

    rocprofv3 --kernel-trace -d this -o this -- python tools/decode_launches.py run
    FVHD_LIB=/path/to/other/libfvhd.so rocprofv3 --kernel-trace -d other -o other -- python tools/decode_launches.py run
    python tools/decode_launches.py list this/.../this_results.db > this.txt       (likewise other.txt; then diff other.txt this.txt)

`run beam` instead of `run`: two plain eager beam searches at the 0.5B stand-in (2 prompts x 2 beams, 3 new tokens), greedy and sampled - the
start, the expanding reorder, and two whole steps (reorder, decode step with logits, top continuations) of each.

`run`: the feature set of `tools/decode_bits.py dump x.pt features` at the 0.5B stand-in with 2 new tokens per generation - a start (or
an extend) and ONE eager step of every combination, and the verify steps of two prompt-lookup generations."""
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def launches(path):
    cur = sqlite3.connect(path).cursor()
    return cur.execute("select name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, workgroup_z from kernels order by dispatch_id").fetchall()


if __name__ == "__main__":
    if sys.argv[1:] == ["run"]:
        import decode_bits
        decode_bits.dump_features(None, new=2, names=("0.5B",))
    elif sys.argv[1:] == ["run", "beam"]:
        import torch
        import decode_bits
        from ml_fastvlm_amd.qwen2_decode import Qwen2Generator
        m = decode_bits._model("0.5B")
        g = torch.Generator().manual_seed(1)
        e = (0.5 * torch.randn(2, decode_bits.T, m.config.hidden_size, generator=g)).to("cuda", torch.bfloat16)
        mask = torch.ones(2, decode_bits.T, dtype=torch.long, device="cuda")
        gen = Qwen2Generator.from_hf(m, 4, decode_bits.T + 8)
        for kw in ({}, dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=3)):
            gen.beam_search(e, mask, None, num_beams=2, max_new_tokens=3, pad_token_id=0, graph=False, **kw)
        torch.cuda.synchronize()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        for name, *dims in launches(sys.argv[2]):
            print(f"{name}  grid {dims[0]} x {dims[1]} x {dims[2]}  block {dims[3]} x {dims[4]} x {dims[5]}")
    else:
        sys.exit(__doc__)
