#!/usr/bin/env python3
"""Does another build of the library enqueue the same launches?  The ordered (kernel, grid, block) list of the decode step's features,
from a rocprofv3 kernel trace (no counters in the same run), to be diffed between two builds.

    rocprofv3 --kernel-trace -d this -o this -- python tools/decode_launches.py run
    FVHD_LIB=/path/to/other/libfvhd.so rocprofv3 --kernel-trace -d other -o other -- python tools/decode_launches.py run
    python tools/decode_launches.py list this/.../this_results.db > this.txt       (likewise other.txt; then diff other.txt this.txt)

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
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        for name, *dims in launches(sys.argv[2]):
            print(f"{name}  grid {dims[0]} x {dims[1]} x {dims[2]}  block {dims[3]} x {dims[4]} x {dims[5]}")
    else:
        sys.exit(__doc__)
