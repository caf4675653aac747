"""Compare the kernels of two AMDGPU assembly files (hipcc <the build's flags> -S --cuda-device-only) of the same source file, built from
two commits: per kernel the instruction count, registers, scratch, LDS and occupancy of either side, whether the instruction streams are
identical (labels and register numbers ignored, comments stripped; "N commuted": N instructions differ in the order of their source
operands only; otherwise the index of the first instruction that differs, and whether it lies behind the first MFMA) and whether the K loop - the innermost loop that holds an MFMA, from
its first non-temporal (weight) load to the backward branch - has the same opcode multiset.

    python tools/isa_diff.py parent/llm_decode.s this/llm_decode.s [name filter]  >> profiles/<name>_isa.md
"""
import collections
import re
import sys

EPI = {"4": "RESID", "5": "SWIGLU", "6": "QKV", "7": "ARGMAX"}


def short(name):
    m = re.match(r"_Z\d+(\w+?)I((?:L[ib]\d+E)+)E", name)
    if not m:
        m = re.match(r"_Z\d+([a-z_0-9]+kernel)", name)
        return m.group(1) if m else name
    args = re.findall(r"L[ib](\d+)E", m.group(2))
    if "dec_gemm" in m.group(1):
        args[0] = EPI.get(args[0], args[0])
    return f"{m.group(1)}<{', '.join(args)}>"


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and name is None and not line.startswith(".L"):
            name, body, meta = m.group(1), [], {}
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = [body, meta]
            continue
        m = re.match(r"^; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", line)
        if m and name in out:
            out[name][1][m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":          # the last figure of a kernel's block
                name = None
            continue
        if name in out:
            continue
        code = line.split(";")[0].rstrip()
        if re.match(r"^\.LBB\d+_\d+:", code):
            body.append(code.strip())
        elif code.startswith("\t") and not code.strip().startswith("."):
            body.append(code.strip())
    return {k: v for k, v in out.items() if "Occupancy" in v[1]}


def norm(ins):
    ins = re.sub(r"\.LBB\d+_\d+", "L", ins)
    ins = re.sub(r"\b([vsa])\[\d+:\d+\]", r"\1[#]", ins)
    return re.sub(r"\b([vsa])\d+\b", r"\1#", ins)


def commuted(x, y):
    """the same instruction but for the order of its source operands (s_and_b64 a, b / b, a; the factors of v_mad_i64_i32)"""
    return x.split()[0] == y.split()[0] and sorted(x.replace(",", " ").split()) == sorted(y.replace(",", " ").split())


def k_loop(body):
    """opcode multiset of the innermost MFMA loop, from its first non-temporal load (else its head) to the backward branch"""
    at = {ins[:-1]: i for i, ins in enumerate(body) if ins.endswith(":")}
    best = None
    for i, ins in enumerate(body):
        m = re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)", ins) or re.match(r"s_branch (\.LBB\d+_\d+)", ins)
        if m and at.get(m.group(1), i) < i:
            seg = body[at[m.group(1)]:i + 1]
            if any(s.startswith("v_mfma") for s in seg) and (best is None or len(seg) < len(best)):
                best = seg
    if best is None:
        return None
    nt = [j for j, s in enumerate(best) if s.startswith("global_load") and " nt" in s]
    seg = best[nt[0]:] if nt else best
    return collections.Counter(s.split()[0] for s in seg if not s.endswith(":"))


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pat = sys.argv[3] if len(sys.argv) > 3 else ""
    print("| kernel | instructions | VGPR | AGPR | SGPR | scratch | LDS | occupancy | stream | K loop |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name in a:
        if pat not in name or name not in b:
            continue
        (ba, ma), (bb, mb) = a[name], b[name]
        ia, ib = [norm(s) for s in ba if not s.endswith(":")], [norm(s) for s in bb if not s.endswith(":")]
        cell = lambda k: f"{ma[k]}" if ma[k] == mb[k] else f"{ma[k]} -> {mb[k]}"
        if ia == ib:
            same = "identical"
        elif len(ia) == len(ib) and all(x == y or commuted(x, y) for x, y in zip(ia, ib)):
            same = f"identical but {sum(x != y for x, y in zip(ia, ib))} commuted"
        else:
            first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y and not commuted(x, y)), min(len(ia), len(ib)))
            mf = next((i for i, s in enumerate(ia) if s.startswith("v_mfma")), 0)
            same = f"differs from {first}" + (" (behind the K loop)" if first > mf else "")
        la, lb = k_loop(ba), k_loop(bb)
        loop = "-" if la is None and lb is None else "same opcodes" if la == lb else "DIFFERS"
        n = f"{len(ia)}" if len(ia) == len(ib) else f"{len(ia)} -> {len(ib)}"
        print(f"| `{short(name)}` | {n} | {cell('NumVgprs')} | {cell('NumAgprs')} | {cell('TotalNumSgprs')} | {cell('ScratchSize')} | "
              f"{cell('LDSByteSize')} | {cell('Occupancy')} | {same} | {loop} |")


if __name__ == "__main__":
    main()
