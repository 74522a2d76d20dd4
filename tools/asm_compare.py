"""Compare the kernels of two `hipcc -S` device outputs (dev tool).

    hipcc <flags> -S --cuda-device-only x.hip -o a.s     # once per build to compare
    python tools/asm_compare.py a.s b.s [substring of the kernel names to show]

Per kernel symbol: whether the instruction streams are identical (text after the comments are dropped,
so a renumbered register counts as a difference) and otherwise the per-opcode count differences (a DMA
into LDS counts apart from a plain load: ` lds` is kept on the opcode); then the register and scratch
figures of the metadata, A -> B.
"""
import collections
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")


def parse(path):
    """{kernel symbol: ([instruction lines], {metadata key: value})}"""
    lines = open(path).read().split("\n")
    metas = [{}]
    for ln in lines:
        if ln.startswith("  - "):
            metas.append({})
        f = re.match(r"(?:  - |    )(\.\w+):\s*(\S+)\s*$", ln)
        if f:
            metas[-1][f.group(1)] = f.group(2)
    out = {}
    for md in (x for x in metas if ".name" in x and ".vgpr_count" in x):
        body = lines[next(i for i, ln in enumerate(lines) if ln.startswith(md[".name"] + ":")) + 1:]
        body = body[:next(i for i, ln in enumerate(body) if ln.startswith(".Lfunc_end"))]
        ins = [re.sub(r"\s+", " ", ln.split(";")[0].strip()) for ln in body]
        out[md[".name"]] = ([x for x in ins if x and x[0] != "." and not x.endswith(":")], md)
    return out


def histogram(ins):
    return collections.Counter(x.split()[0] + (" lds" if x.endswith(" lds") else "") for x in ins)


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    want = sys.argv[3] if len(sys.argv) > 3 else ""
    for name in sorted(set(a) | set(b)):
        if want not in name:
            continue
        if name not in a or name not in b:
            print(f"{name}\n  only in {'A' if name in a else 'B'}")
            continue
        (ia, ma), (ib, mb) = a[name], b[name]
        print(f"{name}\n  instructions {len(ia)} -> {len(ib)}: {'identical' if ia == ib else 'DIFFERENT'}")
        ha, hb = histogram(ia), histogram(ib)
        for op in sorted(set(ha) | set(hb)):
            if ha[op] != hb[op]:
                print(f"    {op}: {ha[op]} -> {hb[op]}")
        print("  " + "  ".join(f"{k} {ma.get(k)} -> {mb.get(k)}" for k in META))


if __name__ == "__main__":
    main()
