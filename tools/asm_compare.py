"""Compare the kernels of two `hipcc -S` device outputs (dev tool).

    hipcc <flags> -S --cuda-device-only x.hip -o a.s     # once per build to compare
    python tools/asm_compare.py [--pair REGEX=REPL]... [--labels] a.s b.s [substring of the kernel names to show]

Per kernel symbol: whether the instruction streams are identical (text after the comments are dropped,
so a renumbered register counts as a difference) and otherwise the per-opcode count differences (a DMA
into LDS counts apart from a plain load: ` lds` is kept on the opcode); then the register and scratch
figures of the metadata, A -> B.

--pair REGEX=REPL pairs a renamed kernel: a symbol of A that REGEX matches is compared with the symbol of B that
is, or alone begins with, the match replaced by REPL (a mangled name's argument list may number its
substitutions differently, so the prefix up to it is enough).  --labels drops the function's emission number from
the `.LBB<n>_<m>` branch labels, for two builds that emit the same kernels in another order or file.
"""
import collections
import re
import sys

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")


def parse(path, labels=False):
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
        if labels:
            ins = [re.sub(r"\.LBB\d+_", ".LBB_", x) for x in ins]
        out[md[".name"]] = ([x for x in ins if x and x[0] != "." and not x.endswith(":")], md)
    return out


def histogram(ins):
    return collections.Counter(x.split()[0] + (" lds" if x.endswith(" lds") else "") for x in ins)


def main():
    argv, pairs, labels = sys.argv[1:], [], False
    while argv and argv[0] in ("--labels", "--pair"):
        if argv.pop(0) == "--labels":
            labels = True
        else:
            pairs.append(argv.pop(0).split("=", 1))
    a, b = parse(argv[0], labels), parse(argv[1], labels)
    want = argv[2] if len(argv) > 2 else ""
    new = {}   # symbol of A -> the symbol of B it became
    for name in a:
        for rx, repl in pairs:
            if name not in b and re.search(rx, name):
                to = re.sub(rx, repl, name)
                hit = [x for x in b if x == to] or [x for x in b if x.startswith(to)]
                if len(hit) == 1:
                    new[name] = hit[0]
    for name in sorted((set(a) | set(b)) - set(new.values())):
        if want not in name:
            continue
        other = new.get(name, name)
        if name not in a or other not in b:
            print(f"{name}\n  only in {'A' if name in a else 'B'}")
            continue
        (ia, ma), (ib, mb) = a[name], b[other]
        print(name + (f"\n  -> {other}" if other != name else ""))
        print(f"  instructions {len(ia)} -> {len(ib)}: {'identical' if ia == ib else 'DIFFERENT'}")
        ha, hb = histogram(ia), histogram(ib)
        for op in sorted(set(ha) | set(hb)):
            if ha[op] != hb[op]:
                print(f"    {op}: {ha[op]} -> {hb[op]}")
        print("  " + "  ".join(f"{k} {ma.get(k)} -> {mb.get(k)}" for k in META))


if __name__ == "__main__":
    main()
