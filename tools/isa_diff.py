#!/usr/bin/env python
"""Compare two AMDGPU assembly listings kernel by kernel:  tools/isa_diff.py OLD.s NEW.s [-v]

Per kernel: VGPR / SGPR / LDS / scratch and the instruction count of both, then "identical" (same text once
labels and comments are stripped), "registers only" (same once register numbers are blanked too), or the opcodes that
differ, each marked `loop` when it lies between a label and a backward branch to it. -v prints the differing lines."""
import collections
import difflib
import re
import sys

META = {"vgpr": r"\.amdhsa_next_free_vgpr (\d+)", "sgpr": r"\.amdhsa_next_free_sgpr (\d+)",
        "lds": r"\.amdhsa_group_segment_fixed_size (\d+)", "scratch": r"\.amdhsa_private_segment_fixed_size (\d+)"}

def kernels(path):
    out, cur = {}, None
    text = open(path).read()
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), {"ins": [], "lab": {}})
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r"^(\.L\w+):", line)
        if m:
            cur["lab"][m.group(1)] = len(cur["ins"])
            continue
        line = line.split(";")[0].strip()
        if line and not line.startswith("."):
            cur["ins"].append(line)
    for name, k in out.items():  # resource block: from the kernel descriptor to the end of its comment block
        m = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel(.*?)(?=\n\t\.(?:text|section))" % name, text, re.S)
        blob = m.group(1) + m.group(2) if m else ""
        for key, rx in META.items():
            mm = re.search(rx, blob)
            k[key] = next((g for g in mm.groups() if g), "?") if mm else "?"
        k["loop"] = set()
        for j, ins in enumerate(k["ins"]):
            mm = re.match(r"s_c?branch\w*\s+(\.L\w+)", ins)
            if mm and k["lab"].get(mm.group(1), j + 1) <= j:
                k["loop"].update(range(k["lab"][mm.group(1)], j + 1))
    return out


def blank(ins):
    ins = re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", ins)
    return re.sub(r"\.L\w+", ".L#", ins)


def main():
    verbose = "-v" in sys.argv
    old, new = (kernels(p) for p in [a for a in sys.argv[1:] if a != "-v"][:2])
    for name in old:
        a, b = old[name], new.get(name)
        if b is None:
            print(name, "MISSING in new")
            continue
        res = " ".join("%s %s/%s" % (k, a[k], b[k]) for k in META)
        head = "%s\n  %s ins %d/%d: " % (name, res, len(a["ins"]), len(b["ins"]))
        if [blank(x) if ".L" in x else x for x in a["ins"]] == [blank(x) if ".L" in x else x for x in b["ins"]]:
            print(head + "identical")
            continue
        ba, bb = [blank(x) for x in a["ins"]], [blank(x) for x in b["ins"]]
        if ba == bb:
            print(head + "registers only")
            continue
        ops, n_loop = [], 0
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, ba, bb, autojunk=False).get_opcodes():
            if tag == "equal":
                continue
            in_loop = any(i in a["loop"] for i in range(i1, i2)) or any(j in b["loop"] for j in range(j1, j2))
            n_loop += in_loop
            ops.append("%s-[%s] +[%s]" % ("loop " if in_loop else "", " ".join(x.split()[0] for x in ba[i1:i2]),
                                        " ".join(x.split()[0] for x in bb[j1:j2])))
            if verbose:
                ops += ["      - " + x for x in a["ins"][i1:i2]] + ["      + " + x for x in b["ins"][j1:j2]]
        net = collections.Counter(x.split()[0] for x in bb)
        net.subtract(collections.Counter(x.split()[0] for x in ba))
        net = " ".join("%s%+d" % kv for kv in sorted(net.items()) if kv[1]) or "none (reordered only)"
        print(head + "%d hunks differ, %d inside a loop; net opcode counts: %s" % (sum(not o.startswith("      ") for o in ops), n_loop, net))
        for o in ops:
            print("    " + o)


if __name__ == "__main__":
    main()
