#!/usr/bin/env python3
"""Kernels of one unit in two builds, side by side, from the device assembly the compiler leaves with
`hipcc ... --offload-arch=gfx950 -x hip -c --cuda-device-only -save-temps=obj` (the Makefile's flags).

    python tools/kernel_counts.py PARENT.s NEW.s [--match SUBSTRING ...]

One row per kernel whose demangled name holds one of the substrings (default: all): instructions, code
bytes, VGPRs, SGPRs, scratch bytes and static LDS bytes in either build, and whether the instruction text is
the same once LDS symbol names (which carry the enclosing function's name) and the functions' label
numbers are blanked.  A markdown table on
standard output."""
import argparse
import re
import subprocess


def parse(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        ins = [re.sub(r";.*", "", ln).strip() for ln in m.group(2).split("\n")
               if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_ZZ\w+", "LDS", i)) for i in ins]
        size = re.search(r"; codeLenInByte = (\d+)", txt[m.end():m.end() + 2000])
        out[m.group(1)] = {"ins": ins, "bytes": int(size.group(1)) if size else None}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        d = out.setdefault(m.group(1), {"ins": [], "bytes": None})
        for key, name in (("vgpr", "next_free_vgpr"), ("sgpr", "next_free_sgpr"),
                          ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size")):
            v = re.search(r"\.amdhsa_%s (\S+)" % name, m.group(2))
            d[key] = v.group(1) if v else "-"
    return {k: v for k, v in out.items() if "vgpr" in v}


def cell(d):
    if d is None:
        return "- | - | - | - | - | -"
    return f"{len(d['ins'])} | {d['bytes']} | {d['vgpr']} | {d['sgpr']} | {d['scratch']} | {d['lds']}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--match", nargs="*", default=[])
    a = ap.parse_args()
    p, n = parse(a.parent), parse(a.new)
    names = sorted(set(p) | set(n))
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    print("| kernel | parent: instructions | bytes | VGPRs | SGPRs | scratch | LDS | new: instructions | bytes | VGPRs | SGPRs "
          "| scratch | LDS | same text |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for k, name in zip(names, dem):
        if a.match and not any(s in name for s in a.match):
            continue
        x, y = p.get(k), n.get(k)
        same = "-" if x is None or y is None else ("yes" if x["ins"] == y["ins"] else "no")
        print(f"| `{name}` | {cell(x)} | {cell(y)} | {same} |")


if __name__ == "__main__":
    main()
