#!/usr/bin/env python3
"""Are the kernels of two device-assembly builds the same?  Reads every *.s of two directories (one file per source,
hipcc <the Makefile's flags> --cuda-device-only -S), pairs the kernels by demangled name with namespace qualifiers
dropped (a type moved between namespaces renames the symbols, not the code), and compares each pair's instruction
text, with local labels and the mangled names inside bodies (LDS arrays, jump tables) normalised, and its register
and memory budget (.amdhsa_ lines below).  Prints SAME or DIFF per kernel; exits 1 on any DIFF or unpaired kernel.
A plain text comparison: which file a kernel sits in does not matter.
Usage: tools/isa_same.py DIR_A DIR_B"""
import glob
import os
import re
import subprocess
import sys

BUDGET = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size",
          "private_segment_fixed_size")
LOCAL = re.compile(r"\.(LBB|Ltmp|LJTI|LCPI|Lfunc_begin|Lfunc_end)[0-9_]+")
MANGLED = re.compile(r"_Z[A-Za-z0-9_.$]+")


def demangler(texts):
    """mangled name -> demangled name without namespace qualifiers, for every _Z token of the texts (one c++filt run)"""
    names = sorted({m for t in texts for m in MANGLED.findall(t)})
    filt = next((p for p in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt")
                 if os.path.exists(p)), "c++filt")
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    strip = lambda s: re.sub(r"(\(anonymous namespace\)|[A-Za-z_]\w*)::", "", s)
    return {n: strip(d) for n, d in zip(names, out.splitlines())}


def kernels(directory):
    """{plain name: (normalised body lines, budget dict)} over the directory's *.s files"""
    texts = [open(p).read() for p in sorted(glob.glob(os.path.join(directory, "*.s")))]
    if not texts:
        sys.exit(f"no *.s files in {directory}")
    plain = demangler(texts)
    found = {}
    for text in texts:
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
            sym, desc = m.group(1), m.group(2)
            start = re.search(r"^" + re.escape(sym) + r":.*\n", text, re.M).end()
            body = text[start:text.index(".Lfunc_end", start)]
            lines = []
            for line in body.splitlines():
                line = line.split(";")[0].strip()  # (comments carry source-dependent notes)
                if line:
                    line = MANGLED.sub(lambda t: plain.get(t.group(0), t.group(0)), line)
                    lines.append(LOCAL.sub(lambda t: "." + t.group(1), line))
            budget = {k: re.search(r"\.amdhsa_" + k + r"\s+(\S+)", desc) for k in BUDGET}
            name = plain.get(sym, sym)
            if name in found:
                sys.exit(f"{directory}: two kernels named {name}")
            found[name] = (lines, {k: v.group(1) if v else None for k, v in budget.items()})
    return found


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    names = sorted(set(a) | set(b))
    heads = [n.split("(")[0] for n in names]
    for name, head in zip(names, heads):
        shown = head if heads.count(head) == 1 else name  # the parameter list only where overloads need it
        if name not in a or name not in b:
            print(f"ONLY-{'A' if name in a else 'B'}  {shown}")
            bad += 1
            continue
        why = [k for k in BUDGET if a[name][1][k] != b[name][1][k]]
        if a[name][0] != b[name][0]:
            n = next((i for i, (x, y) in enumerate(zip(a[name][0], b[name][0])) if x != y),
                     min(len(a[name][0]), len(b[name][0])))
            why.append(f"instruction {n} of {len(a[name][0])} / {len(b[name][0])}")
        print(f"{'DIFF' if why else 'SAME'}  {shown}" + (f"  ({', '.join(why)})" if why else ""))
        bad += bool(why)
    print(f"{len(names)} kernels, {bad} differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
