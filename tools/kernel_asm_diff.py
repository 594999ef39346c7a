#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly listings of the same translation unit, for refactors that must not
change the device code.

    build flags of csrc/build.sh + --cuda-device-only -S   ->  OLD.s, NEW.s
    tools/kernel_asm_diff.py OLD.s NEW.s [--rename REGEX REPL] [--table]

Compared per kernel (matched by demangled name): the text between the kernel's label and its .Lfunc_end, split into the
instruction text and the descriptor values (.amdhsa_kernel .. .end_amdhsa_kernel).  Made comparable first: the file-wide
function number in block labels (.LBB26_3 -> .LBB_3), the kernel's own symbol, the padding in front of comments and the
name of the compilation-unit id symbol.  Prints per kernel "identical", or "same instructions" when only assembler
comments differ (the order of the register allocator's `; implicit-def` notes: nothing of it reaches the code object), or
the two instruction counts and the resource values that differ; --table adds the resource table (registers, spills, scratch, LDS, occupancy) of both listings.
--rename rewrites the demangled names of OLD before matching (a kernel whose template parameters changed):
    --rename 'k_gemm<(\\w+, \\w+, \\w+), 2, ' 'k_gemm<\\1, '
Pure text comparison; exit status 1 when a kernel differs or exists on one side only."""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

RES_KEYS = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return [s.replace("(anonymous namespace)::", "") for s in out.splitlines()]


def normalise(line, sym):
    line = line.replace(sym, "<self>")
    line = re.sub(r"\bBB\d+_(\d+)", r"BB_\1", line)
    line = re.sub(r"__hip_cuid_\w+", "__hip_cuid_", line)
    return re.sub(r"\s+", " ", line).strip()


def kernels_of(path):
    """{mangled name: (instruction lines, descriptor lines, resources)} of every .amdhsa_kernel of the listing"""
    lines = open(path).read().splitlines()
    syms = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    spills = {}
    name = None
    for l in lines:        # (.amdgpu_metadata: one record per kernel)
        if m := re.match(r"\s+\.name:\s+(\S+)", l):
            name = m.group(1)
        elif (m := re.match(r"\s+\.(vgpr|sgpr)_spill_count:\s+(\d+)", l)) and name:
            spills.setdefault(name, {})[m.group(1)] = int(m.group(2))
    out = {}
    for sym in syms:
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        text, desc, in_desc = [], [], False
        for l in lines[start + 1:end]:
            s = normalise(l, sym)
            if s.startswith(".amdhsa_kernel"):
                in_desc = True
            elif s.startswith(".end_amdhsa_kernel"):
                in_desc = False
            elif in_desc:
                desc.append(s)
            elif s and not s.startswith((".section", ".p2align")):
                text.append(s)
        res = {}
        for l in lines[end:]:
            if m := re.match(r"; (\w+): (\d+)", l):
                res.setdefault(m.group(1), int(m.group(2)))
            if l.startswith("; Occupancy"):
                break
        res = {k: res.get(k, 0) for k in RES_KEYS}
        res["VgprSpill"] = spills.get(sym, {}).get("vgpr", 0)
        res["SgprSpill"] = spills.get(sym, {}).get("sgpr", 0)
        out[sym] = (text, desc, res)
    return out


def without_comments(text):
    return [t for t in (l.split(";")[0].strip() for l in text) if t]


def count_instructions(text):
    return sum(1 for l in text if not l.startswith((";", ".")) and not l.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--diff", type=int, default=0, metavar="N", help="first N lines of the text diff of a differing kernel")
    a = ap.parse_args()
    sides = []
    for path, renames in ((a.old, a.rename), (a.new, [])):
        k = kernels_of(path)
        names = demangle(list(k)) if k else []
        for rx, repl in renames:
            names = [re.sub(rx, repl, n) for n in names]
        sides.append(dict(zip(names, k.values())))
    old, new = sides
    bad = notes = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(f"{name}: only in {'OLD' if name in old else 'NEW'}")
            bad += 1
            continue
        (to, do, ro), (tn, dn, rn) = old[name], new[name]
        if to == tn and do == dn:
            print(f"{name}: identical")
        elif without_comments(to) == without_comments(tn) and do == dn:
            notes += 1
            print(f"{name}: same instructions (assembler comments differ)")
        else:
            bad += 1
            diff = ", ".join(f"{k} {ro[k]} -> {rn[k]}" for k in ro if ro[k] != rn[k]) or "same resources"
            what = ("text" if to != tn else "") + (" descriptor" if do != dn else "")
            print(f"{name}: DIFFERS ({what.strip()}): instructions {count_instructions(to)} -> {count_instructions(tn)}; {diff}")
            if a.diff:
                for l in list(difflib.unified_diff(to + do, tn + dn, "old", "new", n=2, lineterm=""))[:a.diff]:
                    print("    " + l)
        if a.table:
            for tag, r in (("old", ro), ("new", rn)):
                print(f"    {tag}: " + "  ".join(f"{k}={v}" for k, v in r.items()))
    print(f"{len(set(old) | set(new))} kernels, {notes} with other comments only, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
