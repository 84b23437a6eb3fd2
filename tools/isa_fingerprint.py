#!/usr/bin/env python3
"""Fingerprint the kernels of a gfx950 assembly listing, or compare two listings kernel by kernel.

A refactor of a .hip file must leave its machine code alone.  Compile the file before and after with the Makefile's flags for it plus
--save-temps (for sp_cost.hip: hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=on -fno-slp-vectorize --save-temps
-c sp_cost.hip), keep the two *-gfx950.s files and run

    tools/isa_fingerprint.py OLD.s NEW.s [--only k_cost_pairs] [--rename 'REGEX=REPL'] [--diff] [--contains STR]

Per kernel: sha256 of the instruction text between its label and its .Lfunc_end (comments stripped, the function number of .LBB<n>_<m>
labels dropped, so that adding or removing OTHER kernels does not show), the number of instructions, and the resources of its
.amdhsa_kernel block (VGPRs, SGPRs, LDS, scratch, accum offset).  Kernels are paired by demangled name; --rename rewrites the names of
the FIRST listing (python re.sub, repeatable) where a change renamed a kernel.  --diff prints the unified diff of every pair whose text
differs.  --contains STR (repeatable) lists the kernels of the LAST listing whose name contains STR.  Exit status 1 if a pair differs, a
kernel of the new listing has no partner, or a --contains string matches nothing.
"""
import argparse
import difflib
import hashlib
import re
import shutil
import subprocess
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size", "accum_offset")


def demangle(names):
    exe = shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if exe is None or not names:
        return list(names)
    return subprocess.run([exe], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")[:len(names)]


def kernels_of(path):
    """{demangled name: {"text": [normalised lines], "n_inst": int, "res": {resource: value}}} of the kernels in an assembly listing."""
    lines = open(path).read().split("\n")
    res = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        r = {}
        for l2 in lines[i + 1:]:
            if ".end_amdhsa_kernel" in l2:
                break
            m2 = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", l2)
            if m2 and m2.group(1) in RESOURCES:
                r[m2.group(1)] = m2.group(2)
        res[m.group(1)] = r
    out = {}
    mangled = list(res)
    for name, shown in zip(mangled, demangle(mangled)):
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        text = []
        for ln in lines[start + 1:]:
            if re.match(r"\.Lfunc_end\d+:|\s*\.section\s", ln):          # (the kernel descriptor's section follows the last instruction)
                break
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0]).strip()
            if ln:
                text.append(" ".join(ln.split()))
        n_inst = sum(1 for t in text if not t.endswith(":") and not t.startswith("."))
        out[shown] = {"text": text, "n_inst": n_inst, "res": res[name]}
    return out


def row(k):
    r = k["res"]
    return (f"{hashlib.sha256(chr(10).join(k['text']).encode()).hexdigest()[:16]}  {k['n_inst']:6d} inst  " +
            "  ".join(f"{n.replace('_fixed_size', '').replace('next_free_', '')} {r.get(n, '-')}" for n in RESOURCES))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing", nargs="+", help="one .s file (fingerprints) or two (comparison, old then new)")
    ap.add_argument("--only", default="", help="kernels whose demangled name contains this")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL", help="rewrite kernel names of the first listing")
    ap.add_argument("--diff", action="store_true", help="print the diff of every pair whose instruction text differs")
    ap.add_argument("--contains", action="append", default=[], metavar="STR", help="list the last listing's kernels whose name contains STR")
    a = ap.parse_args()
    if len(a.listing) > 2:
        ap.error("one or two listings")
    sets = [{n: k for n, k in kernels_of(p).items() if a.only in n} for p in a.listing]
    bad = 0
    if len(sets) == 1:
        for n, k in sorted(sets[0].items()):
            print(f"{row(k)}  {n}")
    else:
        old = {}
        for n, k in sets[0].items():
            for r in a.rename:
                pat, repl = r.split("=", 1)
                n = re.sub(pat, repl, n)
            old[n] = k
        new = sets[1]
        print(f"old: {a.listing[0]} ({len(old)} kernels)   new: {a.listing[1]} ({len(new)} kernels)")
        for n in sorted(set(old) | set(new)):
            print(n)
            for tag, s in (("old", old), ("new", new)):
                print(f"  {tag}  {row(s[n]) if n in s else '(no such kernel)'}")
            if n not in new:
                verdict = "removed"
            elif n not in old:
                verdict = "ADDED (nothing to compare with)"
            elif old[n]["text"] == new[n]["text"] and old[n]["res"] == new[n]["res"]:
                verdict = "identical"
            elif old[n]["res"] == new[n]["res"] and old[n]["n_inst"] == new[n]["n_inst"]:
                verdict = "TEXT DIFFERS (same resources, same instruction count)"
            else:
                verdict = "DIFFERS"
            print(f"  ->   {verdict}")
            bad += verdict not in ("identical", "removed")
            if a.diff and n in old and n in new and old[n]["text"] != new[n]["text"]:
                print("\n".join("       " + d for d in difflib.unified_diff(old[n]["text"], new[n]["text"], "old", "new", lineterm="", n=0)))
    last = sets[-1]
    for s in a.contains:
        hits = sorted(n for n in last if s in n)
        print(f"contains {s!r}: {len(hits)}")
        for n in hits:
            print(f"    {n}")
        bad += not hits
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
