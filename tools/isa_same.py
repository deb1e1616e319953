#!/usr/bin/env python3
"""isa_same.py A.s B.s [--map OLD=NEW ...] [--gone NAME ...] - are the kernels of two device assembly files the same code?

A.s and B.s are what hipcc writes with the flags of __graft_entry__.build_device and `--cuda-device-only -S` in place of
`-shared -o lib` (after gen_nif_asm()). The files are split by kernel, and per kernel three things are compared for equality
and nothing else: the instruction text between the kernel's label and its .Lfunc_end, its .amdhsa_kernel block, and its entry
in the metadata (registers, LDS, scratch, spills, workgroup size). The kernel's own symbol and the function number in local
labels (.LBB<n>_, .LJTI<n>_, .Lfunc_end<n>) are normalised away, so a kernel may be renamed and move within the file.

Kernels are matched by demangled name. --map OLD=NEW renames a kernel of A before matching (substrings of the demangled name,
e.g. --map 'kernel<false, 256>=kernel<mi::Small>'); --gone NAME expects a kernel of A (substring) to be absent from B.
One line per kernel: `same` / `DIFF (what)` / `gone` / `only in A` / `only in B`, with the registers, LDS and scratch the
assembler reports. Exit status 1 when anything differs or a kernel is in one file only without being expected to."""
import argparse
import re
import shutil
import subprocess
import sys

META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
             "max_flat_workgroup_size", "wavefront_size", "kernarg_segment_size")


def demangle(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not symbols:
        return {s: s for s in symbols}
    out = subprocess.run([tool], input="\n".join(symbols) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    # (the parameter list says nothing a kernel's template arguments do not: keep `ns::kernel<args>`)
    return {s: re.sub(r"^void ", "", re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d)) for s, d in zip(symbols, out)}


def normalise(lines, symbol):
    text = "\n".join(l.rstrip() for l in lines)
    text = text.replace(symbol, "@SELF").replace(symbol[2:], "@SELF")       # (static LDS variables embed the kernel's encoding: _ZZ<encoding>E<name>)
    return re.sub(r"\b(LBB|BB|LJTI|Lfunc_end|Lfunc_begin)\d+", r"\1N", text)       # (BB<n>_: the same number in the assembler's loop comments)


def kernels_of(path):
    """{demangled name: {"body", "amdhsa", "meta"}} of every kernel (a symbol with an .amdhsa_kernel block) of an assembly file."""
    lines = open(path, errors="replace").read().splitlines()
    label = {}                     # symbol -> line index of its label
    for i, l in enumerate(lines):
        m = re.match(r"^([A-Za-z_$.][\w$.]*):", l)
        if m and not m.group(1).startswith(".L"):
            label.setdefault(m.group(1), i)
    found = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = next(k for k in range(i, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
            found[m.group(1)] = {"amdhsa": normalise(lines[i + 1:j], m.group(1))}
            i = j
        i += 1
    for sym, rec in found.items():
        a = label[sym]
        b = next(k for k in range(a, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[k]))
        rec["body"] = normalise(lines[a + 1:b], sym)
    # metadata: the entries of amdhsa.kernels
    entry = None
    inside = False
    for l in lines:
        if l.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and re.match(r"^amdhsa\.|^\.\.\.|^\s*\.end_amdgpu_metadata", l):
            inside = False
        elif inside:
            if l.startswith("  - "):
                entry = {}
                l = "    " + l[4:]
            m = re.match(r"^    \.(\w+):\s+(\S+)\s*$", l)
            if m and entry is not None:
                if m.group(1) == "name" and m.group(2) in found:
                    found[m.group(2)]["meta"] = entry
                elif m.group(1) in META_KEYS:
                    entry[m.group(1)] = m.group(2)
    names = demangle(list(found))
    return {names[s]: rec for s, rec in found.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--gone", action="append", default=[], metavar="NAME")
    args = ap.parse_args()
    A, B = kernels_of(args.a), kernels_of(args.b)
    renamed = {}
    for name, rec in A.items():
        new = name
        for m in args.map:
            old, _, to = m.partition("=")
            if old in new:
                new = new.replace(old, to)
                break
        renamed[new] = (name, rec)
    bad = 0
    for name in sorted(set(renamed) | set(B)):
        was = renamed[name][0] if name in renamed else None
        title = name if was in (None, name) else f"{name}  (was {was})"
        if name not in B:
            expected = any(g in was for g in args.gone)
            bad += 0 if expected else 1
            print(f"{'gone' if expected else 'only in A':9s} {title}")
            continue
        b = B[name]
        meta = b.get("meta", {})
        res = (f"vgpr {meta.get('vgpr_count', '?')} agpr {meta.get('agpr_count', '0')} sgpr {meta.get('sgpr_count', '?')} lds {meta.get('group_segment_fixed_size', '?')} "
               f"scratch {meta.get('private_segment_fixed_size', '?')} spills v{meta.get('vgpr_spill_count', '?')}/s{meta.get('sgpr_spill_count', '?')} wg {meta.get('max_flat_workgroup_size', '?')}")
        if name not in renamed:
            bad += 1
            print(f"{'only in B':9s} {title}  [{res}]")
            continue
        a = renamed[name][1]
        diff = [what for what in ("body", "amdhsa", "meta") if a.get(what) != b.get(what)]
        bad += 1 if diff else 0
        print(f"{'DIFF (' + ', '.join(diff) + ')' if diff else 'same':9s} {title}  [{res}]")
    print(f"{len(B)} kernels in B, {len(A)} in A: " + ("all that are in both are the same code" if not bad else f"{bad} differ or are unexpected"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
