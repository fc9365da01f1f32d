#!/usr/bin/env python3
"""Compare the gfx950 kernels of two libmsplit_hip.so builds: the check of a "compiles to the same instructions" claim.

    tools/kernel_isa_diff.py OLD.so NEW.so [--tsv FILE [--units a,b,...] [--only REGEX]]

Extracts the gfx950 code objects of both libraries (llvm-objdump --offloading), disassembles them and matches the
kernels by mangled name.  Reports names present on one side only, kernels whose instruction text differs (mnemonics
and operands, the address column and the encodings dropped; branches are relative, so placement does not show) and
kernels whose register, LDS or scratch figures in the code-object metadata differ.  A kernel that a library holds
more than once (in several code objects) must be the same everywhere.  Exits 1 on any difference.  Needs no GPU.

--tsv writes one line per kernel of NEW: name, unit, instruction count, SHA-256 of the instruction text (first 16
hex digits), VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes.  The unit is the index of the code object in link order,
or its name where --units names the code objects in that order; --only keeps the kernels whose name matches.
"""
import argparse
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")
PAD = ("s_nop 0", "s_code_end")  # alignment filler after a kernel's last instruction


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout


def code_objects(lib, tmp):
    """The library's gfx950 code objects, in link order."""
    shutil.copy(lib, os.path.join(tmp, "lib.so"))
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so", cwd=tmp)
    objs = glob.glob(os.path.join(tmp, "lib.so.*gfx950"))
    return sorted(objs, key=lambda p: int(p.split(".")[-2]))


def kernels_of(obj):
    """{name: (instruction lines, figures)} of one code object."""
    meta, entry = {}, None
    for line in run(os.path.join(LLVM, "llvm-readelf"), "--notes", obj).splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s+(.*)$", line)  # the kernel's own keys (its arguments' lie deeper)
        if not m:
            continue
        if m.group(1) == "- ":
            entry = {}
        if entry is not None:
            entry[m.group(2)] = m.group(3).strip("'\"")
            if m.group(2) == "name":
                meta[entry["name"]] = entry
    text, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", obj).splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = text.setdefault(m.group(1), []) if m.group(1) in meta else None
        elif cur is not None and line.strip() not in ("", "..."):
            cur.append(" ".join(line.split("//")[0].split()))
    out = {}
    for name, e in meta.items():
        ins = text.get(name, [])
        while ins and ins[-1] in PAD:
            ins.pop()
        if not ins:
            sys.exit("no instructions found for %s in %s" % (name, obj))
        out[name] = (ins, tuple(int(e.get(k, 0)) for k in FIGURES))
    return out


def load(lib):
    """{name: {(hash, count, figures, unit index)}} over every code object of the library."""
    ks = {}
    with tempfile.TemporaryDirectory() as tmp:
        objs = code_objects(lib, tmp)
        for i, obj in enumerate(objs):
            for name, (ins, fig) in kernels_of(obj).items():
                h = hashlib.sha256("\n".join(ins).encode()).hexdigest()[:16]
                ks.setdefault(name, set()).add((h, len(ins), fig, i))
    return ks, len(objs)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--tsv")
    ap.add_argument("--units", help="names of NEW's code objects, in link order, comma-separated")
    ap.add_argument("--only", default="", help="--tsv: only the kernels whose mangled name matches this regex")
    a = ap.parse_args()
    (old, _), (new, nobj) = load(a.old), load(a.new)
    bad = 0
    for name in sorted(set(old) - set(new)):
        print("only in OLD:", name)
        bad += 1
    for name in sorted(set(new) - set(old)):
        print("only in NEW:", name)
        bad += 1
    for name in sorted(set(old) & set(new)):
        o, n = {v[:3] for v in old[name]}, {v[:3] for v in new[name]}
        if len(o) > 1 or len(n) > 1:
            print("differs between code objects of one library:", name)
            bad += 1
        elif o != n:
            (oh, oc, of), (nh, nc, nf) = next(iter(o)), next(iter(n))
            what = ("instructions (%d -> %d) " % (oc, nc) if (oh, oc) != (nh, nc) else "") + (
                "figures %s: %s -> %s" % ("/".join(FIGURES), of, nf) if of != nf else "")
            print("differs:", name, what)
            bad += 1
    if a.tsv:
        units = a.units.split(",") if a.units else [str(i) for i in range(nobj)]
        if len(units) != nobj:
            sys.exit("--units names %d code objects, NEW holds %d" % (len(units), nobj))
        with open(a.tsv, "w") as f:
            f.write("name\tunit\tinstructions\tsha256_16\tvgpr\tagpr\tsgpr\tlds_bytes\tscratch_bytes\n")
            for name in sorted(n for n in new if re.search(a.only, n)):
                for h, c, fig, i in sorted(new[name], key=lambda v: v[3]):
                    f.write("\t".join([name, units[i], str(c), h] + [str(x) for x in fig]) + "\n")
    print("%d kernel names in OLD, %d in NEW, %d differences" % (len(old), len(new), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
