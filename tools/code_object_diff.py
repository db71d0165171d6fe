"""Kernels of two builds of one translation unit, side by side: for every instantiation of a kernel in the OLD object, its twin in the NEW
one -- matched by demangled name and template arguments, with the trailing `false` of a template parameter added since (RAGGED) dropped (a kernel
that was no template before is matched to its <false>) --
compared by the metadata notes (VGPRs, SGPRs, spills, LDS, scratch; llvm-readelf --notes) and by the disassembled instruction stream.
Also lists the NEW object's instantiations that are no twin of an OLD one -- a RAGGED form, a kernel added beside the old ones --, with their
notes.  Needs no GPU.

    python tools/code_object_diff.py OLD.o NEW.o 'k_stft_ft16<'
    (OLD.o: e.g. make -C zaf-python_amd/csrc OBJDIR=/tmp/old_build on the parent commit)
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
          "private_segment_fixed_size")


def code_object(obj, tmp):
    """The gfx950 code object inside a hipcc host object (.hip_fatbin section, clang offload bundle)."""
    base = os.path.join(tmp, re.sub(r"\W", "_", os.path.abspath(obj)))
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, base + ".fatbin"], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={base}.fatbin", f"--output={base}.co",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    return base + ".co"


def notes(co):
    """The FIELDS of every kernel's metadata entry.  An entry starts at `- .agpr_count:` and names its kernel in `.symbol: NAME.kd`; its
    arguments carry `.name` fields of their own, so the entry is not keyed by that."""
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    res, cur = {}, {}
    for line in txt.splitlines():
        if re.match(r"\s*- \.agpr_count:", line):
            cur = {}
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\d+)\s*$", line)
        if m and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
        m = re.match(r"\s+\.symbol:\s+(\S+)\.kd\s*$", line)
        if m:
            res[m.group(1)] = cur
    return res


def disasm(co):
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True,
                         check=True).stdout
    res, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^<(\S+)>:\s*$", line)
        if m:
            cur = m.group(1)
            res[cur] = []
        elif cur and line.strip() and line.strip() != "...":   # ("...": zero padding behind a kernel, by its place in the object)
            res[cur].append(re.sub(r"\s*//.*$", "", line.strip()))   # (the comment holds the address and the encoding)
    return res


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def key(dem):
    """name<template arguments> of a kernel of namespace zafx (or its anonymous namespace); a kernel that is no template (demangled without its return type): name<>."""
    m = re.match(r"(?:void )?(zafx::(?:\(anonymous namespace\)::)?\w+)(?:<(.*?)>)?\(", dem)
    if not m:
        return dem
    return f"{m.group(1)}<{', '.join(a.strip() for a in m.group(2).split(',')) if m.group(2) else ''}>"


def main(old_obj, new_obj, pattern):
    tmp = tempfile.mkdtemp()
    o, n = code_object(old_obj, tmp), code_object(new_obj, tmp)
    no, nn, do, dn = notes(o), notes(n), disasm(o), disasm(n)
    dm = demangle(sorted(set(no) | set(nn)))
    old = {key(dm[s]): s for s in no if pattern in dm[s]}
    new = {key(dm[s]): s for s in nn if pattern in dm[s]}
    same_notes = same_code = 0
    twins = set()
    for k, so in sorted(old.items()):
        sn = new.get(k[:-1] + ("false>" if k.endswith("<>") else ", false>")) or new.get(k)   # (k_mdct_ft16_f64 was no template before its RAGGED form)
        if sn is None:
            print(f"MISSING  {k}")
            continue
        twins.add(sn)
        nt, code = no[so] == nn[sn], do.get(so) == dn.get(sn)
        same_notes += nt
        same_code += code
        diff = "" if code else f"  ({sum(a != b for a, b in zip(do[so], dn[sn]))} of {len(do[so])} instructions differ)"
        print(f"{'notes same' if nt else 'NOTES DIFFER'}  {'code same' if code else 'code differs'}  {k}  {no[so]}"
              + ("" if nt else f" -> {nn[sn]}") + diff)
    print(f"{len(old)} instantiations: notes identical {same_notes}, instruction streams identical {same_code}")
    added = {k: s for k, s in new.items() if s not in twins}
    if added:
        print("new instantiations (no twin in the old object):")
        for k, s in sorted(added.items()):
            print(f"  {k}  {nn[s]}")


if __name__ == "__main__":
    main(*sys.argv[1:4])
