#!/usr/bin/env python3
"""Register table and per-kernel disassembly digest of a gfx950 code object.

  co_kernel_table.py libtsg_pool.co table.tsv          one line per kernel: name, VGPRs, SGPRs,
                                                       spills, scratch and LDS bytes, code digest
  co_kernel_table.py --diff parent.tsv branch.tsv      names, register fields and digests compared

The digest is the SHA-1 of the kernel's instruction text (llvm-objdump -d, addresses, encodings
and local labels stripped): equal digests = the same instruction stream.
"""
import hashlib
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"
FIELDS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def notes(co):
    text = subprocess.run([LLVM + "llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in text.splitlines():
        if line.startswith("  - ."):  # a kernel's map starts (its keys follow at this depth)
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"    \.(\w+):\s*(\S+)$", line)
        if cur is None or not m:
            continue
        if m.group(1) == "name":
            kernels[m.group(2)] = cur
        elif m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    return kernels


def digests(co):
    text = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                          text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <([^>]+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = [hashlib.sha1(), 0]
        elif name and line.strip():
            out[name][0].update(re.sub(r"\s*//.*$", "", line).strip().encode() + b"\n")  # (address comment off)
            out[name][1] += 1
    return {k: (h.hexdigest()[:12], n) for k, (h, n) in out.items()}


def table(co, path):
    k, d = notes(co), digests(co)
    with open(path, "w") as f:
        f.write("\t".join(("name",) + FIELDS + ("instructions", "digest")) + "\n")
        for name in sorted(k):
            dg, n = d.get(name, ("?", 0))
            f.write("\t".join([name] + [str(k[name].get(x, "?")) for x in FIELDS] + [str(n), dg]) + "\n")
    print("%d kernels -> %s" % (len(k), path))


def read(path):
    rows = [l.rstrip("\n").split("\t") for l in open(path)][1:]
    return {r[0]: r[1:] for r in rows}


def diff(a, b):
    A, B = read(a), read(b)
    print("names: %d / %d, identical lists: %s" % (len(A), len(B), sorted(A) == sorted(B)))
    same = 0
    for name in sorted(set(A) & set(B)):
        ra, rb = A[name], B[name]
        if ra == rb:
            same += 1
            continue
        what = [("%s %s->%s" % (f, x, y)) for f, x, y in zip(FIELDS + ("instructions", "digest"), ra, rb) if x != y]
        print("%s: %s" % (name, ", ".join(what)))
    print("identical (registers and instruction stream): %d of %d" % (same, len(set(A) & set(B))))


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        diff(sys.argv[2], sys.argv[3])
    else:
        table(sys.argv[1], sys.argv[2])
