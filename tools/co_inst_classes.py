#!/usr/bin/env python3
"""Static instruction counts by class of the kernels of a gfx950 code object (a sibling of
co_kernel_table.py: classes only, no instruction is singled out).

  co_inst_classes.py libtsg_pool.co [name-regex] [out.tsv]

Per kernel whose mangled name matches the regex (default: the <3,true,true,true> narrow-scan
instances): the whole kernel and its unit loop, each as VALU / SALU / LDS / VMEM / SMEM / other.
The unit loop is found from the code alone: of the loops (backward branches: target .. branch)
the shortest that holds at least half as many non-temporal stream loads as the loop holding the
most. For the three narrow-scan kernels that is the loop that evaluates and reloads a wave's
units (both units in flight: one trip is two units, 16 entries per lane); the resident kernel's
query loop, which also holds the first two units' loads, is longer and so not chosen.
Lines: kernel, scope, instructions, VALU, SALU, LDS, VMEM, SMEM, other.
"""
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"
CLASSES = ("VALU", "SALU", "LDS", "VMEM", "SMEM", "other")
DEFAULT = r"search_(static|pool|resident)_kernelILi3ELb1ELb1ELb1E"


def classify(mn):
    if mn.startswith("v_"):
        return "VALU"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if mn.startswith(("s_load", "s_buffer_load", "s_memrealtime", "s_memtime")):
        return "SMEM"
    if mn.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_branch", "s_cbranch", "s_endpgm", "s_sleep", "s_setprio",
                      "s_code_end", "s_sendmsg", "s_trap")):
        return "other"
    if mn.startswith("s_"):
        return "SALU"
    return "other"


def kernels(co):
    """-> {name: [(address, mnemonic, text, branch target or None)]}"""
    text = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                          text=True).stdout
    out, name, base = {}, None, 0
    for line in text.splitlines():
        m = re.match(r"([0-9a-f]+) <([^>]+)>:$", line)
        if m:
            base, name = int(m.group(1), 16), m.group(2)
            out[name] = []
            continue
        m = re.match(r"\s+(\S+)(.*?)//\s*([0-9A-Fa-f]+):(.*)$", line)
        if not name or not m:
            continue
        mn, ops, addr, tail = m.group(1), m.group(2), int(m.group(3), 16), m.group(4)
        target = None
        if mn.startswith(("s_cbranch", "s_branch")):
            t = re.search(r"<[^>+]+(?:\+0x([0-9a-f]+))?>", tail)
            if t:
                target = base + int(t.group(1) or "0", 16)
        out[name].append((addr, mn, ops, target))
    return out


def count(insts):
    c = dict.fromkeys(CLASSES, 0)
    for _, mn, _, _ in insts:
        c[classify(mn)] += 1
    return c


def unit_loop(insts):
    loops = []
    for addr, _, _, target in insts:
        if target is None or target > addr:
            continue
        body = [i for i in insts if target <= i[0] <= addr]
        nt = sum(1 for i in body if i[1].startswith("global_load") and re.search(r"\bnt\b", i[2]))
        loops.append((nt, body))
    most = max((nt for nt, _ in loops), default=0)
    if not most:
        return []
    return min((body for nt, body in loops if 2 * nt >= most), key=len)


def main():
    co = sys.argv[1]
    rx = re.compile(sys.argv[2] if len(sys.argv) > 2 else DEFAULT)
    lines = ["\t".join(("kernel", "scope", "instructions") + CLASSES)]
    for name, insts in sorted(kernels(co).items()):
        if not rx.search(name):
            continue
        for scope, body in (("kernel", insts), ("unit_loop", unit_loop(insts))):
            c = count(body)
            lines.append("\t".join([name, scope, str(len(body))] + [str(c[k]) for k in CLASSES]))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
