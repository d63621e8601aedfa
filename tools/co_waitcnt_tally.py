#!/usr/bin/env python3
"""Vector-memory wait counts of the kernels of a gfx950 code object (a sibling of
co_inst_classes.py, whose disassembly reader and unit-loop rule it uses).

  co_waitcnt_tally.py libtsg_pool.co [name-regex] [out.tsv]
  co_waitcnt_tally.py --loop libtsg_pool.co name-regex      the unit loop's loads and waits, in order

Per kernel whose mangled name matches the regex (default: the <3,true,true,true> narrow-scan
instances), for the whole kernel and for its unit loop: the global loads, and how many
`s_waitcnt vmcnt(N)` there are for each N. A wait with N below the loads of one unit (8 for
<3,true,true,true>) cannot leave the other stream's unit outstanding.
Lines: kernel, scope, instructions, global loads, then `N:count` per wait value.
"""
import re
import sys

from co_inst_classes import DEFAULT, kernels, unit_loop


def vmcnt(mn, ops):
    if mn != "s_waitcnt":
        return None
    m = re.search(r"vmcnt\((\d+)\)", ops)
    return int(m.group(1)) if m else None


def tally(body):
    loads = sum(1 for i in body if i[1].startswith("global_load"))
    hist = {}
    for _, mn, ops, _ in body:
        n = vmcnt(mn, ops)
        if n is not None:
            hist[n] = hist.get(n, 0) + 1
    return loads, hist


def main():
    args = sys.argv[1:]
    loop = bool(args) and args[0] == "--loop"
    if loop:
        args = args[1:]
    co = args[0]
    rx = re.compile(args[1] if len(args) > 1 else DEFAULT)
    lines = []
    for name, insts in sorted(kernels(co).items()):
        if not rx.search(name):
            continue
        body = unit_loop(insts)
        if loop:
            lines.append("%s: unit loop %x .. %x, %d instructions" % (name, body[0][0], body[-1][0], len(body)))
            for k, (addr, mn, ops, target) in enumerate(body):
                if mn.startswith(("global_load", "s_cbranch", "s_branch")) or vmcnt(mn, ops) is not None:
                    to = " -> %x" % target if target is not None else ""
                    lines.append("  %6x +%-5d %s %s%s" % (addr, k, mn, ops.strip(), to))
            continue
        for scope, b in (("kernel", insts), ("unit_loop", body)):
            loads, hist = tally(b)
            lines.append("\t".join([name, scope, str(len(b)), str(loads)] + ["%d:%d" % kv for kv in sorted(hist.items())]))
    text = "\n".join(lines) + "\n"
    if not loop and len(args) > 2:
        open(args[2], "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()
