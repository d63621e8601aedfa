#!/usr/bin/env python3
"""The loader's throughput on the bench's config-2 block set: ten 1 M-entry snappy blocks from
tsg_synth_search_block (seed i, profile 0, 1 MiB pages), opened together by one thread each, as
bench.py opens them; GB/s of flatbuffer = sum of the blocks' fb_bytes / wall time of the opens
(bench.py's load_gb_per_s). profiles/load_device has the runs.

    python tools/bench_load.py --write DIR [--blocks 10] [--entries 1000000]
        writes the blocks to DIR (no device needed)
    python tools/bench_load.py --read DIR LABEL [PACKAGE_ROOT] [--prof]
        one run in a process of its own: opens DIR's blocks with the tempo_amd package under
        PACKAGE_ROOT (default: this checkout; a build of an earlier commit reads the same blocks)
        and prints one JSON line. --prof sets TSG_PROF=1 (the open's phase times at exit, on stderr).
At most 16 host threads decode (TSG_HOST_THREADS is left alone when set).
"""
import argparse
import json
import os
import sys
import threading
import time

ap = argparse.ArgumentParser()
ap.add_argument("--write", metavar="DIR")
ap.add_argument("--read", nargs="+", metavar=("DIR", "LABEL"))
ap.add_argument("--blocks", type=int, default=10)
ap.add_argument("--entries", type=int, default=1_000_000)
ap.add_argument("--prof", action="store_true")
ARGS = ap.parse_args()
if bool(ARGS.write) == bool(ARGS.read):
    ap.error("one of --write DIR, --read DIR LABEL [PACKAGE_ROOT]")
if ARGS.read and not 2 <= len(ARGS.read) <= 3:
    ap.error("--read takes DIR LABEL [PACKAGE_ROOT]")
if ARGS.prof:
    os.environ["TSG_PROF"] = "1"
sys.path.insert(0, os.path.abspath(ARGS.read[2]) if ARGS.read and len(ARGS.read) > 2 else
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tempo_amd as T  # noqa: E402


def block_paths(d):
    return [os.path.join(d, "blk%02d" % i) for i in range(ARGS.blocks)]


def parallel(f, items, threads):
    out, errs, todo, lock = [None] * len(items), [], list(enumerate(items)), threading.Lock()

    def work():
        while True:
            with lock:
                if not todo:
                    return
                i, x = todo.pop(0)
            try:
                out[i] = f(x)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

    ths = [threading.Thread(target=work) for _ in range(threads)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    if errs:
        raise errs[0]
    return out


if ARGS.write:
    os.makedirs(ARGS.write, exist_ok=True)
    todo = [(i, p) for i, p in enumerate(block_paths(ARGS.write)) if not os.path.exists(os.path.join(p, "search"))]
    parallel(lambda ip: T.synth_search_block(ip[1], ARGS.entries, seed=ip[0], profile=0, encoding=T.ENC_SNAPPY,
                                             page_size=1024 * 1024), todo, min(8, max(1, len(todo))))
    print("wrote %d blocks of %d entries to %s" % (ARGS.blocks, ARGS.entries, ARGS.write))
    sys.exit(0)

paths = block_paths(ARGS.read[0])
eng = T.Engine(devices=[0])
t0 = time.time()
blocks = parallel(eng.open_block, paths, len(paths))
load_s = time.time() - t0
fb = sum(b.info()["fb_bytes"] for b in blocks)
for b in blocks:
    b.close()
eng.close()
print(json.dumps({"label": ARGS.read[1], "blocks": len(paths), "flatbuffer_gb": round(fb / 1e9, 4),
                  "load_s": round(load_s, 4), "load_gb_per_s": round(fb / load_s / 1e9, 4)}))
