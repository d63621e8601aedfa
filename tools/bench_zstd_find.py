#!/usr/bin/env python3
"""Device time of one tsg_find_ids batch over a zstd v2 block (the workload of
tools/bench_lz4_find.py: 100 000 objects of 250-900 bytes, pages cut every 100 000 object bytes,
2000 present ids over about 515 pages), written by the block writer's own compressor
(profiles/zstd_find/README.md). Every run's tsg_find_result.kernel_ns is printed.

    python tools/bench_zstd_find.py [out.json]
        in one process: the wave decoder (the default) and the one-lane decoder (tsg_debug_set
        "zstd_find_lane") in alternating legs, then the medians
    python tools/bench_zstd_find.py --write DIR
        writes the block and the batch's ids to DIR (no device needed)
    python tools/bench_zstd_find.py --read DIR LABEL [PACKAGE_ROOT]
        one leg in a process of its own: opens DIR's block with the tempo_amd package under
        PACKAGE_ROOT (default: this checkout; a build of an earlier commit reads the same block),
        one call discarded, then RUNS calls
"""
import json
import os
import random
import statistics
import sys
import tempfile

_READ = len(sys.argv) > 2 and sys.argv[1] == "--read"
sys.path.insert(0, os.path.abspath(sys.argv[4]) if _READ and len(sys.argv) > 4 else
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import tempo_amd as T  # noqa: E402

WORDS = [b"span", b"trace", b"service", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select"]
N, BATCH, RUNS, LEGS = 100_000, 2000, 7, 4


def read_leg(d, label):
    pick = np.load(os.path.join(d, "pick.npy"))
    eng = T.Engine(devices=[0])
    blk = eng.open_v2block(os.path.join(d, "zstd"))
    eng.find([blk], pick)  # warm: discarded
    for _ in range(RUNS):
        got, k = eng.find([blk], pick)
        assert sum(1 for g in got if g[2] == T.TSG_OK) == BATCH
        print("%-8s kernel_ns %d" % (label, k), flush=True)
    blk.close()
    eng.close()


def main():
    if _READ:
        return read_leg(sys.argv[2], sys.argv[3])
    rng = random.Random(1)

    def wordy(n):
        out = bytearray()
        while len(out) < n:
            out += rng.choice(WORDS) + str(rng.randrange(1000)).encode()
        return bytes(out[:n])

    pool = [wordy(rng.randrange(300, 900)) for _ in range(5000)]
    objs = [pool[rng.randrange(len(pool))][: rng.randrange(250, 900)] + rng.randbytes(24) for _ in range(N)]
    raw = sorted({rng.randbytes(16) for _ in range(N)})
    ids = np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(-1, 16)
    pick = ids[np.random.default_rng(2).choice(len(ids), BATCH, replace=False)]
    if len(sys.argv) > 2 and sys.argv[1] == "--write":
        os.makedirs(sys.argv[2], exist_ok=True)
        T.write_v2_block(os.path.join(sys.argv[2], "zstd"), ids, objs, encoding=T.ENC_ZSTD, index_downsample_bytes=100_000)
        np.save(os.path.join(sys.argv[2], "pick.npy"), pick)
        return
    eng = T.Engine(devices=[0])
    runs = {"wave": [], "one-lane": []}
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "zstd")
        T.write_v2_block(p, ids, objs, encoding=T.ENC_ZSTD, index_downsample_bytes=100_000)
        blk = eng.open_v2block(p)
        lk, _ = eng.lookup([blk], pick)
        recs = {int(r[2]): int(r[4]) for r in lk}  # the distinct pages of the batch: record -> bytes
        for leg in range(LEGS):
            for name, lane in (("one-lane", 1), ("wave", 0)):
                T.debug_set("zstd_find_lane", lane)
                eng.find([blk], pick)  # warm: discarded
                for _ in range(RUNS):
                    got, k = eng.find([blk], pick)
                    assert sum(1 for g in got if g[2] == T.TSG_OK) == BATCH
                    runs[name].append(k)
                    print("leg %d %-8s kernel_ns %d" % (leg, name, k), flush=True)
        T.debug_set("zstd_find_lane", 0)
        blk.close()
        res = {name: dict(kernel_ns_median=statistics.median(v), kernel_ns_min=min(v), kernel_ns_max=max(v), runs=len(v))
               for name, v in runs.items()}
        res["block"] = dict(pages=len(recs), page_bytes=sum(recs.values()), data_file_bytes=os.path.getsize(os.path.join(p, "data")))
    eng.close()
    print(json.dumps(res), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
