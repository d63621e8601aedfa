#!/usr/bin/env python3
"""Device time of one tsg_find_ids batch over the same v2 block written at none, snappy and
lz4-256k (profiles/lz4_find/README.md). 100 000 objects of 250-900 bytes, pages cut every
100 000 object bytes, 2000 present ids. Per encoding: one call discarded, then RUNS calls;
prints and writes the median / min / max of tsg_find_result.kernel_ns and the page set's size.

    python tools/bench_lz4_find.py [out.json]
"""
import json
import os
import random
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import tempo_amd as T  # noqa: E402

WORDS = [b"span", b"trace", b"service", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select"]
N, BATCH, RUNS = 100_000, 2000, 11


def main():
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
    eng = T.Engine(devices=[0])
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for name, enc in (("none", T.ENC_NONE), ("snappy", T.ENC_SNAPPY), ("lz4-256k", T.ENC_LZ4_256K)):
            p = os.path.join(d, name)
            T.write_v2_block(p, ids, objs, encoding=enc, index_downsample_bytes=100_000)
            blk = eng.open_v2block(p)
            eng.find([blk], pick)  # warm: discarded
            ns = []
            for _ in range(RUNS):
                got, k = eng.find([blk], pick)
                assert sum(1 for g in got if g[2] == T.TSG_OK) == BATCH
                ns.append(k)
            lk, _ = eng.lookup([blk], pick)
            recs = {int(r[2]): int(r[4]) for r in lk}  # the distinct pages of the batch: record -> bytes
            blk.close()
            res[name] = dict(kernel_ns_median=statistics.median(ns), kernel_ns_min=min(ns), kernel_ns_max=max(ns),
                             runs=RUNS, pages=len(recs), page_bytes=sum(recs.values()),
                             data_file_bytes=os.path.getsize(os.path.join(p, "data")))
            print(name, res[name], flush=True)
    eng.close()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
