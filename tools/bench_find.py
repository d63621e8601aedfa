#!/usr/bin/env python3
"""Device time of one tsg_find_ids batch over a v2 block written at ENCODING (none, snappy,
lz4-64k, lz4-256k, lz4-1M, lz4 or zstd) by the block writer's own compressor: 100 000 objects of
250-900 bytes, pages cut every 100 000 object bytes, 2000 present ids over about 515 pages
(profiles/lz4_find, profiles/zstd_find, profiles/find_codecs). Every run's
tsg_find_result.kernel_ns is printed.

    python tools/bench_find.py ENCODING [--lanes] [--out out.json]
        in one process: LEGS legs of one call discarded and RUNS calls, then the median / min / max
        and the batch's page set; --lanes (zstd): each leg once with the one-lane decoder
        (tsg_debug_set "zstd_find_lane") and once with the wave decoder
    python tools/bench_find.py ENCODING --write DIR
        writes the block and the batch's ids to DIR (no device needed)
    python tools/bench_find.py ENCODING --read DIR LABEL [PACKAGE_ROOT]
        one leg in a process of its own: opens DIR's block with the tempo_amd package under
        PACKAGE_ROOT (default: this checkout; a build of an earlier commit reads the same block)
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("encoding")
ap.add_argument("--lanes", action="store_true")
ap.add_argument("--out")
ap.add_argument("--write", metavar="DIR")
ap.add_argument("--read", nargs="+", metavar=("DIR", "LABEL"))
ARGS = ap.parse_args()
if ARGS.read and not 2 <= len(ARGS.read) <= 3:
    ap.error("--read takes DIR LABEL [PACKAGE_ROOT]")
sys.path.insert(0, os.path.abspath(ARGS.read[2]) if ARGS.read and len(ARGS.read) > 2 else
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import tempo_amd as T  # noqa: E402

WORDS = [b"span", b"trace", b"service", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select"]
N, BATCH, RUNS, LEGS = 100_000, 2000, 7, 4
ENC_NAMES = ["none", "gzip", "lz4-64k", "lz4-256k", "lz4-1M", "lz4", "snappy", "zstd", "s2"]  # backend.Encoding.String
if ARGS.encoding not in ENC_NAMES:
    ap.error("ENCODING is one of " + " ".join(ENC_NAMES))


def write(path):
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
    T.write_v2_block(path, ids, objs, encoding=ENC_NAMES.index(ARGS.encoding), index_downsample_bytes=100_000)
    return ids[np.random.default_rng(2).choice(len(ids), BATCH, replace=False)]


def leg(eng, blk, pick, label):
    eng.find([blk], pick)  # warm: discarded
    ns = []
    for _ in range(RUNS):
        got, k = eng.find([blk], pick)
        assert sum(1 for g in got if g[2] == T.TSG_OK) == BATCH
        ns.append(k)
        print("%-10s kernel_ns %d" % (label, k), flush=True)
    return ns


def main():
    if ARGS.write:
        os.makedirs(ARGS.write, exist_ok=True)
        np.save(os.path.join(ARGS.write, "pick.npy"), write(os.path.join(ARGS.write, ARGS.encoding)))
        return
    eng = T.Engine(devices=[0])
    if ARGS.read:
        blk = eng.open_v2block(os.path.join(ARGS.read[0], ARGS.encoding))
        leg(eng, blk, np.load(os.path.join(ARGS.read[0], "pick.npy")), ARGS.read[1])
        blk.close()
        eng.close()
        return
    kinds = (("one-lane", 1), ("wave", 0)) if ARGS.lanes else ((ARGS.encoding, 0),)
    runs = {name: [] for name, _ in kinds}
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, ARGS.encoding)
        pick = write(p)
        blk = eng.open_v2block(p)
        lk, _ = eng.lookup([blk], pick)
        recs = {int(r[2]): int(r[4]) for r in lk}  # the distinct pages of the batch: record -> bytes
        for n in range(LEGS):
            for name, lane in kinds:
                T.debug_set("zstd_find_lane", lane)
                runs[name] += leg(eng, blk, pick, "leg %d %s" % (n, name))
        blk.close()
        res = {name: dict(kernel_ns_median=statistics.median(v), kernel_ns_min=min(v), kernel_ns_max=max(v), runs=len(v))
               for name, v in runs.items()}
        res["block"] = dict(pages=len(recs), page_bytes=sum(recs.values()), data_file_bytes=os.path.getsize(os.path.join(p, "data")))
    eng.close()
    print(json.dumps(res), flush=True)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
