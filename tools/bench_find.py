#!/usr/bin/env python3
"""Device time of one tsg_find_ids batch over a v2 block written at ENCODING (none, snappy,
lz4-64k, lz4-256k, lz4-1M, lz4 or zstd) by the block writer's own compressor: 100 000 objects of
250-900 bytes, pages cut every 100 000 object bytes, 2000 present ids over about 515 pages
(profiles/lz4_find, profiles/zstd_find, profiles/find_codecs). Every run's
tsg_find_result.kernel_ns is printed.

    python tools/bench_find.py ENCODING [--lanes | --on-demand] [--out out.json]
        in one process: LEGS legs of one call discarded and RUNS calls, then the median / min / max
        and the batch's page set; --lanes (zstd): each leg once with the one-lane decoder
        (tsg_debug_set "zstd_find_lane") and once with the wave decoder; --on-demand: each leg once
        on the block opened resident and once on it opened with TSG_V2_DATA_ON_DEMAND (the hit
        pages read from the data file per call; the file was just written, so the page cache
        holds it), with the call's wall time beside kernel_ns (profiles/find_on_demand);
        --stage-bytes N cuts the on-demand batch into rounds of at most N staged bytes
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
import time

ap = argparse.ArgumentParser()
ap.add_argument("encoding")
ap.add_argument("--lanes", action="store_true")
ap.add_argument("--on-demand", action="store_true")
ap.add_argument("--stage-bytes", type=int, default=0, help="with --on-demand: the staging cap (0 = the default, one round)")
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


def find_bare(eng, blk, pick):
    """tsg_find_ids + tsg_find_result_free with nothing of the result converted, as a Go caller pays
    for the call: (objects found, kernel_ns)."""
    import ctypes as C
    from tempo_amd import tsg
    ids = np.ascontiguousarray(pick, dtype=np.uint8).reshape(-1, 16)
    arr = (C.c_void_p * 1)(blk.h)
    o = tsg._LookupOpts(0, 0, None, None)
    rp = C.POINTER(tsg._FindResult)()
    tsg._check(T.lib().tsg_find_ids(eng.h, arr, 1, ids.ctypes.data, ids.shape[0], C.byref(o), C.byref(rp)))
    try:
        r = rp.contents
        return int((np.ctypeslib.as_array(r.status, (int(r.n),)) == T.TSG_OK).sum()), int(r.kernel_ns)
    finally:
        T.lib().tsg_find_result_free(rp)


def leg(eng, blk, pick, label, wall=None):
    eng.find([blk], pick)  # warm: discarded
    ns = []
    for _ in range(RUNS):
        if wall is None:
            got, k = eng.find([blk], pick)
            found, extra = sum(1 for g in got if g[2] == T.TSG_OK), ""
        else:  # the bare call, timed: nothing of the result converted
            t0 = time.perf_counter_ns()
            found, k = find_bare(eng, blk, pick)
            wall.append(time.perf_counter_ns() - t0)
            extra = " wall_ns %d" % wall[-1]
        assert found == BATCH
        ns.append(k)
        print("%-10s kernel_ns %d%s" % (label, k, extra), flush=True)
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
    if ARGS.on_demand:
        kinds = (("resident", 0, T.V2_DATA_RESIDENT), ("on-demand", 0, T.V2_DATA_ON_DEMAND))
    elif ARGS.lanes:
        kinds = (("one-lane", 1, 0), ("wave", 0, 0))
    else:
        kinds = ((ARGS.encoding, 0, 0),)
    runs = {name: [] for name, _, _ in kinds}
    walls = {name: [] for name, _, _ in kinds}
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, ARGS.encoding)
        pick = write(p)
        blks = {mode: eng.open_v2block(p, data_mode=mode) for mode in {m for _, _, m in kinds}}
        lk, _ = eng.lookup([blks[kinds[0][2]]], pick)
        recs = {int(r[2]): int(r[4]) for r in lk}  # the distinct pages of the batch: record -> bytes
        for n in range(LEGS):
            for name, lane, mode in kinds:
                T.debug_set("zstd_find_lane", lane)
                if ARGS.on_demand:
                    T.debug_set("find_stage_bytes", ARGS.stage_bytes if mode == T.V2_DATA_ON_DEMAND else 0)
                runs[name] += leg(eng, blks[mode], pick, "leg %d %s" % (n, name), walls[name] if ARGS.on_demand else None)
        for b in blks.values():
            b.close()
        res = {name: dict(kernel_ns_median=statistics.median(v), kernel_ns_min=min(v), kernel_ns_max=max(v), runs=len(v))
               for name, v in runs.items()}
        for name, v in walls.items():
            if v:
                res[name].update(wall_ns_median=statistics.median(v), wall_ns_min=min(v), wall_ns_max=max(v))
        if ARGS.on_demand:
            res["stage_bytes"] = ARGS.stage_bytes
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
