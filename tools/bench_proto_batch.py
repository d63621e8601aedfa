#!/usr/bin/env python3
"""The fixed cost of a proto-object search job: J page-range jobs over four proto blocks as J
tsg_proto_search calls in a loop (a) and as one tsg_proto_search_batch call (b).
profiles/proto_batch has the runs.

    python tools/bench_proto_batch.py --write DIR [--objects 131072]
        writes four v2 (dataEncoding v2, snappy) blocks of --objects trace objects each to DIR
        (no device needed). Object i is trace i % 1200 of a pool: resource service.name one of 5
        values (5 value sets: a 1-byte column), one span with http.url one of 600 values (600
        value sets: a 2-byte column). Pages of ~64 KiB.
    python tools/bench_proto_batch.py --read DIR LABEL [PACKAGE_ROOT] [--jobs 256] [--reps 5]
        one run in a process of its own with the tempo_amd package under PACKAGE_ROOT (default:
        this checkout; a build of an earlier commit reads the same blocks and times (a) only):
        opens the blocks, cuts each into jobs/4 page ranges of equal page count (about 2200
        objects a job at the defaults) with one of four requests in turn (no tag, service.name,
        http.url, both; limit 20), warms up, then times --reps passes of (a) and of (b) and
        prints one JSON line with the median pass of each, per job.
Algorithmic bytes of a job: objects x (24 + 1 + the widths of its terms' columns).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--write", metavar="DIR")
ap.add_argument("--read", nargs="+", metavar=("DIR", "LABEL"))
ap.add_argument("--objects", type=int, default=131072)
ap.add_argument("--jobs", type=int, default=256)
ap.add_argument("--reps", type=int, default=5)
ARGS = ap.parse_args()
if bool(ARGS.write) == bool(ARGS.read):
    ap.error("one of --write DIR, --read DIR LABEL [PACKAGE_ROOT]")
if ARGS.read and not 2 <= len(ARGS.read) <= 3:
    ap.error("--read takes DIR LABEL [PACKAGE_ROOT]")
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(ARGS.read[2]) if ARGS.read and len(ARGS.read) > 2 else HERE)
import tempo_amd as T  # noqa: E402
from tempo_amd import tsg  # noqa: E402

NBLOCKS, POOL, NSVC, NURL = 4, 1200, 5, 600
T0, SEC = 1_700_000_000, 1_000_000_000
# (tags, the widths of their columns: 5 and 600 value sets, the loader's 1 / 2 / 4-byte rule)
REQUESTS = [({}, 0), ({"service.name": "svc-2"}, 1), ({"http.url": "users/17"}, 2),
            ({"service.name": "svc-1", "http.url": "users/4"}, 3)]


def block_paths(d):
    return [os.path.join(d, "pblk%d" % i) for i in range(NBLOCKS)]


if ARGS.write:
    import numpy as np
    sys.path.insert(0, HERE)
    from oracle import proto_oracle as P  # (its test-data writer encodes the trace protos)
    pool = []
    for i in range(POOL):
        st = (T0 + i) * SEC
        span = {"name": "op-%d" % (i % 7), "start": st, "end": st + (1 + i % 900) * 1_000_000, "parent": b"",
                "code": i % 3, "attrs": {"http.url": "/api/v1/users/%d" % (i % NURL), "http.status_code": 200}}
        pool.append(P.enc_object([{"resource": {"service.name": "svc-%d" % (i % NSVC)}, "spans": [span]}], True,
                                 T0 + i, T0 + i + 1))
    n = ARGS.objects
    ids = np.zeros((n, 16), dtype=np.uint8)
    ids[:, 8:] = np.arange(n, dtype=">u8").view(np.uint8).reshape(n, 8)
    for b, p in enumerate(block_paths(ARGS.write)):
        if os.path.exists(os.path.join(p, "meta.json")):
            continue
        T.write_v2_block(p, ids, [pool[(i + 7 * b) % POOL] for i in range(n)], encoding=T.ENC_SNAPPY,
                         data_encoding="v2", index_downsample_bytes=64 * 1024)
    print("wrote %d blocks of %d objects to %s" % (NBLOCKS, n, ARGS.write))
    sys.exit(0)


class ProtoItem(C.Structure):
    _fields_ = [("block", C.c_void_p), ("req", C.c_void_p)]


L = T.lib()
eng = T.Engine(devices=[0])
blocks = [eng.open_proto_block(p) for p in block_paths(ARGS.read[0])]
J, per = ARGS.jobs, ARGS.jobs // NBLOCKS
keep, reqs, items, widths = [], [], (ProtoItem * J)(), []
for j in range(J):
    blk = blocks[j // per]
    pages = blk.info()["pages"]
    k = (pages + per - 1) // per
    tags, w = REQUESTS[j % len(REQUESTS)]
    kv = [(a.encode(), b.encode()) for a, b in tags.items()]
    m = max(len(kv), 1)
    arrs = ((C.c_char_p * m)(*[a for a, _ in kv]), (C.c_uint32 * m)(*[len(a) for a, _ in kv]),
            (C.c_char_p * m)(*[b for _, b in kv]), (C.c_uint32 * m)(*[len(b) for _, b in kv]))
    keep.append(arrs)
    reqs.append(tsg._ProtoRequest(len(kv), arrs[0], arrs[1], arrs[2], arrs[3], 0, 0, 0, 2 ** 32 - 1, 20,
                                  (j % per) * k, k, 0, 0))
    items[j].block, items[j].req = blk.h, C.addressof(reqs[j])
    widths.append(w)
has_batch = hasattr(L, "tsg_proto_search_batch")
if has_batch:
    L.tsg_proto_search_batch.argtypes = [C.c_void_p, C.POINTER(ProtoItem), C.c_size_t,
                                         C.POINTER(C.POINTER(tsg._ProtoResult)), C.POINTER(C.c_int32)]
outs = (C.POINTER(tsg._ProtoResult) * J)()


def digest(r):
    return (r.n, tuple(r.object_idx[i] for i in range(r.n)), r.inspected_traces, r.inspected_bytes, r.skipped_traces)


def singles():
    """(a): wall seconds, summed kernel_ns, the results' digests, objects per job."""
    rp = C.POINTER(tsg._ProtoResult)()
    res = []
    t0 = time.perf_counter()
    for j in range(J):
        rc = L.tsg_proto_search(eng.h, items[j].block, C.byref(reqs[j]), C.byref(rp))
        if rc:
            raise SystemExit("tsg_proto_search: %d %s" % (rc, L.tsg_last_error()))
        res.append(rp)
        rp = C.POINTER(tsg._ProtoResult)()
    dt = time.perf_counter() - t0
    out = (dt, sum(r.contents.kernel_ns for r in res), [digest(r.contents) for r in res])
    for r in res:
        L.tsg_proto_result_free(r)
    return out


def batch():
    """(b): wall seconds, the launch's kernel_ns, the results' digests."""
    t0 = time.perf_counter()
    rc = L.tsg_proto_search_batch(eng.h, items, J, outs, None)
    dt = time.perf_counter() - t0
    if rc:
        raise SystemExit("tsg_proto_search_batch: %d %s" % (rc, L.tsg_last_error()))
    kn = {outs[j].contents.kernel_ns for j in range(J)} - {0}  # (0: a job without objects)
    assert len(kn) == 1, kn  # (one launch served every job)
    out = (dt, kn.pop(), [digest(outs[j].contents) for j in range(J)])
    for j in range(J):
        L.tsg_proto_result_free(outs[j])
    return out


for _ in range(2):
    ref = singles()[2]
    if has_batch:
        assert batch()[2] == ref  # (the same records and metrics, at the sizes timed)
a = [singles()[:2] for _ in range(ARGS.reps)]
# (limit 20 stops the host replay early: the kernel's objects are the page range's, counted by an
# unlimited pass over the same ranges that matches nothing)
objs = [eng.proto_search(blocks[j // per], tags={"service.name": "no such service"}, start=0, end=2 ** 32 - 1,
                         limit=2 ** 31, start_page=reqs[j].start_page, total_pages=reqs[j].total_pages).inspected_traces
        for j in range(J)]
row = {"label": ARGS.read[1], "jobs": J, "objects_per_job": statistics.median(objs),
       "a_us_per_job": round(statistics.median(t for t, _ in a) / J * 1e6, 3),
       "a_kernel_us_sum": round(statistics.median(k for _, k in a) / 1e3, 1)}
if has_batch:
    b = [batch()[:2] for _ in range(ARGS.reps)]
    kns = statistics.median(k for _, k in b)
    nbytes = sum(o * (25 + w) for o, w in zip(objs, widths))
    row.update({"b_us_per_job": round(statistics.median(t for t, _ in b) / J * 1e6, 3),
                "b_kernel_us": round(kns / 1e3, 1), "b_algorithmic_mb": round(nbytes / 1e6, 3),
                "b_share_of_8tbs": round(nbytes / (kns * 1e-9) / 8e12, 4) if kns else None})
for blk in blocks:
    blk.close()
eng.close()
print(json.dumps(row))
