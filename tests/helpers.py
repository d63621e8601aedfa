"""Shared test helpers: synthetic entries, block writing, oracle/engine comparison."""
import os
import random
import tempfile

from oracle import oracle as O
import tempo_amd as T


def ref_id(i, n=16):
    """binary.LittleEndian.PutUint32(id, uint32(i)) into an n-byte buffer
    (tempodb/search/backend_search_block_test.go:63-64)."""
    return i.to_bytes(4, "little") + bytes(n - 4)


def gen_search_data(i):
    """genSearchData (backend_search_block_test.go:24-31)."""
    return {"key%d" % i: ["value_A_%d" % i, "value_B_%d" % i]}


def write_block(tmpdir, name, entries, enc=T.ENC_SNAPPY, page_size=0):
    path = os.path.join(tmpdir, name)
    T.write_search_block(path, entries, enc, page_size)
    return path


def random_entries(rng, n, nkeys=6, nvals=5, multi=3, id_len=16, with_names=True, t0=1_700_000_000 * 10**9,
                   zero_end_frac=0.02):
    ents = []
    ids = set()
    while len(ids) < n:
        ids.add(bytes(rng.getrandbits(8) for _ in range(id_len)))
    for tid in sorted(ids):
        tags = {}
        for k in range(nkeys):
            if rng.random() < 0.8:
                vals = sorted({"v%d-%s" % (rng.randrange(nvals), "xyz"[rng.randrange(3)])
                               for _ in range(1 + rng.randrange(multi))})
                tags["k%d" % k] = vals
        if with_names:
            tags["root.service.name"] = ["svc-%d" % rng.randrange(4)]
            tags["root.name"] = ["op-%d" % rng.randrange(7)]
        start = t0 + rng.randrange(3600 * 10**9)
        dur = int(rng.lognormvariate(17.7, 1.5))
        end = start + dur
        if rng.random() < zero_end_frac:
            end = 0
        ents.append({"id": tid, "start": start, "end": end, "tags": tags})
    return ents


def match_key(m):
    """Comparable tuple for an oracle match dict."""
    return (m["block_idx"], m["entry_idx"], m["id"], m["start_ns"], m["end_ns"], m["duration_ms"],
            m["root_service"], m["root_name"])


def tsg_key(m):
    return (m.block_idx, m.entry_idx, m.trace_id, m.start_time_unix_nano, m.end_time_unix_nano, m.duration_ms,
            m.root_service_name.encode(), m.root_trace_name.encode())


# ---- damaged blocks (BackendSearchBlock.Search's error paths) ------------------------
def _meta(path):
    import json
    with open(os.path.join(path, "search.meta.json")) as f:
        return json.load(f)


def _write_meta(path, meta):
    import json
    with open(os.path.join(path, "search.meta.json"), "w") as f:
        f.write(json.dumps(meta, separators=(",", ":")))


def index_records(path):
    """The (id, start, length) records of a block's search-index (v2 index pages)."""
    import struct
    meta = _meta(path)
    ps, n = meta["indexPageSize"], meta["indexRecords"]
    rpp = (ps - 14) // 28
    raw = open(os.path.join(path, "search-index"), "rb").read()
    out = []
    for i in range(n):
        p, r = divmod(i, rpp)
        rec = raw[p * ps + 14 + 28 * r: p * ps + 14 + 28 * (r + 1)]
        out.append((rec[:16],) + struct.unpack("<QI", rec[16:]))
    return out


def repage_index(path, rpp):
    """Rewrite search-index with `rpp` records per page (indexPageSize = 14 + 28 rpp, a
    value the reference reads from search.meta.json), so a test can damage page k > 0."""
    import struct
    recs = index_records(path)
    ps = 14 + 28 * rpp
    out = bytearray()
    for p0 in range(0, len(recs), rpp):
        data = b"".join(i + struct.pack("<QI", s, l) for i, s, l in recs[p0:p0 + rpp])
        data += bytes(28 * rpp - len(data))
        out += struct.pack("<IHQ", ps, 8, O.xxhash64(data)) + data
    open(os.path.join(path, "search-index"), "wb").write(bytes(out))
    meta = _meta(path)
    meta["indexPageSize"] = ps
    _write_meta(path, meta)


def damage_index_page_checksum(path, page):
    """Flip a byte of index page `page`'s data: getPage fails its checksum."""
    ps = _meta(path)["indexPageSize"]
    p = os.path.join(path, "search-index")
    b = bytearray(open(p, "rb").read())
    b[page * ps + 14 + 3] ^= 0x5A
    open(p, "wb").write(bytes(b))


def zero_index_record(path, k):
    """Zero record k and re-checksum its page: At(k) fails ('unexpected zero value record')."""
    import struct
    meta = _meta(path)
    ps = meta["indexPageSize"]
    rpp = (ps - 14) // 28
    pg, r = divmod(k, rpp)
    p = os.path.join(path, "search-index")
    b = bytearray(open(p, "rb").read())
    o = pg * ps + 14
    b[o + 28 * r: o + 28 * (r + 1)] = bytes(28)
    b[pg * ps + 6: pg * ps + 14] = struct.pack("<Q", O.xxhash64(bytes(b[o:pg * ps + ps])))
    open(p, "wb").write(bytes(b))


def damage_data_page(path, k, how="payload"):
    """Damage data page k of the `search` file. payload: flip a byte in the middle of the
    (compressed) page payload; length: break the page's totalLength field; truncate: cut
    the file inside page k (its ReadAt fails)."""
    import struct
    _, start, length = index_records(path)[k]
    p = os.path.join(path, "search")
    b = bytearray(open(p, "rb").read())
    if how == "payload":
        b[start + 6 + (length - 6) // 2] ^= 0xA5
    elif how == "length":
        b[start:start + 4] = struct.pack("<I", length + 1)
    elif how == "objlen":  # (encoding none) the object's total length past the page
        b[start + 6:start + 10] = struct.pack("<I", 0x7FFFFFF0)
    elif how == "truncate":
        b = b[:start + length // 2]
    open(p, "wb").write(bytes(b))


def shim_digest(per_block):
    """tsgx_shim_pattern's per-round digest (shim_pattern.cpp result_digest) from the oracle's
    ordered matches of each block of the set: the sum mod 2^64 over blocks i of FNV-1a 64 over
    (i as u32, then per match its scan position u64, its id right-aligned in 16 bytes, its start u64)."""
    import struct
    M = (1 << 64) - 1
    total = 0
    for i, matches in enumerate(per_block):
        h = 0xcbf29ce484222325
        buf = bytearray(struct.pack("<I", i))
        for m in matches:
            buf += struct.pack("<Q", m["entry_idx"]) + bytes(16 - len(m["id"])) + m["id"] + struct.pack("<Q", m["start_ns"])
        for b in buf:
            h = ((h ^ b) * 0x100000001b3) & M
        total = (total + h) & M
    return total


# ---- column results against the oracle ----------------------------------------------
def oracle_columns(exp):
    """The oracle's ordered matches as numpy columns (built once for a large result), the root
    names as indices into `names`."""
    import numpy as np
    n = len(exp)
    col = lambda f, dt: np.fromiter((m[f] for m in exp), dt, n)  # noqa: E731
    out = {"block_idx": col("block_idx", np.uint32), "entry_idx": col("entry_idx", np.uint64),
           "start_ns": col("start_ns", np.uint64), "end_ns": col("end_ns", np.uint64),
           "duration_ms": col("duration_ms", np.uint32),
           "trace_id": np.frombuffer(b"".join(m["id"] for m in exp), np.uint8).reshape(n, 16)}
    names, index = [], {}
    for f in ("root_service", "root_name"):
        out[f] = np.fromiter((index.setdefault(m[f], len(index)) for m in exp), np.int64, n)
    names = sorted(index, key=index.get)
    out["names"] = names
    return out


def columns_equal_oracle(cols, gmet, ocols, omet):
    """Engine.search_columns' result against the oracle's of the same search (oracle_columns
    of its matches, its metrics): the four metrics, then every record in order, field by
    field (block index, scan position, id, start, end, DurationMs, root names). Returns None
    when equal, else a short description of the first difference."""
    import numpy as np
    keys = ("traces_inspected", "bytes_inspected", "blocks_inspected", "blocks_skipped")
    got_m = (gmet.inspected_traces, gmet.inspected_bytes, gmet.inspected_blocks, gmet.skipped_blocks)
    if got_m != tuple(omet[k] for k in keys):
        return "metrics %r != %r" % (got_m, tuple(omet[k] for k in keys))
    n = len(ocols["start_ns"])
    if len(cols["start_ns"]) != n:
        return "%d records, oracle %d" % (len(cols["start_ns"]), n)
    if n == 0:
        return None
    for f in ("block_idx", "entry_idx", "start_ns", "end_ns", "duration_ms"):
        bad = np.nonzero(cols[f] != ocols[f])[0]
        if len(bad):
            return "%s differs at record %d: %r != %r" % (f, bad[0], cols[f][bad[0]], ocols[f][bad[0]])
    bad = np.nonzero((cols["trace_id"] != ocols["trace_id"]).any(axis=1))[0]
    if len(bad):
        return "trace_id differs at record %d" % bad[0]
    # the engine's name indices, translated to the oracle's numbering (-1: a name it does not have)
    oidx = {s: i for i, s in enumerate(ocols["names"])}
    lut = np.fromiter((oidx.get(s, -1) for s in cols["names"]), np.int64, len(cols["names"]))
    for f in ("root_service", "root_name"):
        bad = np.nonzero(lut[cols[f]] != ocols[f])[0]
        if len(bad):
            return "%s differs at record %d" % (f, bad[0])
    return None


# ---- hand-built edge blocks (tests/test_gpu_variants.py) -----------------------------
# The narrow kernels scan 512-entry units; lane l of a unit holds entries 4l + j and
# 256 + 4l + j (j = 0..3). The blocks below put their matches (the "hit set" H) on those
# edges and make every predicate decisive inside H.
EDGE_T0 = 1_700_000_000
EDGE_SIZES = (1, 7, 511, 512, 513, 1025, 4096, 4097)
# the full query of the matrix: terms a..d (substring needles for b and c), whole-ms duration
# bounds, a time range
EDGE_TERMS = (("a", "a-hit"), ("b", "-hit"), ("c", "c-h"), ("d", "d-hit"))
EDGE_MIN_MS, EDGE_MAX_MS = 10, 500
EDGE_START, EDGE_END = EDGE_T0 + 1000, EDGE_T0 + 2000
EDGE_RUN = (1000, 1700)  # the 4097 block's run of 700 consecutive hits: unit 2 whole, units 1 and 3 in part
EDGE_VARIED_POS = 100    # (vary_dicts) the non-H entry of each block that carries the block's own values

_MS, _S = 10**6, 10**9
# role of a hit by its position in the block (every other hit passes every predicate)
_EDGE_ROLES = {
    # lanes 0 and 1 of step 0: one term fails alone
    1: "fail_a", 2: "fail_b", 4: "multi_c", 5: "fail_c", 6: "fail_d",
    # around the step boundary at 256: durations at / 1 ns under / 1 ns over the whole-ms bounds
    251: "dur_min", 252: "dur_min_under", 253: "dur_min_over", 257: "dur_max", 258: "dur_max_under",
    259: "dur_max_over",
    # around the unit boundary at 512: the time range's edges, and the two span escapes
    506: "end_eq_start", 507: "end_before_start", 509: "start_eq_end", 510: "start_after_end",
    513: "end_zero", 514: "span_long",
}


def edge_hits(n):
    """The hit set H of the edge block of n entries -> {position: role}."""
    groups = {
        1: [], 7: [range(0, 10)], 511: [range(0, 10), range(250, 263), range(505, 521)],
        512: [range(0, 10), range(250, 263), range(505, 521)],
        513: [range(0, 10), range(250, 263), range(505, 521)],
        1025: [[511]],          # position 511 alone: the last entry of a unit
        4096: [[255, 256]],     # 255 and 256 alone: both sides of the step boundary
        4097: [range(0, 10), range(250, 263), range(505, 521), range(*EDGE_RUN)],
    }[n]
    h = {}
    for g in groups:
        for p in g:
            if p < n:
                h[p] = _EDGE_ROLES.get(p, "ok")
    for p in range(EDGE_RUN[0], EDGE_RUN[1]):
        if p in h:  # the run: mostly whole lanes of matches, a few single misses
            h[p] = "fail_b" if p % 37 == 0 else "dur_max_over" if p % 41 == 0 else "ok"
    for p in range(max(0, n - 3), n):  # the last three entries pass everything
        h[p] = "ok"
    return h


def _edge_entry(tid, blk, pos, role, vary_dicts):
    tags = {"a": ["a-hit"], "b": ["b-hit"], "c": ["c-hit"], "d": ["d-hit"], "e": ["e-hit"]}
    start, dur = (EDGE_T0 + 1500) * _S + pos * 1000, 100 * _MS + pos
    end = None
    if role is None:  # outside H: term a fails; everything else varies with the position
        h = (pos * 2654435761 + blk * 40503) >> 7
        tags["a"] = ["a-no", "a-alt"][h % 2]
        tags["b"] = ["b-hit", "b-no", "b-alt"][(h >> 1) % 3]
        tags["c"] = [["c-hit"], ["c-no"], ["c-alt"], ["c-alt", "c-hit"]][(h >> 3) % 4]
        tags["d"] = ["d-hit", "d-no", "d-alt"][(h >> 5) % 3]
        tags["e"] = ["e-hit", "e-no", "e-alt"][(h >> 7) % 3]
        dur = 100 * _MS if pos % 97 == 5 else (5 * _MS, 600 * _MS)[h % 2]
        if pos % 89 != 7:
            start = ((EDGE_T0 + 100, EDGE_T0 + 5000)[(h >> 2) % 2]) * _S + pos
        if vary_dicts and pos == EDGE_VARIED_POS:
            tags["a"], tags["b"] = "a-x%d" % blk, "b-x%d" % blk
    elif role.startswith("fail_"):
        tags[role[5:]] = ["%s-no" % role[5:]]
    elif role == "multi_c":
        tags["c"] = ["c-alt", "c-hit"]
    elif role == "dur_min":
        dur = EDGE_MIN_MS * _MS
    elif role == "dur_min_under":
        dur = EDGE_MIN_MS * _MS - 1
    elif role == "dur_min_over":
        dur = EDGE_MIN_MS * _MS + 1
    elif role == "dur_max":
        dur = EDGE_MAX_MS * _MS
    elif role == "dur_max_under":
        dur = EDGE_MAX_MS * _MS - 1
    elif role == "dur_max_over":
        dur = EDGE_MAX_MS * _MS + 1
    elif role == "end_eq_start":      # end_s == req.Start
        start = EDGE_START * _S - 100 * _MS
    elif role == "end_before_start":  # end_s == req.Start - 1
        start, dur = EDGE_START * _S - 100 * _MS - 1, 100 * _MS
    elif role == "start_eq_end":      # start_s == req.End
        start = EDGE_END * _S + _S - 1
    elif role == "start_after_end":   # start_s == req.End + 1
        start = (EDGE_END + 1) * _S
    elif role == "end_zero":
        end = 0
    elif role == "span_long":         # a span over 65535 s
        start, dur = (EDGE_START + 100) * _S, 70_000 * _S
    tags["v"] = "v%03d" % (pos % 254)
    tags["w"] = "w%03d" % (pos % 255)
    tags["x"] = "x%03d" % (pos % 256)
    tags["root.service.name"] = "svc-%d" % (pos % 3)
    tags["root.name"] = "op-%d" % (pos % 5)
    return {"id": tid, "start": start, "end": start + dur if end is None else end, "tags": tags}


def write_edge_blocks(tmpdir, vary_dicts=False):
    """Writes the edge blocks (snappy, 64 KiB pages) and returns their paths.

    The writer takes entries in ascending id order and, as the reference's page builder does,
    lays each page's entries out back to front, so an entry's scan position is not its rank
    by id. An id here is [rank by id over the set, 8 bytes | scan position over the set,
    8 bytes], both big-endian: the low half names the position, and what an entry holds is
    decided by its position. Where the pages are cut depends (slightly) on the entries, so a
    block is rewritten until the positions read back (the oracle's scan of it) are the ones
    its entries were built for.

    vary_dicts: one non-H entry per block carries values of `a` and `b` no other block holds,
    so no two blocks share a dictionary of either key."""
    paths, base = [], 0
    for blk, n in enumerate(EDGE_SIZES):
        hits = edge_hits(n)
        pos_of = list(range(n))  # rank by id within the block -> scan position
        for _ in range(6):
            ents = [_edge_entry((base + r).to_bytes(8, "big") + (base + pos_of[r]).to_bytes(8, "big"), blk, pos_of[r],
                                hits.get(pos_of[r]), vary_dicts) for r in range(n)]
            path = write_block(tmpdir, "edge%d%s" % (blk, "v" if vary_dicts else ""), ents, T.ENC_SNAPPY, 64 << 10)
            scan, _, st = O.search([O.Block(path)])
            assert st == 0 and len(scan) == n
            ranks = [int.from_bytes(m["id"][:8], "big") - base for m in scan]  # scan position -> rank
            if all(pos_of[r] == s for s, r in enumerate(ranks)):
                break
            for s, r in enumerate(ranks):
                pos_of[r] = s
        else:
            raise AssertionError("edge block %d: the page layout did not settle" % blk)
        paths.append(path)
        base += n
    return paths
