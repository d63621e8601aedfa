"""GPU parity for tsg_wal_block_refresh: an open WAL block followed to its grown file.

Every case writes a WAL file with the first entries, opens it, appends the rest (the first
file is a byte prefix of the second) and refreshes. The refreshed handle must equal a fresh
open_wal_block of the grown file in info(), tags, tag values, and in the ordered records and
the four metrics of a fixed list of queries, which are also held against the oracle. The
record-side columns the merge kernel copies (16-byte ids, start_ns, end_ns, id lengths, the
root-name ids, dur64) are what every returned record is made of; the dense query on an engine
whose LDS record buffer is cut to 8 (TSG_POOL_REC) overflows to the look-back path, whose
records are gathered from the host copies of those columns (41 B per entry)."""
import os
import random

import pytest

from oracle import oracle as O
import tempo_amd as T
from tempo_amd import tsg
from tests.helpers import random_entries, tsg_key, write_block
from tests.test_gpu_search import assert_parity

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000
S, MS = 10**9, 10**6
INFO = ("entries", "pages", "keys", "fb_bytes", "min_dur_ns", "max_dur_ns", "partial", "traces", "streaming", "encoding")
QUERIES = [
    dict(tags={"k1": "v2-x"}),                                  # an exact tag
    dict(tags={"k1": "v2"}),                                    # a substring (the exact-value block filter decides)
    dict(min_ms=50, max_ms=50),                                 # both bounds on one whole-ms ds edge
    dict(min_ms=49),
    dict(tags={"k2": "v1-x"}, start=T0 + 600, end=T0 + 2400),   # a time range
    dict(),                                                     # every entry: dense
    dict(tags={"root.service.name": "svc-1"}, max_ms=32767),
]


@pytest.fixture(scope="module")
def small():
    """An engine whose pool kernels hold 8 records per workgroup: dense queries overflow to the
    look-back path (records gathered from the block's host columns)."""
    os.environ["TSG_POOL_REC"] = "8"
    try:
        e = T.Engine()
    finally:
        del os.environ["TSG_POOL_REC"]
    yield e
    e.close()


def wal_path(tmp_path, enc=T.ENC_SNAPPY, sub="w"):
    d = os.path.join(str(tmp_path), sub)
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, T.wal_filename(enc))


def grow(path, entries, enc=T.ENC_SNAPPY):
    """Rewrites the file with `entries` (the earlier entries first): returns the appended bytes."""
    old = open(path, "rb").read() if os.path.exists(path) else b""
    T.write_wal_search(path, entries, enc)
    new = open(path, "rb").read()
    assert new[:len(old)] == old and len(new) >= len(old)
    return len(new) - len(old)


def answers(eng, blk, q, limit):
    req = T.SearchRequest(tags=dict(q.get("tags") or {}), min_duration_ms=q.get("min_ms", 0),
                          max_duration_ms=q.get("max_ms", 0), start=q.get("start", 0), end=q.get("end", 0))
    got, met = eng.search([blk], T.Pipeline(req), limit=limit)
    return got, met


def summary(got, met):
    return ([tsg_key(m) for m in got], met.inspected_traces, met.inspected_bytes, met.inspected_blocks, met.skipped_blocks)


def same_as_fresh(eng, blk, path, extra=(), oracle_path=None):
    """oracle_path: the file the oracle replays, where it does not read `path`'s encoding (lz4):
    the same entries as snappy pages."""
    fresh = eng.open_wal_block(path)
    ob = O.Block(oracle_path or path, wal=True)
    try:
        bi, fi = blk.info(), fresh.info()
        assert {k: bi[k] for k in INFO} == {k: fi[k] for k in INFO}
        assert bi["device"] == fi["device"]
        assert blk.tags() == fresh.tags()
        for k in fresh.tags() + [b"absent"]:
            assert blk.tag_values(k) == fresh.tag_values(k)
        for q in QUERIES + list(extra):
            for limit in (0, 20):
                got, met = answers(eng, blk, q, limit)
                assert summary(got, met) == summary(*answers(eng, fresh, q, limit)), (q, limit)
                exp, omet, st = O.search([ob], tags=q.get("tags"), min_ms=q.get("min_ms", 0), max_ms=q.get("max_ms", 0),
                                         start=q.get("start", 0), end=q.get("end", 0), limit=limit)
                assert st == 0
                assert_parity(got, met, exp, omet)
    finally:
        fresh.close()


def shuffled_entries(seed, n, **kw):
    rng = random.Random(seed)
    ents = random_entries(rng, n, **kw)
    rng.shuffle(ents)  # (random_entries sorts by id: the appended part then falls between the old ids)
    return ents


# ---- case 1 (interleaved inserts) and case 10 (encodings) --------------------------------
@pytest.mark.parametrize("enc", [T.ENC_SNAPPY, T.ENC_LZ4_1M], ids=["snappy", "lz4-1M"])
def test_interleaved_inserts(engine, small, tmp_path, enc):
    ents = shuffled_entries(41, 65)
    lo, hi = min(e["id"] for e in ents), max(e["id"] for e in ents)
    first = [e for e in ents if e["id"] not in (lo, hi)][:40]
    rest = [e for e in ents if e not in first]  # 25 with the smallest and the largest id among them
    assert len(rest) == 25 and min(e["id"] for e in first) > lo and max(e["id"] for e in first) < hi
    for eng in (engine, small):
        p = wal_path(tmp_path, enc, "e%d" % id(eng))
        grow(p, first, enc)
        old = eng.open_wal_block(p)
        added = grow(p, first + rest, enc)
        blk, st = eng.refresh_wal_block(old, p)
        try:
            assert st["mode"] == 1 and st["bytes_replayed"] == added and st["pages_replayed"] == 25
            assert st["entries_added"] == 25 and st["entries_combined"] == 0
            assert st["upload_bytes"] > 0 and blk.info()["entries"] == 65
            twin = None
            if enc != T.ENC_SNAPPY:
                twin = wal_path(tmp_path, T.ENC_SNAPPY, "twin%d" % id(eng))
                T.write_wal_search(twin, first + rest, T.ENC_SNAPPY)
            same_as_fresh(eng, blk, p, oracle_path=twin)
            if eng is small:  # the dense query's records did overflow the pool kernels' buffer
                assert answers(eng, blk, dict(), 0)[1].path & T.PATH_OTHER
        finally:
            blk.close()
            old.close()


# ---- case 2: combine ---------------------------------------------------------------------
def test_combine(engine, small, tmp_path):
    ents = shuffled_entries(42, 60)
    base = (T0 + 100) * S
    ents[3].update(start=base, end=base + 50 * MS - 1)    # 49.999999 ms: below the 50 ms edge
    ents[7].update(start=base + 5 * S, end=base + 6 * S)
    more = [
        {"id": ents[3]["id"], "start": base, "end": base + 50 * MS, "tags": {"k1": ["v2-x", "extra"]}},  # exactly 50 ms now
        {"id": ents[7]["id"], "start": base - 70_000 * S, "end": base + 6 * S, "tags": {"late": ["x"]}},  # span >= 65535 s
        {"id": ents[11]["id"], "start": ents[11]["start"] - S, "end": 0, "tags": {"k0": ["v0-x"], "k9": ["nine"]}},
        {"id": ents[20]["id"], "start": 0, "end": ents[20]["end"] + 3 * S if ents[20]["end"] else 0, "tags": {"root.name": ["op-new"]}},
        {"id": ents[11]["id"], "start": 0, "end": ents[11]["start"] + 40 * S, "tags": {"root.service.name": ["svc-zz"]}},
    ]
    extra = [dict(tags={"k1": "extra"}), dict(tags={"late": "x"}), dict(tags={"k9": "nine"}, min_ms=1000),
             dict(tags={"root.name": "op-new"}), dict(start=T0 - 69_950, end=T0 - 69_000), dict(min_ms=60_000_000)]
    for eng in (engine, small):
        p = wal_path(tmp_path, sub="c%d" % id(eng))
        grow(p, ents)
        old = eng.open_wal_block(p)
        before = summary(*answers(eng, old, dict(min_ms=50, max_ms=50), 0))
        added = grow(p, ents + more)
        blk, st = eng.refresh_wal_block(old, p)
        try:
            assert st["mode"] == 1 and st["bytes_replayed"] == added
            assert st["entries_combined"] == 5 and st["entries_added"] == 0 and blk.info()["entries"] == 60
            same_as_fresh(eng, blk, p, extra)
            after = summary(*answers(eng, blk, dict(min_ms=50, max_ms=50), 0))
            moved = ents[3]["id"]  # onto the 50 ms edge
            assert moved in [k[2] for k in after[0]] and moved not in [k[2] for k in before[0]]
        finally:
            blk.close()
            old.close()


# ---- case 3: a key outgrows its one-byte column --------------------------------------------
def test_width_change(engine, tmp_path):
    ents = shuffled_entries(43, 260)
    for i, e in enumerate(ents[:250]):
        e["tags"]["grow"] = ["g%03d" % (500 + i)]
    for i, e in enumerate(ents[250:]):
        e["tags"]["grow"] = ["g%03d" % (100 + 37 * i)]  # sort before and between the old values
    p = wal_path(tmp_path)
    grow(p, ents[:250])
    old = engine.open_wal_block(p)
    grow(p, ents)
    blk, st = engine.refresh_wal_block(old, p)
    try:
        assert st["mode"] == 1 and st["entries_added"] == 10
        same_as_fresh(engine, blk, p, [dict(tags={"grow": "g749"}), dict(tags={"grow": "g500"}),  # only old entries
                                       dict(tags={"grow": "g100"}), dict(tags={"grow": "g433"}),  # only new ones
                                       dict(tags={"grow": "g999"})])
        got, _ = answers(engine, blk, dict(tags={"grow": "g500"}), 0)
        assert [m.trace_id for m in got] == [ents[0]["id"]]
        got, _ = answers(engine, blk, dict(tags={"grow": "g433"}), 0)
        assert [m.trace_id for m in got] == [ents[259]["id"]]
    finally:
        blk.close()
        old.close()


# ---- case 4: a key that first appears in the appended part -----------------------------------
def test_new_key(engine, tmp_path):
    ents = shuffled_entries(44, 90)
    for i, e in enumerate(ents[60:]):
        e["tags"]["fresh.key"] = ["f%d" % (i % 4)]
    p = wal_path(tmp_path)
    grow(p, ents[:60])
    old = engine.open_wal_block(p)
    assert b"fresh.key" not in old.tags()
    grow(p, ents)
    blk, st = engine.refresh_wal_block(old, p)
    try:
        assert st["mode"] == 1 and blk.info()["keys"] == old.info()["keys"] + 1
        same_as_fresh(engine, blk, p, [dict(tags={"fresh.key": "f1"}), dict(tags={"fresh.key": "f1", "k1": "v2-x"})])
        got, _ = answers(engine, blk, dict(tags={"fresh.key": "f1"}), 0)
        assert sorted(m.trace_id for m in got) == sorted(e["id"] for i, e in enumerate(ents[60:]) if i % 4 == 1)
    finally:
        blk.close()
        old.close()


# ---- case 5: the 512-entry unit and the column padding --------------------------------------
@pytest.mark.parametrize("n0,n1", [(511, 513), (512, 514)])
def test_padding_edges(engine, tmp_path, n0, n1):
    ents = shuffled_entries(45, n1)
    p = wal_path(tmp_path)
    grow(p, ents[:n0])
    old = engine.open_wal_block(p)
    grow(p, ents)
    blk, st = engine.refresh_wal_block(old, p)
    try:
        assert st["mode"] == 1 and st["entries_added"] == n1 - n0
        same_as_fresh(engine, blk, p)
    finally:
        blk.close()
        old.close()


# ---- case 6: nothing new, and refreshing a refreshed handle -----------------------------------
def test_nothing_new_and_repeated_refresh(engine, tmp_path):
    ents = shuffled_entries(46, 120)
    p = wal_path(tmp_path)
    grow(p, ents[:70])
    b0 = engine.open_wal_block(p)
    b1, s1 = engine.refresh_wal_block(b0, p)
    b2, s2 = engine.refresh_wal_block(b1, open(p, "rb").read())  # (the _mem entry point)
    try:
        for st in (s1, s2):
            assert st["mode"] == 0 and st["bytes_replayed"] == 0 and st["entries_added"] == 0
        same_as_fresh(engine, b1, p)
        same_as_fresh(engine, b2, p)
        added = grow(p, ents[:100])
        b3, s3 = engine.refresh_wal_block(b2, p)
        assert s3["mode"] == 1 and s3["bytes_replayed"] == added and s3["entries_added"] == 30
        same_as_fresh(engine, b3, p)
        added = grow(p, ents)
        b4, s4 = engine.refresh_wal_block(b3, open(p, "rb").read())
        assert s4["mode"] == 1 and s4["bytes_replayed"] == added and s4["entries_added"] == 20
        same_as_fresh(engine, b4, p)
        b3.close()
        b4.close()
    finally:
        for b in (b0, b1, b2):
            b.close()


# ---- case 7: a damaged appended page ------------------------------------------------------------
def test_damaged_appended_page(engine, tmp_path):
    ents = shuffled_entries(47, 80)
    p = wal_path(tmp_path)
    grow(p, ents[:50])
    n_old = os.path.getsize(p)
    old = engine.open_wal_block(p)
    grow(p, ents)
    data = bytearray(open(p, "rb").read())
    off = n_old
    for _ in range(12):  # the 13th appended page: its header checksum
        off += int.from_bytes(data[off:off + 4], "little")
    data[off + 6] ^= 1
    with open(p, "wb") as f:
        f.write(data)
    blk, st = engine.refresh_wal_block(old, p)
    try:
        info = blk.info()
        assert st["mode"] == 1 and st["pages_replayed"] == 12 and st["bytes_replayed"] == off - n_old
        assert info["partial"] == 1 and info["entries"] == 62
        same_as_fresh(engine, blk, p)
        again, st2 = engine.refresh_wal_block(blk, p)  # a partial block: nothing behind the damage is reached
        assert st2["mode"] == 0 and again.info()["partial"] == 1 and again.info()["entries"] == 62
        same_as_fresh(engine, again, p)
        again.close()
    finally:
        blk.close()
        old.close()


# ---- case 8: not the same file any more; not a WAL block ---------------------------------------
def test_prefix_mismatch_falls_back(engine, tmp_path):
    ents = shuffled_entries(48, 90)
    p = wal_path(tmp_path)
    grow(p, ents[:60])
    old = engine.open_wal_block(p)
    T.write_wal_search(p, ents[30:], T.ENC_SNAPPY)  # rotated under the same name: other pages, same count
    blk, st = engine.refresh_wal_block(old, p)
    try:
        assert st["mode"] == 2 and "reopened" in T.lib().tsg_last_error().decode()
        same_as_fresh(engine, blk, p)
    finally:
        blk.close()
    full = open(p, "rb").read()
    T.write_wal_search(p, ents[:60], T.ENC_SNAPPY)
    cut = open(p, "rb").read()
    cut = cut[:len(cut) - int.from_bytes(cut[:4], "little") // 2]  # shorter than what `old` was replayed from
    with open(p, "wb") as f:
        f.write(cut)
    blk, st = engine.refresh_wal_block(old, p)
    try:
        assert st["mode"] == 2 and blk.info()["partial"] == 1 and blk.info()["entries"] == 59
        same_as_fresh(engine, blk, p)
    finally:
        blk.close()
        old.close()
    assert len(full) > len(cut)
    bp = write_block(str(tmp_path), "backend", sorted(ents, key=lambda e: e["id"]))
    bb = engine.open_block(bp)
    try:
        with pytest.raises(T.TsgError) as ei:
            engine.refresh_wal_block(bb, p)
        assert ei.value.code == tsg.TSG_E_UNSUPPORTED
    finally:
        bb.close()


# ---- case 9: the old handle stays valid ----------------------------------------------------------
@pytest.mark.parametrize("close_old_first", [True, False])
def test_old_stays_valid(engine, tmp_path, close_old_first):
    ents = shuffled_entries(49, 100)
    p = wal_path(tmp_path)
    grow(p, ents[:70])
    old = engine.open_wal_block(p)
    before = [(summary(*answers(engine, old, q, limit)), old.info()["entries"]) for q in QUERIES for limit in (0, 20)]
    grow(p, ents)
    blk, st = engine.refresh_wal_block(old, p)
    assert st["mode"] == 1
    after = [(summary(*answers(engine, old, q, limit)), old.info()["entries"]) for q in QUERIES for limit in (0, 20)]
    assert after == before and old.info()["entries"] == 70 and blk.info()["entries"] == 100
    if close_old_first:
        old.close()
        same_as_fresh(engine, blk, p)
        blk.close()
    else:
        same_as_fresh(engine, blk, p)
        blk.close()
        assert [(summary(*answers(engine, old, q, limit)), 70) for q in QUERIES for limit in (0, 20)] == before
        old.close()
