"""The narrow kernels' terms-first mode (pool_kernels.hpp load_unit / unit_mask with TF: the packed
scan word is loaded only by a lane one of whose four entries of a step passed every term) against
the oracle: every record field, the order and the metrics, with the mode forced off and forced on
(tsg_debug_set "terms_first" 0 / 1), through the resident, the static and the claim-based pool
kernel, at limits 0 and 20. The counter resident_counters()["terms_first_queries"] must show which
instance ran. Blocks hold at most 3000 entries. The query is {a: a1, b: b1}, 10..1000 ms,
[T0 + 100, T0 + 3000] unless a case says otherwise; an entry that is not mentioned fails the terms
and passes both filters.

* sizes: blocks of 1, 255, 256, 257, 511, 512, 513 and 1025 entries whose first, middle and last
  entries pass the terms: the block-end cut meets a gated step;
* positions: one block of 1500 entries, one query per position whose term only that entry passes:
  first and last entry of a step in lane 0 (0, 3, 256, 259) and in lane 63 (252, 255, 508, 511), the
  first entry of the second unit (512), the last valid entry of the cut unit (1499);
* filters: term-passing entries that fail exactly one filter: durations one ns either side of 10 ms
  and of 1000 ms, start seconds one either side of End, end seconds one either side of Start;
* escapes: term-passing entries with end = 0 (saturated code) and with a start 10 h from the
  block's median (outside the 15-bit window), asked with a range that holds them and one that does
  not; one lane's group of four holds an escaped entry that fails the terms and a plain one that
  passes them;
* none / all: no entry passes the terms (each value exists, never together); every entry passes
  them and the duration filter keeps five;
* blocks: ten blocks with ten dictionaries for a (a bitmap slot each; b's is shared: a launch has
  16 slots), one of them without key b (the host skips it); in test_auto_mode a WAL block refreshed
  in place (no per-set counts) among counted ones;
* dense: the first 600 entries all match (limit 20: unit_cap).

In auto mode (the default) a launch holding the refreshed WAL block keeps the default instance, the
same query over the counted blocks alone runs terms first (at the latest from its eighth query in
a row: a live launch of the default instance is not left for one query), and a conjunction most
entries pass does not."""
import gc
import os
import random

import pytest

from oracle import oracle as O
import tempo_amd as T
from tests.helpers import write_block
from tests.test_gpu_search import assert_parity
from tests.test_gpu_variants import extra_engine

pytestmark = pytest.mark.gpu
MS, S = 10**6, 10**9
T0 = 1_700_000_000
QS, QE = T0 + 100, T0 + 3000
SIZES = (1, 255, 256, 257, 511, 512, 513, 1025)
POSITIONS = (0, 3, 252, 255, 256, 259, 508, 511, 512, 1499)
FAR = T0 + 1000 + 36_000
BASE = dict(tags={"a": "a1", "b": "b1"}, min_ms=10, max_ms=1000, start=QS, end=QE)


def _entry(i, hit=False, start=None, end=None, dur=100 * MS, tags=None):
    start = (T0 + 1000) * S + i if start is None else start
    t = {"root.service.name": ["svc"], "root.name": ["op"], "a": ["a1" if hit else "a0"], "b": ["b1" if hit else "b0"]}
    t.update(tags or {})
    return {"id": i.to_bytes(16, "big"), "start": start, "end": start + dur if end is None else end, "tags": t}


def _blocks(d):
    out, queries = {}, {}
    out["sizes"] = [write_block(d, "n%d" % n, [_entry(i, hit=i in (0, n // 2, n - 1)) for i in range(n)]) for n in SIZES]
    queries["sizes"] = [BASE]
    out["positions"] = [write_block(d, "pos", [_entry(i, tags={"a": ["p%d" % i]} if i in POSITIONS else None) for i in range(1500)])]
    queries["positions"] = [dict(BASE, tags={"a": "p%d" % p, "b": "b0"}) for p in POSITIONS]
    # one filter failing at a time (positions spread over lanes and steps; 64..67 share a lane)
    ents = [_entry(i) for i in range(700)]
    durs = [10 * MS - 1, 10 * MS, 10 * MS + 1, 1000 * MS - 1, 1000 * MS, 1000 * MS + 1]
    for k, dur in enumerate(durs):
        ents[64 + k] = _entry(64 + k, hit=True, dur=dur)
    for k, sec in enumerate((QE - 1, QE, QE + 1)):  # start seconds around End
        ents[300 + 5 * k] = _entry(300 + 5 * k, hit=True, start=sec * S + 7)
    # end seconds around Start: QS - 1 (starts and ends inside that second), QS, QS + 1
    ents[520] = _entry(520, hit=True, start=(QS - 1) * S + 100 * MS, dur=50 * MS)
    ents[523] = _entry(523, hit=True, start=QS * S - 50 * MS)
    ents[526] = _entry(526, hit=True, start=(QS + 1) * S - 50 * MS)
    out["filters"] = [write_block(d, "filters", ents)]
    queries["filters"] = [BASE]
    # escapes
    ents = [_entry(i) for i in range(900)]
    ents[40] = _entry(40, hit=False, end=0)          # escaped, fails the terms ...
    ents[41] = _entry(41, hit=True)                   # ... beside a plain one that passes them
    ents[200] = _entry(200, hit=True, end=0)          # end escape, passes the terms
    ents[511] = _entry(511, hit=True, start=FAR * S, dur=70 * MS)     # start escape
    ents[512] = _entry(512, hit=True, start=FAR * S, dur=40_000 * MS)  # both
    ents[899] = _entry(899, hit=True, dur=40_000 * MS)                 # saturated duration
    out["escapes"] = [write_block(d, "escapes", ents)]
    queries["escapes"] = [BASE, dict(BASE, end=FAR + 10), dict(BASE, min_ms=0, max_ms=0, end=FAR + 10),
                          dict(tags=BASE["tags"], min_ms=5), dict(tags=BASE["tags"], start=FAR, end=FAR)]
    # no entry passes both terms; every entry passes them and the duration keeps five
    ents = [_entry(i, tags={"a": ["a1" if i % 2 else "a0"], "b": ["b0" if i % 2 else "b1"]}) for i in range(1100)]
    out["none"] = [write_block(d, "none", ents)]
    queries["none"] = [BASE]
    ents = [_entry(i, hit=True, dur=(100 if i in (0, 255, 256, 777, 1299) else 5) * MS) for i in range(1300)]
    out["all"] = [write_block(d, "all", ents)]
    queries["all"] = [BASE]
    # ten dictionaries for a; block 4 has no key b
    many = []
    for bi in range(10):
        ents = []
        for i in range(600 + 37 * bi):
            tags = {"a": ["a1" if i % (50 + bi) == bi else "x%d" % ((i + bi) % (3 + bi))],
                    "b": ["b1" if i % 3 != 1 else "y%d" % (i % 2)]}
            e = _entry(i, tags=tags)
            if bi == 4:
                del e["tags"]["b"]
            ents.append(e)
        many.append(write_block(d, "many%d" % bi, ents))
    out["blocks"] = many
    queries["blocks"] = [BASE, dict(BASE, tags={"a": "a1"})]
    out["dense"] = [write_block(d, "dense", [_entry(i, hit=i < 600) for i in range(2000)])]
    queries["dense"] = [BASE]
    return out, queries


def _wal(d):
    """A WAL file written in two steps: the first 300 entries, then 200 more (one passes a = a1)."""
    rng = random.Random(9)
    ents = []
    for i in range(500):
        e = _entry(i, tags={"a": ["a1" if i == 403 else "w%d" % (i % 5)], "b": ["b1" if i % 2 else "w0"]})
        e["id"] = bytes(rng.getrandbits(8) for _ in range(16))
        ents.append(e)
    os.makedirs(os.path.join(d, "wal"), exist_ok=True)
    path = os.path.join(d, "wal", T.wal_filename(T.ENC_SNAPPY))
    return path, ents[:300], ents


def _req(q):
    return T.SearchRequest(tags=dict(q.get("tags", {})), min_duration_ms=q.get("min_ms", 0),
                           max_duration_ms=q.get("max_ms", 0), start=q.get("start", 0), end=q.get("end", 0))


def _oracle(obs, q, limit):
    exp, omet, st = O.search(obs, tags=q.get("tags"), min_ms=q.get("min_ms", 0), max_ms=q.get("max_ms", 0),
                             start=q.get("start", 0), end=q.get("end", 0), limit=limit, nthreads=1)
    assert st == 0
    return exp, omet


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("terms_first"))
    sets, queries = _blocks(d)
    cases = []  # (set name, block slice, query, limit, expected records, expected metrics)
    for name, paths in sets.items():
        parts = [slice(i, i + 1) for i in range(len(paths))] if name == "sizes" else [slice(None)]
        for part in parts:
            obs = [O.Block(p) for p in paths[part]]
            for q in queries[name]:
                for limit in (0, 20):
                    cases.append((name, part, q, limit) + _oracle(obs, q, limit))
    count = lambda name, limit=0: [len(c[4]) for c in cases if c[0] == name and c[3] == limit]  # noqa: E731
    # the fixture does what it says
    assert count("sizes") == [len({0, n // 2, n - 1}) for n in SIZES]
    assert count("positions") == [1] * len(POSITIONS)
    assert count("filters") == [4 + 2 + 2]
    assert count("escapes") == [1, 2, 4, 5, 2]
    assert count("none") == [0] and count("all") == [5]
    assert count("dense") == [600] and count("dense", 20) == [20]
    assert all(n > 0 for n in count("blocks"))
    return sets, cases


@pytest.fixture(autouse=True)
def _alone():
    gc.collect()
    yield
    T.debug_set("terms_first", 2)


def _plain_ok(path):
    return path & T.PATH_PLAIN != 0 and path & (T.PATH_RESIDENT | T.PATH_OTHER) == 0


def _narrow_ok(path):
    return path & (T.PATH_RESIDENT | T.PATH_PLAIN) != 0 and path & T.PATH_OTHER == 0


def _check(eng, data, path_ok):
    sets, cases = data
    blocks = {name: [eng.open_block(p) for p in paths] for name, paths in sets.items()}
    bad = []
    try:
        for mode in (0, 1):
            T.debug_set("terms_first", mode)
            for name, part, q, limit, exp, omet in cases:
                c0 = eng.resident_counters()["terms_first_queries"]
                got, met = eng.search(blocks[name][part], T.Pipeline(_req(q)), limit=limit)
                ran = eng.resident_counters()["terms_first_queries"] - c0
                try:
                    assert_parity(got, met, exp, omet)
                    assert path_ok(met.path), "path %d" % met.path
                    assert (ran > 0) == (mode == 1), "terms-first launches %d in mode %d" % (ran, mode)
                except AssertionError as e:
                    bad.append((mode, name, part, q, limit, str(e)[:200]))
    finally:
        T.debug_set("terms_first", 2)
        for bl in blocks.values():
            for b in bl:
                b.close()
    assert not bad, "%d of %d cases: %r" % (len(bad), 2 * len(cases), bad[:4])


def test_resident_kernel(engine, data):
    _check(engine, data, _narrow_ok)


def test_static_kernel(engine, data):
    """A second context on the device turns the resident kernel off: plain launches of
    search_static_kernel (searches this small are below the pool kernel's threshold)."""
    with extra_engine(devices=[0]):
        _check(engine, data, _plain_ok)


def test_pool_kernel(data):
    """search_pool_kernel at every size, every unit claimed from the device counter."""
    with extra_engine({"TSG_POOL_SMALL": "0", "TSG_POOL_STATIC_UNITS": "0"}) as e:
        _check(e, data, _plain_ok)


def test_shapes_without_the_mode_keep_their_instances(engine, data):
    """No duration or range filter, or no term: forcing the mode changes nothing (the instance does
    not exist), and the answers are the oracle's."""
    sets, _ = data
    obs = [O.Block(p) for p in sets["blocks"]]
    blocks = [engine.open_block(p) for p in sets["blocks"]]
    try:
        T.debug_set("terms_first", 1)
        for q in (dict(tags={"a": "a1", "b": "b1"}), dict(min_ms=10, max_ms=1000, start=QS, end=QE)):
            c0 = engine.resident_counters()["terms_first_queries"]
            got, met = engine.search(blocks, T.Pipeline(_req(q)), limit=20)
            assert_parity(got, met, *_oracle(obs, q, 20))
            assert engine.resident_counters()["terms_first_queries"] == c0
    finally:
        T.debug_set("terms_first", 2)
        for b in blocks:
            b.close()


def test_auto_mode(engine, data, tmp_path):
    """The choice from the counts: a sparse conjunction over counted blocks runs terms first; the
    same launch with a refreshed WAL block (no counts) among them does not; a conjunction most
    entries pass does not. The answers are the oracle's either way."""
    sets, _ = data
    wpath, first, every = _wal(str(tmp_path))
    T.write_wal_search(wpath, first, T.ENC_SNAPPY)
    old = engine.open_wal_block(wpath)
    T.write_wal_search(wpath, every, T.ENC_SNAPPY)
    wal, st = engine.refresh_wal_block(old, wpath)
    assert st["mode"] == 1 and st["entries_added"] == 200
    fresh = engine.open_wal_block(wpath)  # (the same entries, counted at load)
    # a = a1 passes 1 entry in 3000 and b = b1 two in three: p = 2.2e-4, a step in 18 holds a pass
    paths = []
    for k in range(3):
        ents = [_entry(i, tags={"a": ["a1" if i == 1000 * k + 1 else "a0"], "b": ["b1" if i % 3 != 2 else "b0"]})
                for i in range(3000)]
        ents[7] = _entry(7, dur=500 * MS)  # (the block's longest, without key b: `common` passes the header only)
        del ents[7]["tags"]["b"]
        paths.append(write_block(str(tmp_path), "auto%d" % k, ents))
    counted = [engine.open_block(p) for p in paths]
    ob = [O.Block(p) for p in paths] + [O.Block(wpath, wal=True)]
    sparse = BASE
    common = dict(BASE, tags={"b": "b"}, min_ms=300)  # every entry with the key passes the term, none the duration
    try:
        T.debug_set("terms_first", 2)
        T.debug_set("groups", 2)  # (18 units over 2 workgroups: the planner leaves launches of < 8 units per workgroup alone)
        for blocks, obs, q, want in ((counted, ob[:3], sparse, True), (counted + [wal], ob, sparse, False),
                                     (counted + [fresh], ob, sparse, True), (counted, ob[:3], common, False)):
            # (a live launch of the default instance is left for terms first only after several
            # queries in a row asked for it; the default instance is taken at once)
            for rep in range(10 if want else 1):
                c0 = engine.resident_counters()["terms_first_queries"]
                got, met = engine.search(blocks, T.Pipeline(_req(q)), limit=0)
                assert_parity(got, met, *_oracle(obs, q, 0))
                assert _narrow_ok(met.path)
            assert (engine.resident_counters()["terms_first_queries"] > c0) == want, (len(blocks), q)
        T.debug_set("groups", 0)  # over every CU the same launch is a unit or none per workgroup: left alone
        c0 = engine.resident_counters()["terms_first_queries"]
        for rep in range(10):
            got, met = engine.search(counted, T.Pipeline(_req(sparse)), limit=0)
        assert_parity(got, met, *_oracle(ob[:3], sparse, 0))
        assert engine.resident_counters()["terms_first_queries"] == c0
        for mode in (0, 1):  # the refreshed block among counted ones, forced either way
            T.debug_set("terms_first", mode)
            for limit in (0, 20):
                c0 = engine.resident_counters()["terms_first_queries"]
                got, met = engine.search(counted + [wal], T.Pipeline(_req(sparse)), limit=limit)
                assert_parity(got, met, *_oracle(ob, sparse, limit))
                assert (engine.resident_counters()["terms_first_queries"] > c0) == (mode == 1)
    finally:
        T.debug_set("terms_first", 2)
        T.debug_set("groups", 0)
        for b in counted + [wal, fresh, old]:
            b.close()
