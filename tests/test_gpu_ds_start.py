"""The narrow kernels' packed scan word (ds_word.hpp: duration code | carry | start second
relative to the block's base, decoded in pool_kernels.hpp unit_ends) against the oracle, record
by record and in order, on blocks built at the word's edges:

* three small blocks (513, 2300 and 3100 entries: ragged last units), each around its own hour,
  so each has its own base (median start second - 16383);
* starts planted at median - 16384 (one below the base: the start escape), - 16383 (the base),
  + 16383 (the window's last second), + 16384 (the escape value), at second 1 and 200 000 s
  after the median — as many below the median as above it, so the median stays where the
  offsets were measured from (checked from the entries alone);
* sub-second parts and durations either side of whole seconds (carry 0 and 1), whole ms +- 1 ns
  up to and past the duration code's 32767 ms (the end escape), end = 0 and ends before the start;
* one term column with three values.

Queries put one-second time ranges on the planted entries' exact start and end seconds and one
second either side, duration bounds on the code's edges, and all three filters at once, at limits
0 and 20, through the resident, the static and the claim-based pool kernel; tsg_metrics.path must
name a narrow kernel for every query inside the duration envelope (the other paths read the
exact columns and would pass without reading the word). That envelope ends at 4294 ms (bounds
from 2^32 - 1 ns take the other paths, search.hip), below the code's 32767 ms: the bounds at
31999 .. 32768 ms here check that those paths still answer alike, and the narrow kernels meet
the saturated code through the bounds up to 4294 ms (it passes every minimum, fails every
maximum) and through the end escape under the range queries. A WAL block is refreshed with starts
before its base and past its window (the delta is packed against the old base) and compared
with the oracle and a freshly opened twin (which has its own base); a clone answers as its source.

Reference: tempodb/search/pipeline.go:30-67."""
import gc
import os
import random
from contextlib import contextmanager

import pytest

from oracle import oracle as O
import tempo_amd as T
from tests.helpers import match_key, tsg_key, write_block

pytestmark = pytest.mark.gpu
MS, S = 10**6, 10**9
T0 = 1_700_000_000
SIZES = (513, 2300, 3100)
SUBS = (0, 1, S - 1)
DURS = [0, 1, S - 1, S, S + 1] + [m * MS + d for m in (999, 1000, 1001, 31999, 32000, 32766, 32767, 32768)
                                  for d in (-1, 0, 1)]
# planted entries: (sub-second part of the start, duration) — carry 0 and 1 with floor(dur / 1 s) 0
# and 1, and a saturated duration code
PLANT = [(0, 0), (S - 1, 1), (0, S - 1), (1, S), (S - 1, S - 1), (0, 40_000 * MS)]
BELOW = (-16384, -16383, None)   # None: start second 1
ABOVE = (16383, 16384, 200_000)


def _block_entries(n, hour0, seed):
    """-> (entries, median start second, [(start_s, end_s) of the planted entries])."""
    rng = random.Random(seed)
    m = n - (len(BELOW) + len(ABOVE)) * len(PLANT)
    cluster = []
    for i in range(m):
        start = (hour0 + rng.randrange(3600)) * S + SUBS[rng.randrange(3)]
        kind = rng.randrange(100)
        if kind < 2:
            end = 0
        elif kind < 4:
            end = start - rng.randrange(1, 10 * S)
        elif kind < 60:
            end = start + DURS[rng.randrange(len(DURS))]
        else:
            end = start + int(rng.lognormvariate(17.7, 1.5))
        cluster.append((start, end))
    med = sorted(s // S for s, _ in cluster)[m // 2]
    planted = []
    for off in BELOW + ABOVE:
        for sub, dur in PLANT:
            start = (1 if off is None else med + off) * S + sub
            planted.append((start, start + dur))
    both = cluster + planted
    rng.shuffle(both)
    # the packer's median (the element at sorted index n / 2) is the cluster's: the offsets hold
    assert sorted(s // S for s, _ in both)[n // 2] == med and len(both) == n
    ids = sorted({bytes(rng.getrandbits(8) for _ in range(16)) for _ in range(n + 8)})[:n]
    ents = [{"id": tid, "start": s, "end": e,
             "tags": {"k": ["v%d" % rng.randrange(3)], "root.service.name": ["svc"], "root.name": ["op"]}}
            for tid, (s, e) in zip(ids, both)]
    return ents, med, [(s // S, e // S) for s, e in planted]


@pytest.fixture(scope="module")
def blocks3(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("ds_start"))
    paths, meds, planted = [], [], []
    for i, n in enumerate(SIZES):
        ents, med, pl = _block_entries(n, T0 + 40_000 * i, 70 + i)
        paths.append(write_block(d, "s%d" % i, ents, page_size=64 << 10))
        meds.append(med)
        planted += pl
    return paths, meds, planted


def _queries(meds, planted):
    qs = []
    # range only: one-second windows on the planted starts and ends and one second either side
    xs = sorted({x + d for s, e in planted for x in (s, e) for d in (-1, 0, 1) if x + d > 0})
    qs += [dict(start=x, end=x) for x in xs]
    qs += [dict(start=m - 16384, end=m - 16383) for m in meds] + [dict(start=m + 16383, end=m + 16384) for m in meds]
    # duration only (sparse ones: every kernel keeps them in its record buffer)
    qs += [dict(min_ms=a, max_ms=b) for a, b in ((1000, 1000), (999, 999), (1001, 1001), (31999, 32000), (32766, 32767))]
    # a saturated code passes every minimum and fails every maximum (4294 ms: the narrow kernels' last)
    qs += [dict(max_ms=1), dict(min_ms=4000, max_ms=4294), dict(min_ms=4294), dict(max_ms=4294, start=1, end=2)]
    qs += [dict(min_ms=32767), dict(min_ms=32768)]  # (outside the envelope: the other paths, no path asserted)
    # range + duration + term
    for m in meds:
        qs.append(dict(min_ms=1, max_ms=4294, start=m - 300, end=m + 300, tags={"k": "v1"}))
        qs.append(dict(min_ms=999, max_ms=1001, start=m - 16384, end=m + 16384, tags={"k": "v2"}))
    qs.append(dict(max_ms=4294, start=1, end=2, tags={"k": "v"}))
    return qs


def _narrow(q):
    """Inside the narrow kernels' duration envelope (search.hip): bounds below 2^32 - 1 ns (larger
    ones read dur64) and up to the code's 32767 ms; the first is the tighter one, 4294 ms."""
    return all(q.get(k, 0) * MS < 2**32 - 1 and q.get(k, 0) <= 32767 for k in ("min_ms", "max_ms"))


def _req(q):
    return T.SearchRequest(tags=dict(q.get("tags", {})), min_duration_ms=q.get("min_ms", 0),
                           max_duration_ms=q.get("max_ms", 0), start=q.get("start", 0), end=q.get("end", 0))


def _oracle(oblocks, q, limit):
    exp, omet, st = O.search(oblocks, limit=limit, nthreads=1, **q)
    assert st == 0
    return [match_key(m) for m in exp], (omet["traces_inspected"], omet["bytes_inspected"], omet["blocks_inspected"],
                                         omet["blocks_skipped"])


def _engine(eng, blocks, q, limit):
    got, met = eng.search(blocks, T.Pipeline(_req(q)), limit=limit)
    return ([tsg_key(m) for m in got], (met.inspected_traces, met.inspected_bytes, met.inspected_blocks,
                                        met.skipped_blocks)), met.path


@pytest.fixture(scope="module")
def expected(blocks3):
    """The oracle's answers, computed once: [(query, limit, records and metrics)]."""
    paths, meds, planted = blocks3
    ob = [O.Block(p) for p in paths]
    out = [(q, limit, _oracle(ob, q, limit)) for q in _queries(meds, planted) for limit in (0, 20)]
    # the fixture does what it says: planted starts and ends are found, the seconds beside them are not
    hits = {q["start"]: len(r[0]) for q, limit, r in out if limit == 0 and set(q) == {"start", "end"} and q["start"] == q["end"]}
    for s, e in planted:
        assert hits[s] > 0 and hits[e] > 0
    assert any(n == 0 for n in hits.values())
    return out


@pytest.fixture(autouse=True)
def _alone():
    gc.collect()


@contextmanager
def _extra_engine(env=None, devices=None):
    env = env or {}
    for k, v in env.items():
        os.environ[k] = v
    try:
        e = T.Engine(devices=devices) if devices else T.Engine()
    finally:
        for k in env:
            del os.environ[k]
    try:
        yield e
    finally:
        e.close()


def _check(eng, paths, expected, path_ok):
    blocks = [eng.open_block(p) for p in paths]
    bad = []
    try:
        for q, limit, exp in expected:
            res, path = _engine(eng, blocks, q, limit)
            if res != exp:
                bad.append((q, limit, "%d records vs %d, metrics %r vs %r" % (len(res[0]), len(exp[0]), res[1], exp[1])))
            elif _narrow(q) and not path_ok(path, limit):
                bad.append((q, limit, "path %d" % path))
    finally:
        for b in blocks:
            b.close()
    assert not bad, "%d of %d cases: %r" % (len(bad), len(expected), bad[:6])


def _resident_ok(path, limit):
    narrow = path & (T.PATH_RESIDENT | T.PATH_PLAIN) != 0 and path & T.PATH_OTHER == 0
    return narrow and (limit != 0 or path & T.PATH_RESIDENT != 0)


# (tsg_metrics.path does not tell search_static_kernel from search_pool_kernel: which of the two a
# plain launch is rests on the engines' switches below — under 32 units per workgroup the static
# kernel by default, TSG_POOL_STATIC_UNITS=0 the pool kernel at every size, pool.hip pool_search. A
# limit query may be served by the resident kernel or a plain launch: both decode the word.)
def _plain_ok(path, limit):
    return path & T.PATH_PLAIN != 0 and path & (T.PATH_RESIDENT | T.PATH_OTHER) == 0


def test_resident_kernel(engine, blocks3, expected):
    _check(engine, blocks3[0], expected, _resident_ok)


def test_static_kernel(engine, blocks3, expected):
    """A second context on the device turns the resident kernel off: plain launches of
    search_static_kernel (a search this small is below the pool kernel's threshold)."""
    with _extra_engine(devices=[0]):
        _check(engine, blocks3[0], expected, _plain_ok)


def test_pool_kernel(engine, blocks3, expected):
    """search_pool_kernel at every size, every unit claimed from the device counter."""
    with _extra_engine({"TSG_POOL_SMALL": "0", "TSG_POOL_STATIC_UNITS": "0"}) as e:
        _check(e, blocks3[0], expected, _plain_ok)


def test_clone_answers_as_its_source(engine, blocks3, expected):
    paths = blocks3[0]
    src = [engine.open_block(p) for p in paths]
    clones = [b.clone(engine) for b in src]
    try:
        for q, limit, exp in expected:
            if not _narrow(q):
                continue
            a, pa = _engine(engine, src, q, limit)
            c, pc = _engine(engine, clones, q, limit)
            assert a == c == exp and _resident_ok(pa, limit) and _resident_ok(pc, limit), (q, limit, pa, pc)
    finally:
        for b in clones + src:
            b.close()


def test_wal_refresh_keeps_the_old_base(engine, tmp_path):
    """The first entries sit in one hour (base = their median - 16383). The appended ones start
    one second before that base, at it, on the window's last second, one past it, far before and
    far after, and there are more of them than first entries: a fresh open of the grown file has
    another median and another base. Both must answer as the oracle does."""
    rng = random.Random(11)
    ids = sorted({bytes(rng.getrandbits(8) for _ in range(16)) for _ in range(700)})
    rng.shuffle(ids)
    tags = lambda: {"k": ["v%d" % rng.randrange(3)], "root.service.name": ["svc"], "root.name": ["op"]}  # noqa: E731
    first = []
    for tid in ids[:200]:
        start = (T0 + rng.randrange(3600)) * S + SUBS[rng.randrange(3)]
        first.append({"id": tid, "start": start, "end": start + DURS[rng.randrange(len(DURS))], "tags": tags()})
    med = sorted(e["start"] // S for e in first)[len(first) // 2]
    base = med - 16383
    offs = (base - 1, base, base + 0x7ffe, base + 0x7fff, 1, base + 300_000, base + 40_000, base + 40_001)
    rest = []
    for i, tid in enumerate(ids[200:]):
        sub, dur = PLANT[i % len(PLANT)]
        start = offs[i % len(offs)] * S + sub
        rest.append({"id": tid, "start": start, "end": 0 if i % 50 == 7 else start + dur, "tags": tags()})
    d = os.path.join(str(tmp_path), "w")
    os.makedirs(d)
    p = os.path.join(d, T.wal_filename(T.ENC_SNAPPY))
    T.write_wal_search(p, first, T.ENC_SNAPPY)
    old = engine.open_wal_block(p)
    T.write_wal_search(p, first + rest, T.ENC_SNAPPY)
    blk, st = engine.refresh_wal_block(old, p)
    fresh = engine.open_wal_block(p)
    ob = [O.Block(p, wal=True)]
    try:
        assert st["mode"] == 1 and st["entries_added"] == len(rest)
        qs = [dict(start=x + dd, end=x + dd) for x in offs for dd in (-1, 0, 1, 2) if x + dd > 0]
        qs += [dict(start=base - 1, end=base + 0x7fff), dict(min_ms=1000, max_ms=1000), dict(min_ms=4000), dict(min_ms=32767),
               dict(min_ms=1, max_ms=4294, start=base + 0x7ffe, end=base + 40_000, tags={"k": "v1"})]
        for q in qs:
            for limit in (0, 20):
                exp = _oracle(ob, q, limit)
                a, pa = _engine(engine, [blk], q, limit)
                f, pf = _engine(engine, [fresh], q, limit)
                assert a == exp and f == exp, (q, limit, len(a[0]), len(f[0]), len(exp[0]))
                assert not _narrow(q) or (_resident_ok(pa, limit) and _resident_ok(pf, limit)), (q, limit, pa, pf)
    finally:
        fresh.close()
        blk.close()
        old.close()
