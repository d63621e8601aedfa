"""The narrow kernels' short predicate forms (ds_word.hpp; pool_kernels.hpp unit_mask and
stage_term_tables) against the oracle, record by record and in order, through the resident, the
static and the claim-based pool kernel, at limits 0 and 20 (cap_unit_mask after the new mask):

* blocks of 1, 511, 512, 513 and 1025 entries in which every entry matches: a partial last unit,
  exactly full units, a one-entry tail (the per-unit validity mask);
* three blocks in one launch whose dictionaries for key "k" differ (several bitmap slots, another
  table per block), one of them without the key (the host skips it), and in the other two every
  fifth entry without the key: the all-ones id 255 in a column whose dictionary has the key, where
  x < ns is false;
* a key with 254 value sets queried for the value of its last set and for a needle in no set;
* three terms of which exactly one fails per entry, each in turn;
* duration bounds 10 / 1000 ms with entries one nanosecond either side of each, min only, max
  only, min > max (nothing);
* the range's two inclusive edges (start second = the query's end, end second = the query's
  start), their neighbours one second off, and durations whose carry bit is 1;
* both escapes beside ordinary entries in one lane's group of four: end = 0, a 40 s duration, a
  start 10 h from the median.

Cases the issue lists with 255 value sets use 254 here: 255 sets make the column two bytes wide
(block.hpp KeyColumn::width) and the narrow scan declines it. Reference: tempodb/search/pipeline.go:30-67."""
import gc
import random

import pytest

from oracle import oracle as O
import tempo_amd as T
from tests.helpers import match_key, tsg_key, write_block
from tests.test_gpu_variants import extra_engine

pytestmark = pytest.mark.gpu
MS, S = 10**6, 10**9
T0 = 1_700_000_000
SIZES = (1, 511, 512, 513, 1025)


def _ids(rng, n):
    return sorted({bytes(rng.getrandbits(8) for _ in range(16)) for _ in range(n + 8)})[:n]


def _entry(tid, start, end, tags):
    t = {"root.service.name": ["svc"], "root.name": ["op"]}
    t.update(tags)
    return {"id": tid, "start": start, "end": end, "tags": t}


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("scan_pred"))
    rng = random.Random(5)
    out = {}
    # every entry matches {k: v1}, 100 ms, inside the hour
    out["sizes"] = [write_block(d, "n%d" % n, [_entry(t, (T0 + i % 3600) * S + i, (T0 + i % 3600) * S + i + 100 * MS,
                                                     {"k": ["v1"], "a": ["a1"], "b": ["b1"]})
                                              for i, t in enumerate(_ids(rng, n))]) for n in SIZES]
    # three dictionaries for k: another value order, and a block without the key
    dicts = []
    for bi, vals in enumerate((["v0", "v1", "v2"], ["v2", "zz", "v1", "v0", "yy"], None)):
        ents = []
        for i, t in enumerate(_ids(rng, 700)):
            tags = {"o": ["o%d" % (i % 2)]}
            if vals and i % 5 != 3:  # (every fifth entry of a block that has the key lacks it)
                tags["k"] = [vals[(i * 7 + bi) % len(vals)]]
            ents.append(_entry(t, (T0 + i) * S, (T0 + i) * S + 50 * MS, tags))
        dicts.append(write_block(d, "d%d" % bi, ents))
    out["dicts"] = dicts
    # 254 value sets; three terms failing one at a time; the duration, range and escape edges
    ents = []
    durs = [10 * MS - 1, 10 * MS, 10 * MS + 1, 1000 * MS - 1, 1000 * MS, 1000 * MS + 1, 0, 5 * MS, 1500 * MS, 40_000 * MS]
    for i, t in enumerate(_ids(rng, 1300)):
        tags = {"v": ["v%03d" % (i % 254)], "a": ["a1" if i % 4 != 1 else "a0"], "b": ["b1" if i % 4 != 2 else "b0"],
                "c": ["c1" if i % 4 != 3 else "c0"]}
        sec, sub = T0 + 1000 + (i % 7) - 3, (0, 1, S - 1)[i % 3]
        start = sec * S + sub
        end = start + durs[i % len(durs)]
        if i % 97 == 5:
            end = 0                      # end escape beside ordinary entries
        if i % 101 == 6:
            start, end = (T0 + 1000 + 36_000) * S, (T0 + 1000 + 36_000) * S + 7 * MS  # start escape
        if i % 89 == 3:
            end = start + (S - sub)      # ends on the next second: carry 1 with floor(dur / 1 s) = 0
        ents.append(_entry(t, start, end, tags))
    out["edges"] = [write_block(d, "edges", ents)]
    return out


QUERIES = {
    "sizes": [dict(tags={"k": "v1"}), dict(tags={"k": "v1", "a": "a1", "b": "b1"}, min_ms=100, max_ms=100, start=T0, end=T0 + 3600)],
    "dicts": [dict(tags={"k": "v1"}), dict(tags={"k": "v"}), dict(tags={"k": "zz"}), dict(tags={"k": "nope"}),
              dict(tags={"k": "v0", "o": "o1"}, max_ms=50, start=T0 + 10, end=T0 + 600)],
    "edges": [dict(tags={"v": "v253"}), dict(tags={"v": "v254"}), dict(tags={"v": "v000"}),
              dict(tags={"a": "a1", "b": "b1", "c": "c1"}), dict(tags={"a": "a0", "b": "b1", "c": "c1"}),
              dict(tags={"a": "a1", "b": "b0", "c": "c1"}), dict(tags={"a": "a1", "b": "b1", "c": "c0"}),
              dict(min_ms=10, max_ms=1000), dict(min_ms=10), dict(max_ms=1000), dict(min_ms=1000, max_ms=10),
              dict(min_ms=10, max_ms=1000, tags={"a": "a1"}, start=T0 + 999, end=T0 + 1001)] +
             [dict(start=T0 + 1000 + a, end=T0 + 1000 + b) for a in (-4, -3, 0, 3, 4, 5) for b in (a, a + 1)] +
             [dict(start=1, end=2), dict(start=T0 + 1000 + 36_000, end=T0 + 1000 + 36_000), dict(start=T0, end=T0 + 1000 + 35_999)],
}


def _part(name):
    """"sizes:2" is the third block of the set alone (every entry matches: one block at a time keeps a
    workgroup's matches inside its 2048-record buffer, so the narrow kernel's answer is the one kept)."""
    return slice(int(name.split(":")[1]), int(name.split(":")[1]) + 1) if ":" in name else slice(None)


def _req(q):
    return T.SearchRequest(tags=dict(q.get("tags", {})), min_duration_ms=q.get("min_ms", 0),
                           max_duration_ms=q.get("max_ms", 0), start=q.get("start", 0), end=q.get("end", 0))


@pytest.fixture(scope="module")
def expected(sets):
    out = []
    cases = [(n, qs) for n, qs in QUERIES.items() if n != "sizes"] + [("sizes:%d" % i, QUERIES["sizes"]) for i in range(len(SIZES))]
    for name, qs in cases:
        ob = [O.Block(p) for p in sets[name.split(":")[0]][_part(name)]]
        for q in qs:
            for limit in (0, 20):
                exp, omet, st = O.search(ob, limit=limit, nthreads=1, **q)
                assert st == 0
                out.append((name, q, limit, ([match_key(m) for m in exp], omet["traces_inspected"])))
    # the fixture does what it says: every entry of the size blocks matches, some edge query is empty
    assert [len(r[0]) for n, q, l, r in out if n.startswith("sizes") and l == 0] == [n for n in SIZES for _ in range(2)]
    assert any(not r[0] for n, q, l, r in out if n == "edges") and any(r[0] for n, q, l, r in out if n == "edges")
    return out


@pytest.fixture(autouse=True)
def _alone():
    gc.collect()


def _check(eng, sets, expected, path_ok):
    blocks = {name: [eng.open_block(p) for p in sets[name.split(":")[0]][_part(name)]] for name in {e[0] for e in expected}}
    bad = []
    try:
        for name, q, limit, exp in expected:
            got, met = eng.search(blocks[name], T.Pipeline(_req(q)), limit=limit)
            res = ([tsg_key(m) for m in got], met.inspected_traces)
            if res != exp:
                bad.append((name, q, limit, "%d records vs %d" % (len(res[0]), len(exp[0]))))
            elif not path_ok(met.path, limit) and not (met.path == 0 and not exp[0]):  # (no value holds the needle: no launch)
                bad.append((name, q, limit, "path %d" % met.path))
    finally:
        for bl in blocks.values():
            for b in bl:
                b.close()
    assert not bad, "%d of %d cases: %r" % (len(bad), len(expected), bad[:6])


def _resident_ok(path, limit):
    narrow = path & (T.PATH_RESIDENT | T.PATH_PLAIN) != 0 and path & T.PATH_OTHER == 0
    return narrow and (limit != 0 or path & T.PATH_RESIDENT != 0)


def _plain_ok(path, limit):
    return path & T.PATH_PLAIN != 0 and path & (T.PATH_RESIDENT | T.PATH_OTHER) == 0


def test_resident_kernel(engine, sets, expected):
    _check(engine, sets, expected, _resident_ok)


def test_static_kernel(engine, sets, expected):
    """A second context on the device turns the resident kernel off: plain launches of
    search_static_kernel (searches this small are below the pool kernel's threshold)."""
    with extra_engine(devices=[0]):
        _check(engine, sets, expected, _plain_ok)


def test_pool_kernel(engine, sets, expected):
    """search_pool_kernel at every size, every unit claimed from the device counter."""
    with extra_engine({"TSG_POOL_SMALL": "0", "TSG_POOL_STATIC_UNITS": "0"}) as e:
        _check(e, sets, expected, _plain_ok)
