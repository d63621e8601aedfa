"""The resident kernel's unit loop past a wave's first two units (pool_kernels.hpp
search_resident_kernel: the peeled steady state with unconditional loads, then the rolled loop for
the last units), and unit_mask's escape reloads gated on the lanes that can still match.

A workgroup's twelve waves take their first two units each without a claim, so a workgroup's run
must be longer than 24 units before a claimed unit is scanned at all: with every CU a workgroup no
test block is that large. tsg_debug_set("groups", G) plans for G workgroups, and small blocks give
long runs. Every result is compared with the oracle: all fields of every record, in order, and
the four metrics; tsg_metrics.path must be PATH_RESIDENT alone (a fallback to another path would
pass the comparison without running the loop).

* run lengths: one block, 8 workgroups, runs of 1, 11, 12, 13, 23, 24, 25, 26 and 49 units (no
  steady loop / one stream only / exactly two units per wave / the first claim / several steady
  trips), whole and with a partial last unit, and one size whose runs differ by a unit;
* three blocks of unequal size whose boundaries fall among the claimed units of runs of 26 and
  27 units;
* where matches lie (checked from the oracle's records alone): in a wave's first two units, in a
  claimed unit, in the run's last unit, two in one lane of one unit; no workgroup past the LDS
  record buffer; a limit-20 query;
* escapes: a block with escaped starts, saturated durations and end = 0 entries, of which some
  pass the terms and the duration and some fail them, through the resident, the static and the
  pool kernel;
* back to back: two run lengths alternating for 20 queries on one resident launch.

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
UNIT, GROUPS, WAVES = 512, 8, 12
REC_CAP = 2048              # records a workgroup's LDS buffer holds
RUNS = (1, 11, 12, 13, 23, 24, 25, 26, 49)
# three terms, a duration and a time range: the main line's kernel instance. About 1.4 % of the
# synthetic entries match (svc-07 is one service of 50), 0.17 % with the method as well.
DENSE = dict(tags={"service.name": "svc-07", "status.code": "0", "error": "false"}, min_ms=1, max_ms=4000,
             start=T0 + 300, end=T0 + 3300)
SPARSE = dict(tags={"service.name": "svc-07", "status.code": "0", "http.method": "get"}, min_ms=1, max_ms=4000,
              start=T0 + 300, end=T0 + 3300)


def _req(q):
    return T.SearchRequest(tags=dict(q.get("tags", {})), min_duration_ms=q.get("min_ms", 0),
                           max_duration_ms=q.get("max_ms", 0), start=q.get("start", 0), end=q.get("end", 0))


def _oracle(paths, q, limit=0):
    exp, omet, st = O.search([O.Block(p) for p in paths], limit=limit, nthreads=1, **q)
    assert st == 0
    return [match_key(m) for m in exp], (omet["traces_inspected"], omet["bytes_inspected"], omet["blocks_inspected"],
                                         omet["blocks_skipped"])


def _engine(eng, blocks, q, limit=0):
    got, met = eng.search(blocks, T.Pipeline(_req(q)), limit=limit)
    return ([tsg_key(m) for m in got], (met.inspected_traces, met.inspected_bytes, met.inspected_blocks,
                                        met.skipped_blocks)), met.path


@pytest.fixture(autouse=True)
def _alone():
    gc.collect()


@contextmanager
def _groups(n):
    T.debug_set("groups", n)
    try:
        yield
    finally:
        T.debug_set("groups", 0)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """Synthetic blocks by entry count, written once each."""
    d = tmp_path_factory.mktemp("inflight")
    made = {}

    def get(n):
        if n not in made:
            made[n] = str(d / ("n%d" % n))
            T.synth_search_block(made[n], n, seed=900 + len(made), profile=0, encoding=T.ENC_SNAPPY)
        return made[n]
    return get


def _check_resident(eng, paths, cases):
    """cases: (query, limit). Every answer the oracle's, from the resident kernel alone."""
    blocks = [eng.open_block(p) for p in paths]
    bad = []
    try:
        for q, limit in cases:
            exp = _oracle(paths, q, limit)
            res, path = _engine(eng, blocks, q, limit)
            if res != exp:
                bad.append((q, limit, "%d records vs %d, metrics %r vs %r" % (len(res[0]), len(exp[0]), res[1], exp[1])))
            elif path != T.PATH_RESIDENT:
                bad.append((q, limit, "path %d" % path))
    finally:
        for b in blocks:
            b.close()
    assert not bad, "%d of %d cases: %r" % (len(bad), len(cases), bad[:4])


def _runs(units, groups=GROUPS):
    """The workgroups' unit runs [(first unit, length)] (pool.hip: wq, wr)."""
    wq, wr = divmod(units, groups)
    return [(w * wq + min(w, wr), wq + (w < wr)) for w in range(groups)]


@pytest.mark.parametrize("nk", RUNS)
def test_run_lengths(engine, synth, nk):
    """Every workgroup scans nk units; minus 300 entries the last workgroup's last unit is partial."""
    with _groups(GROUPS):
        for n in (GROUPS * nk * UNIT, GROUPS * nk * UNIT - 300):
            assert all(r[1] == nk for r in _runs((n + UNIT - 1) // UNIT))
            _check_resident(engine, [synth(n)], [(DENSE, 0), (SPARSE, 0)])


def test_runs_differ_by_one_unit(engine, synth):
    """203 units over 8 workgroups: three runs of 26 units, five of 25 (wr = 3)."""
    n = (GROUPS * 25 + 3) * UNIT - 77
    assert sorted({r[1] for r in _runs((n + UNIT - 1) // UNIT)}) == [25, 26]
    with _groups(GROUPS):
        _check_resident(engine, [synth(n)], [(DENSE, 0), (SPARSE, 0)])


def test_block_boundaries_inside_runs(engine, synth):
    """52 + 105 + 53 units, each block's last unit partial: runs of 27 and 26 units, and the blocks'
    first units (52 and 157) are claimed units of the second and the sixth workgroup's runs: a
    wave's block walk moves on in the steady loop's loads."""
    sizes = (51 * UNIT + 100, 104 * UNIT + 300, 52 * UNIT + 17)
    ub = [0]
    for n in sizes:
        ub.append(ub[-1] + (n + UNIT - 1) // UNIT)
    runs = _runs(ub[-1])
    assert min(r[1] for r in runs) >= 25
    for edge in ub[1:-1]:
        assert any(a + 2 * WAVES <= edge < a + n for a, n in runs), (edge, runs)
    with _groups(GROUPS):
        _check_resident(engine, [synth(n) for n in sizes], [(DENSE, 0), (SPARSE, 0), (DENSE, 20)])


def test_where_matches_lie(engine, synth):
    """Runs of 49 units. From the oracle's records alone: matches in a wave's first two units, in
    claimed units and in a run's last unit, two of them in one lane of a unit, and no workgroup
    with more records than its LDS buffer holds (the host would rerun the query elsewhere)."""
    nk = 49
    n = GROUPS * nk * UNIT - 300
    path = synth(n)
    pos = [k[1] for k in _oracle([path], DENSE)[0]]  # scan positions
    runs = _runs((n + UNIT - 1) // UNIT)
    per_wg = [sum(1 for p in pos if a <= p // UNIT < a + ln) for a, ln in runs]
    assert max(per_wg) <= REC_CAP and min(per_wg) > 0, per_wg
    place = {"first_two": 0, "claimed": 0, "last": 0}
    for p in pos:
        k = p // UNIT % nk  # (every run is nk units)
        place["first_two" if k < 2 * WAVES else "claimed"] += 1
        place["last"] += k == nk - 1
    assert all(place.values()), place
    lanes = {}
    for p in pos:  # lane l of a unit holds its entries 4l .. 4l + 3 and 256 + 4l .. 256 + 4l + 3
        key = (p // UNIT, p % 256 // 4)
        lanes[key] = lanes.get(key, 0) + 1
    assert max(lanes.values()) >= 2
    assert len(_oracle([path], DENSE, 20)[0]) == 20
    with _groups(GROUPS):
        _check_resident(engine, [path], [(DENSE, 0), (SPARSE, 0), (DENSE, 20), (SPARSE, 20)])


def test_back_to_back_run_lengths(engine, synth):
    """Runs of 49 and 13 units in turn, 20 queries on one resident launch: the per-unit tables in
    LDS are reused, and a count left by the long run's units would show in the short one's."""
    paths = [synth(GROUPS * 49 * UNIT - 300), synth(GROUPS * 13 * UNIT)]
    exp = [_oracle([p], DENSE) for p in paths]
    assert all(len(e[0]) for e in exp)
    blocks = [engine.open_block(p) for p in paths]
    try:
        with _groups(GROUPS):
            assert _engine(engine, [blocks[0]], DENSE)[0] == exp[0]  # (the launch for 8 workgroups is up)
            c0 = engine.resident_counters()
            for i in range(20):
                res, path = _engine(engine, [blocks[i & 1]], DENSE)
                assert res == exp[i & 1] and path == T.PATH_RESIDENT, (i, len(res[0]), path)
            c1 = engine.resident_counters()
            assert c1["queries"] - c0["queries"] == 20 and c1["launches"] == c0["launches"], (c0, c1)
    finally:
        for b in blocks:
            b.close()


# ---- escapes ------------------------------------------------------------------------------------
# One workgroup (groups = 1), 27 units and a partial 28th: a wave's first two units, claimed units
# and steady trips all hold escaped words. The block is built as tests/test_gpu_ds_start.py builds
# its own: a cluster of starts inside one hour (the block's base is its median - 16383), planted
# starts outside the word's 15-bit window on both sides in equal numbers (the median stays), end = 0,
# ends before the start and durations either side of the code's 32767 ms.
ESC_N = 27 * UNIT + 200
ESC_DURS = [0, 1, 999 * MS, 1000 * MS, 1001 * MS, 2 * S, 3 * S + 1, 32767 * MS, 32768 * MS, 40_000 * MS, 70_000 * S]
ESC_BELOW = (-16384, -20000, None)  # None: start second 1
ESC_ABOVE = (16384, 20000, 200_000)
ESC_COPIES = 40  # of each planted (offset, duration) pair, with the three values of the term in turn


def _escape_entries():
    rng = random.Random(1234)
    planted = []
    for c in range(ESC_COPIES):
        for off in ESC_BELOW + ESC_ABOVE:
            for i, dur in enumerate(ESC_DURS):
                start = (1 if off is None else T0 + 1800 + off) * S + (0, 1, S - 1)[(c + i) % 3]
                planted.append((start, start + dur, "v%d" % ((c + i) % 3)))
    cluster = []
    for i in range(ESC_N - len(planted)):
        start = (T0 + rng.randrange(3600)) * S + (0, 1, S - 1)[rng.randrange(3)]
        kind = rng.randrange(100)
        if kind < 3:
            end = 0
        elif kind < 6:
            end = start - rng.randrange(1, 10 * S)
        elif kind < 40:
            end = start + ESC_DURS[rng.randrange(len(ESC_DURS))]
        else:
            end = start + int(rng.lognormvariate(17.7, 1.5))
        cluster.append((start, end, "v%d" % rng.randrange(3)))
    both = cluster + planted
    rng.shuffle(both)
    ids = sorted({bytes(rng.getrandbits(8) for _ in range(16)) for _ in range(ESC_N + 8)})[:ESC_N]
    ents = [{"id": tid, "start": s, "end": e, "tags": {"k": [v], "root.service.name": ["svc"], "root.name": ["op"]}}
            for tid, (s, e, v) in zip(ids, both)]
    return ents, both


def _escape_queries(med):
    far = [1 if off is None else T0 + 1800 + off for off in ESC_BELOW + ESC_ABOVE]
    qs = []
    for x in far:
        # the escaped starts' seconds and the seconds their ends fall in: the exact columns decide,
        # for the entries whose term and duration pass; v2 and the 2 .. 4 s band fail the others
        qs.append(dict(start=x, end=x, tags={"k": "v1"}))
        qs.append(dict(start=x - 1, end=x + 40, min_ms=999, max_ms=1001, tags={"k": "v0"}))
        qs.append(dict(start=x + 30, end=x + 41, min_ms=4000, tags={"k": "v2"}))  # saturated codes pass a minimum
        qs.append(dict(start=x, end=x + 3, min_ms=2000, max_ms=4000))
    # inside the window: end = 0 and ends before the start fail the range, whatever the term says
    qs.append(dict(start=med - 200, end=med + 200, min_ms=4000, tags={"k": "v1"}))
    qs.append(dict(start=med - 200, end=med + 200, min_ms=1000, max_ms=1000, tags={"k": "v0"}))
    qs.append(dict(start=med - 16384, end=med - 16383))
    qs.append(dict(start=med + 16383, end=med + 16384, tags={"k": "v"}))
    qs.append(dict(start=1, end=2, max_ms=4294, tags={"k": "v"}))
    qs.append(dict(start=100, end=200, min_ms=999, max_ms=1001))  # (nothing: the long spans over it fail the duration)
    return qs


@pytest.fixture(scope="module")
def escapes(tmp_path_factory):
    """-> (block path, [(query, limit, the oracle's answer)])."""
    ents, both = _escape_entries()
    path = write_block(str(tmp_path_factory.mktemp("inflight_esc")), "esc", ents, page_size=64 << 10)
    med = sorted(s // S for s, _, _ in both)[ESC_N // 2]
    assert T0 <= med < T0 + 3600  # (the planted starts left the median in the cluster)
    base = med - 16383
    esc_start = [s // S - base not in range(0x7fff) for s, _, _ in both]
    esc_end = [not 0 <= e - s < 32768 * MS for s, e, _ in both]
    assert sum(esc_start) >= 6 * ESC_COPIES * len(ESC_DURS) and sum(esc_end) > ESC_N // 20
    out = [(q, limit, _oracle([path], q, limit)) for q in _escape_queries(med) for limit in (0, 20)]
    full = [r[0] for q, limit, r in out if limit == 0]
    assert sum(1 for r in full if r) >= len(full) // 2 and any(not r for r in full)
    assert max(len(r) for r in full) <= REC_CAP
    # escaped entries among the records, in a wave's first two units and in claimed ones
    hit = {p // UNIT >= 2 * WAVES for r in full for p in (k[1] for k in r)}
    assert hit == {False, True}
    return path, out


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


def _plain(p):
    return p & T.PATH_PLAIN != 0 and p & (T.PATH_RESIDENT | T.PATH_OTHER) == 0


def _check_escapes(eng, escapes, path_ok):
    path, cases = escapes
    blk = eng.open_block(path)
    bad = []
    try:
        with _groups(1):
            for q, limit, exp in cases:
                res, p = _engine(eng, [blk], q, limit)
                if res != exp:
                    bad.append((q, limit, "%d records vs %d, metrics %r vs %r" % (len(res[0]), len(exp[0]), res[1], exp[1])))
                elif not path_ok(p):
                    bad.append((q, limit, "path %d" % p))
    finally:
        blk.close()
    assert not bad, "%d of %d cases: %r" % (len(bad), len(cases), bad[:4])


def test_escapes_resident(engine, escapes):
    _check_escapes(engine, escapes, lambda p: p == T.PATH_RESIDENT)


def test_escapes_static_kernel(engine, escapes):
    """A second context on the device turns the resident kernel off: a plain launch, of
    search_static_kernel at this size (28 units are below the pool kernel's threshold)."""
    with _extra_engine(devices=[0]):
        _check_escapes(engine, escapes, _plain)


def test_escapes_pool_kernel(engine, escapes):
    """search_pool_kernel at every size, every unit claimed from the device counter."""
    with _extra_engine({"TSG_POOL_SMALL": "0", "TSG_POOL_STATIC_UNITS": "0"}) as e:
        _check_escapes(e, escapes, _plain)
