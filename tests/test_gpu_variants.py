"""Every narrow-scan kernel instance against the oracle, on hand-built edge blocks.

The narrow scan is three kernels in pool_kernels.hpp (search_resident_kernel, search_static_kernel,
search_pool_kernel), each a template over <NT 0..4, DUR, RANGE, NTL>: 40 instances per kernel,
picked on the host by the query's shape (pool.hip with_shape: pool_fn, kernel_symbol). This file
asks for each of the 20 (NT, DUR, RANGE) shapes on purpose and asserts, through
tsg_metrics.path, which kind of kernel served it.

Instances run here (100 of the 120):
- search_resident_kernel <NT, DUR, RANGE, NTL=true>, all 20 shapes (the session engine, alone
  on the device), at the device's workgroup count and at 1 and 3 workgroups;
- search_static_kernel, all 40: NTL=true on the session engine while a second context is open
  (the resident kernel is then off), NTL=false on an engine started with TSG_POOL_NT=0;
- search_pool_kernel, all 40: engines started with TSG_POOL_SMALL=0 TSG_POOL_STATIC_UNITS=0
  (every unit claimed from the device counter), with and without TSG_POOL_NT=0.
Left out: the 20 search_resident_kernel <.., NTL=false> instances. They need a lone engine
started with TSG_POOL_NT=0, and the session's engine (default loads) is open for the whole run.
(Their unit load, ranks and record store are the shared helpers load_unit, unit_ranks and put_rec
that the 100 instances above run.)
The same shapes also run on the fast kernel (TSG_NO_POOL=1) and the general path (TSG_NO_FAST=1).

The fixture (tests/helpers.py write_edge_blocks): 8 blocks of 1, 7, 511, 512, 513, 1025, 4096
and 4097 entries, the low 8 bytes of an id = the big-endian scan position. A lane of a 512-entry unit holds entries
e0 + 256k + 4 lane + j; the hit set H puts matches on positions 0..9, 250..262 (the step boundary),
505..520 (the unit boundary), 511 alone, 255 and 256 alone, the last three entries of every block,
and a run of 700 consecutive entries (one unit matched whole). Inside H single entries fail
exactly one term, sit at / 1 ns under / 1 ns over the whole-ms duration bounds, on the time
range's edges, or take the span escape (end = 0, a span over 65535 s). Outside H term a fails.

Column widths (block.cpp KeyColumn::width: one byte while the key has fewer than 255 value
sets, since code 255 is the absent entry; an absent key adds no set):
- a..e: 2..4 value sets each: one byte;
- v ("v%03d" % (pos % 254)): 254 sets in the blocks of 511 entries and more: the largest
  one-byte dictionary (set ids 0..253, bits in every word of the 256-bit map);
- w ("w%03d" % (pos % 255)): 255 sets there: the first 16-bit column (narrow scan declines);
- x (256 values): 16 bits.

Nothing expected is derived from the code under test: the checker is oracle/ (all integer
work, bit-exact parity). Reference anchor: tempodb/search/backend_search_block.go:184-298,
tempodb/search/pipeline.go:26-157.
"""
import gc
import os
from contextlib import contextmanager

import pytest

from oracle import oracle as O
import tempo_amd as T
from tests import helpers as H
from tests.helpers import match_key, tsg_key

pytestmark = pytest.mark.gpu

SHAPES = [(nt, dur, rng) for nt in range(5) for dur in (False, True) for rng in (False, True)]
LIMITS = (0, 1, 3, 5, 20)
REC_CAP = 2048  # records a workgroup's LDS buffer holds (pool.hip: 96 KiB of 48-byte records)


def shape_query(nt, dur, rng, terms=H.EDGE_TERMS):
    q = dict(tags=dict(terms[:nt]))
    if dur:
        q.update(min_ms=H.EDGE_MIN_MS, max_ms=H.EDGE_MAX_MS)
    if rng:
        q.update(start=H.EDGE_START, end=H.EDGE_END)
    return q


def request(q):
    return T.SearchRequest(tags=dict(q.get("tags", {})), min_duration_ms=q.get("min_ms", 0),
                           max_duration_ms=q.get("max_ms", 0), start=q.get("start", 0), end=q.get("end", 0))


_exp_cache = {}


def expected(paths, q, limit=0, nthreads=1):
    """The oracle's (ordered records, metrics), computed once per (blocks, query, limit)."""
    key = (tuple(paths), repr(sorted(q.items())), limit)
    if key not in _exp_cache:
        exp, met, st = O.search([O.Block(p) for p in paths], limit=limit, nthreads=1 if limit else nthreads, **q)
        assert st == 0
        _exp_cache[key] = ([match_key(m) for m in exp], (met["traces_inspected"], met["bytes_inspected"],
                                                          met["blocks_inspected"], met["blocks_skipped"]))
    return _exp_cache[key]


def run(engine, blocks, q, limit=0):
    got, met = engine.search(blocks, T.Pipeline(request(q)), limit=limit)
    return ([tsg_key(m) for m in got], (met.inspected_traces, met.inspected_bytes, met.inspected_blocks,
                                        met.skipped_blocks)), met.path


@pytest.fixture(autouse=True)
def _alone():
    gc.collect()


@pytest.fixture(scope="module")
def edge(tmp_path_factory):
    return H.write_edge_blocks(str(tmp_path_factory.mktemp("edge")))


@pytest.fixture(scope="module")
def varied(tmp_path_factory):
    return H.write_edge_blocks(str(tmp_path_factory.mktemp("edgev")), vary_dicts=True)


@contextmanager
def opened(engine, paths):
    blocks = [engine.open_block(p) for p in paths]
    try:
        yield blocks
    finally:
        for b in blocks:
            b.close()


@contextmanager
def extra_engine(env=None, devices=None):
    """A second engine (the environment set around T.Engine() only), closed on exit."""
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


def check_matrix(engine, paths, path_ok, limits=LIMITS):
    """Every shape at every limit on `engine` against the oracle; path_ok(path bits, shape,
    limit, the shape's oracle record count at limit 0) -> bool. (A shape that can overflow a
    record buffer is answered by the other path, and skips the narrow kernels for its next 16
    searches whatever their limit: no path is asserted for it.) Collects every failing case
    before asserting."""
    bad = []
    with opened(engine, paths) as blocks:
        for shape in SHAPES:
            q = shape_query(*shape)
            n0 = len(expected(paths, q)[0])
            for limit in limits:
                exp = expected(paths, q, limit)
                res, path = run(engine, blocks, q, limit)
                if res != exp:
                    d = next((i for i, (g, e) in enumerate(zip(res[0], exp[0])) if g != e), min(len(res[0]), len(exp[0])))
                    bad.append((shape, limit, "records %d vs %d, first difference at %d, metrics %r vs %r"
                                % (len(res[0]), len(exp[0]), d, res[1], exp[1])))
                elif not path_ok(path, shape, limit, n0):
                    bad.append((shape, limit, "path %d" % path))
    assert not bad, "%d of %d cases: %r" % (len(bad), len(SHAPES) * len(limits), bad[:6])


def resident_ok(path, shape, limit, n):
    return path & T.PATH_RESIDENT != 0 if limit == 0 and n < REC_CAP else True


def plain_ok(path, shape, limit, n):
    return path & T.PATH_PLAIN != 0 and path & T.PATH_RESIDENT == 0 if n < REC_CAP else True


def other_ok(path, shape, limit, n):  # (never a narrow kernel, dense or not)
    return path & T.PATH_OTHER != 0 and path & (T.PATH_RESIDENT | T.PATH_PLAIN) == 0


def test_fixture_conditions(edge):
    """From the oracle alone: every predicate of the full query is decisive, every shape
    matches something, and only "no predicate" matches more than a record buffer."""
    full = shape_query(4, True, True)
    e_full = expected(edge, full)[0]
    assert e_full
    for k in range(4):  # one term dropped
        q = dict(full, tags=dict(t for i, t in enumerate(H.EDGE_TERMS) if i != k))
        assert expected(edge, q)[0] != e_full, H.EDGE_TERMS[k]
    for drop in (("min_ms", "max_ms"), ("min_ms",), ("max_ms",), ("start", "end")):
        q = {k: v for k, v in full.items() if k not in drop}
        assert expected(edge, q)[0] != e_full, drop
    sizes = {shape: len(expected(edge, shape_query(*shape))[0]) for shape in SHAPES}
    assert all(n > 0 for n in sizes.values()), sizes
    assert sizes[(0, False, False)] == sum(H.EDGE_SIZES)
    assert all(n <= REC_CAP for shape, n in sizes.items() if shape != (0, False, False)), sizes
    # the hit set is where the docstring says: the full query's matches are H's "ok" entries
    # (and those on the passing side of a bound), ids = scan positions
    base, want = 0, []
    for n in H.EDGE_SIZES:
        passing = ("ok", "multi_c", "dur_min", "dur_min_over", "dur_max", "dur_max_under", "end_eq_start", "start_eq_end")
        want += [base + p for p, role in sorted(H.edge_hits(n).items()) if role in passing]
        base += n
    assert [int.from_bytes(m[2][8:], "big") for m in e_full] == want
    # ... and the low half of every id is the entry's scan position over the set
    bases = [sum(H.EDGE_SIZES[:i]) for i in range(len(H.EDGE_SIZES))]
    every = expected(edge, {})[0]
    assert [int.from_bytes(m[2][8:], "big") for m in every] == [bases[m[0]] + m[1] for m in every] == list(range(len(every)))


def test_matrix_resident(engine, edge):
    """search_resident_kernel <NT, DUR, RANGE, true>: the session engine alone on the device."""
    check_matrix(engine, edge, resident_ok)


@pytest.mark.parametrize("groups", [1, 3])
def test_matrix_resident_workgroup_counts(engine, edge, groups):
    """One workgroup walks every block boundary in one run (26 units); three have a remainder
    (wr = 2). At the device's count (above) most workgroups have no unit."""
    T.debug_set("groups", groups)
    try:
        check_matrix(engine, edge, resident_ok, limits=(0,))
    finally:
        T.debug_set("groups", 0)


def test_matrix_static_plain(engine, edge):
    """search_static_kernel <.., true>: a second context on the device turns the resident kernel off."""
    with extra_engine(devices=[0]):
        check_matrix(engine, edge, plain_ok)


def test_matrix_pool_dynamic(engine, edge):
    """search_pool_kernel <.., true>, every unit claimed from the device counter."""
    with extra_engine({"TSG_POOL_SMALL": "0", "TSG_POOL_STATIC_UNITS": "0"}) as e:
        check_matrix(e, edge, plain_ok)


def test_matrix_default_loads_static(engine, edge):
    """search_static_kernel <.., NTL=false> (TSG_POOL_NT=0)."""
    with extra_engine({"TSG_POOL_NT": "0"}) as e:
        check_matrix(e, edge, plain_ok)


def test_matrix_default_loads_pool(engine, edge):
    """search_pool_kernel <.., NTL=false>."""
    with extra_engine({"TSG_POOL_NT": "0", "TSG_POOL_SMALL": "0", "TSG_POOL_STATIC_UNITS": "0"}) as e:
        check_matrix(e, edge, plain_ok)


def test_matrix_fast_kernel(engine, edge):
    with extra_engine({"TSG_NO_POOL": "1"}) as e:
        check_matrix(e, edge, other_ok)


def test_matrix_general_path(engine, edge):
    with extra_engine({"TSG_NO_FAST": "1"}) as e:
        check_matrix(e, edge, other_ok)


def test_five_terms_and_wide_column(engine, edge):
    """Five terms (the switches' default: maps NT >= 4 to 4; the host must not take the narrow
    path at all) and a term on the 16-bit column x: exact, and served by the other kernels."""
    five = dict(shape_query(4, True, True), tags=dict(H.EDGE_TERMS + (("e", "e-hit"),)))
    qs = [five, dict(tags=dict(H.EDGE_TERMS + (("e", "e-hit"),))), dict(tags={"x": "x255"}),
          dict(tags={"a": "a-hit", "x": "x00"}, min_ms=H.EDGE_MIN_MS)]
    with opened(engine, edge) as blocks:
        for q in qs:
            exp = expected(edge, q)
            assert exp[0], q
            res, path = run(engine, blocks, q)
            assert res == exp, q
            assert path & T.PATH_OTHER and not path & (T.PATH_RESIDENT | T.PATH_PLAIN), (q, path)


# one needle per 32-bit word of the 256-bit set map at its bit 0 and its highest bit in use
# (v has set ids 0..253: word 7 ends at bit 29), a substring that selects many sets, no set
V_NEEDLES = ["v%03d" % i for w in range(8) for i in (32 * w, min(32 * w + 31, 253))] + ["v2", "v25", "v254", "nope"]
# the issue's needles on w: 255 sets, so a 16-bit column (module docstring)
W_NEEDLES = ["w000", "w031", "w032", "w063", "w064", "w127", "w128", "w191", "w192", "w224", "w254", "w2", "w255"]


def check_needles(engine, paths, blocks, key, needles, path_ok):
    for needle in needles:
        for q in (dict(tags={key: needle}), dict(tags={"a": "a-hit", key: needle}, start=H.EDGE_START, end=H.EDGE_END)):
            exp = expected(paths, q)
            res, path = run(engine, blocks, q)
            assert res == exp, q
            if exp[1][2] == 0:  # (the oracle skipped every block by its header: nothing to launch)
                assert path == 0, (q, path)
            else:
                assert path_ok(path, None, 0, len(exp[0])), (q, path)
    sizes = [len(expected(paths, dict(tags={key: n}))[0]) for n in needles]
    assert sizes[0] > 0 and sizes[-1] == 0 and max(sizes) > 10 * sizes[0], sizes


def test_bitmap_words_resident(engine, edge):
    with opened(engine, edge) as blocks:
        check_needles(engine, edge, blocks, "v", V_NEEDLES, resident_ok)
        check_needles(engine, edge, blocks, "w", W_NEEDLES, other_ok)


def test_bitmap_words_plain(engine, edge):
    with extra_engine(devices=[0]), opened(engine, edge) as blocks:
        check_needles(engine, edge, blocks, "v", V_NEEDLES, plain_ok)
        check_needles(engine, edge, blocks, "w", W_NEEDLES, other_ok)


def test_bitmap_budget(engine, varied):
    """No two blocks of `varied` share a dictionary of a or of b (one own value each; the blocks
    of 1 and 7 entries hold fewer values): a query on a and b needs 8 + 8 = kArgBms bitmaps, one
    on a, b and c more than that. Identical dictionaries share one NarrowDict (devctx.hip
    intern_narrow, block.cpp canonicalize_narrow_keys), so 16 is exactly the count of distinct
    (dictionary, term) pairs and the query at the budget stays on the resident kernel."""
    at = dict(tags=dict(H.EDGE_TERMS[:2]), min_ms=H.EDGE_MIN_MS, max_ms=H.EDGE_MAX_MS)
    over = dict(at, tags=dict(H.EDGE_TERMS[:3]))
    with opened(engine, varied) as blocks:
        for q, want in ((at, T.PATH_RESIDENT), (over, T.PATH_OTHER)):
            exp = expected(varied, q)
            assert 0 < len(exp[0]) < REC_CAP
            for limit in (0, 3):
                res, path = run(engine, blocks, q, limit)
                assert res == expected(varied, q, limit), (q, limit)
                if limit == 0:
                    assert path == want, (q, path)


# ---- run-length edges at one workgroup ------------------------------------------------
RUN_T0 = 1_700_000_000
RUN_CFG2 = dict(tags={"service.name": "svc-07", "http.method": "get", "status.code": "error"},
                min_ms=10, max_ms=1000, start=RUN_T0 + 900, end=RUN_T0 + 2700)
RUN_ONE = dict(tags={"service.name": "svc-07"})


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """1536, 1, 511 and 1 units."""
    d = tmp_path_factory.mktemp("runs")
    out = []
    for i, n in enumerate((786_432, 512, 261_632, 512)):
        p = str(d / ("r%d" % i))
        T.synth_search_block(p, n, seed=1300 + i, profile=0, encoding=T.ENC_SNAPPY)
        out.append(p)
    return out


@pytest.mark.parametrize("nblocks,units", [(1, 1536), (2, 1537), (3, 2048), (4, 2049)])
def test_run_length_edges_one_workgroup(engine, runs, nblocks, units):
    """One workgroup ("groups" = 1) over 1536 units (the last run one prefix pass covers), 1537
    (a second pass), 2048 (kResMaxUnits: the last the resident kernel takes) and 2049 (it
    declines: a plain launch). The one-term query may match more than the 2048-record buffer
    holds; such a prefix is answered by the other path and only its parity is asserted."""
    paths = runs[:nblocks]
    T.debug_set("groups", 1)
    try:
        with opened(engine, paths) as blocks:
            assert sum((b.info()["entries"] + 511) // 512 for b in blocks) == units
            for q in (RUN_CFG2, RUN_ONE):
                exp = expected(paths, q, nthreads=8)
                res, path = run(engine, blocks, q)
                assert res == exp, q
                if len(exp[0]) > REC_CAP:
                    continue  # (overflow: parity only)
                assert path == (T.PATH_RESIDENT if units <= 2048 else T.PATH_PLAIN), (q, path)
    finally:
        T.debug_set("groups", 0)
