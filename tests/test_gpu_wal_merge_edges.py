"""wal_merge_kernel (tempo_amd/csrc/wal_merge.hip) through tsg_wal_block_refresh on the constructed
refreshes of tests/wal_merge_cases.py. Every case writes `first`, opens it, and refreshes the handle
to the grown file; the call must take the incremental path (mode 1) with the case's counts, and the
refreshed handle must equal a fresh open_wal_block of the grown file and the oracle
(test_gpu_wal_refresh.same_as_fresh: info, tags, tag values, and the ordered records and metrics of
its query list plus the case's own; the dense query returns every entry's id, start, end, duration
and both root names in order). The cases are held to their aim, and the model of the kernel's index
arithmetic to a sorted merge, in tests/test_wal_merge_cases.py.

  family   what it pins
  runs     real entries at positions >= 2048 (kRun): blockIdx.x >= 1 with data, from the delta and
           from the old block; the `t` loop's break inside a run that is partly real
  pad      n crossing 4096 (kColPad): the scan job's source stride 4096 against its destination
           stride 8192, kCopy / kNames ending at n_new inside a run whose kScan / kTerm go on to npad
  delta    2047, 2048 (s_ins[2048]) and 2049 delta entries: staged in LDS, at capacity, searched in
           global memory; inserts interleaved with replacements above the capacity
  layout   n_old of 1 and 65: runs of inserts before entry 0 and behind the last, replacements of
           both ends, insert / replace / insert on neighbours, every entry replaced, alternating
  widths   one key at 253 .. 256 value sets (one byte to one byte with every id moved, widening at
           the cap, two bytes to two), 300 -> 340 sets over more than a run, a key the tail brings
           with 300 sets; every value of the key is queried
  names    both root-name tables renumbered; an entry without root names; a block that had none
  base     appended starts before the old block's base, at both edges of its 15-bit window and far
           behind it: the packed scan word escapes to the exact columns

The runs, pad and delta families run again on an engine whose pool kernels hold 8 records per
workgroup: the dense query then gathers its records from the block's host columns (the look-back
path), the first run reads them from the device columns. test_chained refreshes a refreshed handle
across the stride change: the second merge reads columns, padding included, that the first wrote."""
import pytest

import tempo_amd as T
from tests import wal_merge_cases as W
from tests.test_gpu_wal_refresh import answers, same_as_fresh, small  # noqa: F401  (small: the 8-record engine fixture)

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in W.all_cases()}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> the paths of a case's two files, written on first use and shared by both engines."""
    root, done = str(tmp_path_factory.mktemp("wal_merge")), {}

    def paths(c):
        if c.name not in done:
            done[c.name] = W.write_stages(root, c.name, [c.first, c.appended])
        return done[c.name]
    return paths


def refresh_step(eng, old, path, first, appended, by_bytes=False):
    """old -> the handle refreshed to `path`, after the call's stats were held to the entry lists."""
    p = W.plan(first, appended)
    blk, st = eng.refresh_wal_block(old, open(path, "rb").read() if by_bytes else path)
    print("%d -> %d entries, ndelta %d (%d inserts, %d replacements), npad %d -> %d: %r"
          % (p.n_old, p.n_new, p.ndelta, p.inserts, p.replacements, W.npad(p.n_old), W.npad(p.n_new), st))
    try:
        assert st["mode"] == 1 and st["pages_replayed"] == len(appended)
        assert st["entries_added"] == p.inserts and st["entries_combined"] == p.replacements
        assert st["upload_bytes"] > 0 and blk.info()["entries"] == p.n_new
    except BaseException:
        blk.close()
        raise
    return blk, p


def run_case(eng, c, paths, by_bytes=False):
    old = eng.open_wal_block(paths[0])
    try:
        assert old.info()["entries"] == len(c.first)
        blk, p = refresh_step(eng, old, paths[1], c.first, c.appended, by_bytes)
        try:
            same_as_fresh(eng, blk, paths[1], c.queries + c.probes)
            got, met = answers(eng, blk, dict(), 0)
            assert [m.trace_id for m in got] == sorted(set(p.old) | set(p.delta))  # every record, in id order
            return blk, met
        except BaseException:
            blk.close()
            raise
    finally:
        old.close()


@pytest.mark.parametrize("name", list(CASES))
def test_case(engine, files, name):
    c = CASES[name]
    blk, _ = run_case(engine, c, files(c))
    try:
        if c.family == "widths":  # every value of the key: the ids of the entries that hold it
            key, tags = c.meta["key"], W.merged_tags(c)
            values = sorted({v for t in tags.values() for v in t.get(key, ())})
            assert len(values) >= max(c.meta["sets"])
            for v in values:
                got, _ = answers(engine, blk, dict(tags={key: v}), 0)
                assert [m.trace_id for m in got] == sorted(i for i, t in tags.items() if v in t.get(key, ())), (name, v)
    finally:
        blk.close()


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.family in ("runs", "pad", "delta")])
def test_case_on_small_engine(small, files, name):  # noqa: F811
    c = CASES[name]
    blk, met = run_case(small, c, files(c), by_bytes=True)  # (the _mem entry point)
    try:
        assert met.path & T.PATH_OTHER  # the dense query's records did overflow the pool kernels' buffer
    finally:
        blk.close()


def test_chained(engine, tmp_path_factory):
    """2047 -> 2049 -> 4097: the second refresh's source is what the first one's kernel wrote."""
    stages = W.chained_stages()
    paths = W.write_stages(str(tmp_path_factory.mktemp("wal_merge_chain")), "chain", stages)
    b0 = engine.open_wal_block(paths[0])
    handles = [b0]
    try:
        b1, p1 = refresh_step(engine, b0, paths[1], stages[0], stages[1])
        handles.append(b1)
        assert (p1.n_old, p1.n_new, W.npad(p1.n_new)) == (2047, 2049, 4096)
        b2, p2 = refresh_step(engine, b1, paths[2], stages[0] + stages[1], stages[2])
        handles.append(b2)
        assert (p2.n_old, p2.n_new, W.npad(p2.n_old), W.npad(p2.n_new)) == (2049, 4097, 4096, 8192)
        same_as_fresh(engine, b2, paths[2], [dict(tags={"k3": "a1"})])
        same_as_fresh(engine, b1, paths[1])  # (the handle in between still answers as its own file)
        got, _ = answers(engine, b2, dict(), 0)
        assert [m.trace_id for m in got] == sorted(e["id"] for s in stages for e in s)
    finally:
        for b in handles:
            b.close()
