"""GPU parity for the batched proto-object search (tsg_proto_search_batch: one
proto_scan_batch_kernel launch per device for many (block, request) jobs).

Every batch item is compared with the oracle (oracle/proto_oracle.py ProtoBlock.search: the
full ordered result and the three metrics, or both sides fail) and with engine.proto_search
of the same item. Oracle and single-call results are computed once per (block, request) and
shared by the tests.
"""
import os
import random

import pytest

from oracle import proto_oracle as P
import tempo_amd as T
from tests.test_gpu_proto import GOLD, T0, key, make_block, okey, queries

pytestmark = pytest.mark.gpu
EDGE = (1, 63, 64, 65, 255, 256, 257, 400)
ALL = dict(start=0, end=2 ** 32 - 1, limit=100000)


class Blocks:
    """The blocks of this module, open on the engine and in the oracle, with the expected
    (oracle) and single-call outcome of every (block, request) the tests ask for."""

    def __init__(self, engine, root):
        self.engine, self.root = engine, root
        self.blk, self.ob, self.exp, self.one = {}, {}, {}, {}

    def add(self, name, path=None, **kw):
        if path is None:
            path = os.path.join(self.root, name)
            make_block(path, **kw)
        self.blk[name] = self.engine.open_proto_block(path)
        self.ob[name] = P.ProtoBlock(path)

    @staticmethod
    def _ck(name, kw):
        return name, repr(sorted((k, sorted(v.items()) if isinstance(v, dict) else v) for k, v in kw.items()))

    def expected(self, name, kw):
        """The oracle's outcome: (traces, metrics) or "error"."""
        ck = self._ck(name, kw)
        if ck not in self.exp and kw.get("total_pages", 0) > 0 and kw.get("start_page", 0) > self.ob[name].total:
            # (the oracle counts the objects before start_page by reading those pages, which do
            # not exist here; partialIterator past the last record is io.EOF at its first Next)
            self.exp[ck] = ([], (0, 0, 0))
        if ck not in self.exp:
            okw = dict(kw)
            if "tags" in okw:  # (a map: a repeated key keeps its last value)
                okw["tags"] = dict(okw["tags"].items() if isinstance(okw["tags"], dict) else okw["tags"])
            try:
                self.exp[ck] = okey(self.ob[name].search(**okw))
            except P.ProtoError:
                self.exp[ck] = "error"
        return self.exp[ck]

    def single(self, name, kw):
        """engine.proto_search's outcome: (traces, metrics) or ("error", code)."""
        ck = self._ck(name, kw)
        if ck not in self.one:
            try:
                self.one[ck] = key(self.engine.proto_search(self.blk[name], **kw))
            except T.TsgError as e:
                self.one[ck] = ("error", e.code)
        return self.one[ck]

    def batch(self, items, oracle=True):
        """Runs items [(block name, request)] as one batch and checks every item against the
        oracle and the single call, and the call's return value against the first failure.
        Returns the per-item outcomes."""
        res, rc = self.engine.proto_search_batch([(self.blk[n], kw) for n, kw in items], raw=True)
        assert len(res) == len(items)
        got = [("error", r.code) if isinstance(r, T.TsgError) else key(r) for r in res]
        for (n, kw), g in zip(items, got):
            assert g == self.single(n, kw), (n, kw)
            if oracle:
                e = self.expected(n, kw)
                assert g == (("error", T.TSG_E_CORRUPT) if e == "error" else e), (n, kw)
        codes = [g[1] for g in got if g[0] == "error"]
        assert rc == (codes[0] if codes else T.TSG_OK)
        return got


@pytest.fixture(scope="module")
def blocks(engine, tmp_path_factory):
    B = Blocks(engine, str(tmp_path_factory.mktemp("pbatch")))
    # one object per page (index_downsample_bytes 1): a range of k pages is a job of k objects
    for n in EDGE:
        B.add("e%d" % n, rng=random.Random(100 + n), n=n, v2=True, encoding=T.ENC_NONE, downsample=1)
    B.add("v1s", rng=random.Random(21), n=300, v2=False, encoding=T.ENC_SNAPPY)
    B.add("v2n", rng=random.Random(22), n=300, v2=True, encoding=T.ENC_NONE)
    B.add("bad", rng=random.Random(23), n=200, v2=True, encoding=T.ENC_NONE, corrupt=(37, 150))
    B.add("cli", path=os.path.join(GOLD, "tempo_cli"))
    yield B
    for b in B.blk.values():
        b.close()


def test_edge_sizes(blocks):
    """Jobs of 1 .. 400 objects in one batch: whole blocks and page ranges (one object per
    page) whose object counts lie on each side of a 64-object ballot and of a 256-object
    workgroup, at both ends of a block."""
    items = []
    for n in EDGE:
        name = "e%d" % n
        assert blocks.blk[name].info()["pages"] == n
        items.append((name, dict(ALL)))
        items.append((name, dict(ALL, tags={"service.name": "cart"})))
    counts = {}
    for k in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320):
        for sp in (0, 3, 400 - k):
            items.append(("e400", dict(ALL, start_page=sp, total_pages=k)))
            counts[len(items) - 1] = k
    items.append(("e257", dict(ALL, start_page=1, total_pages=256)))
    counts[len(items) - 1] = 256
    items.append(("e65", dict(ALL, start_page=1, total_pages=64, tags={"http.url": "/api"})))
    counts[len(items) - 1] = 64
    got = blocks.batch(items)
    for i, k in counts.items():
        assert got[i][1][0] == k  # inspected_traces: the job had exactly k objects
    assert sum(len(g[0]) for g in got) > 1000


def test_empty_jobs(blocks):
    """Page ranges at and past the last page (no objects, no workgroup) first, last, next to
    each other and between jobs of different blocks: they give no traces and zero metrics, and
    their neighbours are served as if they were not there."""
    def e(name, n, d):
        return name, dict(ALL, start_page=n + d, total_pages=2)
    full = [("e257", dict(ALL)), ("e63", dict(ALL)), ("e400", dict(ALL, start_page=100, total_pages=130)),
            ("v1s", dict(ALL))]
    items = [e("e1", 1, 0), e("e400", 400, 5), full[0], e("e63", 63, 0), e("e63", 63, 1000), e("e257", 257, 0), full[1],
             full[2], e("e400", 400, 0), full[3], e("e64", 64, 2 ** 31), e("e1", 1, 1)]
    got = blocks.batch(items)
    for (n, kw), g in zip(items, got):
        if kw.get("total_pages") == 2:
            assert g == ([], (0, 0, 0))
    assert [g for (n, kw), g in zip(items, got) if (n, kw) in full] == blocks.batch(full)
    assert all(len(g[0]) > 50 for g in blocks.batch(full))
    # a batch of empty jobs only: nothing is launched
    assert blocks.batch([items[0], items[1], items[-1]]) == [([], (0, 0, 0))] * 3


def mixed_items():
    rng = random.Random(7)
    items = []
    for name in ("v1s", "v2n", "bad"):
        qs = list(queries(rng))
        items += [(name, q) for q in qs[:4] + rng.sample(qs[4:], 36)]
    cli = [dict(ALL), dict(ALL, tags={"service.name": "a"}, limit=20), dict(ALL, tags={"name": "x", "error": "true"}),
           dict(ALL, limit=0), dict(ALL, start_page=1, total_pages=1), dict(ALL, tags={"status.code": "ok"}, limit=5),
           dict(ALL, tags={"service.name": "o", "status.code": "unset"}, min_ms=10)]
    items += [("cli", q) for q in cli]
    # tag counts 0 (above), 1, 3, 16; a key absent from the block; a repeated key (the last value wins)
    many = {"k%d" % i: "v" for i in range(13)}
    items += [("v2n", dict(ALL, tags={"service.name": "cart"})),
              ("v2n", dict(ALL, tags={"service.name": "cart", "http.url": "/api", "status.code": "unset"})),
              ("v1s", dict(ALL, tags=dict(many, **{"service.name": "cart", "cluster": "prod", "name": "GET /api"}))),
              ("v1s", dict(ALL, tags={"missing.key": "x"})),
              ("v2n", dict(ALL, tags=[("service.name", "nothing-has-this")] * 15 + [("service.name", "cart")])),
              ("v2n", dict(ALL, tags=[("service.name", "cart"), ("service.name", "nothing-has-this")])),
              ("bad", dict(ALL, tags=[("cluster", "x"), ("http.url", "/api"), ("cluster", "prod")]))]
    # the corrupt block read to its end (an error) and cut short before object 37 (none)
    items += [("bad", dict(ALL)), ("bad", dict(ALL, limit=5)), ("bad", dict(ALL, start_page=0, total_pages=1))]
    rng.shuffle(items)
    items += [items[3], items[3], items[40], items[11]]  # identical items, next to each other and apart
    return items


def test_mixed_batch(blocks):
    """~150 items over a v1 snappy block, a v2 none block, a v2 block with corrupt objects and
    the tempo-cli block, each named many times: items that fail with TSG_E_CORRUPT sit between
    items that succeed, and the call returns the first failure's code."""
    items = mixed_items()
    assert 140 <= len(items) <= 160
    ntags = {len(kw.get("tags", ())) for _, kw in items}
    assert {0, 1, 3, 16} <= ntags
    got = blocks.batch(items)
    errs = [g[0] == "error" for g in got]
    assert any(errs) and not all(errs)
    assert all(g[1] == T.TSG_E_CORRUPT for g in got if g[0] == "error")
    assert any(errs[i] and not (errs[i - 1] and errs[i + 1]) for i in range(1, len(errs) - 1))
    assert sum(len(g[0]) for g in got if g[0] != "error") > 1000
    # the repeated key: only the last value counts
    v = {repr(kw.get("tags")): g for (n, kw), g in zip(items, got) if n == "v2n"}
    assert v[repr([("service.name", "nothing-has-this")] * 15 + [("service.name", "cart")])] == \
        v[repr({"service.name": "cart"})] and len(v[repr({"service.name": "cart"})][0]) > 10
    assert v[repr([("service.name", "cart"), ("service.name", "nothing-has-this")])][0] == []


def test_item_errors(blocks):
    """17 tags in one item: that item alone is TSG_E_UNSUPPORTED, the rest are served."""
    ok = [("v2n", dict(ALL, tags={"service.name": "cart"})), ("e65", dict(ALL)), ("v1s", dict(ALL, limit=5))]
    bad = ("v2n", dict(ALL, tags={"k%d" % i: "v" for i in range(17)}))
    got = blocks.batch([ok[0], ok[1], bad, ok[2]], oracle=False)
    assert got[2] == ("error", T.TSG_E_UNSUPPORTED)
    assert [got[0], got[1], got[3]] == blocks.batch(ok) and all(g[0] != "error" for g in got[:2])


def test_chunked_launches(blocks):
    """The mixed batch as launches of at most 1, 3 and 64 jobs: the same results."""
    items = mixed_items()
    want = blocks.batch(items)
    try:
        for k in (1, 3, 64):
            T.debug_set("proto_batch_jobs", k)
            assert blocks.batch(items) == want, k
    finally:
        T.debug_set("proto_batch_jobs", 0)


def test_wide_columns(blocks):
    """A 1200-object block whose http.url column is 2 bytes wide (255 or more distinct value
    sets; counted here from the oracle's decoded objects), beside 1-byte columns. The suite
    reaches widths 1 and 2. A 4-byte column needs 65535 distinct value sets of one key, so a
    block of at least that many objects: the generator does not get there in a few seconds,
    and the 4-byte branch of the decision is not reached by any test."""
    import struct
    blocks.add("wide", rng=random.Random(31), n=1200, v2=True, encoding=T.ENC_NONE)
    ob, sets = blocks.ob["wide"], set()
    for p in range(ob.total):
        pg, i = ob.page(*ob.at(p)), 0
        while i < len(pg):
            tl, il = struct.unpack_from("<II", pg, i)
            vals = set()
            for b in P.prepare_for_read(pg[i + 8 + il + 8:i + tl]):
                for s in b["spans"]:
                    vals |= {v for k, v in s["attrs"] if k == b"http.url"}
            sets.add(frozenset(vals))
            i += tl
    assert 255 <= len(sets) < 65535
    rng = random.Random(32)
    items = [("wide", dict(ALL, tags={"http.url": u})) for u in ("/api", "users/1", "items", "/static/app.js", "/cart/7/")]
    items += [("wide", dict(ALL, tags={"http.url": "users/%d" % rng.randrange(100), "service.name": "cart"}))
              for _ in range(4)]
    items += [("wide", dict(ALL, tags={"http.url": "/api"}, start_page=2, total_pages=40)), ("e65", dict(ALL)),
              ("wide", dict(ALL, tags={"http.url": "items", "cluster": "prod"}, limit=7))]
    got = blocks.batch(items)
    assert all(len(g[0]) > 0 for g in got[:5]) and sum(len(g[0]) for g in got) > 500


def test_interleaved_with_resident_search(blocks, engine, tmp_path):
    """A batch, a narrow flatbuffer search (served by the resident kernel, which then holds
    the device), another batch: both batches are right, and so is the search between them."""
    from oracle import oracle as O
    path = os.path.join(str(tmp_path), "fb")
    T.synth_search_block(path, 20_000, seed=42)
    fb = engine.open_block(path)
    items = [("v2n", dict(ALL, tags={"service.name": "cart"})), ("e257", dict(ALL)), ("v1s", dict(ALL, limit=20)),
             ("e400", dict(ALL, start_page=399, total_pages=4)), ("e1", dict(ALL))]
    first = blocks.batch(items)
    q = dict(tags={"service.name": "svc-07"}, min_ms=10, max_ms=1000, start=1_700_000_900, end=1_700_002_700)
    got, met = engine.search([fb], T.Pipeline(T.SearchRequest(tags=q["tags"], min_duration_ms=q["min_ms"],
                                                              max_duration_ms=q["max_ms"], start=q["start"],
                                                              end=q["end"])))
    exp, omet, st = O.search([O.Block(path)], **q)
    assert st == 0 and [(m.entry_idx, m.trace_id) for m in got] == [(m["entry_idx"], m["id"]) for m in exp]
    assert blocks.batch(items) == first
    assert sum(len(g[0]) for g in first) > 300
    fb.close()
