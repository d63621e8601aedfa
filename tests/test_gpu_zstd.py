"""zstd pages (backend.Encoding 7) on the device and through the loaders, mirroring
tests/test_gpu_lz4.py: the search / WAL / proto loaders against the block's ENC_NONE (or snappy)
twin, findOne over pages of the block writer and over golden frames of an independent encoder
(tests/golden/zstd, put into a block by write_v2_block_pages), the writer's edge pages and forced
forms, and three fixed damaged pages, each under the wave decoder (the default) and the one-lane
decoder (tsg_debug_set "zstd_find_lane"). The host side: tests/test_zstd_writer.py."""
import json
import os
import random
import struct

import numpy as np
import pytest

from oracle import oracle as O
import tempo_amd as T
from tests.helpers import random_entries, write_block
from tests.test_gpu_lz4 import (assert_oracle_parity, check_pages, find_all, one_per_page, page_spans, seq_ids, wal_result,
                                wordy)
from tests.test_zstd_writer import FLAG_CASES, GOLDEN, edge_inputs, flag_objects

pytestmark = pytest.mark.gpu
Z = T.ENC_ZSTD


@pytest.fixture(params=[0, 1], ids=["wave", "one-lane"])
def kernel(request):
    T.debug_set("zstd_find_lane", request.param)
    yield request.param
    T.debug_set("zstd_find_lane", 0)


@pytest.fixture(scope="module")
def search_twin(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("twin"))
    ents = random_entries(random.Random(21), 3000)
    return ents, write_block(d, "n", ents, T.ENC_NONE, page_size=4096), write_block(d, "z", ents, Z, page_size=4096)


def test_search_block_opens_like_its_twin(engine, search_twin):
    _, twin, p = search_twin
    blk, tb = engine.open_block(p), engine.open_block(twin)
    try:
        info, tinfo = blk.info(), tb.info()
        assert info["encoding"] == Z and tinfo["encoding"] == T.ENC_NONE
        assert info["entries"] == 3000 and info["pages"] > 20 and info["stop_status"] == 0
        assert [info[k] for k in ("entries", "pages", "fb_bytes")] == [tinfo[k] for k in ("entries", "pages", "fb_bytes")]
        assert blk.tags() == tb.tags() and len(blk.tags()) >= 8
        for k in (b"k1", b"root.name", b"absent"):
            assert blk.tag_values(k) == tb.tag_values(k)
    finally:
        blk.close()
        tb.close()


def test_search_block(engine, search_twin):
    _, twin, p = search_twin
    blk = engine.open_block(p)
    try:
        n = []
        for tags, limit in (({"k1": "v2-x", "root.name": "op-3"}, 0), ({"root.service.name": "svc"}, 0), ({"k0": "v"}, 20)):
            got, met = engine.search([blk], T.Pipeline(T.SearchRequest(tags=dict(tags))), limit=limit)
            exp, omet, st = O.search([O.Block(twin)], tags=tags, limit=limit)
            assert st == 0
            assert_oracle_parity(got, met, exp, omet)
            n.append(len(got))
        assert 0 < n[0] < 300 and n[1] == 3000 and n[2] == 20  # narrow, dense, limit
    finally:
        blk.close()


def test_wal_replays_like_its_snappy_twin(engine, tmp_path):
    ents = random_entries(random.Random(22), 300)
    res = {}
    for e in (Z, T.ENC_SNAPPY):
        d = os.path.join(str(tmp_path), "w%d" % e)
        os.makedirs(d)
        p = os.path.join(d, T.wal_filename(e))
        assert ":v2:%s:" % T.tsg.ENC_NAMES[e] in p
        T.write_wal_search(p, ents, e)
        res[e] = wal_result(engine, p, e, 300)
    assert res[Z] == res[T.ENC_SNAPPY]
    assert len(res[Z][2][0]) == 300 and 10 < len(res[Z][3][0]) < 300


def test_wal_damaged_page(engine, tmp_path):
    ents = random_entries(random.Random(23), 40)
    d = os.path.join(str(tmp_path), "w")
    os.makedirs(d)
    p = os.path.join(d, T.wal_filename(Z))
    T.write_wal_search(p, ents, Z)
    data = bytearray(open(p, "rb").read())
    spans = page_spans(bytes(data))
    assert len(spans) == 40
    data[spans[25][0] + 4] ^= 8  # page 25: the frame header descriptor's reserved bit (the header checksum of lz4 has no twin here)
    with open(p, "wb") as f:
        f.write(data)
    blk = engine.open_wal_block(p)
    info = blk.info()
    blk.close()
    assert info["partial"] == 1 and info["entries"] == 25


def test_proto_block(engine, tmp_path):
    from tests.test_gpu_proto import key, make_block
    res = {}
    for enc in (Z, T.ENC_NONE):
        path = os.path.join(str(tmp_path), "p%d" % enc)
        make_block(path, random.Random(31), 300, True, enc)
        blk = engine.open_proto_block(path)
        assert blk.info()["objects"] == 300
        res[enc] = [key(engine.proto_search(blk, **q)) for q in
                    (dict(start=0, end=2 ** 32 - 1, limit=1000), dict(tags={"service.name": "cart"}, start=0, end=2 ** 32 - 1, limit=20),
                     dict(tags={"http.url": "/api"}, start=0, end=2 ** 32 - 1, limit=1000, chunk_size_bytes=10_000))]
        blk.close()
    assert res[Z] == res[T.ENC_NONE] and len(res[T.ENC_NONE][0][0]) > 100


@pytest.fixture(scope="module")
def find_blocks(tmp_path_factory):
    rng = random.Random(7)
    n = 400
    raw = sorted({rng.randbytes(16) for _ in range(n)})
    ids = np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(-1, 16)
    objs = [wordy(rng, rng.randrange(500, 3500)) if i % 9 else rng.randbytes(rng.randrange(200, 3000)) for i in range(n)]
    paths = {}
    for e in (Z, T.ENC_NONE):
        paths[e] = os.path.join(str(tmp_path_factory.mktemp("find")), "b%d" % e)
        T.write_v2_block(paths[e], ids, objs, encoding=e, index_downsample_bytes=100_000)
    return ids, objs, paths


def test_find_on_zstd_pages(engine, find_blocks, kernel):
    ids, objs, paths = find_blocks
    n = len(objs)
    assert 5 <= len(page_spans(open(os.path.join(paths[Z], "data"), "rb").read())) <= 12
    absent = np.frombuffer(random.Random(99).randbytes(16 * 50), dtype=np.uint8).reshape(-1, 16)
    probe = np.concatenate([ids, absent])
    got = find_all(engine, paths[Z], probe)
    twin = find_all(engine, paths[T.ENC_NONE], probe)
    assert got == twin  # the same hit list, statuses and bytes as the uncompressed twin
    found = {i: obj for i, _, st, obj in got if st == T.TSG_OK}
    assert sorted(found) == list(range(n))
    assert all(found[i] == objs[i] for i in range(n))
    assert all(st == T.TSG_E_NOT_FOUND for i, _, st, _ in got if i >= n)  # bloom false positives


def test_find_on_golden_frames(engine, tmp_path, kernel):
    """Frames of an independent encoder (libzstd), one per page, through write_v2_block_pages."""
    pa = pytest.importorskip("pyarrow")  # (to learn the objects the frames hold)
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    ids, objs, payloads = [], [], []
    for m in man:
        frame = open(os.path.join(GOLDEN, m["file"]), "rb").read()
        if m["case"] == "two_frames":  # (libzstd's one-shot call reads one frame)
            cut = frame.index(b"\x28\xb5\x2f\xfd", 4)
            sizes = (11_000, m["decoded_bytes"] - 11_000)  # (tools/gen_zstd_golden.py cuts the page there)
            page = b"".join(pa.Codec("zstd").decompress(f, decompressed_size=n, asbytes=True)
                            for f, n in zip((frame[:cut], frame[cut:]), sizes))
        else:
            page = pa.Codec("zstd").decompress(frame[20:] if m["case"] == "skippable" else frame,
                                               decompressed_size=m["decoded_bytes"], asbytes=True)
        assert len(page) == m["decoded_bytes"]
        ids.append(page[8:24])
        objs.append(page[24:])
        payloads.append(frame)
    path = os.path.join(str(tmp_path), "g")
    idarr = np.frombuffer(b"".join(ids), dtype=np.uint8).reshape(-1, 16)
    T.write_v2_block_pages(path, idarr, objs, list(range(len(objs))), payloads, Z)
    got = find_all(engine, path, idarr)
    assert [g[0] for g in got] == list(range(len(objs)))
    for i, _, st, obj in got:
        assert st == T.TSG_OK and obj == objs[i], (man[i]["file"], st)


def page_per_object(path, objs, bits=0):
    """A block whose every object, however small, is a page of its own."""
    try:
        T.debug_set("zstd_writer_flags", bits)
        T.write_v2_block(path, seq_ids(len(objs)), objs, encoding=Z, index_downsample_bytes=1)
    finally:
        T.debug_set("zstd_writer_flags", 0)
    assert len(page_spans(open(os.path.join(path, "data"), "rb").read())) == len(objs)


def test_writer_edge_pages(engine, tmp_path, kernel):
    """All inputs of the CPU round-trip list (the empty and the one-byte object included: a tiny raw
    block, no sequences), then a run that ends in an RLE block, a short-period match, mixed text."""
    objs = list(edge_inputs().values())
    assert [len(o) for o in objs[:2]] == [0, 1] and len(objs) == 8
    rng = random.Random(8)
    objs += [b"\x07" * (2 * 131_072), b"ab" * 4000 + wordy(rng, 1500), wordy(rng, 200) + rng.randbytes(900)]
    path = os.path.join(str(tmp_path), "e")
    page_per_object(path, objs)
    check_pages(engine, path, objs)


@pytest.mark.parametrize("case", sorted(FLAG_CASES))
def test_writer_forced_forms(engine, tmp_path, kernel, case):
    objs = list(flag_objects().values())
    path = os.path.join(str(tmp_path), "f")
    page_per_object(path, objs, FLAG_CASES[case][0])
    check_pages(engine, path, objs)


def test_damaged_pages(engine, tmp_path, kernel):
    """The last 10 bytes of a frame cut (the page length patched to match), a block header whose
    size exceeds the page, a frame content size off by one: the hits on those pages report
    TSG_E_CORRUPT, their neighbours are untouched. (tools/zstd_host_check.cpp --fuzz runs the same
    three patterns on every writer frame under ASan: tests/test_zstd_writer.py.)"""
    rng = random.Random(13)
    objs = [b"\x07" * 400 + wordy(rng, 3000 + 500 * i) for i in range(7)]
    path = os.path.join(str(tmp_path), "d")
    data, spans = one_per_page(path, objs, Z)
    data = bytearray(data)
    # 1: cut. The page keeps its place in the file (the index record's start) and loses 10 bytes of
    # its frame: [u32 total - 10][u16 0][frame minus 10 bytes], the index record's length patched too.
    a, b = spans[1]
    struct.pack_into("<I", data, a - 6, b - a + 6 - 10)
    idx = bytearray(open(os.path.join(path, "index"), "rb").read())
    rec = 14 + 28 * 1
    assert struct.unpack_from("<QI", idx, rec + 16) == (a - 6, b - a + 6)
    page_size = struct.unpack_from("<I", idx, 0)[0]
    assert struct.unpack_from("<Q", idx, 6)[0] == _xxh64(bytes(idx[14:page_size]))
    struct.pack_into("<I", idx, rec + 24, b - a + 6 - 10)
    struct.pack_into("<Q", idx, 6, _xxh64(bytes(idx[14:page_size])))  # (the index page's checksum covers its records)
    # 3: the first block header's size beyond the page (frame: magic 4, descriptor 1, window 1, content size 4)
    a3 = spans[3][0]
    data[a3 + 11] = 0xFF
    data[a3 + 12] = 0xFF
    # 5: content size off by one
    data[spans[5][0] + 6] ^= 1
    with open(os.path.join(path, "data"), "wb") as f:
        f.write(data)
    with open(os.path.join(path, "index"), "wb") as f:
        f.write(idx)
    check_pages(engine, path, objs, bad={1, 3, 5})


def _xxh64(b):
    """XXH64 (seed 0) of the index page's record area, as index_writer.go computes it."""
    M = (1 << 64) - 1
    P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
    rotl = lambda x, r: ((x << r) | (x >> (64 - r))) & M
    rnd = lambda acc, v: (rotl((acc + v * P2) & M, 31) * P1) & M
    n, i = len(b), 0
    if n >= 32:
        v = [(P1 + P2) & M, P2, 0, (-P1) & M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(b[i + 8 * k:i + 8 * k + 8], "little"))
            i += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = P5
    h = (h + n) & M
    while i + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(b[i:i + 8], "little")), 27) * P1 + P4) & M
        i += 8
    if i + 4 <= n:
        h = (rotl(h ^ (int.from_bytes(b[i:i + 4], "little") * P1 & M), 23) * P2 + P3) & M
        i += 4
    while i < n:
        h = (rotl(h ^ (b[i] * P5 & M), 11) * P1) & M
        i += 1
    h ^= h >> 33
    h = h * P2 & M
    h ^= h >> 29
    h = h * P3 & M
    h ^= h >> 32
    return h
