"""tsg_find_ids over v2 blocks opened with TSG_V2_DATA_ON_DEMAND (tsg_v2block_open_mode): the data
file stays on disk, held open, and device_find stages the pages its hits name (find.hip,
find_rounds.hpp). One corpus of 300 objects in 6..12 pages, written at none, snappy,
lz4-256k and zstd; the oracle reads none and snappy itself and stands for the other two through the
uncompressed twin, whose pages are cut at the same objects.

  equality     resident and on-demand opens of the same directory give the same (id_idx, block_idx,
               status, object) list, the oracle's, for present ids (every page's last id and the
               next page's first among them) and absent ones (bloom false positives included: made
               ones, see the corpus)
  rounds       staging caps of one page, one byte below the largest page, 1, and exactly the first three
               pages: the same list, the rounds counter advanced by the plan's count, the bytes counter
               by the hit pages' lengths
  mixed        resident and on-demand blocks of different encodings in one call, on one device (the
               resident block between the two others) and on two, with and without a small cap
  held         the data file renamed away after the open
  damage       the file truncated inside its last page after the open; a payload byte flipped before it
  no data      a directory without a data file: TSG_E_UNSUPPORTED per hit in both modes
  HBM          the on-demand open takes the data file's length less device memory; a context's staging
               buffers are freed when it closes
  lookup       tsg_lookup_ids is the same in both modes"""
import os
import random
import shutil
import struct

import numpy as np
import pytest

from oracle import oracle as O
import tempo_amd as T

pytestmark = pytest.mark.gpu
ENCS = [T.ENC_NONE, T.ENC_SNAPPY, T.ENC_LZ4_256K, T.ENC_ZSTD]
ENC_IDS = [T.tsg.ENC_NAMES[e] for e in ENCS]
OD = T.V2_DATA_ON_DEMAND
WORDS = [b"span", b"trace", b"service", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select"]
N = 300


def wordy(rng, n):
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS) + str(rng.randrange(1000)).encode()
    return bytes(out[:n])


def pages_of(path):
    """[(start, length)] of the pages of a block's data file."""
    data = open(os.path.join(path, "data"), "rb").read()
    off, out = 0, []
    while off < len(data):
        (tl,) = struct.unpack_from("<I", data, off)
        out.append((off, tl))
        off += tl
    return out


def oracle_list(path, probe):
    """The oracle's answer for one block: [(id_idx, 0, status, object)] per lookup hit, in its order."""
    ob = O.V2Block(path)
    rc, hits = O.lookup([ob], probe)
    assert rc == 0
    out = []
    for i, _, _, _, _ in hits:
        rc, obj = ob.find(bytes(probe[i]), status=True)
        out.append((i, 0, T.TSG_OK if obj is not None else rc if rc else T.TSG_E_NOT_FOUND, obj))
    return out


class Corpus:
    pass


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    c = Corpus()
    root = str(tmp_path_factory.mktemp("on_demand"))
    rng = random.Random(7)
    raw = sorted({rng.randbytes(16) for _ in range(N)})
    c.ids = np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(-1, 16)
    c.index = {t: i for i, t in enumerate(raw)}
    c.objs = [wordy(rng, rng.randrange(300, 2500)) if i % 7 else rng.randbytes(rng.randrange(200, 2000)) for i in range(N)]
    c.paths = {}
    for e in ENCS:
        c.paths[e] = os.path.join(root, "b%d" % e)
        T.write_v2_block(c.paths[e], c.ids, c.objs, encoding=e, index_downsample_bytes=50_000)
    c.pages = {e: pages_of(c.paths[e]) for e in ENCS}
    assert 6 <= len(c.pages[T.ENC_NONE]) <= 12 and len({len(p) for p in c.pages.values()}) == 1
    # The writer's bloom filter of so few ids passes no id it does not hold, so false positives are
    # made: 60 ids no block stores, and every block gets the bloom shards of a block that stores them too
    ghosts = sorted({rng.randbytes(16) for _ in range(60)})
    both = sorted(raw + ghosts)
    side = os.path.join(root, "ghosts")
    T.write_v2_block(side, np.frombuffer(b"".join(both), dtype=np.uint8).reshape(-1, 16),
                     [c.objs[c.index[t]] if t in c.index else b"ghost" for t in both], encoding=T.ENC_NONE)
    shards = sorted(f for f in os.listdir(side) if f.startswith("bloom-"))
    for e in ENCS:
        assert sorted(f for f in os.listdir(c.paths[e]) if f.startswith("bloom-")) == shards
        for f in shards:
            shutil.copyfile(os.path.join(side, f), os.path.join(c.paths[e], f))
    absent = np.frombuffer(b"".join(ghosts) + random.Random(99).randbytes(16 * 2000), dtype=np.uint8).reshape(-1, 16)
    c.probe = np.concatenate([c.ids, absent])
    c.probe = c.probe[np.random.default_rng(3).permutation(len(c.probe))]
    # the oracle: on the block itself where it reads the encoding, else on the uncompressed twin
    c.want = oracle_list(c.paths[T.ENC_NONE], c.probe)
    assert oracle_list(c.paths[T.ENC_SNAPPY], c.probe) == c.want
    assert sum(w[2] == T.TSG_OK for w in c.want) == N
    assert sum(w[2] == T.TSG_E_NOT_FOUND for w in c.want) >= 50  # (a ghost past the last record's id is no hit)
    # the page of every stored id, and the ids at the pages' edges
    ob = O.V2Block(c.paths[T.ENC_NONE])
    c.rec = [ob.index_find(t)[0] for t in raw]
    c.edges = [(raw[i], raw[i + 1]) for i in range(N - 1) if c.rec[i] != c.rec[i + 1]]
    assert len(c.edges) == len(c.pages[T.ENC_NONE]) - 1
    return c


def find_one(engine, path, probe, mode, device=0):
    blk = engine.open_v2block(path, device=device, data_mode=mode)
    try:
        got, _ = engine.find([blk], probe)
    finally:
        blk.close()
    return got


def test_unknown_mode_is_invalid(engine, corpus):
    with pytest.raises(T.TsgError) as e:
        engine.open_v2block(corpus.paths[T.ENC_NONE], data_mode=2)
    assert e.value.code == T.TSG_E_INVALID


@pytest.mark.parametrize("enc", ENCS, ids=ENC_IDS)
def test_equal_to_resident_and_oracle(engine, corpus, enc):
    c = corpus
    res = find_one(engine, c.paths[enc], c.probe, T.V2_DATA_RESIDENT)
    od = find_one(engine, c.paths[enc], c.probe, OD)
    assert od == res
    assert od == c.want
    # a page's last id and the next page's first are found, each in its own page's bytes
    at = {bytes(c.probe[g[0]]): g for g in od if g[2] == T.TSG_OK}
    for last, first in c.edges:
        assert at[last][3] == c.objs[c.index[last]] and at[first][3] == c.objs[c.index[first]]


def model_rounds(lens, cap):
    """Rounds of pages of those lengths: maximal runs whose bytes, packed at 16-byte offsets, fit cap."""
    n, end, count = 1, 0, 0
    for ln in lens:
        off = -(-end // 16) * 16
        if count and off + ln > cap:
            n, off, count = n + 1, 0, 0
        end, count = off + ln, count + 1
    return n


@pytest.mark.parametrize("enc", ENCS, ids=ENC_IDS)
def test_rounds(engine, corpus, enc):
    c = corpus
    lens = [ln for _, ln in c.pages[enc]]  # (every page holds a probed id: the batch's pages, in order)
    three = -(-(-(-lens[0] // 16) * 16 + lens[1]) // 16) * 16 + lens[2]  # the first three pages, packed: they fill it
    caps = {"one page": lens[0], "largest - 1": max(lens) - 1, "1": 1, "three pages": three}
    blk = engine.open_v2block(c.paths[enc], data_mode=OD)
    try:
        base, _ = engine.find([blk], c.probe)
        assert base == c.want
        for name, cap in caps.items():
            T.debug_set("find_stage_bytes", cap)
            c0 = engine.resident_counters(0)
            got, _ = engine.find([blk], c.probe)
            c1 = engine.resident_counters(0)
            assert got == base, name
            want_rounds = model_rounds(lens, cap)
            assert c1["find_rounds"] - c0["find_rounds"] == want_rounds, name
            assert c1["find_read_bytes"] - c0["find_read_bytes"] == sum(lens), name
            assert want_rounds == len(lens) if cap == 1 else 1 < want_rounds <= len(lens), name
            assert name != "three pages" or want_rounds <= len(lens) // 2
    finally:
        T.debug_set("find_stage_bytes", 0)
        blk.close()
    # the default cap: one round
    c0 = engine.resident_counters(0)
    assert find_one(engine, c.paths[enc], c.probe, OD) == base
    c1 = engine.resident_counters(0)
    assert c1["find_rounds"] - c0["find_rounds"] == 1


def mixed_want(c, nblocks):
    """Every block holds the same ids: the oracle's list with each hit once per block."""
    return [(i, b, st, obj) for i, _, st, obj in c.want for b in range(nblocks)]


@pytest.mark.parametrize("cap", [0, 1, "one page"], ids=["default", "cap-1", "cap-one-page"])
def test_mixed_call_on_one_device(engine, corpus, cap):
    """An on-demand lz4 block, a resident snappy one and an on-demand zstd one: the resident pages lie
    between the staged ones in page order and ride in the first round."""
    c = corpus
    order = [(T.ENC_LZ4_256K, OD), (T.ENC_SNAPPY, T.V2_DATA_RESIDENT), (T.ENC_ZSTD, OD)]
    blocks = [engine.open_v2block(c.paths[e], data_mode=m) for e, m in order]
    try:
        T.debug_set("find_stage_bytes", c.pages[T.ENC_LZ4_256K][0][1] if cap == "one page" else cap)
        c0 = engine.resident_counters(0)
        got, _ = engine.find(blocks, c.probe)
        c1 = engine.resident_counters(0)
    finally:
        T.debug_set("find_stage_bytes", 0)
        for b in blocks:
            b.close()
    assert got == mixed_want(c, 3)
    staged = [ln for e in (T.ENC_LZ4_256K, T.ENC_ZSTD) for _, ln in c.pages[e]]
    assert c1["find_read_bytes"] - c0["find_read_bytes"] == sum(staged)
    assert c1["find_rounds"] - c0["find_rounds"] == (1 if cap == 0 else len(staged) if cap == 1 else
                                                     model_rounds(staged, c.pages[T.ENC_LZ4_256K][0][1]))


def test_mixed_call_on_two_devices(corpus):
    """Two device contexts (both on ordinal 0, as tests/test_gpu_lookup.py does it): a resident block and an
    on-demand one on the first, an on-demand one on the second; the per-device lists merge."""
    c = corpus
    eng = T.Engine(devices=[0, 0])
    order = [(T.ENC_NONE, T.V2_DATA_RESIDENT, 0), (T.ENC_ZSTD, OD, 1), (T.ENC_SNAPPY, OD, 0), (T.ENC_LZ4_256K, OD, 1)]
    blocks = [eng.open_v2block(c.paths[e], device=d, data_mode=m) for e, m, d in order]
    try:
        got, _ = eng.find(blocks, c.probe)
        T.debug_set("find_stage_bytes", 1)
        small, _ = eng.find(blocks, c.probe)
    finally:
        T.debug_set("find_stage_bytes", 0)
        for b in blocks:
            b.close()
        eng.close()
    assert got == mixed_want(c, 4)
    assert small == got


def copy_of(c, enc, tmp_path):
    dst = os.path.join(str(tmp_path), "copy%d" % enc)
    shutil.copytree(c.paths[enc], dst)
    return dst


def test_file_is_held_not_reopened(engine, corpus, tmp_path):
    c = corpus
    path = copy_of(c, T.ENC_SNAPPY, tmp_path)
    blk = engine.open_v2block(path, data_mode=OD)
    try:
        os.rename(os.path.join(path, "data"), os.path.join(path, "data.moved"))
        got, _ = engine.find([blk], c.probe)
        again, _ = engine.find([blk], c.probe)
    finally:
        blk.close()
    assert got == c.want and again == c.want


@pytest.mark.parametrize("enc", [T.ENC_NONE, T.ENC_ZSTD], ids=["none", "zstd"])
def test_truncated_after_the_open(engine, corpus, tmp_path, enc):
    c = corpus
    path = copy_of(c, enc, tmp_path)
    start, ln = c.pages[enc][-1]
    last = len(c.pages[enc]) - 1
    blk = engine.open_v2block(path, data_mode=OD)
    try:
        os.truncate(os.path.join(path, "data"), start + ln // 2)
        got, _ = engine.find([blk], c.probe)
        err = T.lib().tsg_last_error().decode()
        T.debug_set("find_stage_bytes", 1)  # the damaged page in a round of its own
        small, _ = engine.find([blk], c.probe)
        lk, _ = engine.lookup([blk], c.probe)
    finally:
        T.debug_set("find_stage_bytes", 0)
        blk.close()
    assert "the file ends inside the page" in err and str(start) in err
    assert small == got and [g[:2] for g in got] == [w[:2] for w in c.want] == [(int(r[0]), int(r[1])) for r in lk]
    nbad = 0
    for g, w, row in zip(got, c.want, lk):
        if row[2] == last:  # the hit's index record is the last page's
            assert g[2] == T.TSG_E_CORRUPT and g[3] is None, g[:3]
            nbad += 1
        else:
            assert g == w
    assert nbad >= c.rec.count(last) > 0 and nbad < len(got) - 200  # (its stored ids, and the ghosts it would hold)


@pytest.mark.parametrize("enc", [T.ENC_SNAPPY, T.ENC_LZ4_256K, T.ENC_ZSTD], ids=["snappy", "lz4-256k", "zstd"])
def test_flipped_payload_byte(engine, corpus, tmp_path, enc):
    """Whatever the resident open of the damaged directory reports for the page, the on-demand one
    reports; the hits of the other pages are untouched."""
    c = corpus
    path = copy_of(c, enc, tmp_path)
    start, ln = c.pages[enc][3]
    with open(os.path.join(path, "data"), "r+b") as f:
        f.seek(start + ln // 2)
        b = f.read(1)
        f.seek(start + ln // 2)
        f.write(bytes([b[0] ^ 0x5A]))
    res = find_one(engine, path, c.probe, T.V2_DATA_RESIDENT)
    od = find_one(engine, path, c.probe, OD)
    assert od == res
    blk = engine.open_v2block(path, data_mode=OD)
    try:
        lk, _ = engine.lookup([blk], c.probe)
    finally:
        blk.close()
    differs = [int(row[2]) for g, w, row in zip(od, c.want, lk) if g != w]
    assert differs and set(differs) == {3}


def test_no_data_file(engine, corpus, tmp_path):
    c = corpus
    path = copy_of(c, T.ENC_SNAPPY, tmp_path)
    os.remove(os.path.join(path, "data"))
    res = find_one(engine, path, c.probe, T.V2_DATA_RESIDENT)
    od = find_one(engine, path, c.probe, OD)
    assert od == res
    assert [g[:2] for g in od] == [w[:2] for w in c.want]
    assert all(g[2] == T.TSG_E_UNSUPPORTED and g[3] is None for g in od)


def test_lookup_is_the_same(engine, corpus):
    c = corpus
    for enc in ENCS:
        rows = []
        for mode in (T.V2_DATA_RESIDENT, OD):
            blk = engine.open_v2block(c.paths[enc], data_mode=mode)
            try:
                rows.append(engine.lookup([blk], c.probe)[0])
            finally:
                blk.close()
        np.testing.assert_array_equal(rows[0], rows[1])
        rc, hits = O.lookup([O.V2Block(c.paths[enc])], c.probe)
        assert rc == 0
        np.testing.assert_array_equal(rows[1], np.array(hits, dtype=np.int64).reshape(-1, 5))


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """A block of 6 or 7 pages of 2 MB, uncompressed: (path, ids, objects, data file length)."""
    rng = random.Random(5)
    n = 288
    raw = sorted({rng.randbytes(16) for _ in range(n)})
    ids = np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(-1, 16)
    objs = [rng.randbytes(40_000 + 16 * i) for i in range(n)]
    path = os.path.join(str(tmp_path_factory.mktemp("on_demand_big")), "big")
    T.write_v2_block(path, ids, objs, encoding=T.ENC_NONE, index_downsample_bytes=2_000_000)
    data_len = os.path.getsize(os.path.join(path, "data"))
    assert data_len > 11_000_000 and 5 <= len(pages_of(path)) <= 7
    return path, ids, objs, data_len


def test_hbm_stays_free(engine, big):
    """The on-demand open leaves the data file's length of device memory free that the resident open
    takes (hipMemGetInfo around the opens, one 2 MiB allocation granule of margin), and its finds,
    read by several threads, equal the resident block's."""
    import torch
    path, ids, objs, data_len = big
    free0 = torch.cuda.mem_get_info(0)[0]
    od = engine.open_v2block(path, data_mode=OD)
    free1 = torch.cuda.mem_get_info(0)[0]
    res = engine.open_v2block(path)
    free2 = torch.cuda.mem_get_info(0)[0]
    try:
        assert (free1 - free2) - (free0 - free1) >= data_len - (2 << 20), (free0, free1, free2, data_len)
        pick = ids[::3]
        got, _ = engine.find([od], pick)
        assert got == engine.find([res], pick)[0]
        assert [(g[0], g[2]) for g in got] == [(i, T.TSG_OK) for i in range(len(pick))]
        assert all(g[3] == objs[3 * g[0]] for g in got)
    finally:
        od.close()
        res.close()


def test_staging_is_freed_with_the_context(big):
    """Three contexts in turn, each serving one on-demand find of every page (12 MB staged, 12 MB
    decoded) and closing: while a context is open its staging and arena show in hipMemGetInfo, and
    the device's free memory after the third close is that after the first (a context that kept
    its staging buffer would leave 24 MB less; the margin is one 2 MiB granule)."""
    import torch
    path, ids, objs, data_len = big
    after = []
    for _ in range(3):
        before = torch.cuda.mem_get_info(0)[0]
        eng = T.Engine(devices=[0])
        blk = eng.open_v2block(path, data_mode=OD)
        try:
            got, _ = eng.find([blk], ids)
            held = before - torch.cuda.mem_get_info(0)[0]
        finally:
            blk.close()
            eng.close()
        assert len(got) == len(ids) and all(g[2] == T.TSG_OK for g in got)
        assert held >= 2 * data_len - (2 << 20), (held, data_len)
        after.append(torch.cuda.mem_get_info(0)[0])
    assert after[2] >= after[0] - (2 << 20), after
