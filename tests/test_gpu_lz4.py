"""lz4 page encodings (backend.Encoding 2..5) on the device and through the loaders:
findOne over lz4 v2 pages (find_decode_lz4_kernel), the decoder's edge cases (asserted to be
present in the writer's output), checksummed frames, three fixed damaged pages, and the
search / WAL / proto loaders, each against the block's ENC_NONE (or snappy) twin or the oracle
run on that twin. The host side of the same parser: tests/test_lz4_host.py."""
import os
import random
import struct

import numpy as np
import pytest

from oracle import oracle as O
import tempo_amd as T
from tests.helpers import match_key, random_entries, tsg_key, write_block

pytestmark = pytest.mark.gpu
LZ4 = [T.ENC_LZ4_64K, T.ENC_LZ4_256K, T.ENC_LZ4_1M, T.ENC_LZ4_4M]
WORDS = [b"span", b"trace", b"service", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select"]


def wordy(rng, n):
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS) + str(rng.randrange(1000)).encode()
    return bytes(out[:n])


def seq_ids(n):
    ids = np.zeros((n, 16), dtype=np.uint8)
    ids[:, 0] = 0x40
    ids[:, 14] = np.arange(n) >> 8
    ids[:, 15] = np.arange(n) & 255
    return ids


def page_spans(data):
    """[(payload start, payload end)] of a v2 data file."""
    off, out = 0, []
    while off < len(data):
        (tl,) = struct.unpack_from("<I", data, off)
        out.append((off + 6, off + tl))
        off += tl
    return out


def parse_frame(f):
    """Blocks of one of the writer's frames: (stored, decoded length, [(decoded position, literals,
    offset, match length, position of the offset bytes in f)])."""
    flags, o, blocks = f[4], 7, []
    while True:
        (x,) = struct.unpack_from("<I", f, o)
        o += 4
        if x == 0:
            return blocks
        size, stored = x & 0x7FFFFFFF, bool(x >> 31)
        s, end, d, seqs = o, o + size, 0, []
        while not stored:
            tok = f[s]
            s += 1
            ll = tok >> 4
            if ll == 15:
                while True:
                    ll += f[s]
                    s += 1
                    if f[s - 1] != 255:
                        break
            s += ll
            d += ll
            if s == end:
                seqs.append((d - ll, ll, 0, 0, -1))
                break
            off, at = f[s] | f[s + 1] << 8, s
            s += 2
            ml = 4 + (tok & 15)
            if tok & 15 == 15:
                while True:
                    ml += f[s]
                    s += 1
                    if f[s - 1] != 255:
                        break
            seqs.append((d - ll, ll, off, ml, at))
            d += ml
        blocks.append((stored, size if stored else d, seqs))
        o = end + (4 if flags & 16 else 0)


def find_all(engine, path, ids):
    blk = engine.open_v2block(path)
    try:
        got, _ = engine.find([blk], ids)
    finally:
        blk.close()
    return got


def one_per_page(path, objs, enc):
    """A block whose every object (> 1000 bytes) is a page of its own: page k holds object k."""
    assert all(len(o) > 1000 for o in objs)
    T.write_v2_block(path, seq_ids(len(objs)), objs, encoding=enc, index_downsample_bytes=1000)
    data = open(os.path.join(path, "data"), "rb").read()
    spans = page_spans(data)
    assert len(spans) == len(objs)
    return data, spans


def check_pages(engine, path, objs, bad=()):
    """Every object comes back byte-exact, except those of the pages in `bad`: TSG_E_CORRUPT."""
    got = find_all(engine, path, seq_ids(len(objs)))
    assert [g[0] for g in got] == list(range(len(objs)))
    for i, _, st, obj in got:
        if i in bad:
            assert st == T.TSG_E_CORRUPT and obj is None, (i, st)
        else:
            assert st == T.TSG_OK and obj == objs[i], (i, st)


@pytest.mark.parametrize("enc", LZ4, ids=[T.tsg.ENC_NAMES[e] for e in LZ4])
def test_find_on_lz4_pages(engine, tmp_path, enc):
    rng = random.Random(enc)
    n = 400
    raw = sorted({rng.randbytes(16) for _ in range(n)})
    ids = np.frombuffer(b"".join(raw), dtype=np.uint8).reshape(-1, 16)
    objs = [wordy(rng, rng.randrange(500, 3500)) if i % 9 else rng.randbytes(rng.randrange(200, 3000)) for i in range(n)]
    paths = {}
    for e in (enc, T.ENC_NONE):
        paths[e] = os.path.join(str(tmp_path), "b%d" % e)
        T.write_v2_block(paths[e], ids, objs, encoding=e, index_downsample_bytes=100_000)
    assert 5 <= len(page_spans(open(os.path.join(paths[enc], "data"), "rb").read())) <= 12
    absent = np.frombuffer(random.Random(99).randbytes(16 * 50), dtype=np.uint8).reshape(-1, 16)
    probe = np.concatenate([ids, absent])
    got = find_all(engine, paths[enc], probe)
    twin = find_all(engine, paths[T.ENC_NONE], probe)
    assert got == twin  # the same hit list, statuses and bytes as the uncompressed twin
    found = {i: obj for i, _, st, obj in got if st == T.TSG_OK}
    assert sorted(found) == list(range(n))
    assert all(found[i] == objs[i] for i in range(n))
    assert all(st == T.TSG_E_NOT_FOUND for i, _, st, _ in got if i >= n)  # bloom false positives


def test_decoder_edges(engine, tmp_path):
    rng = random.Random(77)
    R, C = rng.randbytes(40), rng.randbytes(2000)
    small = [
        b"\x07" * 400 + wordy(rng, 2000),                 # a match of offset 1, >= 300 (and >= 19 + 255) long
        rng.randbytes(70_000),                            # a stored first block
        wordy(rng, 65_536 - 24),                          # exactly one full block (24: the object's header)
        wordy(rng, 65_537 - 24),                          # and one byte more
        wordy(rng, 3000) + rng.randbytes(3000) + wordy(rng, 3000),  # a literal run >= 15 + 255 + 1
    ]
    big = [
        wordy(rng, 1000) + R + bytes(65_535 - 40) + R + wordy(rng, 1000),       # a match of offset 65 535
        wordy(rng, 70_000) + C + bytes(60_500) + C + wordy(rng, 8000),          # the ring wraps
    ]
    p64, p256 = os.path.join(str(tmp_path), "e64"), os.path.join(str(tmp_path), "e256")
    d64, s64 = one_per_page(p64, small, T.ENC_LZ4_64K)
    d256, s256 = one_per_page(p256, big, T.ENC_LZ4_256K)
    f64 = [parse_frame(d64[a:b]) for a, b in s64]
    f256 = [parse_frame(d256[a:b]) for a, b in s256]
    # the writer's output holds every case
    assert any(off == 1 and ml >= 300 for _, _, off, ml, _ in f64[0][0][2])
    assert f64[1][0][0] and f64[1][0][1] == 65_536
    assert [b[1] for b in f64[2]] == [65_536] and [b[1] for b in f64[3]] == [65_536, 1]
    assert any(ll >= 15 + 255 + 1 for _, ll, _, _, _ in f64[4][0][2])
    assert any(off == 65_535 for _, _, off, _, _ in f256[0][0][2])
    assert len(f256[1]) == 1 and f256[1][0][1] > 131_072
    assert any(off > 60_000 and d + ll > 65_536 and ml >= 1000 for d, ll, off, ml, _ in f256[1][0][2])
    check_pages(engine, p64, small)
    check_pages(engine, p256, big)


@pytest.mark.parametrize("bits", [3, 6], ids=["sum-of-decoded", "sum-of-stored"])
def test_checksummed_frames(engine, tmp_path, bits):
    rng = random.Random(bits)
    objs = [wordy(rng, 30_000), rng.randbytes(5000), wordy(rng, 150_000), b"ab" * 4000, wordy(rng, 2000)]
    path = os.path.join(str(tmp_path), "c")
    try:
        T.debug_set("lz4_writer_flags", bits)
        data, spans = one_per_page(path, objs, T.ENC_LZ4_64K)
    finally:
        T.debug_set("lz4_writer_flags", 0)
    assert all(data[a + 4] == 0x40 | 32 | 16 | 4 for a, _ in spans)
    check_pages(engine, path, objs)
    # one payload byte of page 2 flipped (inside its second block's data)
    blocks = parse_frame(data[spans[2][0]:spans[2][1]])
    assert len(blocks) == 3 and not blocks[1][0]
    at = spans[2][0] + blocks[1][2][0][4] - 1  # a literal byte of the second block's first sequence
    assert blocks[1][2][0][1] > 0
    with open(os.path.join(path, "data"), "r+b") as f:
        f.seek(at)
        f.write(bytes([data[at] ^ 0x20]))
    check_pages(engine, path, objs, bad={2})


def test_damaged_pages(engine, tmp_path):
    """A truncated frame (a block that claims more bytes than the page has), a match offset
    of 0 and a block size above the frame's maximum: the hits on those pages report
    TSG_E_CORRUPT, their neighbours are untouched."""
    rng = random.Random(13)
    objs = [b"\x07" * 400 + wordy(rng, 3000 + 500 * i) for i in range(7)]
    path = os.path.join(str(tmp_path), "d")
    data, spans = one_per_page(path, objs, T.ENC_LZ4_64K)
    frames = [parse_frame(data[a:b]) for a, b in spans]
    patch = {}
    (size,) = struct.unpack_from("<I", data, spans[1][0] + 7)
    patch[spans[1][0] + 7] = struct.pack("<I", size + 100)                # 1: truncated
    first_match = next(s for s in frames[3][0][2] if s[2])
    patch[spans[3][0] + first_match[4]] = b"\x00\x00"                      # 3: offset 0
    patch[spans[5][0] + 7] = struct.pack("<I", 65_537)                     # 5: above the 64 KiB maximum
    with open(os.path.join(path, "data"), "r+b") as f:
        for at, b in patch.items():
            f.seek(at)
            f.write(b)
    check_pages(engine, path, objs, bad={1, 3, 5})


@pytest.fixture(scope="module")
def search_twin(tmp_path_factory):
    """3000 entries in pages of 4096 bytes, written once at ENC_NONE: the twin of every lz4 block."""
    d = str(tmp_path_factory.mktemp("twin"))
    ents = random_entries(random.Random(21), 3000)
    return ents, write_block(d, "n", ents, T.ENC_NONE, page_size=4096)


@pytest.mark.parametrize("enc", LZ4, ids=[T.tsg.ENC_NAMES[e] for e in LZ4])
def test_search_block_opens_like_its_twin(engine, tmp_path, search_twin, enc):
    ents, twin = search_twin
    p = write_block(str(tmp_path), "s", ents, enc, page_size=4096)
    blk, tb = engine.open_block(p), engine.open_block(twin)
    try:
        info, tinfo = blk.info(), tb.info()
        assert info["encoding"] == enc and tinfo["encoding"] == T.ENC_NONE
        assert info["entries"] == 3000 and info["pages"] > 20 and info["stop_status"] == 0
        assert [info[k] for k in ("entries", "pages", "fb_bytes")] == [tinfo[k] for k in ("entries", "pages", "fb_bytes")]
        assert blk.tags() == tb.tags() and len(blk.tags()) >= 8
        for k in (b"k1", b"root.name", b"absent"):
            assert blk.tag_values(k) == tb.tag_values(k)
    finally:
        blk.close()
        tb.close()


def assert_oracle_parity(got, met, exp, omet):
    assert [tsg_key(m) for m in got] == [match_key(m) for m in exp]
    assert (met.inspected_traces, met.inspected_bytes, met.inspected_blocks, met.skipped_blocks, met.block_status) == \
        (omet["traces_inspected"], omet["bytes_inspected"], omet["blocks_inspected"], omet["blocks_skipped"],
         omet["block_status"])


@pytest.mark.parametrize("enc", [T.ENC_LZ4_64K, T.ENC_LZ4_4M], ids=["lz4-64k", "lz4"])
def test_search_block(engine, tmp_path, search_twin, enc):
    ents, twin = search_twin
    p = write_block(str(tmp_path), "s", ents, enc, page_size=4096)
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


def wal_result(engine, path, enc, n):
    blk = engine.open_wal_block(path)
    try:
        info = blk.info()
        assert info["encoding"] == enc and info["streaming"] == 1 and info["partial"] == 0 and info["entries"] == n
        out = [[info[k] for k in ("entries", "pages", "keys", "fb_bytes", "min_dur_ns", "max_dur_ns")], blk.tags()]
        for tags in ({}, {"k2": "v1-x"}):  # every entry, then a filtered search
            got, met = engine.search([blk], T.Pipeline(T.SearchRequest(tags=dict(tags))))
            out.append(([tsg_key(m) for m in got], met.inspected_traces, met.inspected_bytes))
        return out
    finally:
        blk.close()


@pytest.mark.parametrize("enc", [T.ENC_LZ4_1M, T.ENC_LZ4_256K], ids=["lz4-1M", "lz4-256k"])
def test_wal_replays_like_its_snappy_twin(engine, tmp_path, enc):
    ents = random_entries(random.Random(22), 300)
    res = {}
    for e in (enc, T.ENC_SNAPPY):
        d = os.path.join(str(tmp_path), "w%d" % e)
        os.makedirs(d)
        p = os.path.join(d, T.wal_filename(e))
        assert ":v2:%s:" % T.tsg.ENC_NAMES[e] in p
        T.write_wal_search(p, ents, e)
        res[e] = wal_result(engine, p, e, 300)
    assert res[enc] == res[T.ENC_SNAPPY]
    assert len(res[enc][2][0]) == 300 and 10 < len(res[enc][3][0]) < 300


def test_wal_damaged_page_and_unsupported(engine, tmp_path):
    ents = random_entries(random.Random(23), 40)
    d = os.path.join(str(tmp_path), "w")
    os.makedirs(d)
    p = os.path.join(d, T.wal_filename(T.ENC_LZ4_1M))
    T.write_wal_search(p, ents, T.ENC_LZ4_1M)
    data = bytearray(open(p, "rb").read())
    spans = page_spans(bytes(data))
    data[spans[25][0] + 6] ^= 1  # page 25: header checksum; the 25 pages before it are replayed
    with open(p, "wb") as f:
        f.write(data)
    blk = engine.open_wal_block(p)
    info = blk.info()
    blk.close()
    assert info["partial"] == 1 and info["entries"] == 25
    # s2 and gzip stay out
    for name in ("s2", "gzip"):
        q = os.path.join(str(tmp_path), name)
        os.makedirs(q)
        q = os.path.join(q, T.wal_filename(T.ENC_SNAPPY).replace("snappy", name))
        with open(q, "wb") as f:
            f.write(bytes(data))
        with pytest.raises(T.TsgError) as ei:
            engine.open_wal_block(q)
        assert ei.value.code == T.TSG_E_UNSUPPORTED_ENCODING


def test_proto_block(engine, tmp_path):
    from tests.test_gpu_proto import key, make_block
    res = {}
    for enc in (T.ENC_LZ4_1M, T.ENC_NONE):
        path = os.path.join(str(tmp_path), "p%d" % enc)
        make_block(path, random.Random(31), 300, True, enc)
        blk = engine.open_proto_block(path)
        assert blk.info()["objects"] == 300
        res[enc] = [key(engine.proto_search(blk, **q)) for q in
                    (dict(start=0, end=2 ** 32 - 1, limit=1000), dict(tags={"service.name": "cart"}, start=0, end=2 ** 32 - 1, limit=20),
                     dict(tags={"http.url": "/api"}, start=0, end=2 ** 32 - 1, limit=1000, chunk_size_bytes=10_000))]
        blk.close()
    assert res[T.ENC_LZ4_1M] == res[T.ENC_NONE] and len(res[T.ENC_NONE][0][0]) > 100
