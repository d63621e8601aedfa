"""The lz4 frame decoder (tempo_amd/csrc/lz4_dev.hpp), built for the host by
tools/lz4_host_check.cpp, against independent encoders:

* pyarrow's lz4 codec (LZ4 frames, 64 KiB independent blocks) over pages of 0 B .. 1.1 MB;
* frames made once with liblz4 in the variants pyarrow does not emit (tests/golden/lz4,
  tools/gen_lz4_golden.py): linked blocks, block / content checksums, content size, a leading
  skippable frame, bytes after the frame, 256 KiB / 1 MiB / 4 MiB block sizes;
* the project's own writer at encodings 2..5 (decoded here and by pyarrow);
* hand-built frames the reference Reader rejects: each gives TSG_E_CORRUPT;
* the same binary built with -fsanitize=address,undefined over the rejections and over
  3000 single-byte mutations of three valid frames (fixed seed): it must end clean.
The same parser runs on the GPU in find.hip (tests/test_gpu_lz4.py)."""
import hashlib
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lz4")
E_CORRUPT, E_UNSUPPORTED = 2, 8
SIZES = [0, 1, 17, 1000, 65_535, 65_536, 65_537, 300_000, 1_100_000]


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", *extra, os.path.join(ROOT, "tools", "lz4_host_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def lcheck(tmp_path_factory):
    return _build(tmp_path_factory, "lcheck", ["-O2"])


@pytest.fixture(scope="module")
def lcheck_san(tmp_path_factory):
    return _build(tmp_path_factory, "lcheck_san",
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def page(frame):
    return struct.pack("<IH", len(frame) + 6, 0) + frame


def pages_of(data):
    off, out = 0, []
    while off < len(data):
        tl, hl = struct.unpack_from("<IH", data, off)
        out.append(data[off + 6 + hl:off + tl])
        off += tl
    return out


def run(exe, path):
    p = subprocess.run([exe, path], capture_output=True)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    assert p.stderr == b""
    out, res, o = p.stdout, [], 0
    while o < len(out):
        (l,) = struct.unpack_from("<I", out, o)
        o += 4
        if l == 0xFFFFFFFF:
            res.append(struct.unpack_from("<i", out, o)[0])
            o += 4
        else:
            res.append(out[o:o + l])
            o += l
    return res


def run_frames(exe, tmp_path, frames, name="pages"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(b"".join(page(fr) for fr in frames))
    got = run(exe, p)
    assert len(got) == len(frames)
    return got


def synth(rng, kind, n):
    if kind == 0:
        return rng.randbytes(n)
    if kind == 1:
        words = [b"span", b"trace", b"service", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select"]
        out = bytearray()
        while len(out) < n:
            out += rng.choice(words) + str(rng.randrange(1000)).encode()
        return bytes(out[:n])
    if kind == 2:
        return bytes([rng.randrange(3)]) * n
    base = rng.randbytes(257)
    return (base * (n // 257 + 1))[:n]


# ---- xxh32 and a frame builder of the test's own (xxHash / LZ4 frame specifications) ----------
P1, P2, P3, P4, P5, M = 2654435761, 2246822519, 3266489917, 668265263, 374761393, 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M


def xxh32(b, seed=0):
    n, i = len(b), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while i + 16 <= n:
            for q in range(4):
                v[q] = _rotl((v[q] + struct.unpack_from("<I", b, i + 4 * q)[0] * P2) & M, 13) * P1 & M
            i += 16
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while i + 4 <= n:
        h = _rotl((h + struct.unpack_from("<I", b, i)[0] * P3) & M, 17) * P4 & M
        i += 4
    while i < n:
        h = _rotl((h + b[i] * P5) & M, 11) * P1 & M
        i += 1
    h ^= h >> 15
    h = h * P2 & M
    h ^= h >> 13
    h = h * P3 & M
    return h ^ (h >> 16)


F_CSUM, F_SIZE, F_BSUM, F_INDEP = 4, 8, 16, 32


def header(flags=F_INDEP, idx=4, csize=None, hc_xor=0):
    d = bytes([0x40 | flags | (F_SIZE if csize is not None else 0), idx << 4])
    if csize is not None:
        d += struct.pack("<Q", csize)
    return struct.pack("<I", 0x184D2204) + d + bytes([((xxh32(d) >> 8) & 0xFF) ^ hc_xor])


def block(data, stored=False, bsum=None):
    out = struct.pack("<I", len(data) | (0x80000000 if stored else 0)) + data
    return out + (struct.pack("<I", bsum) if bsum is not None else b"")


END = b"\x00\x00\x00\x00"
SEQ = bytes([0x14]) + b"a" + b"\x01\x00" + bytes([0x50]) + b"bbbbb"  # 'a', 8 x 'a' (offset 1), 'bbbbb'
SEQ_OUT = b"a" * 9 + b"bbbbb"


def test_xxh32_vectors():
    assert xxh32(b"") == 0x02CC5D05  # the xxHash specification's empty-input value
    d = bytes([0x60, 0x40])  # pyarrow's descriptor: its header checksum byte is 0x82
    assert (xxh32(d) >> 8) & 0xFF == 0x82


def test_pyarrow_pages(lcheck, tmp_path):
    pa = pytest.importorskip("pyarrow")
    if not pa.Codec.is_available("lz4"):
        pytest.skip("pyarrow without lz4")
    rng = random.Random(11)
    codec = pa.Codec("lz4")
    contents = [synth(rng, kind, n) for n in SIZES for kind in range(4)]
    frames = [codec.compress(c, asbytes=True) for c in contents]
    assert frames[4][:6] == bytes.fromhex("04224d186040")
    got = run_frames(lcheck, tmp_path, frames)
    for c, g in zip(contents, got):
        assert g == c


def golden_plain(seed, n):
    words = [b"span", b"trace", b"service.name=", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select ",
             b"http.status_code", b"\x0a\x12\x08"]
    out, i = bytearray(), 0
    while len(out) < n:
        h = hashlib.sha256(b"%d:%d" % (seed, i)).digest()
        out += words[h[0] % len(words)] + h[2:2 + h[1] % 6].hex().encode()
        i += 1
    return bytes(out[:n])


def test_golden_variants(lcheck, tmp_path):
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    assert len(man) == 10
    frames = {m["file"]: open(os.path.join(GOLDEN, m["file"]), "rb").read() for m in man}
    # the variants are what their names say (FLG bits, BD index)
    flg = {k: v[4] for k, v in frames.items() if k != "skippable_first.lz4"}
    assert not flg["linked_64k.lz4"] & F_INDEP and not flg["linked_all_flags.lz4"] & F_INDEP
    assert flg["block_checksum.lz4"] & F_BSUM and flg["content_checksum.lz4"] & F_CSUM
    assert flg["content_size.lz4"] & F_SIZE and flg["linked_all_flags.lz4"] & (F_BSUM | F_CSUM | F_SIZE) == 28
    assert [frames[f][5] >> 4 for f in ("block_256k.lz4", "block_1m.lz4", "block_4m.lz4")] == [5, 6, 7]
    assert frames["skippable_first.lz4"][:4] == struct.pack("<I", 0x184D2A53)
    got = run_frames(lcheck, tmp_path, [frames[m["file"]] for m in man])
    for m, g in zip(man, got):
        plain = golden_plain(m["seed"], m["n"])
        assert hashlib.sha256(plain).hexdigest() == m["sha256"]
        assert g == plain, m["file"]


def test_handmade_accepted(lcheck, tmp_path):
    linked = (header(flags=F_BSUM | F_CSUM) + block(b"abcdefghij", stored=True, bsum=xxh32(b"abcdefghij")) +
              block(bytes([0x04, 10, 0, 0x50]) + b"vwxyz", bsum=xxh32(b"abcdefghvwxyz")) + END +
              struct.pack("<I", xxh32(b"abcdefghijabcdefghvwxyz")))
    frames = [
        header() + END,
        header() + block(SEQ) + END + b"trailing",
        header(flags=F_INDEP | F_BSUM) + block(SEQ, bsum=xxh32(SEQ_OUT)) + END,  # the reference's form
        header(flags=F_INDEP | F_BSUM) + block(SEQ, bsum=xxh32(SEQ)) + END,      # the frame format's form
        header(csize=len(SEQ_OUT)) + block(SEQ) + END,
        struct.pack("<II", 0x184D2AFF, 3) + b"xyz" + header() + block(b"stored", stored=True) + END,
        linked,
        header(idx=7) + block(b"", stored=True) + block(SEQ) + END,
    ]
    got = run_frames(lcheck, tmp_path, frames)
    assert got == [b"", SEQ_OUT, SEQ_OUT, SEQ_OUT, SEQ_OUT, b"stored", b"abcdefghijabcdefghvwxyz", SEQ_OUT]


def rejections():
    ok = header() + block(SEQ) + END
    long_match = bytes([0x1F]) + b"a" + b"\x01\x00" + b"\xff" * 274 + bytes([111, 0x50]) + b"bbbbb"  # 70 000
    return {
        "bad magic": b"\x05" + ok[1:],
        "bad header checksum": header(hc_xor=1) + block(SEQ) + END,
        "invalid block-size index": header(idx=3) + block(SEQ) + END,
        "block size above the maximum": header() + block(b"x" * 70_000, stored=True) + END,
        "compressed block size above the maximum": header() + block(bytes([0xF0]) + b"\xff" * 300 + b"x" * 70_000) + END,
        "truncated block": ok[:len(header()) + 4 + 5],
        "truncated before the end mark": ok[:-4],
        "offset 0": header() + block(bytes([0x14]) + b"a" + b"\x00\x00" + bytes([0x50]) + b"bbbbb") + END,
        "offset before the start": header() + block(bytes([0x14]) + b"a" + b"\x02\x00" + bytes([0x50]) + b"bbbbb") + END,
        "literal run past the input": header() + block(bytes([0xF0, 0xFF, 0x10]) + b"a") + END,
        "block ends inside a sequence": header() + block(bytes([0x14]) + b"a" + b"\x01") + END,
        "match past the block maximum": header() + block(long_match) + END,
        "wrong block checksum": header(flags=F_INDEP | F_BSUM) + block(SEQ, bsum=xxh32(SEQ_OUT) ^ 1) + END,
        "wrong content checksum": header(flags=F_INDEP | F_CSUM) + block(SEQ) + END + struct.pack("<I", xxh32(SEQ_OUT) ^ 1),
        "missing content checksum": header(flags=F_INDEP | F_CSUM) + block(SEQ) + END,
        "content size that disagrees": header(csize=len(SEQ_OUT) + 1) + block(SEQ) + END,
        "content size above what the block headers allow": header(csize=1 << 30) + block(SEQ) + END,
        "content size too small": header(csize=len(SEQ_OUT) - 1) + block(SEQ) + END,
        "linked offset before the frame": header(flags=0) + block(b"abc", stored=True) + block(bytes([0x04, 4, 0, 0x50]) + b"vwxyz") + END,
        "empty": b"",
    }


def test_rejections(lcheck, tmp_path):
    rej = rejections()
    got = run_frames(lcheck, tmp_path, list(rej.values()))
    assert dict(zip(rej, got)) == {k: E_CORRUPT for k in rej}
    legacy = struct.pack("<I", 0x184C2102) + block(SEQ)
    assert run_frames(lcheck, tmp_path, [legacy], "legacy") == [E_UNSUPPORTED]


def test_sanitizer_build(lcheck_san, tmp_path):
    rej = rejections()
    assert run_frames(lcheck_san, tmp_path, list(rej.values()), "rej") == [E_CORRUPT] * len(rej)
    rng = random.Random(2024)
    valid = [open(os.path.join(GOLDEN, "skippable_first.lz4"), "rb").read(),
             open(os.path.join(GOLDEN, "trailing_bytes.lz4"), "rb").read(),
             header(flags=F_BSUM | F_CSUM) + block(b"abcdefghij", stored=True, bsum=xxh32(b"abcdefghij")) +
             block(bytes([0x04, 10, 0, 0x50]) + b"vwxyz", bsum=xxh32(b"abcdefghvwxyz")) + END +
             struct.pack("<I", xxh32(b"abcdefghijabcdefghvwxyz"))]
    assert all(isinstance(g, bytes) for g in run_frames(lcheck_san, tmp_path, valid, "valid"))
    frames = []
    for v in valid:
        for _ in range(1000):
            m = bytearray(v)
            m[rng.randrange(len(m))] = rng.randrange(256)
            frames.append(bytes(m))
    got = run_frames(lcheck_san, tmp_path, frames, "mut")  # (run() asserts exit 0 and an empty stderr)
    assert all(isinstance(g, bytes) or g in (E_CORRUPT, E_UNSUPPORTED) for g in got)
    # a checksummed frame notices a changed payload byte: most mutations are rejected
    assert sum(1 for g in got[1000:2000] if g == E_CORRUPT) > 900


# ---- the project's own writer -------------------------------------------------------------------
def test_own_writer(lcheck, tmp_path):
    import tempo_amd as T
    try:
        import pyarrow as pa
        codec = pa.Codec("lz4") if pa.Codec.is_available("lz4") else None
    except ImportError:
        codec = None
    rng = random.Random(5)
    n = 40
    ids = np.zeros((n, 16), dtype=np.uint8)
    ids[:, 15] = np.arange(n)
    objs = [synth(rng, i % 4, rng.choice([10, 3000, 40_000, 150_000])) for i in range(n)]
    T.write_v2_block(str(tmp_path / "none"), ids, objs, encoding=T.ENC_NONE, index_downsample_bytes=100_000)
    want = pages_of(open(tmp_path / "none" / "data", "rb").read())
    assert len(want) > 5 and max(map(len, want)) > 65_536
    entries = [dict(id=bytes([i]) * 16, start=i, end=i + 5, tags={"k%d" % (i % 7): ["v%d" % i, "svc"]}) for i in range(50)]
    T.write_wal_search(str(tmp_path / "wal_none"), entries, T.ENC_NONE)
    want_wal = pages_of(open(tmp_path / "wal_none", "rb").read())
    for enc, idx in ((T.ENC_LZ4_64K, 4), (T.ENC_LZ4_256K, 5), (T.ENC_LZ4_1M, 6), (T.ENC_LZ4_4M, 7)):
        d = tmp_path / ("e%d" % enc)
        T.write_v2_block(str(d), ids, objs, encoding=enc, index_downsample_bytes=100_000)
        assert '"encoding":"%s"' % T.tsg.ENC_NAMES[enc] in open(d / "meta.json").read().replace(" ", "")
        frames = pages_of(open(d / "data", "rb").read())
        assert len(frames) == len(want)
        for f in frames:  # the frame the reference Writer emits: independent blocks, no checksums, BD by encoding
            assert f[:7] == header(idx=idx) and f[-4:] == END
        assert run(lcheck, str(d / "data")) == want
        if codec is not None:
            for f, w in zip(frames, want):
                assert bytes(codec.decompress(f, decompressed_size=len(w))) == w
        T.write_wal_search(str(tmp_path / ("wal%d" % enc)), entries, enc)
        assert run(lcheck, str(tmp_path / ("wal%d" % enc))) == want_wal
    assert sum(map(len, pages_of(open(tmp_path / "e2" / "data", "rb").read()))) < sum(map(len, want))


def test_writer_checksum_knob(lcheck, tmp_path):
    import tempo_amd as T
    ids = np.zeros((3, 16), dtype=np.uint8)
    ids[:, 15] = np.arange(3)
    objs = [b"abcdefgh" * 3000, random.Random(1).randbytes(5000), b"z" * 70_000]
    T.write_v2_block(str(tmp_path / "none"), ids, objs, encoding=T.ENC_NONE)
    want = pages_of(open(tmp_path / "none" / "data", "rb").read())
    try:
        for bits, flg in ((3, F_BSUM | F_CSUM), (6, F_BSUM | F_CSUM), (2, F_CSUM), (1, F_BSUM)):
            T.debug_set("lz4_writer_flags", bits)
            d = tmp_path / ("k%d" % bits)
            T.write_v2_block(str(d), ids, objs, encoding=T.ENC_LZ4_64K)
            frames = pages_of(open(d / "data", "rb").read())
            assert all(f[4] == 0x40 | F_INDEP | flg for f in frames)
            assert run(lcheck, str(d / "data")) == want
    finally:
        T.debug_set("lz4_writer_flags", 0)
    with pytest.raises(T.TsgError):
        T.write_v2_block(str(tmp_path / "gz"), ids, objs, encoding=1)
