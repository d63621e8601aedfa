"""The zstd page writer (tempo_amd/csrc/zstd_enc.hpp, encoding 7) without a GPU: its frames
round-trip through an independent zstd (libzstd through pyarrow) and through the host build of
the device decoders; every zstd_writer_flags bit produces the form it names (asserted from the
stats mode of tools/zstd_host_check.cpp); the golden frames of tests/golden/zstd still hold the
cases they were made for; and a stand-alone ASan + UBSan build of the decoders and the compressor
survives 3000 mutations of writer and golden frames plus three fixed damage patterns per frame.
The device side: tests/test_gpu_zstd.py."""
import hashlib
import json
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import tempo_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "zstd")
WORDS = [b"span", b"trace", b"service", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select"]
# tsg_debug_set("zstd_writer_flags", bits)
CHECKSUM, RAW_LIT, DIRECT_W, FSE_W, FSE_SEQ, LIT_ONLY = 1, 2, 4, 8, 16, 32


def wordy(rng, n):
    out = bytearray()
    while len(out) < n:
        out += rng.choice(WORDS) + str(rng.randrange(1000)).encode()
    return bytes(out[:n])


def far_input(rng):
    """1000 bytes R, 100 KB of low-entropy filler, R again: the second R is a match of offset 101 000."""
    r = rng.randbytes(1000)
    return r + bytes(rng.choice(b"abcd") for _ in range(100_000)) + r


def edge_inputs():
    """name -> object; an object's page is 24 bytes longer (its header), hence the '- 24'."""
    rng = random.Random(5)
    return {
        "empty": b"", "one_byte": b"x", "random_70000": rng.randbytes(70_000), "run_100000": b"\x07" * 100_000,
        "text_block": wordy(rng, 131_072 - 24), "text_block_plus_1": wordy(rng, 131_073 - 24),
        "text_300000": wordy(rng, 300_000), "far_offset": far_input(rng),
    }


def seq_ids(n):
    ids = np.zeros((n, 16), dtype=np.uint8)
    ids[:, 0] = 0x40
    ids[:, 14] = np.arange(n) >> 8
    ids[:, 15] = np.arange(n) & 255
    return ids


def page_spans(data):
    off, out = 0, []
    while off < len(data):
        (tl,) = struct.unpack_from("<I", data, off)
        out.append((off + 6, off + tl))
        off += tl
    return out


def build_zcheck(path, *flags):
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "tempo_amd", "csrc"),
                           os.path.join(ROOT, "tools", "zstd_host_check.cpp"), "-o", path])
    return path


@pytest.fixture(scope="module")
def zcheck(tmp_path_factory):
    return build_zcheck(str(tmp_path_factory.mktemp("z") / "zcheck"), "-O2")


def writer_pages(tmpdir, name, objs, flags=0):
    """The writer's pages (one per object) as (data file path, [payload bytes])."""
    path = os.path.join(tmpdir, name)
    try:
        T.debug_set("zstd_writer_flags", flags)
        T.write_v2_block(path, seq_ids(len(objs)), objs, encoding=T.ENC_ZSTD, index_downsample_bytes=1)
    finally:
        T.debug_set("zstd_writer_flags", 0)
    data = open(os.path.join(path, "data"), "rb").read()
    spans = page_spans(data)
    assert len(spans) == len(objs)
    return os.path.join(path, "data"), [data[a:b] for a, b in spans]


def host_decode(zcheck, path):
    out = subprocess.run([zcheck, path], check=True, capture_output=True).stdout
    res, o = [], 0
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


def stats_of(zcheck, path):
    return [json.loads(ln) for ln in subprocess.check_output([zcheck, "--stats", path]).splitlines()]


def libzstd(frame, n):
    """The independent pin: libzstd through pyarrow (only the tests that call this need pyarrow)."""
    pa = pytest.importorskip("pyarrow")
    if not pa.Codec.is_available("zstd"):
        pytest.skip("pyarrow without zstd")
    return pa.Codec("zstd").decompress(frame, decompressed_size=n, asbytes=True) if n else b""


@pytest.fixture(scope="module")
def edge_pages(tmp_path_factory, zcheck):
    objs = edge_inputs()
    path, frames = writer_pages(str(tmp_path_factory.mktemp("edge")), "e", list(objs.values()))
    return objs, path, frames, stats_of(zcheck, path)


def test_writer_round_trips(edge_pages, zcheck):
    objs, path, frames, stats = edge_pages
    pages = [T.marshal_objects([i], [o]) for i, o in zip(seq_ids(len(objs)), objs.values())]
    decoded = host_decode(zcheck, path)  # (both host decoders; they must agree or the tool fails)
    for name, frame, page, got in zip(objs, frames, pages, decoded):
        assert frame[:4] == b"\x28\xb5\x2f\xfd", name
        assert struct.unpack_from("<I", frame, 6)[0] == len(page), name  # the frame content size
        assert libzstd(frame, len(page)) == page, name
        assert got == page, name


def test_writer_block_forms(edge_pages):
    objs, _, frames, stats = edge_pages
    st = dict(zip(objs, stats))
    assert all(s["status"] == 0 for s in stats)
    assert st["random_70000"]["blocks"] == {"raw": 1, "rle": 0, "compressed": 0}  # compression does not pay
    assert st["run_100000"]["blocks"]["compressed"] == 1  # (the object's header, then a match of offset 1)
    assert sum(st["text_block"]["blocks"].values()) == 1 and sum(st["text_block_plus_1"]["blocks"].values()) == 2
    assert st["text_300000"]["blocks"]["compressed"] == 3 and st["text_300000"]["streams"]["4"] >= 2
    assert st["text_300000"]["seq_tables"]["predefined"] == 9 and st["text_300000"]["repeat_offsets"] > 0
    assert st["far_offset"]["max_offset"] > 65_536
    assert st["text_300000"]["max_offset"] > 131_072  # a match that reaches back past the block before


def test_writer_rle_block_and_repeat_offset(tmp_path, zcheck):
    rng = random.Random(8)
    r = rng.randbytes(64)
    again = bytearray(r)
    again[20] ^= 0xFF  # two matches of offset 64 around one literal: the second repeats the offset
    objs = [b"\x07" * (2 * 131_072), r + bytes(again) + wordy(rng, 1200)]
    path, frames = writer_pages(str(tmp_path), "r", objs)
    s = stats_of(zcheck, path)
    assert s[0]["blocks"]["rle"] >= 1  # the second block of the run is one byte throughout
    assert s[1]["repeat_offsets"] >= 1
    for i, (o, f) in enumerate(zip(objs, frames)):
        page = T.marshal_objects([seq_ids(2)[i]], [o])
        assert libzstd(f, len(page)) == page
    assert host_decode(zcheck, path) == [T.marshal_objects([seq_ids(2)[i]], [o]) for i, o in enumerate(objs)]


FLAG_CASES = {
    # bits -> (object, what the stats must show)
    "checksum": (CHECKSUM, "text", lambda s, f: f[4] & 4 and s["literals"]["huffman"] >= 1),
    "raw_literals": (RAW_LIT, "text", lambda s, f: s["literals"] == {"raw": 1, "rle": 0, "huffman": 0, "treeless": 0}),
    # (literals-only blocks hold 64 KiB: the second one is the run alone)
    "rle_literals": (LIT_ONLY, "run", lambda s, f: s["literals"]["rle"] == 1 and s["blocks"] == {"raw": 0, "rle": 0, "compressed": 2}),
    "literals_only": (LIT_ONLY | RAW_LIT, "text", lambda s, f: s["literals"]["raw"] >= 1 and s["seq_tables"]["predefined"] == 0
                      and s["blocks"] == {"raw": 0, "rle": 0, "compressed": s["blocks"]["compressed"]}),
    "huffman_1_stream": (0, "text200", lambda s, f: s["streams"] == {"1": 1, "4": 0}),
    "huffman_4_streams": (0, "text", lambda s, f: s["streams"] == {"1": 0, "4": 1}),
    "direct_weights": (DIRECT_W, "text", lambda s, f: s["weights"] == {"fse": 0, "direct": 1}),
    "fse_weights": (FSE_W, "text", lambda s, f: s["weights"] == {"fse": 1, "direct": 0}),
    "predefined_tables": (0, "text", lambda s, f: s["seq_tables"] == {"predefined": 3, "rle": 0, "fse": 0, "repeat": 0}),
    "fse_tables": (FSE_SEQ, "text", lambda s, f: s["seq_tables"]["predefined"] == 0 and s["seq_tables"]["fse"] >= 2
                   and s["seq_tables"]["fse"] + s["seq_tables"]["rle"] == 3),
}


def flag_objects():
    rng = random.Random(9)
    return {"text": wordy(rng, 30_000), "run": b"\x07" * 70_000, "text200": wordy(rng, 230)}


@pytest.mark.parametrize("case", sorted(FLAG_CASES))
def test_writer_flag_produces_its_form(tmp_path, zcheck, case):
    bits, which, check = FLAG_CASES[case]
    obj = flag_objects()[which]
    path, frames = writer_pages(str(tmp_path), "f", [obj], bits)
    (s,) = stats_of(zcheck, path)
    assert s["status"] == 0 and check(s, frames[0]), s
    page = T.marshal_objects([seq_ids(1)[0]], [obj])
    assert libzstd(frames[0], len(page)) == page
    assert host_decode(zcheck, path) == [page]


def golden_manifest():
    return json.load(open(os.path.join(GOLDEN, "manifest.json")))


def test_golden_cases_are_present(zcheck):
    """The frames of an independent encoder still hold what they were made for (the stats are taken
    again here, not read from the manifest), and decode through both host decoders."""
    want = {
        "compressed": lambda s: s["blocks"]["compressed"] >= 1 and s["streams"]["4"] >= 1 and s["seq_tables"]["fse"] >= 1,
        "multi_block": lambda s: s["blocks"]["compressed"] >= 3 and s["repeat_offsets"] > 0 and s["max_offset"] > 131_072,
        "raw_block": lambda s: s["blocks"]["raw"] >= 1,
        "rle_block": lambda s: s["blocks"]["rle"] >= 1,
        "one_stream": lambda s: s["streams"]["1"] >= 1,
        "far_offset": lambda s: s["max_offset"] > 65_536,
        "two_frames": lambda s: s["blocks"]["compressed"] == 2,
        "skippable": lambda s: s["blocks"]["compressed"] >= 1,
    }
    man = golden_manifest()
    assert {m["case"] for m in man} == set(want)
    for m in man:
        path = os.path.join(GOLDEN, m["file"])
        assert os.path.getsize(path) < 150_000
        (s,) = stats_of(zcheck, path)
        assert s == m["stats"] and s["status"] == 0, m["file"]
        assert want[m["case"]](s), (m["file"], s)
        (page,) = host_decode(zcheck, path)
        assert len(page) == m["decoded_bytes"] and hashlib.sha256(page).hexdigest() == m["sha256"], m["file"]
        assert page[8:24].hex() == m["id"] and struct.unpack_from("<II", page, 0) == (len(page), 16)
    frame = open(os.path.join(GOLDEN, "skippable_first.zst"), "rb").read()
    assert struct.unpack_from("<I", frame, 0)[0] & 0xFFFFFFF0 == 0x184D2A50
    two = open(os.path.join(GOLDEN, "two_frames.zst"), "rb").read()
    assert two.count(b"\x28\xb5\x2f\xfd") >= 2
    # treeless literals (a Huffman table reused across blocks) and a repeated sequence table occur somewhere
    assert any(m["stats"]["literals"]["treeless"] for m in man) and any(m["stats"]["seq_tables"]["repeat"] for m in man)


def test_sanitized_decoders_survive_mutations(tmp_path, edge_pages):
    """ASan + UBSan, stand-alone (its own main, nothing preloaded): the three fixed damage patterns of
    tests/test_gpu_zstd.py on every writer frame, then 3000 single-byte and truncation mutations of
    writer and golden frames through both decoders; --encode runs the compressor under the same build."""
    exe = build_zcheck(str(tmp_path / "zcheck_san"), "-O1", "-g", "-fsanitize=address,undefined",
                       "-fno-sanitize-recover=undefined")
    _, path, _, _ = edge_pages
    flagged, _ = writer_pages(str(tmp_path), "m", list(flag_objects().values()), FSE_SEQ | FSE_W | CHECKSUM)
    golden = [os.path.join(GOLDEN, m["file"]) for m in golden_manifest()]
    r = subprocess.run([exe, "--fuzz", "3000", "11", path, flagged, *golden], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = json.loads(r.stdout)
    assert out["mutations"] == 3000 and out["fixed"] >= 3 * 7 and out["corrupt"] > 1000 and out["ok"] > len(golden)
    src = tmp_path / "in.bin"
    src.write_bytes(flag_objects()["text"])
    for bits in (0, CHECKSUM | FSE_SEQ | FSE_W, DIRECT_W, LIT_ONLY):
        r = subprocess.run([exe, "--encode", str(bits), str(src), str(tmp_path / "out.zst")], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
        assert libzstd((tmp_path / "out.zst").read_bytes(), 30_000) == flag_objects()["text"]


def test_loaders_and_names_accept_zstd():
    assert T.ENC_ZSTD == 7 and ":v2:zstd:" in T.wal_filename(T.ENC_ZSTD)
