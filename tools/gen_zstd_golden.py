#!/usr/bin/env python3
"""Writes tests/golden/zstd/: zstd frames made by an independent encoder (the libzstd that pyarrow
carries), each the payload of one v2 data page holding one object, in the forms the block
writer's own compressor does not produce or that the device decoder treats specially (Huffman
table reuse and repeat offsets across blocks, raw and RLE blocks, 1-stream Huffman, an offset
above 65 536, two frames back to back, a leading skippable frame). The manifest records each
page's id, the sha256 of its decoded bytes and what tools/zstd_host_check.cpp --stats saw in it;
tests/test_zstd_writer.py asserts from the manifest that every case is really present.
Run once; the tests read only the committed files."""
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import pyarrow as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "zstd")

WORDS = [b"span", b"trace", b"service.name=", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select ",
         b"http.status_code", b"\x0a\x12\x08"]


def plain(seed: int, n: int) -> bytes:
    out, i = bytearray(), 0
    while len(out) < n:
        h = hashlib.sha256(b"%d:%d" % (seed, i)).digest()
        out += WORDS[h[0] % len(WORDS)] + h[2:2 + h[1] % 6].hex().encode()
        i += 1
    return bytes(out[:n])


def noise(seed: int, n: int, alphabet: bytes = bytes(range(256))) -> bytes:
    out, i = bytearray(), 0
    while len(out) < n:
        out += bytes(alphabet[b % len(alphabet)] for b in hashlib.sha256(b"n%d:%d" % (seed, i)).digest())
        i += 1
    return bytes(out[:n])


def page(k: int, obj: bytes) -> bytes:
    """One marshalled object (object.go:25-48) under the id of case k."""
    tid = bytes([0x40, k]) + bytes(14)
    return struct.pack("<II", len(obj) + 24, 16) + tid + obj


def z(data: bytes, level: int) -> bytes:
    return pa.Codec("zstd", compression_level=level).compress(data, asbytes=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    r = noise(7, 1000)
    cases = [  # (name, object, level, what the frame must show)
        ("text40k_low", plain(1, 40_000), 1, "compressed"),
        ("text40k_high", plain(1, 40_000), 19, "compressed"),
        ("text300k_low", plain(2, 300_000), 1, "multi_block"),
        ("text300k_high", plain(2, 300_000), 19, "multi_block"),
        ("random5k", noise(3, 5000), 3, "raw_block"),
        # (the object's header keeps the first block from being a run: the second block is all one byte)
        ("run100k", b"\x07" * (131_072 - 24 + 100_000), 3, "rle_block"),
        ("text200", plain(4, 200), 3, "one_stream"),
        ("far_offset", r + noise(5, 100_000, b"abcd") + r, 19, "far_offset"),
        ("two_frames", plain(6, 30_000), 3, "two_frames"),
        ("skippable_first", plain(8, 20_000), 3, "skippable"),
    ]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "zcheck")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "tempo_amd", "csrc"),
                               os.path.join(ROOT, "tools", "zstd_host_check.cpp"), "-o", exe])
        manifest = []
        for k, (name, obj, level, case) in enumerate(cases):
            pg = page(k, obj)
            if case == "two_frames":
                frame = z(pg[:11_000], level) + z(pg[11_000:], level)
            elif case == "skippable":
                frame = struct.pack("<II", 0x184D2A53, 12) + b"not a frame!" + z(pg, level)
            else:
                frame = z(pg, level)
            path = os.path.join(OUT, name + ".zst")
            with open(path, "wb") as f:
                f.write(frame)
            stats = json.loads(subprocess.check_output([exe, "--stats", path]))
            assert stats["status"] == 0 and stats["bytes"] == len(pg), (name, stats)
            manifest.append({"file": name + ".zst", "case": case, "level": level, "id": pg[8:24].hex(),
                             "decoded_bytes": len(pg), "sha256": hashlib.sha256(pg).hexdigest(), "stats": stats})
            print(name, len(frame), stats, file=sys.stderr)
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
