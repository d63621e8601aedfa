#!/usr/bin/env python3
"""Writes tests/golden/lz4/: LZ4 frames in the variants that neither the block writer nor
pyarrow emits (linked blocks, block / content checksums, content size, a leading skippable
frame, bytes after the end mark, the larger block sizes), made with the system liblz4
(LZ4F_compressFrame through ctypes). Each frame's plaintext is plain(seed, n) below; the
manifest records seed and n, and tests/test_lz4_host.py regenerates it the same way.
Run once; the tests read only the committed files."""
import ctypes as C
import hashlib
import json
import os
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lz4")

WORDS = [b"span", b"trace", b"service.name=", b"GET /api/v1/users/", b"\x00\x00\x10", b"db.statement select ",
         b"http.status_code", b"\x0a\x12\x08"]


def plain(seed: int, n: int) -> bytes:
    out, i = bytearray(), 0
    while len(out) < n:
        h = hashlib.sha256(b"%d:%d" % (seed, i)).digest()
        out += WORDS[h[0] % len(WORDS)] + h[2:2 + h[1] % 6].hex().encode()
        i += 1
    return bytes(out[:n])


class FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int),
                ("frameType", C.c_int), ("contentSize", C.c_ulonglong), ("dictID", C.c_uint),
                ("blockChecksumFlag", C.c_int)]


class Prefs(C.Structure):
    _fields_ = [("frameInfo", FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint),
                ("favorDecSpeed", C.c_uint), ("reserved", C.c_uint * 3)]


def compress(lib, data, block_id=4, linked=False, csum=False, bsum=False, csize=False):
    p = Prefs()
    p.frameInfo.blockSizeID = block_id
    p.frameInfo.blockMode = 0 if linked else 1
    p.frameInfo.contentChecksumFlag = int(csum)
    p.frameInfo.blockChecksumFlag = int(bsum)
    p.frameInfo.contentSize = len(data) if csize else 0
    cap = lib.LZ4F_compressFrameBound(len(data), C.byref(p))
    dst = C.create_string_buffer(cap)
    n = lib.LZ4F_compressFrame(dst, cap, data, len(data), C.byref(p))
    assert not lib.LZ4F_isError(n), n
    return dst.raw[:n]


def main():
    lib = C.CDLL("liblz4.so.1")
    lib.LZ4F_compressFrameBound.restype = C.c_size_t
    lib.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
    lib.LZ4F_compressFrame.restype = C.c_size_t
    lib.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p]
    lib.LZ4F_isError.argtypes = [C.c_size_t]
    os.makedirs(OUT, exist_ok=True)
    variants = [
        ("linked_64k", 200_000, dict(linked=True)),
        ("block_checksum", 150_000, dict(bsum=True)),
        ("content_checksum", 100_000, dict(csum=True)),
        ("content_size", 70_000, dict(csize=True)),
        ("linked_all_flags", 200_000, dict(linked=True, bsum=True, csum=True, csize=True)),
        ("skippable_first", 5_000, dict()),
        ("trailing_bytes", 5_000, dict(csum=True)),
        ("block_256k", 300_000, dict(block_id=5)),
        ("block_1m", 300_000, dict(block_id=6)),
        ("block_4m", 1_100_000, dict(block_id=7)),  # (liblz4 lowers the id to the smallest that holds the input)
    ]
    manifest = []
    for seed, (name, n, kw) in enumerate(variants, 1):
        frame = compress(lib, plain(seed, n), **kw)
        if name == "skippable_first":
            frame = struct.pack("<II", 0x184D2A53, 7) + b"skipped" + frame
        if name == "trailing_bytes":
            frame += b"bytes after the content checksum"
        with open(os.path.join(OUT, name + ".lz4"), "wb") as f:
            f.write(frame)
        manifest.append(dict(file=name + ".lz4", seed=seed, n=n, sha256=hashlib.sha256(plain(seed, n)).hexdigest()))
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
