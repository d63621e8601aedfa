"""Snappy framed streams assembled by hand (chunk headers, masked CRC-32C, block tags), for the
host and the device decoder: tests/test_snappy_frames.py runs them through the oracle,
tests/test_gpu_snappy.py through findOne. Format: vendor/github.com/golang/snappy/decode.go:121-232
(framing), decode_other.go:41-102 (block tags), decode.go:32-43 (the decoded-length varint).

Every frame decodes to the marshalled form of exactly one object of at least 1000 bytes
([u32 total][u32 16][id][object], object.go:25-48), so a block written from a list of frames with
write_v2_block_pages has page k = frame k, and frame k is built for the id frame_id(k).

ACCEPTED and REJECTED are lists of Case(name, build): build(id) -> (payload, page). `payload` is the
framed stream; `page` is what it decodes to (ACCEPTED), or what it would decode to without its one
damage (REJECTED)."""
import random
import struct
from collections import namedtuple

from oracle import oracle as O

Case = namedtuple("Case", "name build")
MAX_BLOCK = 65536
HDR = 24  # [u32 total][u32 id length][16 id bytes]


def frame_id(k):
    return bytes([0x40]) + bytes(13) + bytes([k >> 8, k & 255])


def rnd(n, seed):
    return random.Random(seed).randbytes(n)


# ---- block ops: what a block is made of; X is raw bytes the model below does not execute ---------
def L(data, nb=None):
    """A literal; nb forces the number of length-extension bytes (0: the length is in the tag)."""
    return ("L", data, nb)


def C1(off, n):
    return ("C", 1, off, n)


def C2(off, n):
    return ("C", 2, off, n)


def C4(off, n):
    return ("C", 4, off, n)


def X(raw):
    return ("X", raw)


def copy_bytes(kind, off, n):
    if kind == 1:
        assert 4 <= n <= 11 and off < 2048
        return bytes([(off >> 8) << 5 | (n - 4) << 2 | 1, off & 255])
    assert 1 <= n <= 64
    return bytes([(n - 1) << 2 | (2 if kind == 2 else 3)]) + off.to_bytes(2 if kind == 2 else 4, "little")


def literal_tag(n, nb=None):
    m = n - 1
    if nb is None:
        nb = 0 if m < 60 else (m.bit_length() + 7) // 8
    if nb == 0:
        assert m < 60
        return bytes([m << 2])
    return bytes([(59 + nb) << 2]) + m.to_bytes(nb, "little")


def block_bytes(ops):
    out = bytearray()
    for op in ops:
        if op[0] == "L":
            out += literal_tag(len(op[1]), op[2]) + op[1]
        elif op[0] == "C":
            out += copy_bytes(*op[1:])
        else:
            out += op[1]
    return bytes(out)


def run(ops):
    """What the ops decode to (X skipped): the model the expected pages come from."""
    d = bytearray()
    for op in ops:
        if op[0] == "L":
            d += op[1]
        elif op[0] == "C":
            _, _, off, n = op
            assert 0 < off <= len(d)
            for _ in range(n):
                d.append(d[-off])
    return bytes(d)


# ---- chunks --------------------------------------------------------------------------------------
def mask(c):
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF  # snappy.go:61-64


def uvarint(v, pad=0):
    """v as a varint, padded with continuation bytes to `pad` bytes when that is longer."""
    out = bytearray()
    while v >= 0x80:
        out.append(v & 0x7F | 0x80)
        v >>= 7
    out.append(v)
    while len(out) < pad:
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def chunk(ctype, body, length=None):
    return bytes([ctype]) + (len(body) if length is None else length).to_bytes(3, "little") + body


IDENT = chunk(0xFF, b"sNaPpY")


def Z(ops, ulen=None, varint=None, crc_xor=0, length=None):
    """A compressed chunk (0x00): [crc of the decoded bytes][varint decoded length][block]. ulen: the
    declared decoded length when not the model's; varint: the length's bytes when not the shortest."""
    dec = run(ops)
    vb = varint if varint is not None else uvarint(len(dec) if ulen is None else ulen)
    body = struct.pack("<I", mask(O.crc32c(dec)) ^ crc_xor) + vb + block_bytes(ops)
    return chunk(0x00, body, length), dec


def U(data):
    """An uncompressed chunk (0x01): [crc][bytes]."""
    return chunk(0x01, struct.pack("<I", mask(O.crc32c(data))) + data), data


def RAW(data):
    """Bytes between the data chunks that decode to nothing."""
    return data, b""


def case(name, parts_of, tail=b""):
    """parts_of(h) -> the stream's parts, each (bytes, decoded bytes), where h is the page's 24-byte
    object header and the first decoded bytes start with it. The total length the header states is
    learnt from a first pass with a blank header."""
    def build(tid):
        total = sum(len(dec) for _, dec in parts_of(bytes(HDR)))
        h = struct.pack("<II", total, 16) + tid
        parts = parts_of(h)
        page = b"".join(dec for _, dec in parts)
        assert page[:HDR] == h and len(page) == total >= HDR + 1000
        return b"".join(raw for raw, _ in parts) + tail, page
    return Case(name, build)


# ---- accepted ------------------------------------------------------------------------------------
def _literals(h):
    # lengths 60 (the longest held in the tag), 1, 61 (one extension byte), 257 (two), 2 spelled with four
    return [RAW(IDENT), Z([L(h + rnd(36, 1)), L(rnd(1, 2)), L(rnd(61, 3)), L(rnd(257, 4)), L(rnd(2, 5), nb=4),
                           L(rnd(700, 6))])]


def _full_block_three_byte_literal(h):
    # one chunk of exactly 65 536 bytes, a single literal whose length takes three extension bytes
    return [RAW(IDENT), Z([L(h + rnd(MAX_BLOCK - HDR, 7), nb=3)])]


def _copies(h):
    ops = [L(h + rnd(100, 8)),
           C1(1, 11),             # periodic: offset below length
           L(rnd(2000, 9)),
           C1(2047, 8),           # the largest copy-1 offset
           C2(2100, 64),          # copy-2, the longest copy, offset >= 2048
           C4(300, 40),           # copy-4
           C2(3, 64)]             # periodic copy-2
    d = len(run(ops))
    ops.append(C2(d, HDR))        # offset = decoded position: reaches the block's first byte
    d += HDR
    assert d < 3072 - 40
    ops.append(L(rnd(3072 - 10 - d, 10)))
    ops.append(C2(500, 30))       # crosses a 1024-byte boundary of the decoded block (3072)
    ops.append(L(rnd(50, 11)))
    return [RAW(IDENT), Z(ops)]


def _two_chunks(h):
    # 65 536 + 1 decoded bytes: a full chunk and a chunk of one byte
    return [RAW(IDENT), Z([L(h + rnd(3000, 12)), C2(2900, 64), L(rnd(MAX_BLOCK - HDR - 3064, 13))]), Z([L(b"\x5a")])]


def _chunk_types(h):
    # an uncompressed chunk, a skippable one, padding and a second stream identifier between data chunks
    return [RAW(IDENT), U(h + rnd(600, 14)), RAW(chunk(0x80, b"skip me")), Z([L(rnd(300, 15)), C1(5, 9)]),
            RAW(chunk(0xFE, bytes(13))), RAW(IDENT), Z([L(rnd(200, 16)), C2(150, 33)])]


def _base_ops(h):
    return [L(h + rnd(500, 17)), C1(7, 9), L(rnd(600, 18))]


def _varint(pad):
    def parts(h):
        ops = _base_ops(h)
        return [RAW(IDENT), Z(ops, varint=uvarint(len(run(ops)), pad))]
    return parts


ACCEPTED = [
    case("literals", _literals),
    case("full-block-three-byte-literal", _full_block_three_byte_literal),
    case("copies", _copies),
    case("two-chunks-65537", _two_chunks),
    case("chunk-types", _chunk_types),
    case("varint-padded-to-6", _varint(6)),
    case("varint-padded-to-10", _varint(10)),
]


# ---- rejected: the intact frame below with one damage each -----------------------------------------
def _intact(h):
    return [RAW(IDENT), Z(_base_ops(h))]


INTACT = case("intact", _intact)


def _z(**kw):
    return lambda h: [RAW(IDENT), Z(_base_ops(h), **kw)]


def _block(tail_ops, grow):
    """The intact block followed by tail_ops; the declared length counts `grow` bytes for them."""
    def parts(h):
        ops = _base_ops(h)
        return [RAW(IDENT), Z(ops + tail_ops(len(run(ops))), ulen=len(run(ops)) + grow)]
    return parts


def _tenth_byte_2(h):
    # the intact length spelled in 10 bytes whose last is 2: binary.Uvarint's overflow
    ops = _base_ops(h)
    n = len(run(ops))
    assert 0x80 <= n < 0x4000
    return [RAW(IDENT), Z(ops, varint=bytes([n & 0x7F | 0x80, n >> 7 | 0x80]) + b"\x80" * 7 + b"\x02")]


REJECTED = [
    # framing
    case("checksum-flipped", _z(crc_xor=1)),
    case("chunk-length-past-page", lambda h: [RAW(IDENT), Z(_base_ops(h), length=4000)]),
    case("partial-chunk-header", _intact, tail=b"\xfe\x00\x00"),
    case("no-stream-identifier", lambda h: [Z(_base_ops(h))]),
    case("wrong-stream-identifier", lambda h: [RAW(chunk(0xFF, b"sNaPpy")), Z(_base_ops(h))]),
    case("reserved-unskippable-chunk", lambda h: [RAW(IDENT), RAW(chunk(0x02, b"xx")), Z(_base_ops(h))]),
    case("uncompressed-chunk-below-4", lambda h: [RAW(IDENT), RAW(chunk(0x01, b"abc")), Z(_base_ops(h))]),
    # decoded length
    case("length-above-65536", _z(ulen=MAX_BLOCK + 1)),
    case("length-above-block", _block(lambda d: [], 1)),
    case("length-below-block", _block(lambda d: [], -1)),
    case("varint-tenth-byte-2", _tenth_byte_2),
    # block contents
    case("literal-past-block", _block(lambda d: [X(literal_tag(20) + bytes(15))], 20)),
    case("copy-offset-0", _block(lambda d: [X(copy_bytes(2, 0, 10))], 10)),
    case("copy-offset-above-position", _block(lambda d: [X(copy_bytes(2, d + 1, 10))], 10)),
    case("copy-2-cut-off", _block(lambda d: [X(copy_bytes(2, 100, 10)[:2])], 10)),
]
