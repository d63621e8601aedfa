"""Trace-ID lookup corpus at the shapes where the lookup kernels pick another path, and a pure-Python
model of one lookup (a second reference beside the C oracle). tests/test_lookup_cases.py holds the
oracle to the model and checks that the corpus is not vacuous; tests/test_gpu_lookup_edges.py runs the
same cases on the device.

A block here is what write_v2_block leaves (index, data: one record per id) with its bloom-N files and
meta.json written again in Python, so bloom parameters, shard counts, bit densities, meta ids and times
are the case's, not the writer's. The bloom bits are random: they need not contain the block's ids,
device and oracle only have to agree on what the bits say. All shards of a block share (m, k, bitlen).
Unsorted indexes and duplicate record ids are out of scope (the writer insists on ascending ids).

A Case is (name, paths, ids, kw, slab): the blocks in call order, the probe ids, the oracle's keyword
arguments (ts / te) and the TSG_LK_SLAB value the device call runs under (None: unset)."""
import base64
import bisect
import datetime
import json
import os
import struct
import uuid
from collections import namedtuple

import numpy as np

import tempo_amd as T

Case = namedtuple("Case", "name paths ids kw slab")
Family = namedtuple("Family", "paths ids pools")

SLAB_J = (1, 2, 31, 32, 33, 63, 64, 65, 128, 129, 255, 256, 257)
CALL_SIZES = (1, 63, 64, 65, 255, 256, 257, 256 * 130 + 1)
T0 = 1_700_000_000
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1


def as_ids(seq):
    """(n, 16) uint8 of a sequence of 16-byte ids."""
    return np.frombuffer(b"".join(seq), dtype=np.uint8).reshape(-1, 16).copy()


def b128(v):
    return int(v).to_bytes(16, "big")


def i128(b):
    return int.from_bytes(bytes(b), "big")


# ---- writing one block ---------------------------------------------------------------------------
def bloom_bytes(m, k, bitlen, density, rng):
    """willf/bloom WriteTo: big-endian m, k, bitlen, then ceil(bitlen / 64) words; bit `loc` is bit
    loc & 63 of word loc >> 6."""
    words = (bitlen + 63) // 64
    bits = np.zeros(words * 64, dtype=np.uint8)
    bits[:bitlen] = rng.random(bitlen) < density
    w = np.packbits(bits, bitorder="little").view("<u8")
    return struct.pack(">QQQ", m, k, bitlen) + w.astype(">u8").tobytes()


def rfc3339(unix):
    return datetime.datetime.fromtimestamp(unix, datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ")


def make_block(dir, ids, *, m, bitlen, k, shards, density, seed, min_id=None, max_id=None, start=None, end=None,
               drop_shards_field=False):
    """One block of the given (ascending) record ids; returns dir. min_id / max_id of any length 0..16
    (None: the writer's, the first and last record), start / end in unix seconds (None: the writer's).
    drop_shards_field removes bloomShards from the meta and writes the legacy 10 shard files.
    index_downsample_bytes=1 cuts a data page, hence an index record, after every object (0 would
    mean the writer's default of 1 MiB per record)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 16)
    T.write_v2_block(dir, ids, [b"x"] * len(ids), encoding=T.ENC_NONE, index_downsample_bytes=1)
    for f in os.listdir(dir):
        if f.startswith("bloom-"):
            os.remove(os.path.join(dir, f))
    nshards = 10 if drop_shards_field else shards
    rng = np.random.default_rng(seed)
    for s in range(nshards):
        with open(os.path.join(dir, "bloom-%d" % s), "wb") as f:
            f.write(bloom_bytes(m, k, bitlen, density, rng))
    with open(os.path.join(dir, "meta.json")) as f:
        meta = json.load(f)
    assert meta["totalRecords"] == len(ids)
    meta["bloomShards"] = nshards
    if drop_shards_field:
        del meta["bloomShards"]
    if min_id is not None:
        meta["minID"] = base64.b64encode(min_id).decode()
    if max_id is not None:
        meta["maxID"] = base64.b64encode(max_id).decode()
    if start is not None:
        meta["startTime"] = rfc3339(start)
    if end is not None:
        meta["endTime"] = rfc3339(end)
    meta["blockID"] = str(uuid.uuid5(uuid.NAMESPACE_OID, os.path.basename(dir)))
    with open(os.path.join(dir, "meta.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    return dir


# ---- the model: one lookup in plain Python ints ------------------------------------------------------
def fnv1_32(b):
    h = 2166136261
    for c in b:
        h = ((h * 16777619) & 0xFFFFFFFF) ^ c
    return h


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    return k ^ (k >> 33)


def murmur3_128(b):
    """murmur3 x64-128, seed 0 (spaolacci/murmur3 murmur128.go): (h1, h2)."""
    c1, c2 = 0x87C37B91114253D5, 0x4CF5AD432745937F
    h1 = h2 = 0
    nb = len(b) // 16
    for i in range(nb):
        k1, k2 = struct.unpack_from("<QQ", b, 16 * i)
        h1 ^= (_rotl((k1 * c1) & M64, 31) * c2) & M64
        h1 = ((_rotl(h1, 27) + h2) * 5 + 0x52DCE729) & M64
        h2 ^= (_rotl((k2 * c2) & M64, 33) * c1) & M64
        h2 = ((_rotl(h2, 31) + h1) * 5 + 0x38495AB5) & M64
    tail = b[16 * nb:]
    if len(tail) > 8:
        h2 ^= (_rotl((int.from_bytes(tail[8:], "little") * c2) & M64, 33) * c1) & M64
    if tail:
        h1 ^= (_rotl((int.from_bytes(tail[:8], "little") * c1) & M64, 31) * c2) & M64
    h1 ^= len(b)
    h2 ^= len(b)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1, h2 = _fmix(h1), _fmix(h2)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return h1, h2


def bloom_locations(h, m, k):
    """willf/bloom location(h, i) % m for i < k; h = the four base hashes (id, id || 0x01)."""
    return [((h[i % 2] + i * h[2 + (((i + (i % 2)) % 4) // 2)]) & M64) % m for i in range(k)]


class ModelBlock:
    """What a lookup reads of one block directory, parsed in Python."""

    def __init__(self, path):
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        self.min_id = base64.b64decode(meta.get("minID", ""))
        self.max_id = base64.b64decode(meta.get("maxID", ""))
        parse = lambda s: int(datetime.datetime.strptime(s, "%Y-%m-%dT%H:%M:%S%z").timestamp())  # noqa: E731
        self.start, self.end = parse(meta["startTime"]), parse(meta["endTime"])
        self.blooms = []  # per shard: (m, k, bitlen, the bits as one int)
        for s in range(meta.get("bloomShards", 0) or 10):
            with open(os.path.join(path, "bloom-%d" % s), "rb") as f:
                raw = f.read()
            m, k, bitlen = struct.unpack_from(">QQQ", raw)
            words = struct.unpack_from(">%dQ" % ((bitlen + 63) // 64), raw, 24)
            self.blooms.append((m, k, bitlen, sum(w << (64 * i) for i, w in enumerate(words))))
        with open(os.path.join(path, "index"), "rb") as f:
            idx = f.read()
        page, n = meta["indexPageSize"], meta["totalRecords"]
        per = (page - 14) // 28  # [u32 total][u16 header length = 8][u64 xxhash64] then 28-byte records
        self.rec_ids, self.rec_start, self.rec_len = [], [], []
        for r in range(n):
            o = (r // per) * page + 14 + (r % per) * 28
            self.rec_ids.append(idx[o:o + 16])
            s, ln = struct.unpack_from("<QI", idx, o + 16)
            self.rec_start.append(s)
            self.rec_len.append(ln)

    def probe(self, id, fnv, h, locs):
        """Record index of the hit, or -1: includeBlock's id range (bytes.Compare is Python's bytes
        order), the id's bloom shard, then the first record >= id."""
        if id < self.min_id or id > self.max_id:
            return -1
        m, k, bitlen, bits = self.blooms[fnv % len(self.blooms)]
        if (m, k) not in locs:
            locs[(m, k)] = bloom_locations(h, m, k)
        for loc in locs[(m, k)]:
            if loc >= bitlen or not (bits >> loc) & 1:
                return -1
        r = bisect.bisect_left(self.rec_ids, id)
        return r if r < len(self.rec_ids) else -1


def model_lookup(blocks, ids, ts=0, te=0):
    """(hits, 5) int64: id_idx, block_idx, record_idx, record_start, record_length, by (id, block)."""
    live = [(b, blk) for b, blk in enumerate(blocks)
            if not (ts != 0 and te != 0 and (blk.start >= te or blk.end <= ts))]
    out = []
    for i, row in enumerate(np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 16)):
        id = row.tobytes()
        h = murmur3_128(id) + murmur3_128(id + b"\x01")
        fnv, locs = fnv1_32(id), {}
        for b, blk in live:
            r = blk.probe(id, fnv, h, locs)
            if r >= 0:
                out.append((i, b, r, blk.rec_start[r], blk.rec_len[r]))
    return np.array(out, dtype=np.int64).reshape(-1, 5)


# ---- record sets shared by the slab, parameter and mixed families ------------------------------------
def record_pools(rng):
    """8 nested id ranges: set s spans first bytes [0x10 + 12 s, 0xef - 12 s], so an id lies in the
    min/max range of sets 0..d for some depth d (or of none), and a call sees ids with no, few and
    many candidate blocks."""
    pools = []
    for s in range(8):
        lo, hi = 0x10 + 12 * s, 0xEF - 12 * s
        body = rng.integers(0, 256, size=(100, 16), dtype=np.uint8)
        body[:, 0] = rng.integers(lo, hi + 1, size=100)
        first, last = bytes([lo]) + bytes(14) + b"\x01", bytes([hi]) + b"\xff" * 15
        pools.append((first, sorted({r.tobytes() for r in body} - {first, last}), last))
    return pools


def pool_subset(pool, rng, n=78):
    first, body, last = pool
    keep = sorted(rng.choice(len(body), size=min(n, len(body)), replace=False))
    return as_ids([first] + [body[i] for i in keep] + [last])


def probe_ids(pools, rng, nrandom=1200):
    """Every pooled record plus uniform ids, shuffled."""
    rec = [r for first, body, last in pools for r in [first] + body + [last]]
    ids = np.concatenate([as_ids(rec), rng.integers(0, 256, size=(nrandom, 16), dtype=np.uint8)])
    rng.shuffle(ids)
    return ids


# ---- slab family --------------------------------------------------------------------------------
_FIRST8 = (0.8, 0.97, 0.97, 0.97, 0.97, 0.97, 0.97, 0.97)


def slab_family(root, nblocks=257):
    """257 distinct blocks of identical bloom parameters (m = bitlen = 1000: a partial last word, k = 7,
    one shard). Block b holds ~80 records of set b % 8, has its own bloom seed and a density drawn from
    {0.6, 0.8, 0.97}: the two widest sets mostly sparse, so ids only they cover get a few hits."""
    rng = np.random.default_rng(1000)
    pools = record_pools(rng)
    paths = []
    for b in range(nblocks):
        s = b % 8
        dens = _FIRST8[b] if b < 8 else float(rng.choice([0.6, 0.8, 0.97], p=[0.9, 0.1, 0.0] if s < 2 else [1 / 3] * 3))
        paths.append(make_block(os.path.join(root, "s%03d" % b), pool_subset(pools[s], rng), m=1000, bitlen=1000, k=7,
                                shards=1, density=dens, seed=5000 + b))
    return Family(paths, probe_ids(pools, rng), pools)


def slab_cases(fam):
    return [Case("slab/J%d" % j, fam.paths[:j], fam.ids, {}, None) for j in SLAB_J]


def size_cases(fam):
    """Call sizes on tile and wave edges over two slab-family blocks, a call without a single hit and
    a call over no blocks."""
    rng = np.random.default_rng(77)
    two = fam.paths[1:3]
    cases = [Case("size/n%d" % n, two, rng.integers(0, 256, size=(n, 16), dtype=np.uint8), {}, None) for n in CALL_SIZES]
    none = rng.integers(0, 256, size=(300, 16), dtype=np.uint8)
    none[:, 0] = 0xFF  # above every set's range
    cases.append(Case("size/nohits", two, none, {}, None))
    cases.append(Case("size/noblocks", [], fam.ids[:300], {}, None))
    return cases


# ---- parameter family ---------------------------------------------------------------------------
# name, m, bitlen, k, shards, bloomShards dropped, ((record set, density), ...)
PARAMS = (
    ("m37k1", 37, 37, 1, 1, False, ((0, 0.5), (3, 0.3))),
    ("m64k2s3", 64, 64, 2, 3, False, ((0, 0.8), (3, 0.6))),
    ("m1024k8s2", 1024, 1024, 8, 2, False, ((0, 0.9), (3, 0.8))),
    ("m1000b900k7", 1000, 900, 7, 1, False, ((0, 0.97), (3, 0.9))),
    ("m1k3", 1, 1, 3, 1, False, ((5, 1.0), (2, 0.0))),
    ("m4099k13legacy", 4099, 4099, 13, 10, True, ((0, 0.95), (3, 0.9))),
    ("writer1shard", 819200, 819200, 7, 1, False, ((0, 0.9), (3, 0.8))),
    ("writer3shards", 819200, 819200, 7, 3, False, ((0, 0.9), (3, 0.8))),
)


def param_cases(root, fam):
    """Two blocks per parameter set over the slab family's record sets and probe ids."""
    rng = np.random.default_rng(2000)
    cases = []
    for n, (name, m, bitlen, k, shards, drop, blocks) in enumerate(PARAMS):
        paths = [make_block(os.path.join(root, "p_%s_%d" % (name, j)), pool_subset(fam.pools[s], rng), m=m, bitlen=bitlen,
                            k=k, shards=shards, density=d, seed=6000 + 10 * n + j, drop_shards_field=drop)
                 for j, (s, d) in enumerate(blocks)]
        cases.append(Case("param/" + name, paths, fam.ids, {}, None))
    return cases


# ---- mixed call ---------------------------------------------------------------------------------
def mixed_cases(root, fam):
    """Three parameter groups interleaved in block order: A (m = 1000, k = 7) at the even positions,
    B (m = 1024, k = 8, 2 shards) at the odd ones, the singleton C (m = 4099, k = 13, legacy shards) at
    position 5. Block i spans [T0 + 1000 i, T0 + 1000 i + 500]: the window keeps blocks 2..8."""
    rng = np.random.default_rng(3000)
    paths = []
    for i in range(11):
        par = (dict(m=4099, bitlen=4099, k=13, shards=10, drop_shards_field=True) if i == 5 else
               dict(m=1000, bitlen=1000, k=7, shards=1) if i % 2 == 0 else dict(m=1024, bitlen=1024, k=8, shards=2))
        paths.append(make_block(os.path.join(root, "x%02d" % i), pool_subset(fam.pools[i % 4], rng), density=0.97,
                                seed=7000 + i, start=T0 + 1000 * i, end=T0 + 1000 * i + 500, **par))
    win = dict(ts=T0 + 2100, te=T0 + 8200)
    return ([Case("mixed/slab=%s" % s, paths, fam.ids, {}, s) for s in (None, "1", "0")] +
            [Case("mixed/window/slab=%s" % s, paths, fam.ids, win, s) for s in (None, "1")])


# ---- index family -------------------------------------------------------------------------------
def common_prefix(a, b):
    n = 0
    while n < 16 and a[n] == b[n]:
        n += 1
    return n


def dir_shape(recs):
    """(prefix bytes, directory bits) of the index directory the device builds over these records
    (64 records and more: ~4 records per bucket over the 32 id bits after the common prefix, which
    caps at 12 bytes), or None below 64 records."""
    n = len(recs)
    if n < 64:
        return None
    bits = 0
    while (2 << bits) <= n // 4 and bits < 20:
        bits += 1
    return min(common_prefix(recs[0], recs[-1]), 12), max(bits, 1)


def index_probe_ids(recs, min_id, max_id):
    """Probe ids around everything the index search and the range check compare against."""
    vals = {0, M128}
    for r in recs:
        vals.update((i128(r) - 1, i128(r), i128(r) + 1))
    for meta in (min_id, max_id):
        for pad in (b"\x00", b"\xff"):
            v = i128((meta + pad * 16)[:16])
            vals.update((v - 1, v, v + 1))
    # ids that leave the records' common prefix in one byte, below and above it, in either half; the
    # bytes after it zero, all-ff, and a record's own
    mid = recs[len(recs) // 2]
    for j in range(common_prefix(recs[0], recs[-1]) if len(recs) > 1 else 0):
        for d in (-1, 1):
            if 0 <= mid[j] + d <= 255:
                head = mid[:j] + bytes([mid[j] + d])
                vals.update(i128(head + t[j + 1:]) for t in (bytes(16), b"\xff" * 16, mid))
    shape = dir_shape(recs)
    if shape:  # each bucket's first and last possible id
        cp, bits = shape
        for bk in range(1 << bits):
            for key, pad in ((bk << (32 - bits), b"\x00"), (((bk + 1) << (32 - bits)) - 1, b"\xff")):
                vals.add(i128((recs[0][:cp] + key.to_bytes(4, "big") + pad * 12)[:16]))
    return as_ids([b128(v) for v in sorted(vals) if 0 <= v <= M128])


def index_record_sets():
    """{name: sorted 16-byte record ids}."""
    rng = np.random.default_rng(4000)
    rnd = lambda n, w=16: [rng.integers(0, 256, size=w, dtype=np.uint8).tobytes() for _ in range(n)]  # noqa: E731
    sets = {"n%d" % n: rnd(n) for n in (1, 2, 63, 64, 65, 600)}
    pfx = bytes(range(0x41, 0x51))
    for cp in (0, 1, 7, 8, 9, 12):  # byte cp takes both halves of its range: the prefix is exactly cp bytes
        tails = rnd(200, 16 - cp)
        sets["cp%d" % cp] = [pfx[:cp] + bytes([t[0] & 0x7F if i % 2 else t[0] | 0x80]) + t[1:] for i, t in enumerate(tails)]
    sets["cp15"] = [pfx[:15] + bytes([v]) for v in rng.choice(256, size=100, replace=False)]
    # 64 buckets, 298 of 300 records in bucket 32
    sets["onebucket"] = [b"\x02" + bytes(15), b"\xfd" + b"\xff" * 15] + [b"\x80\x00\x00\x00" + t for t in rnd(298, 12)]
    sets["meta"] = rnd(600)
    return {k: sorted(set(v)) for k, v in sets.items()}


WIDE = (bytes(16), b"\xff" * 16)


def index_cases(root):
    """One saturated-bloom block per case (so every id in the meta range reaches the index search), and
    one call over all of them. Meta ids are 16 x 00 / 16 x ff unless the case name says otherwise."""
    sets = index_record_sets()
    blocks = [(name, recs, WIDE) for name, recs in sets.items() if name != "meta"]
    m = sets["meta"]
    blocks += [("meta_own", m, (None, None)), ("meta_8byte", m, (m[0][:8], m[-1][:8])),
               ("meta_1byte", m, (m[0][:1], m[-1][:1])), ("meta_emptymax", m, (bytes(16), b"")),
               # (an 8-byte max equal to the records' first 8 bytes would reject every one of them)
               ("cp12_min8", sets["cp12"], (sets["cp12"][0][:8], WIDE[1]))]
    cases = []
    for n, (name, recs, (mn, mx)) in enumerate(blocks):
        path = make_block(os.path.join(root, "i_" + name), as_ids(recs), m=64, bitlen=64, k=3, shards=1, density=1.0,
                          seed=8000 + n, min_id=mn, max_id=mx)
        ids = index_probe_ids(recs, recs[0] if mn is None else mn, recs[-1] if mx is None else mx)
        cases.append(Case("index/" + name, [path], ids, {}, None))
    every = np.concatenate([c.ids for c in cases if c.name in ("index/cp9", "index/n2", "index/onebucket", "index/meta_8byte")])
    cases.append(Case("index/all", [c.paths[0] for c in cases], every, {}, None))
    return cases
