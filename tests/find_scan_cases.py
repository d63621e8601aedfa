"""Decoded v2 data pages built byte by byte for findOne's object scan (find_scan_kernel, find.hip
step 4) and the gather behind it (step 5), a Python model of findOne on one page, and a replay of the
kernel's window tiling. tests/test_find_scan_cases.py holds the oracle to the model and asserts that
every case sits where it was aimed; tests/test_gpu_find_scan_edges.py runs the cases on the device.

A case is one page plus the ids the index sends to it (`pending`, ascending). write_block puts the
cases of a block behind each other with write_v2_block_pages: the bloom and the index are built from
the pending ids alone, the payload is free, so an id can be routed to a page that does not hold it,
holds it twice, or holds it behind damage.

findOne (finder_paged.go:79-110) reads a page through NewIterator(bytes.NewReader(page)), whose Next
is object.UnmarshalObjectFromReader (iterator.go:30-32, object.go:50-80). With R bytes left at an
object start:
  R == 0 or R == 4         io.EOF from binary.Read: the clean end, (nil, nil)
  R in 1..3, 5..7          io.ErrUnexpectedEOF
  R == 8                   r.Read at the reader's end: io.EOF whatever the header holds
  R > 8, total < 8         the uint32 length wraps: a short read, error (object.go:69-71)
  R > 8, total - 8 > R - 8 short read, error
  R > 8, il > total - 8    error (object.go:72-74)
  otherwise                id = il bytes, object = the rest; total == 8 is an empty id and object
findOne returns at the first id that bytes.Equal's the wanted one; an error reaches only an id not
found before it.

Stale bytes. The cases named windows/stale/* hold, r = 9..23 bytes before the end of a full window, an
object whose id equals a pending id X in the r - 8 id bytes inside the window and differs in every
byte beyond it; X itself is nowhere in the page. A scan that compares without sliding reads the other
24 - r id bytes from win[65536 .. 65536 + 24 - r), the 16 bytes of slack behind the window. No window
load ever writes there (a window covers at most 65536 bytes, window_trace asserts it), so those bytes
cannot be made to hold X's: what such a scan matches is not in the page's hands. What the page does
decide: a scan that compares only the bytes it has matches X wrongly, and a scan that compares against
whatever the slack holds misses the straddling object when it is the wanted one (windows/*/at, r =
9..23), since it then steps over it."""
import bisect
import random
import struct
from collections import namedtuple

import numpy as np

import tempo_amd as T
from tests import snappy_frames as F

WINDOW = 65536          # kFindWindow
PASS = 256              # kFindPer * kFindThreads: pending ids per pass
OK, NOT_FOUND, CORRUPT = T.TSG_OK, T.TSG_E_NOT_FOUND, T.TSG_E_CORRUPT
PENDING_SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
GATHER_LENGTHS = (0, 1, 255, 256, 257, 70_000)

Case = namedtuple("Case", "name page pending meta")
Family = namedtuple("Family", "name blocks ask")  # blocks: [[Case]]; ask: the ids of a find call, in order
Trace = namedtuple("Trace", "starts slides covered windows")

_BLOB = random.Random(4).randbytes(1 << 17)


def body(n, salt):
    """n bytes that differ from case to case."""
    at = (salt * 7919) % len(_BLOB)
    if at + n <= len(_BLOB):
        return _BLOB[at:at + n]
    return (_BLOB[at:] + _BLOB * (n // len(_BLOB) + 1))[:n]


def raw_obj(total, il, rest):
    return struct.pack("<II", total & 0xFFFFFFFF, il & 0xFFFFFFFF) + rest


def obj(tid, data):
    """object.MarshalObjectToWriter (object.go:25-48)"""
    return raw_obj(8 + len(tid) + len(data), len(tid), tid + data)


class Ids:
    """Ascending ids of one family: [0x40, family, 0 * 12, hi, lo], in the style of seq_ids."""

    def __init__(self, fam):
        self.fam, self.n, self.nfill = fam, 0, 0

    def take(self, n):
        out = [bytes([0x40, self.fam]) + bytes(12) + struct.pack(">H", self.n + k) for k in range(n)]
        self.n += n
        return out

    def filler(self):
        """An id no call asks for."""
        self.nfill += 1
        return bytes([0x7F, self.fam]) + bytes(10) + struct.pack(">I", self.nfill)

    def fill(self, n):
        """Whole filler objects of exactly n bytes (n == 0 or n >= 24)."""
        out = bytearray()
        while n > 3100:
            s = 24 + (self.nfill * 37) % 2977
            out += obj(self.filler(), body(s - 24, self.nfill))
            n -= s
        if n:
            assert n >= 24, n
            out += obj(self.filler(), body(n - 24, self.nfill))
        return bytes(out)


# ---- the model -------------------------------------------------------------------------------------
def model_find(page, tid):
    """(status, object or None) of findOne for `tid` on the decoded page."""
    at, end = 0, len(page)
    while True:
        left = end - at
        if left in (0, 4, 8):
            return NOT_FOUND, None
        if left < 8:
            return CORRUPT, None
        total, il = struct.unpack_from("<II", page, at)
        have = left - 8
        want = (total - 8) % (1 << 32)
        if want > have or il > want:
            return CORRUPT, None
        if page[at + 8:at + 8 + il] == tid:
            return OK, page[at + 8 + il:at + 8 + want]
        at += 8 + want


def window_trace(page):
    """The kernel's tiling of a page when no id is ever found: the window starts (page offsets), the
    slides as (object start, window end - object start), the most bytes a window covered and the number
    of windows (a last one of no bytes, after an object that ends the page at a window's end, is in
    `starts` but is not counted). For coverage assertions only."""
    L, p = len(page), 0
    starts, slides, covered = [], [], 0
    while True:
        wl = min(L - p, WINDOW)
        starts.append(p)
        covered = max(covered, wl)
        w, done = 0, False
        while True:
            R = L - (p + w)
            if R < 8:
                done = True
                break
            if wl - w < 8:
                slides.append((p + w, wl - w))
                break
            total, il = struct.unpack_from("<II", page, p + w)
            if R == 8 or total < 8 or total - 8 > R - 8 or il > total - 8:
                done = True
                break
            if il == 16 and wl - w < 24:
                slides.append((p + w, wl - w))
                break
            w += total
            if w >= wl:
                slides.append((p + w, wl - w))
                break
        if done:
            return Trace(starts, slides, covered, sum(1 for s in starts if s < L) or 1)
        assert w > 0
        p += w


# ---- blocks ----------------------------------------------------------------------------------------
def frame(page, enc):
    if enc == T.ENC_NONE:
        return page
    assert enc == T.ENC_SNAPPY
    return F.IDENT + b"".join(F.U(page[o:o + F.MAX_BLOCK])[0] for o in range(0, len(page), F.MAX_BLOCK))


def write_block(path, cases, enc=T.ENC_NONE):
    pend = [i for c in cases for i in c.pending]
    assert all(a < b for a, b in zip(pend, pend[1:])) and all(c.pending for c in cases)
    first = [0]
    for c in cases[:-1]:
        first.append(first[-1] + len(c.pending))
    ids = np.frombuffer(b"".join(pend), dtype=np.uint8).reshape(-1, 16)
    T.write_v2_block_pages(path, ids, [b""] * len(pend), first, [frame(c.page, enc) for c in cases], enc)
    return path


def page_of(cases, tid):
    """The case whose page the index names for tid: the first record (a page's last id) >= tid."""
    k = bisect.bisect_left([c.pending[-1] for c in cases], tid)
    return cases[k] if k < len(cases) else None


def as_ids(seq):
    return np.frombuffer(b"".join(seq), dtype=np.uint8).reshape(-1, 16)


def expected(blocks, ask, hits):
    """The model's (id_idx, block_idx, status, object) for the lookup's hits, in their order."""
    out = []
    for i, b in hits:
        st, o = model_find(page_of(blocks[b], ask[i]).page, ask[i])
        out.append((i, b, st, o))
    return out


# ---- windows ---------------------------------------------------------------------------------------
def _window_case(ids, name, lead, r, which, salt):
    """An object r bytes before the end of the window that `lead` sets up (lead: the page up to where
    that window ends, minus r). which: at / after (the wanted id is that object / the one behind it) or
    stale (neither: the pending id X is the object's id in the window and differs beyond it)."""
    x, z = ids.take(2)
    at_id, after_id, pending = ids.filler(), ids.filler(), [x]
    if which == "at":
        at_id = x
    elif which == "after":
        after_id = x
    else:
        at_id = x[:r - 8] + bytes(b ^ 0xA5 for b in x[r - 8:])
        after_id, pending = z, [x, z]
    start = len(lead)
    page = lead + obj(at_id, body(200, salt)) + obj(after_id, body(300, salt + 1)) + ids.fill(6000)
    return Case(name, page, pending, dict(r=r, start=start, which=which))


def windows_family():
    ids = Ids(1)
    cases = []
    for r in range(25):
        for which in ("at", "after"):  # the end of the first window
            c = _window_case(ids, "windows/first/r%d/%s" % (r, which), ids.fill(WINDOW - r), r, which, r)
            c.meta.update(window=0, wstart=0)
            cases.append(c)
    for r in range(25):
        for which in ("at", "after"):  # the end of the second window, which starts where the first one slid to
            dist = 5 + r % 3 if r % 2 == 0 else 100 + 37 * r  # the first window's end, seen from the object astride it
            lead = ids.fill(WINDOW - dist)
            q = len(lead) if dist < 8 else len(lead) + 3000  # a header astride: slide to it; else to the object behind it
            lead += obj(ids.filler(), body(3000 - 24, r))
            lead += ids.fill(q + WINDOW - r - len(lead))
            c = _window_case(ids, "windows/second/r%d/%s" % (r, which), lead, r, which, 50 + r)
            c.meta.update(window=1, wstart=q)
            cases.append(c)
    for size in (70_000, 140_000):  # one object longer than one window, than two
        (x,) = ids.take(1)
        lead = ids.fill(2000)
        page = lead + obj(ids.filler(), body(size - 24, size)) + obj(x, body(100, size + 1)) + ids.fill(500)
        cases.append(Case("windows/long%d" % size, page, [x], dict(long=size, start=len(lead), which="behind")))
    for r in range(9, 24):
        c = _window_case(ids, "windows/stale/r%d" % r, ids.fill(WINDOW - r), r, "stale", 100 + r)
        c.meta.update(window=0, wstart=0)
        cases.append(c)
    return Family("windows", [cases], [i for c in cases for i in c.pending])


# ---- tails -----------------------------------------------------------------------------------------
def _tails(R):
    if R == 8:
        return [("valid8", raw_obj(8, 0, b"")), ("valid24", raw_obj(24, 16, b"")), ("garbage", b"\xee" * 8)]
    return [("garbage", bytes([0xEE - k for k in range(R)]))]


def tails_family():
    ids = Ids(2)
    cases = []
    for at_window in (False, True):
        for R in range(10):
            for kind, tail in _tails(R):
                present, absent = ids.take(2)
                o = obj(present, body(50, R))
                if at_window:  # the first window full of whole objects, the tail alone in the second
                    prefix = ids.fill(30_000) + o
                    prefix += ids.fill(WINDOW - len(prefix))
                else:
                    prefix = ids.fill(300) + o + ids.fill(200)
                name = "tails/%sR%d/%s" % ("window/" if at_window else "", R, kind)
                cases.append(Case(name, prefix + tail, [present, absent],
                                  dict(R=R, prefix=len(prefix), windows=2 if at_window and R else 1)))
    cases.append(Case("tails/empty", b"", ids.take(1), dict(R=0, prefix=0, windows=1)))
    return Family("tails", [cases], [i for c in cases for i in c.pending])


# ---- malformed -------------------------------------------------------------------------------------
def malformed_family():
    """[object of `before`][fillers][the malformed object][fillers][object of `after`][fillers]; `mid` is
    pending too and is held only where a variant says so. want: the statuses of (before, mid, after)."""
    ids = Ids(3)
    cases = []

    def add(name, make, want):
        before, mid, after = ids.take(3)
        head = obj(before, body(40, len(cases))) + ids.fill(200)
        rest = ids.fill(150) + obj(after, body(60, len(cases))) + ids.fill(100)
        bad = make(mid, len(rest))
        cases.append(Case("malformed/" + name, head + bad + rest, [before, mid, after],
                          dict(at=len(head), bad=len(bad), want=want)))

    junk = b"\xee" * 16 + bytes(range(16))  # 32 bytes behind the header of a variant that ends the walk
    err = (OK, CORRUPT, CORRUPT)
    add("total0", lambda m, n: raw_obj(0, 16, junk), err)
    add("total7", lambda m, n: raw_obj(7, 16, junk), err)
    add("totalR+1", lambda m, n: raw_obj(40 + n + 1, 16, junk), err)
    add("totalR", lambda m, n: raw_obj(40 + n, 16, junk), (OK, NOT_FOUND, NOT_FOUND))  # valid: the page's last object
    add("totalmax", lambda m, n: raw_obj(0xFFFFFFFF, 16, junk), err)
    add("il_past", lambda m, n: raw_obj(40, 33, junk), err)
    add("il16_empty", lambda m, n: raw_obj(24, 16, m), (OK, OK, OK))  # found, an empty object
    add("il0", lambda m, n: raw_obj(8 + 16, 0, m), (OK, NOT_FOUND, OK))         # the object begins with the id
    add("il15", lambda m, n: raw_obj(8 + 20, 15, m + b"abcd"), (OK, NOT_FOUND, OK))   # the id's first 15 bytes
    add("il17", lambda m, n: raw_obj(8 + 21, 17, m + b"abcde"), (OK, NOT_FOUND, OK))  # the id and one byte more
    add("il32", lambda m, n: raw_obj(8 + 36, 32, b"\xee" * 16 + m + b"abcd"), (OK, NOT_FOUND, OK))  # the id inside
    add("il32_first", lambda m, n: raw_obj(8 + 36, 32, m + b"\xee" * 16 + b"abcd"), (OK, NOT_FOUND, OK))
    add("total8", lambda m, n: raw_obj(8, 0, b""), (OK, NOT_FOUND, OK))  # an empty id and object: the walk goes on
    return Family("malformed", [cases], [i for c in cases for i in c.pending])


# ---- duplicates ------------------------------------------------------------------------------------
def duplicates_family():
    """Block 0 holds `twice` two times with different objects (the first wins); block 1 holds the same
    id with a third object. The call asks for `twice` two times."""
    ids = Ids(4)
    twice, other, last = ids.take(3)
    # (`other` lies behind the second one, so the walk passes it while an id is still pending)
    p0 = (ids.fill(100) + obj(twice, b"first " + body(90, 1)) + ids.fill(400) + obj(twice, b"second " + body(70, 3)) +
          obj(other, body(30, 2)) + ids.fill(50))
    p1 = ids.fill(60) + obj(twice, b"third " + body(55, 4)) + obj(last, body(10, 5))
    b0 = [Case("duplicates/page", p0, [twice, other], dict(twice=twice))]
    b1 = [Case("duplicates/other_block", p1, [twice, last], dict(twice=twice))]
    return Family("duplicates", [b0, b1], [twice, other, twice, last])


# ---- pending ---------------------------------------------------------------------------------------
def _pending_case(ids, name, nhit, tail, all_present, rng):
    pend = ids.take(nhit)
    absent = set() if all_present else {j for j in range(nhit) if j % 7 == 3 and j != nhit - 1}
    held = [j for j in range(nhit) if j not in absent]
    order = held[:-1]
    rng.shuffle(order)
    page = bytearray()
    for n, j in enumerate(order + held[-1:]):  # the last present id is the page's last object
        if n % 5 == 0:
            page += obj(ids.filler(), body(n % 9, n))
        page += obj(pend[j], body(j % 8, j))
    return Case(name, bytes(page) + tail, pend,
                dict(nhit=nhit, passes=-(-nhit // PASS), absent=sorted(absent), R=len(tail), last=pend[held[-1]]))


def pending_family():
    ids = Ids(5)
    rng = random.Random(11)
    cases = [_pending_case(ids, "pending/n%d" % n, n, b"", False, rng) for n in PENDING_SIZES]
    cases.append(_pending_case(ids, "pending/n513_tail5", 513, b"\xee" * 5, False, rng))
    cases.append(_pending_case(ids, "pending/n300_found_before_tail5", 300, b"\xee" * 5, True, rng))
    ask = [i for c in cases for i in c.pending]
    rng.shuffle(ask)
    return Family("pending", [cases], ask)


# ---- gather ----------------------------------------------------------------------------------------
def gather_family():
    """Objects of GATHER_LENGTHS found in one call, with a hit that finds nothing and a hit on a corrupt
    page between them: the gather's destination offsets skip those two."""
    ids = Ids(6)
    g = ids.take(2)
    (nf,) = ids.take(1)
    g += ids.take(1)
    (bad,) = ids.take(1)
    g += ids.take(3)
    o = [obj(i, body(n, n)) for i, n in zip(g, GATHER_LENGTHS)]
    cases = [
        Case("gather/p0", o[0] + ids.fill(40) + o[1], [g[0], g[1], nf], dict(lengths=GATHER_LENGTHS[:2])),
        Case("gather/p1", o[2] + b"\xee" * 3, [g[2], bad], dict(lengths=GATHER_LENGTHS[2:3])),
        Case("gather/p2", o[3] + o[4] + ids.fill(24) + o[5], g[3:], dict(lengths=GATHER_LENGTHS[3:])),
    ]
    return Family("gather", [cases], [i for c in cases for i in c.pending])


def all_families():
    return [windows_family(), tails_family(), malformed_family(), duplicates_family(), pending_family(),
            gather_family()]
