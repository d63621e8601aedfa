"""Dictionaries built to put a needle at the edges of dict_stream_kernel (search.hip), and a plain
model of the byte stream that kernel scans. tests/test_dict_stream_cases.py holds the oracle to the
model and asserts that every case reaches the edge it was built for; tests/test_gpu_dict_stream_edges.py
runs the same cases on the device.

The stream of a key is its dictionary values back to back, in dictionary order. The device copy sits
right behind the key's nvals + 1 value offsets in one allocation (devctx.hip upload_key_dict; hipMalloc
aligns to far more than 16 bytes), and the kernel works in "aligned coordinates": byte p of the stream
is at lead + p, lead = the low four address bits of the first byte = 4 * ((nvals + 1) % 4). A Stream is
built for a lead and finish() appends plain values until the value count gives that lead.

Dictionary order: first seen in scan order for a key with 255 or more value sets, byte order for a
narrower one (block.cpp canonicalize_narrow_keys). Every value starts with its index as five digits,
so both orders are the order the values were added in; the one exception, an empty value in the
middle, is only allowed in a dictionary of 255 values or more. Each value is the single value of one
entry (an identity key: value id = set id = entry index), so a needle's matches are the indices of the
values that contain it.

Needles are letters, the filler is "." (decoys change one byte to "y"), prefixes are digits: a needle
occurs where a case put it and nowhere else, which the host test checks with a count over the stream.

A Case is (name, values, queries, dmin, spans, note): the values in dictionary order, the queries as
(needle, streams) pairs (streams: the gate of search.hip lets the term stream), the "dict_stream_min"
hook value the case runs under (0: none, a real dictionary over 1 MiB), the "dict_stream_span" values
to run it under (0: the planned span) and what the host test needs to check the case's coverage."""
import os
from collections import namedtuple

import numpy as np

from tests.helpers import write_block

KEY = "db.statement"
Case = namedtuple("Case", "name values queries dmin spans note")
T0 = 1_700_000_000 * 10**9
MASTER = "abcdefghijklmnopq"  # residue sweep: the needle of length nl is its first nl bytes
RESIDUE_NL = (2, 3, 4, 5, 12, 13, 16, 17)
PAIR_MAX = 11  # kStreamPairMax
TAIL = "!#$%&()*+,/:;<=>?@[]^_{|}~"  # what follows a needle's leading letters


# ---- the model ------------------------------------------------------------------------------------
class Model:
    def __init__(self, values):
        self.values = list(values)
        self.off = [0]
        for v in self.values:
            self.off.append(self.off[-1] + len(v))
        self.stream = "".join(self.values)
        self.nbytes = len(self.stream)
        self.lead = 4 * ((len(self.values) + 1) % 4)

    def apos(self, v):
        """aligned coordinate of value v's first byte"""
        return self.lead + self.off[v]

    def matches(self, needle):
        return [i for i, v in enumerate(self.values) if needle in v]

    def occurrences(self, needle):
        """aligned coordinates of every occurrence in the stream, those across values included"""
        out, k = [], self.stream.find(needle)
        while k >= 0:
            out.append(self.lead + k)
            k = self.stream.find(needle, k + 1)
        return out

    def streams(self, needle, dmin):
        """the gate of search.hip: the term is matched by dict_stream_kernel"""
        return (self.nbytes > (dmin or 1 << 20) and 2 <= len(needle) <= 1024
                and self.nbytes >= 16 * len(self.values))

    def pair_counts(self):
        """block.cpp: byte-pair counts over 64 windows of 16 KiB, dictionaries over 1 MiB only"""
        if self.nbytes <= 1 << 20:
            return None
        b = np.frombuffer(self.stream.encode(), dtype=np.uint8).astype(np.uint32)
        cnt = np.zeros(65536, dtype=np.int64)
        for w in range(64):
            a = (self.nbytes - 16384) // 63 * w
            p = b[a:a + 16384]
            cnt += np.bincount((p[:-1] << 8) | p[1:], minlength=65536)
        return cnt

    def pj(self, needle, counts=None):
        """the second pair the host picks (search.hip plan): 0 = none"""
        nl = len(needle)
        if nl < 4:
            return 0
        hi = min(nl - 2, PAIR_MAX)
        if counts is None:
            return hi
        best, at = None, hi
        for j in range(2, hi + 1):
            f = counts[(ord(needle[j]) << 8) | ord(needle[j + 1])]
            if best is None or f < best:
                best, at = f, j
        return at


def entries(values):
    """One entry per value. The writer lays a page's entries out last first, so the ids descend with
    the value index and the block is one page: the scan order (hence the first-seen dictionary order
    and the entry index of a match) is the order of `values`."""
    n = len(values)
    return [{"id": (n - i).to_bytes(16, "big"), "start": T0 + i, "end": T0 + i + 1000, "tags": {KEY: [values[i]]}}
            for i in reversed(range(n))]


def write_case(dir, case):
    return write_block(dir, case.name, entries(case.values), page_size=64 << 20)


class Stream:
    """Values added in order for an assumed lead."""

    def __init__(self, lead):
        self.lead, self.values, self.n = lead, [], 0

    def pos(self):
        """aligned coordinate of the next value's first byte"""
        return self.lead + self.n

    def add(self, body, prefix=True):
        v = ("%05d" % len(self.values) if prefix else "") + body
        self.values.append(v)
        self.n += len(v)
        return v

    def add_at(self, residue, mod, needle, tail="..."):
        """a value whose needle starts at an aligned coordinate = residue (mod `mod`); returns it"""
        pad = (residue - (self.pos() + 5)) % mod
        at = self.pos() + 5 + pad
        self.add("." * pad + needle + tail)
        return at

    def sweep(self, targets, mod, tail="..."):
        """one value per (residue, needle) target, the nearest pending residue first; {needle: [at]}"""
        pending, at = list(targets), {}
        while pending:
            base = self.pos() + 5
            k = min(range(len(pending)), key=lambda i: (pending[i][0] - base) % mod)
            r, nd = pending.pop(k)
            at.setdefault(nd, []).append(self.add_at(r, mod, nd, tail))
        return at

    def finish_with(self, body):
        """finish() with `body` as the last value: plain values go before it, not after"""
        while 4 * ((len(self.values) + 2) % 4) != self.lead:
            self.add("." * 11)
        self.add(body)
        return self.finish()

    def finish(self):
        while 4 * ((len(self.values) + 1) % 4) != self.lead:
            self.add("." * 11)
        m = Model(self.values)
        assert m.lead == self.lead
        return m


def letters(i, n=3):
    s = ""
    for _ in range(n):
        s = chr(97 + i % 26) + s
        i //= 26
    assert i == 0
    return s


def needle_of(i, nl):
    """needle number i of length nl: distinct for distinct i, letters only"""
    if nl == 2:
        return letters(i, 2)
    return letters(i, 3) + (TAIL * (nl // len(TAIL) + 1))[:nl - 3]


# ---- the cases ------------------------------------------------------------------------------------
def residues_case():
    """Every start position of a 1 KiB step in a real dictionary (> 1 MiB, no hooks): values of 1021
    bytes, alternately holding MASTER at a start whose residue mod 1024 is still uncovered and a near
    miss (MASTER with byte nl - 1 changed, nl over RESIDUE_NL in turn)."""
    L, st, uncovered, i = 1021, Stream(0), set(range(1024)), 0
    room = L - 5 - len(MASTER)
    while uncovered or st.n <= (1 << 20) + 4096:
        base = st.pos() + 5
        if i % 2 == 0:
            o = next((o for o in range(room + 1) if (base + o) % 1024 in uncovered), 0)
            uncovered.discard((base + o) % 1024)
            word = MASTER
        else:
            k = RESIDUE_NL[(i // 2) % len(RESIDUE_NL)] - 1
            o, word = (i * 7) % (room + 1), MASTER[:k] + "-" + MASTER[k + 1:]
        st.add("." * o + word + "." * (room - o))
        i += 1
    m = st.finish()
    return Case("residues", m.values, [(MASTER[:nl], True) for nl in RESIDUE_NL], 0, (0,), None)


SPAN_NL = (2, 17, 1024)


def span_tokens(n):
    """n bytes of distinct 4-byte tokens: every window of 8 bytes or more occurs once"""
    assert n % 4 == 0
    return "".join(letters(k, 3) + "!" for k in range(n // 4))


def span_cases():
    """A needle's only occurrence at every offset from nl + 16 bytes before a span boundary to 16 bytes
    after it (offset 0: a span's first byte), each offset its own needle: one value per needle for
    lengths 2 and 17; for 1024 the needles are the 1024-byte windows of one run of distinct tokens
    laid across a boundary. Also the stream's first and last nl bytes."""
    out = []
    for span in (1024, 8192, 65536):
        for nl in SPAN_NL:
            st = Stream(0)
            ds = list(range(-(nl + 16), 17))
            if nl == 1024:
                bound = max(span, 2048)  # (room for the prefix before the run)
                run = span_tokens(nl + 16 + 16 + nl)
                st.add("." * (bound - (nl + 16) - st.pos() - 5) + run + "...")
                needles = [run[k:k + nl] for k in range(len(ds))]
            else:
                needles = [needle_of(i, nl) for i in range(len(ds))]
                st.sweep([(d % span, needles[i]) for i, d in enumerate(ds)], span)
            while len(st.values) < 256:  # (a key of fewer than 255 values is matched on the host)
                st.add("." * 11)
            last = needle_of(len(ds), nl) if nl != 1024 else "zzz" + (TAIL * 40)[:nl - 3]
            m = st.finish_with("." * 11 + last)
            q = [(nd, True) for nd in needles]
            # the stream's first nl bytes (the first value's prefix is part of the needle) and its last
            q += [(m.stream[:nl], True), (last, True)]
            spans = (span, 0) if span == 8192 else (span,)
            out.append(Case("span%d_nl%d" % (span, nl), m.values, q, 1024, spans,
                            {"span": span, "nl": nl, "ds": ds, "needles": needles, "last": last}))
    return out


def value_boundary_case():
    """Needles split between two values (every split of lengths 2, 5 and 17), split around an empty
    value, one byte longer than a value: no match. Equal to a value, at its first and at its last
    byte: a match. Several matches in one long value, then one in the next (mdone)."""
    st, q, note = Stream(0), [], {"split": [], "empty": [], "short": [], "hit": [], "mdone": None}
    for _ in range(8):
        st.add("." * 11)
    c = 0
    for nl in (2, 5, 17):
        for s in range(1, nl):
            t = chr(97 + c) * s
            c += 1
            st.add("." * 11 + t)
            nxt = st.add("=" * max(0, nl - s - 5) + "." * 11)
            q.append((t + nxt[:nl - s], True))
            note["split"].append((q[-1][0], nl, s))
    for nl in (5,):  # (a dictionary holds one empty value)
        s = max(1, nl // 2)
        t = chr(97 + c) * s
        c += 1
        st.add("." * 11 + t)
        st.add("", prefix=False)
        nxt = st.add("=" * max(0, nl - s - 5) + "." * 11)
        q.append((t + nxt[:nl - s], True))
        note["empty"].append(q[-1][0])
    assert c <= 26
    v = st.add("abcdefghijklmnopq")
    st.add("." * 11)
    q.append((v + "0", True))  # the whole value and the next one's first byte
    note["short"].append(q[-1][0])
    for tag in ("ab", "cdefg", "hijklmnopqrstuvw~"):
        v = st.add("." * 7 + tag)
        q += [(v, True), (v[:len(tag)], True), (tag, True)]  # equal; first bytes; last bytes
        note["hit"] += [(v, len(st.values) - 1)] * 1 + [(v[:len(tag)], len(st.values) - 1), (tag, len(st.values) - 1)]
    long = st.add("." * 20 + "r$" + "." * 300 + "r$" + "." * 700 + "r$" + "." * 9)
    st.add("r$" + "." * 11)
    st.add("." * 30)
    st.add("." * 3 + "r$")
    q.append(("r$", True))
    note["mdone"] = [len(st.values) - 4, len(st.values) - 3, len(st.values) - 1]
    assert long.count("r$") == 3
    # A needle that no value holds is refused by the block header's value list before any kernel runs,
    # unless the dictionary is over 1 MiB (its header values are then left to the device pass)
    while st.n <= (1 << 20) + 4096:
        st.add("." * 1000)
    m = st.finish()
    return Case("value_bounds", m.values, q, 0, (0, 1024), note)


def pair_needle(nl):
    return chr(97 + nl) + TAIL[:nl - 1]


PAIR_NL = tuple(range(3, 15))
PAIR_RES = tuple(range(992, 1024)) + tuple(range(0, 16))


def second_pair_case():
    """Without pair counts (a dictionary under 1 MiB) the second pair is the needle's last one in
    reach, pj = min(nl - 2, 11): needle lengths 4..13 give every pj in 2..11, 3 gives none, 14 gives 11
    with bytes after the pair. Each needle at every start in the last two lanes of a step and the first
    lane of the next, and decoys (both tested pairs match, one byte between or after them differs)."""
    st, note = Stream(0), {"at": {}, "decoys": {}}
    targets = [(r, pair_needle(nl)) for nl in PAIR_NL for r in PAIR_RES]
    for nl in PAIR_NL:
        nd, pj = pair_needle(nl), min(nl - 2, PAIR_MAX) if nl >= 4 else 0
        ds = [b for b in range(2, nl) if not (pj and pj <= b <= pj + 1)]
        note["decoys"][nd] = [nd[:b] + "-" + nd[b + 1:] for b in ds]
        for r in (1000, 1012, 1023, 5):
            targets += [(r, d) for d in note["decoys"][nd]]
    note["at"] = st.sweep(targets, 1024)
    m = st.finish()
    return Case("second_pair", m.values, [(pair_needle(nl), True) for nl in PAIR_NL], 1024, (0,), note)


STEER_J = tuple(range(2, 12))


def steer_needle(j):
    """14 bytes, a letter of its own between punctuation: each of its 13 byte pairs is its alone"""
    c = chr(97 + j)
    return "".join(c + TAIL[k] for k in range(7))


def steered_pair_case():
    """A dictionary over 1 MiB, so the host picks the needle's rarest pair from the sampled counts
    (block.cpp): for each j in 2..11 a needle whose pairs 2..11 all fill the filler except pair j.
    Each needle at every start in the last two lanes of a step and the first lane of the next; decoys
    keep both tested pairs and change a byte between them or after them. Lengths 4 (only j = 2) and 3
    (no second pair) ride along."""
    st, note = Stream(0), {"decoys": {}, "pj": {}}
    small = {4: "y" + TAIL[7:10], 3: "z" + TAIL[10:12]}
    targets = [(r, steer_needle(j)) for j in STEER_J for r in PAIR_RES]
    targets += [(r, nd) for nd in small.values() for r in PAIR_RES]
    for j in STEER_J:
        nd = steer_needle(j)
        bs = [b for b in (j - 1, j + 2) if 2 <= b < len(nd) and not j <= b <= j + 1]
        note["decoys"][nd] = [nd[:b] + "-" + nd[b + 1:] for b in bs]
        note["pj"][nd] = j
        targets += [(r, d) for d in note["decoys"][nd] for r in (1000, 1012, 1023, 5)]
    st.sweep(targets, 1024)
    while st.n <= (1 << 20) + (64 << 10):
        for j in STEER_J:
            nd = steer_needle(j)
            for k in range(2, PAIR_MAX + 1):
                if k != j:
                    st.add((nd[k:k + 2] + ".") * 330)
    m = st.finish()
    q = [(steer_needle(j), True) for j in STEER_J] + [(nd, True) for nd in small.values()]
    return Case("steered_pair", m.values, q, 0, (0,), note)


def short_values_case(nvals):
    """Values of 16..24 bytes, every third holding "qz": 64 verified starts of one batch lie in more
    than 128 values (the search of the global offsets past the staged ones); the first and the last
    value hold needles of their own (value_at over nvals + 1 offsets)."""
    st = Stream(4 * ((nvals + 1) % 4))
    for i in range(nvals):
        body = "." * (11 + i % 9)
        if i % 3 == 0:
            body = body[:4] + "qz" + body[6:]
        if i == 0:
            body = "fir" + body[3:]
        if i == nvals - 1:
            body = body[:-4] + "last"
        st.add(body)
    m = st.finish()
    assert len(m.values) == nvals
    return Case("short%d" % nvals, m.values, [("qz", True), ("fir", True), ("last", True), ("st", True)], 8, (0,),
                {"nvals": nvals})


def run_cases():
    """Steps of one repeated byte (16 candidates in every lane), the list at exactly 1024 candidates
    before the next step arrives and at 1025, and steps with at most one candidate per lane."""
    out = []
    for extra in (0, 1):
        st = Stream(0)
        # `extra` candidates in step 0, then a KiB-aligned run of 1025 "a": 1024 starts of "aa" in step 1
        st.add("." * 10 + ("aa" if extra else "..") + "." * 1007 + "a" * 1025 + "." * 1006)
        assert st.values[0].index("a" * 1025) == 1024
        st.add("." * 51)
        st.add("".join("aa" + "." * 14 for _ in range(64)))
        m = st.finish()
        out.append(Case("runs%d" % extra, m.values, [("aa", True), ("aaa", True), ("aa.", True), (".a", True)], 64, (0,),
                        {"extra": extra}))
    return out


END_NL = (2, 3, 4, 5)


def end_cases():
    """The needle ends at the stream's last byte: nbytes mod 16 over 0..15, nl mod 4 over 0..3, the
    four leads; every dictionary's last value ends in "vwxyz" and the needles are its suffixes."""
    out = []
    for lead in (0, 4, 8, 12):
        nvals = next(n for n in (3, 4, 5, 6) if 4 * ((n + 1) % 4) == lead)
        for r in range(16):
            st = Stream(lead)
            for _ in range(nvals - 1):
                st.add("." * 11)
            pad = (r - (st.n + 5 + 5)) % 16 + 16
            st.add("." * pad + "vwxyz")
            m = st.finish()
            assert len(m.values) == nvals and m.nbytes % 16 == r
            out.append(Case("end_l%d_r%d" % (lead, r), m.values, [("vwxyz"[-nl:], True) for nl in END_NL], 16, (0,),
                            {"lead": lead, "r": r}))
    # a dictionary exactly as long as the needle (a longer needle never reaches a kernel: no header
    # value holds it, and a dictionary over 1 MiB is longer than any streamed needle)
    st = Stream(8)
    v = st.add("." * 6 + "exactlythis")
    m = st.finish()
    out.append(Case("end_exact", m.values, [(v, True)], 16, (0,), {"exact": v}))
    # A dictionary shorter than the needle. No search can bring one to a dictionary kernel: the block's
    # header lists the key's values and a block none of whose values holds the needle is skipped, unless
    # the dictionary is over 1 MiB, and a streamed needle has 1024 bytes at most. `None`: no dictionary
    # job of either kind runs; the host test asserts that the oracle skips the block.
    out.append(Case("end_short", m.values, [(v + ".", None), (v[1:] + "..", None)], 16, (0,), {"exact": v}))
    return out


def gate_cases():
    """What the gate of search.hip lets stream: needles of 2..1024 bytes, dictionaries of more than the
    threshold, a mean value length of 16 bytes or more."""
    out = []
    st = Stream(0)
    big = st.add("g" * 1100)
    for _ in range(2):
        st.add("." * 11)
    m = st.finish()
    q = [("g", False), ("gg", True), (big[5:5 + 1024], True), (big[5:5 + 1025], False), ("0", False)]
    out.append(Case("gate_needle", m.values, q, 64, (0,), None))
    for over in (0, 1):  # a dictionary at the threshold (4096) and one byte over it
        st = Stream(12)
        st.add("." * 1000 + "th")
        st.add("." * (4096 + over - st.n - 5))
        m = st.finish()
        assert m.nbytes == 4096 + over
        out.append(Case("gate_min%d" % over, m.values, [("th", bool(over))], 4096, (0,), None))
    for short in (1, 0):  # mean value length one byte under 16 x nvals in all, and exactly 16
        st = Stream(0)
        for i in range(6):
            st.add("." * 9 + "mv" if i == 3 else "." * 11)
        st.add("." * (11 - short))
        m = st.finish()
        assert m.nbytes == 16 * len(m.values) - short
        out.append(Case("gate_mean%d" % short, m.values, [("mv", not short)], 16, (0,), None))
    return out


def all_cases():
    cases = [residues_case()] + span_cases() + [value_boundary_case(), second_pair_case(), steered_pair_case()]
    cases += [short_values_case(n) for n in (1, 63, 64, 1000, 4095, 4096)]
    cases += run_cases() + end_cases() + gate_cases()
    for c in cases:
        m = Model(c.values)
        assert len(set(c.values)) == len(c.values), c.name
        inorder = all(a < b for a, b in zip(c.values, c.values[1:]))
        assert inorder or (len(c.values) >= 255 and sorted(v for v in c.values if v) == [v for v in c.values if v]), c.name
        for nd, streams in c.queries:
            if streams is None:  # refused by the block's header
                assert m.matches(nd) == [] and m.nbytes <= 1 << 20, (c.name, nd)
            else:
                assert m.streams(nd, c.dmin) == streams, (c.name, nd)
    return cases


# ---- several jobs in one search ---------------------------------------------------------------------
JOB_NVALS = (64, 65, 95, 300, 513)  # entries per block = values of the identity keys: nvals mod 32 = 0, 1, 31, ...
JOB_DMIN, JOB_SPAN = 64, 1024
# (tags, stream jobs, lane jobs) over the five blocks
JOB_QUERIES = (({"ka": "ja#", "kb": "jb$"}, 10, 0),  # two streamed identity terms: ten jobs
               ({"ka": "ja#", "kc": "c1"}, 5, 5),    # a streamed term beside a lane-path one (kc: short values)
               ({"km": "jm%"}, 5, 0),                # a multi-valued (non-identity) streamed key
               ({"ka": "ja#"}, 5, 0),
               ({"kb": "jb$", "km": "jm%"}, 10, 0),
               ({"ka": "....", "kb": "jb$"}, 10, 0))  # every value of ka matches


def jobs_blocks():
    """Five blocks of four keys: ka, kb one distinct value per entry (identity; ka's matches sit at the
    edges of its 32-value bitmap words), kc short values (mean under 16 bytes: the lane path), km one
    to three values per entry out of 37 (value sets). Every block holds every needle."""
    blocks = []
    for b, n in enumerate(JOB_NVALS):
        ents = []
        for i in range(n):
            hit = i in (0, 31, 32, 63, n - 1) or i % 11 == b
            ka = "%05d" % i + "." * (20 + (i * 7 + b) % 40) + ("ja#" if hit else "")
            kb = "%05d" % i + "." * (30 + i % 25) + ("jb$" if i % 3 == 0 or i == n - 1 else "")
            kc = "c%d" % (i % 50) + ("!" if i % 4 == 0 else "")
            ks = sorted({(i * 5 + k * 7 + b) % 37 for k in range(1 + i % 3)})
            km = ["m%02d" % x + "." * 20 + ("jm%" if x in (3, 36) else "") for x in ks]
            ents.append({"ka": [ka], "kb": [kb], "kc": [kc], "km": km})
        blocks.append(ents)
    return blocks


def jobs_expected(blocks, tags):
    """(block, entry) of the entries that have, for every term, a value holding its needle"""
    return [(b, i) for b, ents in enumerate(blocks) for i, e in enumerate(ents)
            if all(any(nd in v for v in e[k]) for k, nd in tags.items())]


def write_jobs_blocks(dir, blocks):
    paths = []
    for b, ents in enumerate(blocks):
        n = len(ents)
        es = [{"id": (n - i).to_bytes(16, "big"), "start": T0 + i, "end": T0 + i + 1000, "tags": ents[i]}
              for i in reversed(range(n))]
        paths.append(write_block(dir, "jobs%d" % b, es, page_size=64 << 20))
    return paths
