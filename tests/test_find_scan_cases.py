"""The findOne pages of tests/find_scan_cases.py on the CPU: the C oracle (orc_v2_find, which reads a
page as findOne does, through UnmarshalObjectFromReader over a bytes.Reader) against the Python model
for every case and pending id, status and bytes; and that every case sits where it was aimed: its
distance to the window end, its number of windows, its tail, its passes. The coverage assertions are
statements about the pages and the kernel's tiling rule (window_trace), never about results.

test_model_equals_oracle fails on an oracle that walks the page with UnmarshalAndAdvanceBuffer
(object.go:82-113): that form reports an error with 4 bytes left and parses a header in the last 8."""
import os
import struct

import pytest

from oracle import oracle as O
from tests import find_scan_cases as S

OK, NOT_FOUND, CORRUPT, WINDOW = S.OK, S.NOT_FOUND, S.CORRUPT, S.WINDOW


@pytest.fixture(scope="module")
def families():
    return {f.name: f for f in S.all_families()}


def oracle_find(blk, tid):
    rc, o = blk.find(tid, status=True)
    assert rc == 0 or o is None
    return (rc, None) if rc else (OK, o) if o is not None else (NOT_FOUND, None)


def objects(page, end=None):
    """[(start, total, id)] of the whole objects of page[0 .. end)."""
    at, out = 0, []
    end = len(page) if end is None else end
    while at < end:
        total, il = struct.unpack_from("<II", page, at)
        assert 8 + il <= total <= end - at
        out.append((at, total, page[at + 8:at + 8 + il]))
        at += total
    return out


def test_model_equals_oracle(families, tmp_path):
    seen = set()
    for fam in families.values():
        for k, cases in enumerate(fam.blocks):
            blk = O.V2Block(S.write_block(os.path.join(str(tmp_path), "%s%d" % (fam.name, k)), cases))
            for c in cases:
                for tid in c.pending:
                    assert blk.index_find(tid)[0] == cases.index(c), c.name  # the index sends the id to this page
                    want = S.model_find(c.page, tid)
                    assert oracle_find(blk, tid) == want, (c.name, tid.hex())
                    seen.add(want[0])
    assert seen == {OK, NOT_FOUND, CORRUPT}
    # an id of one block asked of the other (the same id in two blocks)
    d = families["duplicates"]
    twice = d.blocks[0][0].meta["twice"]
    a, b = S.model_find(d.blocks[0][0].page, twice), S.model_find(d.blocks[1][0].page, twice)
    assert a[0] == b[0] == OK and a[1].startswith(b"first ") and b[1].startswith(b"third ")
    assert d.ask.count(twice) == 2
    page, other = d.blocks[0][0].page, d.blocks[0][0].pending[1]
    assert page.count(twice) == 2 and page.find(twice) < page.rfind(twice) < page.find(other)  # the walk passes the second one


def test_existing_callers_keep_working(tmp_path):
    """find(tid) without status: the object or None, an assertion on a page error."""
    fam = S.tails_family()
    blk = O.V2Block(S.write_block(os.path.join(str(tmp_path), "t"), fam.blocks[0]))
    c = next(c for c in fam.blocks[0] if c.name == "tails/R5/garbage")
    assert blk.find(c.pending[0]) == S.model_find(c.page, c.pending[0])[1] is not None
    with pytest.raises(AssertionError):
        blk.find(c.pending[1])
    c = next(c for c in fam.blocks[0] if c.name == "tails/R4/garbage")
    assert blk.find(c.pending[1]) is None


def test_sizes(families):
    pages = [c for f in families.values() for b in f.blocks for c in b]
    assert max(len(c.page) for c in pages) <= 200 * 1024
    assert len(pages) <= 250  # the GPU file scans each at most three times, the windows and tails four


def test_windows(families):
    cases = families["windows"].blocks[0]
    aimed = {}
    for c in cases:
        t, m = S.window_trace(c.page), c.meta
        assert 70 * 1024 <= len(c.page) <= 200 * 1024, c.name
        assert t.covered == WINDOW
        if "long" in m:
            behind = m["start"] + m["long"]
            assert m["long"] > (WINDOW if m["long"] < 100_000 else 2 * WINDOW)
            assert t.starts[:2] == [0, behind] and t.windows == 2 and c.page[behind + 8:behind + 24] == c.pending[0], c.name
            assert S.model_find(c.page, c.pending[0])[0] == OK
            continue
        r, start, k = m["r"], m["start"], m["window"]
        aimed.setdefault((k, m["which"]), set()).add(r)
        assert t.starts[k] == m["wstart"] and m["wstart"] + WINDOW - start == r, c.name  # r bytes before the window's end
        assert t.windows == k + 2, c.name
        assert struct.unpack_from("<II", c.page, start) == (224, 16)
        if k == 1:  # the second window starts where the first one slid to: at a header astride its end, or behind an object astride it
            first = t.slides[0]
            assert first[0] == m["wstart"] and (0 < first[1] < 8 if r % 2 == 0 else first[1] < 0), c.name
        if r < 24:  # slides to the object: next >= wl (0), a header astride (1..7), an id astride (8..23)
            assert t.slides[k] == (start, r) and t.starts[k + 1] == start, c.name
        else:       # header and id inside: compared in this window, the slide goes to the object behind it
            assert t.slides[k] == (start + 224, 24 - 224) and t.starts[k + 1] == start + 224, c.name
        wanted = {"at": start, "after": start + 224}
        if m["which"] in wanted:
            at = wanted[m["which"]]
            assert c.page[at + 8:at + 24] == c.pending[0] and S.model_find(c.page, c.pending[0])[0] == OK, c.name
            continue
        # stale: X is the object's id inside the window and differs in every byte beyond it
        x, z = c.pending
        oid, inside = c.page[start + 8:start + 24], r - 8
        assert 1 <= inside <= 15 and oid[:inside] == x[:inside], c.name
        assert all(oid[j] != x[j] for j in range(inside, 16)), c.name
        assert c.page.find(x) < 0 and S.model_find(c.page, x) == (NOT_FOUND, None), c.name
        assert S.model_find(c.page, z)[0] == OK, c.name  # the walk goes on behind it
        # where a compare that does not slide reads the id, as LDS offsets of this window
        lds = [start - m["wstart"] + 8 + j for j in range(16)]
        assert all(c.page[m["wstart"] + lds[j]] == x[j] for j in range(inside)), c.name
        assert all(WINDOW <= lds[j] < WINDOW + 16 for j in range(inside, 16)), c.name
        # ... which is the slack behind the window: no window load reaches it (t.covered, above), so the
        # page cannot put X's bytes there (find_scan_cases.py, "Stale bytes")
    every = set(range(25))
    assert aimed == {(0, "at"): every, (0, "after"): every, (1, "at"): every, (1, "after"): every,
                     (0, "stale"): set(range(9, 24))}


def test_tails(families):
    cases = families["tails"].blocks[0]
    seen = set()
    for c in cases:
        m, t = c.meta, S.window_trace(c.page)
        R = len(c.page) - m["prefix"]
        assert R == m["R"] and objects(c.page, m["prefix"]) is not None, c.name  # whole objects, then R bytes
        assert t.windows == m["windows"], c.name
        if c.name == "tails/empty":
            assert c.page == b"" and S.model_find(c.page, c.pending[0]) == (NOT_FOUND, None)
            continue
        if "/window/" in c.name:
            assert t.starts == [0, WINDOW] and m["prefix"] == WINDOW, c.name
        present, absent = c.pending
        assert S.model_find(c.page, present)[0] == OK, c.name
        assert S.model_find(c.page, absent)[0] == (NOT_FOUND if R in (0, 4, 8) else CORRUPT), c.name
        seen.add((2 if "/window/" in c.name else 1, R, c.name.rsplit("/", 1)[1]))
    want = {(w, R, "garbage") for w in (1, 2) for R in range(10)} | \
        {(w, 8, k) for w in (1, 2) for k in ("valid8", "valid24")}
    assert seen == want
    v8, v24 = (next(c for c in cases if c.name == "tails/R8/" + k) for k in ("valid8", "valid24"))
    assert struct.unpack("<II", v8.page[-8:]) == (8, 0) and struct.unpack("<II", v24.page[-8:]) == (24, 16)


def test_malformed(families):
    cases = families["malformed"].blocks[0]
    for c in cases:
        m = c.meta
        objs = objects(c.page, m["at"])
        assert len(objs) >= 2 and objs[0][2] == c.pending[0], c.name            # not the first object
        assert len(c.page) - m["at"] - m["bad"] > 24, c.name                     # nor the last bytes
        assert tuple(S.model_find(c.page, i)[0] for i in c.pending) == m["want"], c.name
    by = {c.name.split("/")[1]: c for c in cases}
    header = lambda c: struct.unpack_from("<II", c.page, c.meta["at"])
    R = lambda c: len(c.page) - c.meta["at"]
    assert [header(by[k])[0] for k in ("total0", "total7", "totalmax", "total8")] == [0, 7, 0xFFFFFFFF, 8]
    assert header(by["totalR+1"])[0] == R(by["totalR+1"]) + 1 and header(by["totalR"])[0] == R(by["totalR"])
    assert header(by["il_past"])[1] == header(by["il_past"])[0] - 8 + 1
    assert header(by["il16_empty"]) == (24, 16) and S.model_find(by["il16_empty"].page, by["il16_empty"].pending[1]) == (OK, b"")
    for k, il in (("il0", 0), ("il15", 15), ("il17", 17), ("il32", 32), ("il32_first", 32)):
        c = by[k]
        assert header(c)[1] == il and c.page.count(c.pending[1]) == 1, k  # the id's 16 bytes are there, and do not match
        assert c.meta["at"] + 8 <= c.page.find(c.pending[1]) <= c.meta["at"] + 8 + 16
    assert header(by["total8"]) == (8, 0) and by["total8"].meta["want"][2] == OK


def test_pending(families):
    fam = families["pending"]
    cases = fam.blocks[0]
    assert [c.meta["nhit"] for c in cases[:len(S.PENDING_SIZES)]] == list(S.PENDING_SIZES)
    assert {c.meta["nhit"]: c.meta["passes"] for c in cases} == {1: 1, 63: 1, 64: 1, 65: 1, 255: 1, 256: 1, 257: 2,
                                                                 513: 3, 300: 2}
    for c in cases:
        m = c.meta
        assert len(c.pending) == m["nhit"] and m["passes"] == -(-len(c.pending) // S.PASS)
        objs = objects(c.page, len(c.page) - m["R"])
        assert objs[-1][2] == m["last"] == max(i for i in c.pending if c.page.find(i) >= 0), c.name
        assert max(t for _, t, _ in objs) <= 24 + 8  # tiny objects
        st = [S.model_find(c.page, i)[0] for i in c.pending]
        if c.name == "pending/n300_found_before_tail5":
            assert m["R"] == 5 and st == [OK] * 300
            continue
        miss = CORRUPT if m["R"] else NOT_FOUND
        assert m["R"] == (5 if c.name == "pending/n513_tail5" else 0)
        assert st == [miss if j % 7 == 3 and j != m["nhit"] - 1 else OK for j in range(m["nhit"])], c.name
        assert st[-1] == OK and (m["nhit"] < 4 or miss in st)
    ordered = [i for c in cases for i in c.pending]
    assert sorted(fam.ask) == ordered and fam.ask != ordered  # shuffled


def test_gather(families):
    fam = families["gather"]
    cases = fam.blocks[0]
    got = [S.model_find(S.page_of(cases, i).page, i) for i in fam.ask]
    assert [st for st, _ in got] == [OK, OK, NOT_FOUND, OK, CORRUPT, OK, OK, OK]
    assert tuple(len(o) for st, o in got if st == OK) == S.GATHER_LENGTHS == (0, 1, 255, 256, 257, 70_000)
