"""Constructed WAL refreshes for wal_merge_kernel (tempo_amd/csrc/wal_merge.hip), and a plain model of
the merge at the entry level. tests/test_wal_merge_cases.py holds the cases to their aim on the CPU;
tests/test_gpu_wal_merge_edges.py runs them through tsg_wal_block_refresh.

A case is two entry lists: `first` (the file the block is opened from) and `appended` (the pages the
file grows by), plus the queries that pin it. Every entry is one page. An id is a 16-byte big-endian
number: old entry i of a case has the number 1000 (i + 1), so up to 999 ids fit before entry 0, between
two neighbours and behind the last one, and what an entry holds follows from its number alone.

The model: plan() computes from the two id lists the delta as block.cpp plan_wal_refresh defines it
(dlo = lower bound among the old ids, drep = the id was there, dins = inserts among the delta entries
before, ndelta + 1 values; dpos = dlo + dins as devctx.hip block_refresh uploads it); source_map()
is the kernel's search for every output position j < n_new (c = delta entries placed before j; delta
entry c if dpos[c] == j, else old entry j - dins[c]); sorted_merge() is what must come out.

Constants of the code the shapes are aimed at: kRun = 2048 entries per workgroup and kLdsDelta = 2048
staged delta positions (wal_merge.hip), kColPad = 4096 (engine.hpp: the scan and term columns' stride),
a key's column is one byte wide while it has fewer than 255 value sets (block.hpp KeyColumn::width).

Widths. A key's value sets only ever join its dictionary, so the refreshed block's dictionary holds the
old sets and the delta's, also where a combined entry no longer uses its old set. The `widths` family
counts distinct value vectors over the entries (what a fresh open interns). The shapes at 254, 255 and
256 sets are kept as they were asked for; by KeyColumn::width a column is two bytes from 255 sets on,
so of those only 254 -> 255 meets the one-byte cap (it widens there), and the shapes at 253 are added:
253 -> 254 and 253 -> 253 stay one byte with the largest table (lut_n = 253), every id moved, and
254 -> 254, where the refreshed column widens and a fresh open's does not.

Not here, on purpose:
* 2 -> 4 byte widening needs >= 65 535 distinct sets of one key, which is not a seconds-sized test. That
  path stays pinned only by the host replay of the stand-alone sanitizer program
  (tests/sanitize/san_wal_refresh.cpp).
* The kernel's table read for a column that is not one byte wide (`wo != 1 && J.lut`) cannot be reached
  through the public API: canonicalize_narrow_keys (block.cpp) fills a key's renumbering map only when
  its width is 1, plan_wal_refresh's lut_of leaves set_lut[k] empty when both maps are empty, and a key's
  set count never shrinks, so a key that was wider than one byte is never narrow afterwards. A table
  therefore always comes with wo == 1 (or wo == 0, which has no old column to translate)."""
import bisect

T0 = 1_700_000_000
S, MS = 10**9, 10**6
K_RUN = 2048        # wal_merge.hip kRun
K_LDS_DELTA = 2048  # wal_merge.hip kLdsDelta
K_COL_PAD = 4096    # engine.hpp kColPad
DS_BASE_BACK = 16383  # ds_word.hpp kDsBaseBack
DS_REL_ESC = 0x7fff   # ds_word.hpp kDsRelEsc
GAP = 1000
FAMILIES = ("runs", "pad", "delta", "layout", "widths", "names", "base")
MUTANTS = ("search_le", "dins_next", "rep_as_insert", "delta_cap")


def tid(x):
    return x.to_bytes(16, "big")


def num(i):
    """The id number of old entry i."""
    return GAP * (i + 1)


def entry(x, names=True, **over):
    """The entry of id number x: two tag keys, a third that tells old from appended, root names, a start
    within the hour behind T0, a duration around the whole-millisecond edge at 50 ms, now and then no end."""
    h = (x * 2654435761 + 0x9e37) & 0xffffffff
    h ^= h >> 15
    tags = {"k1": ["v%d-%s" % (h % 5, "xyz"[(h >> 3) % 3])], "k2": ["v%d-%s" % ((h >> 5) % 5, "xyz"[(h >> 8) % 3])],
            "k3": ["o%d" % ((h >> 10) % 3)]}
    if names:
        tags["root.service.name"] = ["svc-%d" % ((h >> 12) % 4)]
        tags["root.name"] = ["op-%d" % ((h >> 14) % 7)]
    start = (T0 + (h >> 4) % 3600) * S + (h % 1000) * MS
    dur = (50 * MS, 50 * MS - 1, 50 * MS + 1)[x % 11] if x % 11 < 3 else (1 + (h >> 6) % 400) * MS + h % 1000
    e = {"id": tid(x), "start": start, "end": 0 if x % 53 == 7 else start + dur, "tags": tags}
    tags.update(over.pop("tags", {}))
    e.update(over)
    return e


def old_entries(n, **kw):
    return [entry(num(i), **kw) for i in range(n)]


def ins(i, k=500, **kw):
    """An appended entry that lands directly before old entry i (behind the last one: i = n_old), the
    k-th of the up to 999 ids there. Its k3 values (a1 among them: the query that tells
    the appended entries from the old) sort before every old one: the key's table renumbers."""
    x = GAP * i + k
    tags = {"k3": sorted({"a1", "a%d" % (x % 3)})}
    tags.update(kw.pop("tags", {}))
    return entry(x, tags=tags, **kw)


def rep(i, **kw):
    """An appended page with old entry i's id: the two combine (the later end, the tags of both)."""
    o = entry(num(i))
    end = (o["end"] or o["start"]) + 3 * S
    tags = {"k3": sorted({"a1", "a%d" % (i % 3)})}
    tags.update(kw.pop("tags", {}))
    return {"id": o["id"], "start": o["start"], "end": end, "tags": tags}


class Case:
    def __init__(self, family, name, first, appended, queries=(), probes=(), **meta):
        self.family, self.name, self.first, self.appended = family, "%s/%s" % (family, name), first, appended
        # queries: non-empty over the grown file and other than over the old file (test_wal_merge_cases.py);
        # probes: compared as well, whatever they return
        self.queries = [dict(), dict(tags={"k3": "a1"})] + list(queries)
        self.probes = list(probes)
        self.meta = meta

    def __repr__(self):
        return self.name


# ---- the model ------------------------------------------------------------------------------
class Plan:
    def __init__(self, first_ids, app_ids, mutant=None):
        self.old = sorted(set(first_ids))
        self.delta = sorted(set(app_ids))
        self.dlo, self.dins, self.drep = [], [], []
        n = 0
        for i in self.delta:
            lo = bisect.bisect_left(self.old, i)
            found = lo < len(self.old) and self.old[lo] == i
            self.dlo.append(lo)
            self.dins.append(n)
            self.drep.append(found)
            if not found or mutant == "rep_as_insert":
                n += 1
        self.dins.append(n)
        self.n_old, self.ndelta = len(self.old), len(self.delta)
        self.inserts = sum(1 for r in self.drep if not r)
        self.replacements = self.ndelta - self.inserts
        self.n_new = self.n_old + self.inserts
        self.dpos = [a + b for a, b in zip(self.dlo, self.dins)]


def plan(first, appended, mutant=None):
    return Plan([e["id"] for e in first], [e["id"] for e in appended], mutant)


def source_map(p, mutant=None):
    """The source wal_merge_kernel's arithmetic picks for every j < n_new: ("d", delta entry) or
    ("o", old entry); None where it would read outside the old block or the tables."""
    nd = min(p.ndelta, K_LDS_DELTA) if mutant == "delta_cap" else p.ndelta
    out = []
    for j in range(p.n_new):
        lo, hi = 0, nd
        while lo < hi:
            m = (lo + hi) >> 1
            if p.dpos[m] <= j if mutant == "search_le" else p.dpos[m] < j:
                lo = m + 1
            else:
                hi = m
        if lo < nd and p.dpos[lo] == j:
            out.append(("d", lo))
            continue
        c = lo + 1 if mutant == "dins_next" else lo
        idx = j - p.dins[c] if c < len(p.dins) else -1
        out.append(("o", idx) if 0 <= idx < p.n_old else None)
    return out


def mutant_map(first, appended, mutant):
    """source_map with one slip in the index arithmetic: search_le (`pos[m] <= j` in the search), dins_next
    (dins[c + 1] for dins[c]), rep_as_insert (the plan counts a replacement among the inserts), delta_cap
    (only the first kLdsDelta delta entries are searched)."""
    assert mutant in MUTANTS
    return source_map(plan(first, appended, mutant), mutant)


def sorted_merge(p):
    """The same sequence from a plain merge of the two sorted id lists, the delta winning an equal id."""
    d = {i: k for k, i in enumerate(p.delta)}
    o = {i: k for k, i in enumerate(p.old)}
    return [("d", d[i]) if i in d else ("o", o[i]) for i in sorted(set(p.old) | set(p.delta))]


def merged_tags(c):
    """{id: {key: set of values}} of the grown file's entries (pages of one id combine their tags)."""
    out = {}
    for e in c.first + c.appended:
        t = out.setdefault(e["id"], {})
        for k, v in e["tags"].items():
            t.setdefault(k, set()).update(v)
    return out


def value_sets(entries, key):
    """The distinct value vectors of `key` over the entries of a file (pages of one id combined)."""
    by_id = {}
    for e in entries:
        if key in e["tags"]:
            by_id.setdefault(e["id"], set()).update(e["tags"][key])
    return {tuple(sorted(v)) for v in by_id.values()}


def npad(n):
    return (max(n, 1) + K_COL_PAD - 1) // K_COL_PAD * K_COL_PAD


def scan_base(entries):
    """devctx.hip scan_base of a freshly opened file without combined entries: the median start second
    (the upper one) less kDsBaseBack."""
    ss = sorted(e["start"] // S for e in entries)
    return max(ss[len(ss) // 2] - DS_BASE_BACK, 0)


# ---- the families ---------------------------------------------------------------------------
def spread(n_old, k):
    """k inserts spread evenly over the n_old + 1 gaps, round by round."""
    return [ins(i % (n_old + 1), 1 + i // (n_old + 1)) for i in range(k)]


def runs_family():
    f = "runs"
    return [
        Case(f, "2047-2048", old_entries(2047), [ins(2047)]),                        # the last position of run 0
        Case(f, "2047-2049", old_entries(2047), [ins(0), ins(2047)]),                # position 0 and the first of run 1
        Case(f, "2048-2049", old_entries(2048), [ins(2047)]),                        # old 2047 moves into run 1
        Case(f, "2049-2060", old_entries(2049), [ins(100 * i) for i in range(1, 12)]),  # only old entries in run 1, shifted by 11
    ]


def pad_family():
    f = "pad"
    both_sides = [dict(tags={"k3": "a1"}, start=T0 + 600, end=T0 + 2400), dict(tags={"k3": "a1"}, min_ms=50, max_ms=50),
                  dict(start=T0 + 600, end=T0 + 2400), dict(min_ms=50, max_ms=50)]
    return [
        Case(f, "4095-4096", old_entries(4095), [ins(2000)]),
        Case(f, "4095-4097", old_entries(4095), [ins(0), ins(4095)]),
        Case(f, "4096-4097", old_entries(4096), [ins(4095)]),
        # (a quarter of the inserts around position 4096 and behind it, between old entries)
        Case(f, "4000-4200", old_entries(4000), [ins(26 * i) for i in range(150)] + [ins(3900 + 2 * i) for i in range(50)],
             both_sides, both_sides=4),
    ]


def delta_family():
    f = "delta"
    mixed = sorted([ins(i) for i in range(2000)] + [rep(40 * r + 7) for r in range(49)], key=lambda e: e["id"])
    return [
        Case(f, "n100+2047", old_entries(100), spread(100, 2047)),
        Case(f, "n100+2048", old_entries(100), spread(100, 2048)),
        Case(f, "n100+2049", old_entries(100), spread(100, 2049)),
        Case(f, "n2100+2000ins+49rep", old_entries(2100), mixed[::2] + mixed[1::2]),
        Case(f, "rep-first-and-last", old_entries(65), [rep(64), ins(20), ins(21), ins(40), rep(0)]),
    ]


def layout_family():
    f, out = "layout", []
    for n in (1, 65):
        last, mid = n - 1, n // 2
        out += [
            Case(f, "n%d/head3" % n, old_entries(n), [ins(0, k) for k in (3, 1, 2)]),
            Case(f, "n%d/tail3" % n, old_entries(n), [ins(n, k) for k in (2, 3, 1)]),
            Case(f, "n%d/rep-first" % n, old_entries(n), [rep(0)]),
            Case(f, "n%d/ins-rep-ins" % n, old_entries(n), [ins(mid + 1, 1), rep(mid), ins(mid, 999)]),
            Case(f, "n%d/alternating" % n, old_entries(n), [ins(i) for i in range(n + 1)]),
        ]
        if n > 1:
            out += [Case(f, "n%d/rep-last" % n, old_entries(n), [rep(last)]),
                    Case(f, "n%d/all-replaced" % n, old_entries(n), [rep(i) for i in reversed(range(n))])]
    return out


def widths_family():
    f = "widths"

    def olds(n, nsets, fmt="w%03d"):
        return [entry(num(i), tags={"w": [fmt % (i % nsets)]}) for i in range(n)]
    out = []
    # one new set whose value sorts before every old one: every canonical id moves
    for n in (253, 254, 255):
        out.append(Case(f, "%d-%d" % (n, n + 1), olds(n, n), [ins(n // 2, tags={"w": ["a000"]})], [dict(tags={"w": "a000"})],
                        key="w", sets=(n, n + 1)))
    # the count stays: the new value joins the set of an entry that alone held its old one (the refreshed
    # dictionary keeps that set: from 254 the refreshed column is two bytes wide where a fresh open's is one)
    for n in (253, 254, 255):
        out.append(Case(f, "%d-%d" % (n, n), olds(n, n), [rep(n // 2, tags={"w": ["a000"]})], [dict(tags={"w": "a000"})],
                        key="w", sets=(n, n)))
    out.append(Case(f, "300-340/n2100", olds(2100, 300), [ins(50 * i + 3, tags={"w": ["x%03d" % i]}) for i in range(40)],
                    [dict(tags={"w": "x039"})], key="w", sets=(300, 340)))
    out.append(Case(f, "new-key-300", old_entries(50), [ins(i % 51, 1 + i // 51, tags={"nk": ["n%03d" % i]}) for i in range(300)],
                    [dict(tags={"nk": "n299"})], key="nk", sets=(0, 300)))
    return out


def names_family():
    f = "names"
    first = [ins(3, tags={"root.service.name": ["aaa-svc"], "root.name": ["aaa-op"]}), ins(30), ins(65)]
    qs = [dict(tags={"root.service.name": "aaa-svc"}), dict(tags={"root.name": "aaa-op"})]
    return [
        Case(f, "sort-first", old_entries(65), first, qs),
        Case(f, "appended-without", old_entries(65), [ins(0, names=False, tags={"k1": ["bare"]}), ins(10)], [dict(tags={"k1": "bare"})]),
        Case(f, "old-without", old_entries(65, names=False), [ins(0), ins(33, tags={"root.service.name": ["svc-1"]}), ins(65)],
             [dict(tags={"root.service.name": "svc-1"})]),
    ]


def base_family():
    f = "base"
    first = old_entries(65)
    lo = min(e["start"] for e in first) // S
    base = scan_base(first)

    def at(i, sec, dur=7 * MS, end=None, mark=None):
        st = sec * S + 250 * MS
        return ins(i, start=st, end=st + dur if end is None else end, tags={"k1": [mark or "at%d" % i]})
    moved = [at(5, lo - 1), at(15, lo - 70_000, end=0, mark="end0"), at(25, lo + 70_000, dur=50 * MS)]
    # the window of the packed word itself: rel = start second - base in [0, 0x7ffe], else escaped
    window = [at(35, base - 1), at(45, base), at(55, base + DS_REL_ESC - 1), at(60, base + DS_REL_ESC)]
    around = lambda sec: dict(start=sec - 1, end=sec + 1)  # noqa: E731
    qs = [around(lo - 1), around(lo + 70_000), dict(tags={"k1": "end0"}), dict(min_ms=50, max_ms=50, start=lo + 60_000, end=lo + 80_000)]
    qs += [around(base - 1), around(base), around(base + DS_REL_ESC - 1), around(base + DS_REL_ESC)]
    # (an entry without an end is in no time range: its bracket is compared, not required to answer)
    return [Case(f, "moved-and-window", first, moved + window, qs, [around(lo - 70_000), dict(start=lo - 70_001, end=lo + 70_001)],
                 lo=lo, base=base, moved=[lo - 1, lo - 70_000, lo + 70_000])]


def chained_stages():
    """2047 -> 2049 -> 4097: the second refresh reads what the kernel wrote, padding included, and the
    columns' stride changes from 4096 to 8192."""
    a = old_entries(2047)
    b = [ins(0), ins(2047)]
    c = [ins(i, 2) for i in range(2047)] + [ins(2047, 3)]
    return [a, b, c]


_cache = {}


def all_cases():
    if not _cache:
        for fam in (runs_family, pad_family, delta_family, layout_family, widths_family, names_family, base_family):
            for c in fam():
                assert c.name not in _cache
                _cache[c.name] = c
    return list(_cache.values())


def family(name):
    return [c for c in all_cases() if c.family == name]


def write_stages(root, name, stages):
    """One WAL search file per stage under root/name/<stage>/ (the same file name: each is a byte prefix of
    the next, as an appended-to file is) -> their paths."""
    import os

    import tempo_amd as T
    paths, ents, prev = [], [], b""
    for k, st in enumerate(stages):
        d = os.path.join(root, name.replace("/", "_"), str(k))
        os.makedirs(d)
        ents = ents + st
        paths.append(os.path.join(d, T.wal_filename(T.ENC_SNAPPY)))
        T.write_wal_search(paths[-1], ents, T.ENC_SNAPPY)
        data = open(paths[-1], "rb").read()
        assert data[:len(prev)] == prev and len(data) > len(prev)
        prev = data
    return paths
