"""The refreshes of tests/wal_merge_cases.py on the CPU: the model's per-position source map against a
plain sorted merge, every family's defining numbers asserted from the entries alone, the oracle's
answers over the grown file against those over the old one (a case whose queries answer the same
before and after could not notice a stale column), and the model's index arithmetic with one slip
at a time, each caught by named cases. No kernel runs here; the GPU side is
tests/test_gpu_wal_merge_edges.py."""
import pytest

from oracle import oracle as O
from tests import wal_merge_cases as W
from tests.helpers import match_key

S = W.S
# name -> (n_old, n_new, ndelta, inserts, replacements, delta positions among {0, n_new - 1, 2047, 2048})
NUMBERS = {
    "runs/2047-2048": (2047, 2048, 1, 1, 0, {2047}),
    "runs/2047-2049": (2047, 2049, 2, 2, 0, {0, 2048}),
    "runs/2048-2049": (2048, 2049, 1, 1, 0, {2047}),
    "runs/2049-2060": (2049, 2060, 11, 11, 0, set()),
    "pad/4095-4096": (4095, 4096, 1, 1, 0, set()),
    "pad/4095-4097": (4095, 4097, 2, 2, 0, {0, 4096}),
    "pad/4096-4097": (4096, 4097, 1, 1, 0, set()),
    "pad/4000-4200": (4000, 4200, 200, 200, 0, {0}),
    "delta/n100+2047": (100, 2147, 2047, 2047, 0, {0, 2047, 2048, 2146}),
    "delta/n100+2048": (100, 2148, 2048, 2048, 0, {0, 2047, 2048, 2147}),
    "delta/n100+2049": (100, 2149, 2049, 2049, 0, {0, 2047, 2048, 2148}),
    "delta/n2100+2000ins+49rep": (2100, 4100, 2049, 2000, 49, {0, 2048}),
    "delta/rep-first-and-last": (65, 68, 5, 3, 2, {0, 67}),
    "layout/n1/head3": (1, 4, 3, 3, 0, {0}),
    "layout/n1/tail3": (1, 4, 3, 3, 0, {3}),
    "layout/n1/rep-first": (1, 1, 1, 0, 1, {0}),
    "layout/n1/ins-rep-ins": (1, 3, 3, 2, 1, {0, 2}),
    "layout/n1/alternating": (1, 3, 2, 2, 0, {0, 2}),
    "layout/n65/head3": (65, 68, 3, 3, 0, {0}),
    "layout/n65/tail3": (65, 68, 3, 3, 0, {67}),
    "layout/n65/rep-first": (65, 65, 1, 0, 1, {0}),
    "layout/n65/ins-rep-ins": (65, 67, 3, 2, 1, set()),
    "layout/n65/alternating": (65, 131, 66, 66, 0, {0, 130}),
    "layout/n65/rep-last": (65, 65, 1, 0, 1, {64}),
    "layout/n65/all-replaced": (65, 65, 65, 0, 65, {0, 64}),
    "widths/253-254": (253, 254, 1, 1, 0, set()),
    "widths/254-255": (254, 255, 1, 1, 0, set()),
    "widths/255-256": (255, 256, 1, 1, 0, set()),
    "widths/253-253": (253, 253, 1, 0, 1, set()),
    "widths/254-254": (254, 254, 1, 0, 1, set()),
    "widths/255-255": (255, 255, 1, 0, 1, set()),
    "widths/300-340/n2100": (2100, 2140, 40, 40, 0, set()),
    "widths/new-key-300": (50, 350, 300, 300, 0, {0, 349}),
    "names/sort-first": (65, 68, 3, 3, 0, {67}),
    "names/appended-without": (65, 67, 2, 2, 0, {0}),
    "names/old-without": (65, 68, 3, 3, 0, {0, 67}),
    "base/moved-and-window": (65, 72, 7, 7, 0, set()),
}


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in W.all_cases()}


@pytest.fixture(scope="module")
def plans(cases):
    return {n: W.plan(c.first, c.appended) for n, c in cases.items()}


def test_model_reproduces_the_sorted_merge(cases, plans):
    for n, p in plans.items():
        got = W.source_map(p)
        assert got == W.sorted_merge(p), n
        assert len(got) == p.n_new and sorted(k for s, k in got if s == "d") == list(range(p.ndelta)), n
        # the model's plan is a plan: positions ascend strictly, dins counts the inserts
        assert all(a < b for a, b in zip(p.dpos, p.dpos[1:])) and len(p.dins) == p.ndelta + 1 and p.dins[-1] == p.inserts, n
    ents = []
    for st in W.chained_stages():  # each refresh of the chain, on what the one before left
        p = W.plan(ents, st)
        assert W.source_map(p) == W.sorted_merge(p)
        ents = ents + st


def test_numbers(cases, plans):
    assert set(cases) == set(NUMBERS) and {c.family for c in cases.values()} == set(W.FAMILIES)
    for n, p in plans.items():
        c = cases[n]
        edges = set(p.dpos) & {0, p.n_new - 1, 2047, 2048}
        assert (p.n_old, p.n_new, p.ndelta, p.inserts, p.replacements, edges) == NUMBERS[n], n
        # one page per entry, no id twice within a part: the refresh's counters follow from the lists
        assert len({e["id"] for e in c.first}) == len(c.first) == p.n_old, n
        assert len({e["id"] for e in c.appended}) == len(c.appended) == p.ndelta, n
    assert [len(s) for s in W.chained_stages()] == [2047, 2, 2048]


def test_runs(plans):
    """Real entries in the second run of 2048, from the delta and from the old block."""
    second = {n: [s for s in W.source_map(p)[W.K_RUN:]] for n, p in plans.items() if n.startswith("runs/")}
    assert second["runs/2047-2048"] == []                  # run 0 exactly full, its last entry from the delta
    assert second["runs/2047-2049"] == [("d", 1)]          # the first entry of run 1 alone (the `t` loop breaks at once)
    assert second["runs/2048-2049"] == [("o", 2047)]       # ... an old entry, read from run 0's last position
    assert second["runs/2049-2060"] == [("o", k) for k in range(2048 - 11, 2049)]  # inserts below 2048 only
    assert max(plans["runs/2049-2060"].dpos) < W.K_RUN


def test_pad(plans):
    """ceil(n / 4096) changes, or stays, as aimed: the scan columns' stride is the padded length."""
    change = {n: (W.npad(p.n_old), W.npad(p.n_new)) for n, p in plans.items() if n.startswith("pad/")}
    assert change == {"pad/4095-4096": (4096, 4096), "pad/4095-4097": (4096, 8192), "pad/4096-4097": (4096, 8192),
                      "pad/4000-4200": (4096, 8192)}
    assert all(W.npad(p.n_old) == W.npad(p.n_new) == 4096 for n, p in plans.items() if not n.startswith(("pad/", "delta/n2100")))
    p = plans["delta/n2100+2000ins+49rep"]
    assert (W.npad(p.n_old), W.npad(p.n_new)) == (4096, 8192)
    src = W.source_map(plans["pad/4000-4200"])
    assert {s for s, _ in src[:4096]} == {s for s, _ in src[4096:]} == {"d", "o"}  # both sources on both sides of 4096
    stages = W.chained_stages()
    assert [W.npad(n) for n in (2047, 2049, 4097)] == [4096, 4096, 8192]
    assert len(stages[0]) + len(stages[1]) == 2049 and sum(map(len, stages)) == 4097


def test_delta(plans):
    """Below, at and above the staged capacity; replacements at both ends of the delta."""
    assert [plans["delta/n100+%d" % k].ndelta - W.K_LDS_DELTA for k in (2047, 2048, 2049)] == [-1, 0, 1]
    p = plans["delta/n2100+2000ins+49rep"]
    assert p.ndelta > W.K_LDS_DELTA and p.drep.count(True) == 49
    k = [i for i, r in enumerate(p.drep) if r]
    assert k[0] > 0 and k[-1] < p.ndelta - 1 and all(b - a > 1 for a, b in zip(k, k[1:]))  # interleaved with the inserts
    p = plans["delta/rep-first-and-last"]
    assert p.drep[0] and p.drep[-1] and (p.dlo[0], p.dlo[-1]) == (0, p.n_old - 1) and not any(p.drep[1:-1])


def test_layout(plans):
    for n in (1, 65):
        p = plans["layout/n%d/head3" % n]
        assert p.dpos == [0, 1, 2] and p.dlo == [0, 0, 0]
        p = plans["layout/n%d/tail3" % n]
        assert p.dpos == [n, n + 1, n + 2] and p.dlo == [n, n, n]
        p = plans["layout/n%d/rep-first" % n]
        assert p.dpos == [0] and p.drep == [True]
        p = plans["layout/n%d/ins-rep-ins" % n]
        assert p.drep == [False, True, False] and p.dpos == [n // 2, n // 2 + 1, n // 2 + 2]  # neighbours
        p = plans["layout/n%d/alternating" % n]
        assert p.dpos == list(range(0, 2 * n + 1, 2))
    assert plans["layout/n65/rep-last"].dpos == [64] and plans["layout/n65/rep-last"].drep == [True]
    p = plans["layout/n65/all-replaced"]
    assert p.ndelta == p.n_old == p.n_new and all(p.drep) and p.dins == [0] * 66


def test_widths(cases, plans):
    """Distinct value vectors of the case's key before and after, counted over the entries."""
    got = {}
    for n, c in cases.items():
        if c.family != "widths":
            continue
        k = c.meta["key"]
        before, after = W.value_sets(c.first, k), W.value_sets(c.first + c.appended, k)
        assert (len(before), len(after)) == c.meta["sets"], n
        got[n] = c.meta["sets"]
        new_vals = {v for s in after for v in s} - {v for s in before for v in s}
        if before and n != "widths/300-340/n2100":  # a new value that sorts before every old one: every id moves
            assert len(new_vals) == 1 and min(new_vals) < min(v for s in before for v in s), n
    assert got == {"widths/253-254": (253, 254), "widths/254-255": (254, 255), "widths/255-256": (255, 256),
                   "widths/253-253": (253, 253), "widths/254-254": (254, 254), "widths/255-255": (255, 255), "widths/300-340/n2100": (300, 340),
                   "widths/new-key-300": (0, 300)}
    for n in ("widths/253-253", "widths/254-254", "widths/255-255"):  # the count stays through a combined entry: the dictionary still grows
        assert plans[n].replacements == 1 and plans[n].inserts == 0
    assert plans["widths/300-340/n2100"].n_old > W.K_RUN      # the two-byte column crosses a run
    assert plans["widths/new-key-300"].ndelta >= 300
    assert not any("nk" in e["tags"] for e in cases["widths/new-key-300"].first)


def test_names(cases):
    key = lambda es, k: sorted({v for e in es for v in e["tags"].get(k, [])})  # noqa: E731
    c = cases["names/sort-first"]
    for k in ("root.service.name", "root.name"):
        assert key(c.appended, k)[0] < key(c.first, k)[0] and len(key(c.first, k)) > 1
    c = cases["names/appended-without"]
    assert [("root.name" in e["tags"], "root.service.name" in e["tags"]) for e in c.appended] == [(False, False), (True, True)]
    c = cases["names/old-without"]
    assert not key(c.first, "root.name") and not key(c.first, "root.service.name")
    assert key(c.appended, "root.name") and key(c.appended, "root.service.name")


def test_base(cases):
    """Starts against the old block's base (its median start second less 16383) and the 15-bit window."""
    c = cases["base/moved-and-window"]
    lo, base = min(e["start"] for e in c.first) // S, W.scan_base(c.first)
    assert (lo, base) == (c.meta["lo"], c.meta["base"]) and base < lo - 1 < base + W.DS_REL_ESC
    ss = [e["start"] // S for e in c.appended]
    assert ss == [lo - 1, lo - 70_000, lo + 70_000, base - 1, base, base + 0x7ffe, base + 0x7fff]
    escaped = [not 0 <= s - base < W.DS_REL_ESC for s in ss]  # ds_word.hpp ds_pack's rel
    assert escaped == [False, True, True, True, False, False, True]
    assert [e["end"] == 0 for e in c.appended].count(True) == 1 and c.appended[1]["end"] == 0
    assert c.appended[2]["end"] - c.appended[2]["start"] == 50 * W.MS
    for s in ss:  # a time-range query brackets each
        assert any(q.get("start", 0) and q["start"] <= s <= q["end"] and q["end"] - q["start"] <= 2 for q in c.queries + c.probes), s


def search(blk, q):
    exp, met, st = O.search([blk], tags=q.get("tags"), min_ms=q.get("min_ms", 0), max_ms=q.get("max_ms", 0),
                            start=q.get("start", 0), end=q.get("end", 0))
    assert st == 0
    return [match_key(m) for m in exp]


@pytest.mark.parametrize("fam", W.FAMILIES)
def test_queries_answer_and_change(fam, tmp_path):
    for c in W.family(fam):
        old_p, new_p = W.write_stages(str(tmp_path), c.name, [c.first, c.appended])
        old, new = O.Block(old_p, wal=True), O.Block(new_p, wal=True)
        p = W.plan(c.first, c.appended)
        for q in c.queries:
            a, b = search(old, q), search(new, q)
            assert b and a != b, (c.name, q)
        dense = search(new, dict())
        assert [m[2] for m in dense] == sorted(set(p.old) | set(p.delta)), c.name  # every record, in id order
        if "both_sides" in c.meta:  # answers below and at or above position 4096
            for q in c.queries[-c.meta["both_sides"]:]:
                at = [m[1] for m in search(new, q)]
                assert min(at) < W.K_COL_PAD <= max(at), (c.name, q)


# mutant -> cases that must catch it (and, for the cap, the ones at and below it that must not)
CAUGHT_BY = {
    "search_le": ["layout/n1/rep-first", "layout/n65/head3", "runs/2047-2048", "delta/n100+2047"],
    "dins_next": ["layout/n65/tail3", "layout/n1/alternating", "runs/2049-2060", "delta/n100+2048"],
    "rep_as_insert": ["layout/n65/rep-first", "layout/n1/ins-rep-ins", "layout/n65/all-replaced", "delta/rep-first-and-last"],
    "delta_cap": ["delta/n100+2049", "delta/n2100+2000ins+49rep"],
}
NOT_CAUGHT_BY = {"delta_cap": ["delta/n100+2047", "delta/n100+2048"], "rep_as_insert": ["runs/2049-2060", "layout/n65/alternating"]}


def test_mutants_are_caught(cases, plans, capsys):
    table = {}
    for m in W.MUTANTS:
        table[m] = [n for n, c in cases.items() if c.family in ("layout", "runs", "delta")
                    and W.mutant_map(c.first, c.appended, m) != W.sorted_merge(plans[n])]
    with capsys.disabled():
        for m, names in table.items():
            print("\nmutant %s: caught by %d cases: %s" % (m, len(names), ", ".join(names)))
    for m in W.MUTANTS:
        assert set(CAUGHT_BY[m]) <= set(table[m]), m
        assert not set(NOT_CAUGHT_BY.get(m, [])) & set(table[m]), m
    # every case of the three families catches some mutant, and each family catches what it can hold
    assert {n for names in table.values() for n in names} == {n for n, c in cases.items() if c.family in ("layout", "runs", "delta")}
    assert table["delta_cap"] == CAUGHT_BY["delta_cap"]  # nothing else has a delta above 2048
