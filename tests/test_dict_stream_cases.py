"""tests/dict_stream_cases.py on the host: the builder's model of each case equals the oracle, and each
case reaches the edge of dict_stream_kernel it was built for (asserted here, not assumed: a case that
cannot be constructed fails)."""
import pytest

from oracle import oracle as O
from tests import dict_stream_cases as D


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in D.all_cases()}


def test_model_equals_oracle(cases, tmp_path):
    for c in cases.values():
        m, blk = D.Model(c.values), O.Block(D.write_case(str(tmp_path), c))
        for nd, _ in c.queries:
            exp, omet, st = O.search([blk], tags={D.KEY: nd}, nthreads=2)
            assert st == 0
            assert [r["entry_idx"] for r in exp] == m.matches(nd), (c.name, nd)


def test_residues_cover_a_step(cases):
    c = cases["residues"]
    m = D.Model(c.values)
    assert m.nbytes > 1 << 20 and len(set(len(v) for v in c.values)) == 1 and len(c.values[0]) % 2 == 1
    full = m.matches(D.MASTER)
    res = {(m.apos(v) + c.values[v].index(D.MASTER)) % 1024 for v in full}
    assert res == set(range(1024))  # every lane, every start of a lane, lane 63 into the next KiB
    assert all(c.values[v].count(D.MASTER[:2]) == 1 for v in full)
    counts = m.pair_counts()
    for nl in D.RESIDUE_NL:
        got = m.matches(D.MASTER[:nl])
        # the values with the whole needle, and the near misses whose changed byte lies past this needle
        assert set(full) <= set(got) and len(got) < len(c.values)
        near = [v for v in range(len(c.values)) if D.MASTER[:nl - 1] in c.values[v] and v not in got]
        assert near, nl  # values that hold all but the needle's last byte
        assert m.pj(D.MASTER[:nl], counts) in range(2, min(nl - 2, D.PAIR_MAX) + 1) or nl < 4


def test_span_sweeps(cases):
    names = [c.name for c in cases.values() if c.name.startswith("span")]
    assert sorted(names) == sorted("span%d_nl%d" % (s, nl) for s in (1024, 8192, 65536) for nl in (2, 17, 1024))
    for name in names:
        c = cases[name]
        m, span, nl, ds = D.Model(c.values), c.note["span"], c.note["nl"], c.note["ds"]
        assert ds == list(range(-(nl + 16), 17)), name
        assert c.spans == ((8192, 0) if span == 8192 else (span,))  # 8 KiB: forced and as planned
        assert len(set(c.note["needles"])) == len(ds) and all(len(nd) == nl for nd in c.note["needles"])
        seen = []
        for nd in c.note["needles"]:
            occ = m.occurrences(nd)
            assert len(occ) == 1 and len(m.matches(nd)) == 1, (name, nd[:8])
            at = occ[0] % span
            seen.append(at - span if at >= span // 2 else at)
        if span == 1024 and nl == 1024:  # (offsets beyond half a span: taken from the boundary the run crosses)
            seen = [m.occurrences(nd)[0] - 2048 for nd in c.note["needles"]]
        assert seen == ds, name  # offsets of the occurrences from the span boundary
        first, last = c.queries[-2][0], c.queries[-1][0]
        assert m.occurrences(first)[0] == m.lead and len(first) == nl  # the stream's first bytes
        assert m.occurrences(last) == [m.lead + m.nbytes - nl] and last == c.note["last"]  # and its last
        assert m.lead + m.nbytes > span + 16 + nl  # the boundary and everything around it lie in the stream


def test_value_boundaries(cases):
    c = cases["value_bounds"]
    m, n = D.Model(c.values), c.note
    assert len(c.values) >= 255 and "" in c.values[1:-1] and m.nbytes > 1 << 20 and c.dmin == 0
    assert sorted((nl, s) for _, nl, s in n["split"]) == [(nl, s) for nl in (2, 5, 17) for s in range(1, nl)]
    for nd in [x[0] for x in n["split"]] + n["empty"] + n["short"]:
        assert len(m.occurrences(nd)) == 1 and m.matches(nd) == [], nd  # only across two values
    for nd in n["empty"]:
        k = m.stream.index(nd)
        v = max(i for i in range(len(m.off)) if m.off[i] <= k)
        assert c.values[v + 1] == "" and m.off[v + 1] < k + len(nd)
    for nd in n["short"]:
        assert nd[:-1] in c.values
    for nd, v in n["hit"]:
        assert v in m.matches(nd)
    eq, first, last = n["hit"][0::3], n["hit"][1::3], n["hit"][2::3]
    assert all(c.values[v] == nd for nd, v in eq) and all(c.values[v].startswith(nd) for nd, v in first)
    assert all(c.values[v].endswith(nd) and m.matches(nd)[-1] == v for nd, v in last)
    assert m.matches("r$") == n["mdone"] and c.values[n["mdone"][0]].count("r$") == 3


def test_second_pairs(cases):
    c = cases["second_pair"]
    m = D.Model(c.values)
    assert m.pair_counts() is None  # no sampled counts: the last pair in reach
    assert {m.pj(nd) for nd, _ in c.queries} == {0} | set(range(2, 12))
    assert [m.pj(D.pair_needle(nl)) for nl in (3, 4, 13, 14)] == [0, 2, 11, 11]
    for nd, _ in c.queries:
        assert {a % 1024 for a in m.occurrences(nd)} == set(D.PAIR_RES), nd
        assert len(m.matches(nd)) == len(D.PAIR_RES)
        pj = m.pj(nd)
        assert c.note["decoys"][nd] or len(nd) == 4  # (length 4: no byte between or after the pairs)
        for d in c.note["decoys"][nd]:
            assert len(d) == len(nd) and d[:2] == nd[:2] and (not pj or d[pj:pj + 2] == nd[pj:pj + 2])
            assert sum(a != b for a, b in zip(d, nd)) == 1 and nd not in d
            assert {a % 1024 for a in m.occurrences(d)} == {1000, 1012, 1023, 5}


def test_steered_second_pairs(cases):
    c = cases["steered_pair"]
    m = D.Model(c.values)
    counts = m.pair_counts()
    assert counts is not None and c.dmin == 0  # over 1 MiB: the sampled counts decide
    pjs = [m.pj(nd, counts) for nd, _ in c.queries]
    assert pjs == list(range(2, 12)) + [2, 0]  # each j once from needles of 14 bytes; lengths 4 and 3
    assert [len(nd) for nd, _ in c.queries] == [14] * 10 + [4, 3]
    for (nd, _), pj in zip(c.queries, pjs):
        assert {a % 1024 for a in m.occurrences(nd)} == set(D.PAIR_RES), nd
        assert len(m.matches(nd)) == len(D.PAIR_RES)
        if len(nd) == 14:
            ds = c.note["decoys"][nd]
            where = {next(i for i in range(14) if d[i] != nd[i]) for d in ds}
            assert where == {b for b in (pj - 1, pj + 2) if 2 <= b < 14}  # between the pairs, after them
            for d in ds:
                assert d[:2] == nd[:2] and d[pj:pj + 2] == nd[pj:pj + 2] and m.matches(d)
                assert {a % 1024 for a in m.occurrences(d)} == {1000, 1012, 1023, 5}


def test_short_dictionary_never_reaches_a_kernel(cases, tmp_path):
    """The issue's "dictionary shorter than the needle": not constructible. The oracle skips the block on
    its header for such a needle, and only dictionaries over 1 MiB (longer than any streamed needle) are
    exempt from the header."""
    c = cases["end_short"]
    m, blk = D.Model(c.values), O.Block(D.write_case(str(tmp_path), c))
    for nd, streams in c.queries:
        assert streams is None and len(nd) > m.nbytes
        exp, omet, st = O.search([blk], tags={D.KEY: nd}, nthreads=1)
        assert (st, exp, omet["blocks_skipped"], omet["traces_inspected"]) == (0, [], 1, 0)
    assert 1024 < 1 << 20  # kStreamMaxNeedle < kDeferMinBytes


def test_jobs_blocks(tmp_path):
    blocks = D.jobs_blocks()
    assert [len(b) for b in blocks] == list(D.JOB_NVALS) and {n % 32 for n in D.JOB_NVALS} >= {0, 1, 31}
    oblks = [O.Block(p) for p in D.write_jobs_blocks(str(tmp_path), blocks)]
    waves = 0
    for ents in blocks:
        n = len(ents)
        for k in ("ka", "kb"):  # identity: one distinct value per entry; long enough to stream
            vals = [e[k][0] for e in ents]
            assert len(set(vals)) == n and sum(map(len, vals)) >= 16 * n and sum(map(len, vals)) > D.JOB_DMIN
            waves += -(-sum(map(len, vals)) // D.JOB_SPAN)
        kc = {e["kc"][0] for e in ents}
        assert sum(map(len, kc)) < 16 * len(kc) and sum(map(len, kc)) > D.JOB_DMIN  # the gate closes on the mean
        km = {v for e in ents for v in e["km"]}
        assert len(km) == 37 and any(len(e["km"]) > 1 for e in ents) and sum(map(len, km)) >= 16 * 37
        hits = [i for i, e in enumerate(ents) if "ja#" in e["ka"][0]]
        assert {0, 31, 32, 63, n - 1} <= set(hits) and len(hits) < n  # the edges of the bitmap words
    assert waves > 4 * 10  # several waves per job: the job lookup by wave0 sees ten jobs
    assert max(s + l for _, s, l in D.JOB_QUERIES) == 10 and any(s and l for _, s, l in D.JOB_QUERIES)
    for tags, _, _ in D.JOB_QUERIES:
        exp, omet, st = O.search(oblks, tags=tags, nthreads=2)
        want = D.jobs_expected(blocks, tags)
        assert st == 0 and [(r["block_idx"], r["entry_idx"]) for r in exp] == want and want, tags
        assert {b for b, _ in want} == set(range(5)) and omet["blocks_skipped"] == 0  # every block runs its jobs


def test_batches_and_lists(cases):
    for n in (1, 63, 64, 1000, 4095, 4096):
        c = cases["short%d" % n]
        m = D.Model(c.values)
        assert len(c.values) + 1 == n + 1 and all(16 <= len(v) <= 24 for v in c.values)
        hit = m.matches("qz")
        assert hit == list(range(0, n, 3))
        if n >= 1000:  # one batch of 64 verified starts lies in more than 128 values
            assert all(hit[b + 63] - hit[b] > 128 for b in range(0, len(hit) - 63, 64))
        assert m.matches("fir") == [0] and m.matches("last") == [n - 1]
    assert {len(cases["short%d" % n].values) + 1 for n in (1, 63, 64, 4095, 4096)} == {2, 64, 65, 4096, 4097}
    for extra in (0, 1):
        c = cases["runs%d" % extra]
        m = D.Model(c.values)
        occ = m.occurrences("aa")
        step = [a // 1024 for a in occ]
        assert step.count(1) == 1024 and step.count(0) == extra  # the list at 1024 / 1025 when step 1 arrives
        later = [a for a in occ if a // 1024 > 1]
        assert len(later) == 64 and all(b - a == 16 for a, b in zip(later, later[1:]))  # one per lane


def test_end_residues(cases):
    seen = set()
    for c in cases.values():
        if not c.name.startswith("end_l"):
            continue
        m = D.Model(c.values)
        for nd, _ in c.queries:
            assert m.occurrences(nd) == [m.lead + m.nbytes - len(nd)] and m.matches(nd) == [len(c.values) - 1]
            seen.add((m.nbytes % 16, len(nd) % 4, m.lead))
    assert seen == {(r, k, lead) for r in range(16) for k in range(4) for lead in (0, 4, 8, 12)}
    c = cases["end_exact"]
    m = D.Model(c.values)
    assert [len(nd) - m.nbytes for nd, _ in c.queries] == [0] and m.matches(c.queries[0][0]) == [0]


def test_gate(cases):
    g = {c.name: [(len(nd), s) for nd, s in c.queries] for c in cases.values() if c.name.startswith("gate")}
    assert g["gate_needle"][:4] == [(1, False), (2, True), (1024, True), (1025, False)]
    assert (g["gate_min0"], g["gate_min1"]) == ([(2, False)], [(2, True)])
    assert (g["gate_mean1"], g["gate_mean0"]) == ([(2, False)], [(2, True)])
    for name, over in (("gate_min0", 0), ("gate_min1", 1)):
        assert D.Model(cases[name].values).nbytes == cases[name].dmin + over
    for name, short in (("gate_mean1", 1), ("gate_mean0", 0)):
        m = D.Model(cases[name].values)
        assert m.nbytes == 16 * len(m.values) - short
