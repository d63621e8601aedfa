"""dict_stream_kernel and the dict_sets_kernel identity path (search.hip) at constructed edges: the
cases of tests/dict_stream_cases.py (checked against the oracle on the host by
tests/test_dict_stream_cases.py) on the device. Every query is compared with the oracle record for
record, metrics included, and proves through tsg_debug_get that the path it means to test served it:
one dict_stream_kernel job, or one lane-per-value job where the gate must close.

What each case aims at in search.hip:
  residues      step(): the SWAR test of the first pair at all 16 starts of every lane, the DPP shift
                for the next lane's dword and lane 63's nx0 from the next KiB, the ring's slots;
                flush(): the masked last word of needles of 2, 3, 5, 13 and 17 bytes (a real
                dictionary over 1 MiB, no hooks; the second pair is the sampled rarest one)
  span*         qlo / qhi of a wave and `q < qhi`: an occurrence from nl + 16 bytes before a span
                boundary to 16 after it (nl 2, 17, 1024), spans of 1 KiB, 8 KiB (forced and planned)
                and 64 KiB; the stream's first bytes (qlo = lead) and last (qhi = end - nl + 1)
  value_bounds  `p + nl <= vend`: needles across two values, around an empty value, one byte longer
                than a value; equal to a value, at its first and last byte; mdone after several
                matches in one value
  second_pair   pq 0 / 1 / 2 and ps 0..3 of the second pair (pj 2..11 and none) across lane 63's
                hand-over; decoys that pass both pairs and fail verification
  short*        value_at over 2, 64, 65, 4096 and 4097 offsets; a batch of 64 verified starts in
                more than 128 values (the search of the global offsets past the staged s_off)
  runs*         16 candidates in every lane (the five-ballot append), the list at exactly kCandMax
                and at kCandMax + 1 when a step arrives, one candidate per lane (one ballot)
  end_*         last16 / last4: nbytes mod 16, needle length mod 4 and the four leads with the needle
                at the stream's last byte; a dictionary as long as the needle
  steered_pair  the host's choice of the rarest sampled pair (the plan's loop over pair_freq): a
                dictionary over 1 MiB whose filler makes pair j the rarest of a 14-byte needle, j over
                2..11: bytes after the second pair are left to verification; decoys as above
  jobs          `jobs[k].wave0 <= w` with ten jobs of several waves each; vmatch_base between jobs;
                dict_sets_kernel's identity words for nvals mod 32 = 0, 1, 31 and its value-set
                path for a multi-valued streamed key; a lane-path term in the same search
  end_short     a dictionary shorter than the needle: refused by the block's header, no job runs
  gate_*        the plan's `stream` condition: needle lengths 1, 2, 1024, 1025, the size threshold
                and the mean value length, either side
"""
import os

import pytest

from oracle import oracle as O
import tempo_amd as T
from tests import dict_stream_cases as D
from tests.helpers import match_key, tsg_key

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in D.all_cases()}


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dsedges"))
    return {name: D.write_case(d, c) for name, c in CASES.items()}


def _engine(env):
    os.environ.update(env)
    try:
        return T.Engine()
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def general():
    """the general path for every query: a closed gate then means prep_kernel's lane-per-value job"""
    e = _engine({"TSG_NO_FAST": "1"})
    yield e
    e.close()


@pytest.fixture(scope="module")
def lane():
    e = _engine({"TSG_DICT_STREAM": "0"})
    yield e
    e.close()


def counters():
    return T.debug_get("dict_stream_jobs"), T.debug_get("dict_lane_jobs")


def check(eng, blks, oblks, tags, jobs, lane=None, what=None):
    """One search against the oracle, record for record and metrics; `jobs`: the (stream, lane)
    dictionary jobs it must have run; lane = (engine, blocks): the lane-per-value engine must agree."""
    exp, omet, st = O.search(oblks, tags=tags, nthreads=2)
    assert st == 0
    s0, l0 = counters()
    got, met = eng.search(blks, T.Pipeline(T.SearchRequest(tags=tags)))
    s1, l1 = counters()
    assert (s1 - s0, l1 - l0) == jobs, (what, tags)
    assert [tsg_key(m) for m in got] == [match_key(m) for m in exp], (what, tags)
    assert (met.inspected_traces, met.inspected_bytes) == (omet["traces_inspected"], omet["bytes_inspected"]), (what, tags)
    if lane:
        ref, _ = lane[0].search(lane[1], T.Pipeline(T.SearchRequest(tags=tags)))
        assert [tsg_key(m) for m in ref] == [tsg_key(m) for m in got], (what, tags)


def run_case(eng, name, path, lane_eng=None):
    c = CASES[name]
    oblk = O.Block(path)
    blk = eng.open_block(path)
    lblk = lane_eng.open_block(path) if lane_eng else None
    T.debug_set("dict_stream_min", c.dmin)
    try:
        for span in c.spans:
            T.debug_set("dict_stream_span", span)
            for nd, streams in c.queries:
                # (None: the block's header refuses the needle, no dictionary job of either kind)
                jobs = (0, 0) if streams is None else (1, 0) if streams else (0, 1)
                check(eng, [blk], [oblk], {D.KEY: nd}, jobs, (lane_eng, [lblk]) if lblk else None, (name, span))
    finally:
        T.debug_set("dict_stream_span", 0)
        T.debug_set("dict_stream_min", 0)
        blk.close()
        if lblk:
            lblk.close()


def test_hooks_reject_bad_values():
    for bad in (1000, 512, 65536 + 1024, -1024):
        with pytest.raises(T.TsgError):
            T.debug_set("dict_stream_span", bad)
    with pytest.raises(T.TsgError):
        T.debug_get("no_such_counter")


def test_every_start_of_a_step(engine, paths, lane):
    run_case(engine, "residues", paths["residues"], lane)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("span")])
def test_span_boundaries(engine, paths, name):
    run_case(engine, name, paths[name])


def test_value_boundaries(engine, paths, lane):
    run_case(engine, "value_bounds", paths["value_bounds"], lane)


def test_second_pair(engine, paths, lane):
    run_case(engine, "second_pair", paths["second_pair"], lane)


def test_steered_second_pair(engine, paths, lane):
    run_case(engine, "steered_pair", paths["steered_pair"], lane)


@pytest.mark.parametrize("span", [D.JOB_SPAN, 0])
def test_jobs_and_bitmaps(engine, lane, tmp_path_factory, span):
    blocks = D.jobs_blocks()
    ps = D.write_jobs_blocks(str(tmp_path_factory.mktemp("dsjobs")), blocks)
    oblks = [O.Block(p) for p in ps]
    blks, lblks = [engine.open_block(p) for p in ps], [lane.open_block(p) for p in ps]
    T.debug_set("dict_stream_min", D.JOB_DMIN)
    T.debug_set("dict_stream_span", span)
    try:
        for tags, ns, nl in D.JOB_QUERIES:
            check(engine, blks, oblks, tags, (ns, nl), (lane, lblks), ("jobs", span))
    finally:
        T.debug_set("dict_stream_span", 0)
        T.debug_set("dict_stream_min", 0)
        for b in blks + lblks:
            b.close()


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("short") or n.startswith("runs")])
def test_lists_and_batches(engine, paths, name):
    run_case(engine, name, paths[name])


def test_end_of_stream(engine, paths):
    for name in CASES:
        if name.startswith("end_"):
            run_case(engine, name, paths[name])


def test_gate(general, paths):
    for name in CASES:
        if name.startswith("gate"):
            run_case(general, name, paths[name])


def test_no_stale_match_bytes(engine, paths):
    """On one engine in this order: a needle in every value, an absent one, one in a single value. A
    match byte left from the first would show in the later two. (A dictionary over 1 MiB: an absent
    needle reaches the kernel only there, a smaller block is refused by its header's values.)"""
    c, path = CASES["residues"], paths["residues"]
    oblk, blk = O.Block(path), engine.open_block(path)
    try:
        for nd in ("..", "no-such-needle", c.values[0][:8]):
            check(engine, [blk], [oblk], {D.KEY: nd}, (1, 0), None, "stale")
    finally:
        blk.close()
