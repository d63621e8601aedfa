"""The round planner of tsg_find_ids over blocks whose data file stays on disk
(tempo_amd/csrc/find_rounds.hpp plan_find_rounds), through tests/find_rounds_check.cpp,
which includes the header device_find uses. The program is built twice, plainly and with
AddressSanitizer + UBSan, and every case runs through both:

* hand-computed plans: pages that fill the cap exactly, one byte more, a page longer than the cap
  alone in its round, no page at all (one empty round), the 16-byte packing of the offsets, a cap
  of one page (a round per page), a cap of 1 and the default cap;
* the properties of a plan over random page lists: the rounds are consecutive runs that cover the
  list, offsets are multiples of 16 and pages do not overlap, a round of more than one page fits
  the cap, and a round is maximal (the next round's first page would not have fit behind it).

The GPU side (the rounds' results against one big round) is tests/test_gpu_find_on_demand.py."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_CAP = 256 << 20


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fr") / "find_rounds_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if request.param != "plain" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tempo_amd", "csrc")] + san +
                          [os.path.join(ROOT, "tests", "find_rounds_check.cpp"), "-o", out])
    return out


def plan(exe, cap, lens):
    """([(first, count, bytes)], [offset per page])"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe, str(cap)] + [str(n) for n in lens], capture_output=True, text=True, env=env)
    assert res.returncode == 0 and not res.stderr, res.stderr[-4000:]
    lines = res.stdout.splitlines()
    rounds = [tuple(int(x) for x in ln.split()) for ln in lines[:-1]]
    offs = [] if lines[-1] == "-" else [int(x) for x in lines[-1].split()]
    return rounds, offs


def test_pages_that_fill_the_cap_exactly(exe):
    assert plan(exe, 64, [32, 32]) == ([(0, 2, 64)], [0, 32])
    assert plan(exe, 96, [32, 16, 48]) == ([(0, 3, 96)], [0, 32, 48])
    assert plan(exe, 100, [100]) == ([(0, 1, 100)], [0])


def test_one_byte_over_the_cap_starts_a_round(exe):
    assert plan(exe, 64, [32, 33]) == ([(0, 1, 32), (1, 1, 33)], [0, 0])
    assert plan(exe, 96, [32, 16, 49, 47]) == ([(0, 2, 48), (2, 1, 49), (3, 1, 47)], [0, 32, 0, 0])
    # the padding counts: 30 + 34 bytes are 64, but the second page starts at 32
    assert plan(exe, 64, [30, 34]) == ([(0, 1, 30), (1, 1, 34)], [0, 0])
    assert plan(exe, 66, [30, 34]) == ([(0, 2, 66)], [0, 32])


def test_a_page_longer_than_the_cap_is_alone(exe):
    assert plan(exe, 64, [10, 200, 10, 10]) == ([(0, 1, 10), (1, 1, 200), (2, 2, 26)], [0, 0, 0, 16])
    assert plan(exe, 64, [200]) == ([(0, 1, 200)], [0])
    assert plan(exe, 64, [200, 200]) == ([(0, 1, 200), (1, 1, 200)], [0, 0])


def test_no_page_is_one_empty_round(exe):
    for cap in (0, 1, 64):
        assert plan(exe, cap, []) == ([(0, 0, 0)], [])


def test_offsets_are_packed_at_16_bytes(exe):
    rounds, offs = plan(exe, 1 << 20, [1, 15, 16, 17, 6, 31, 32, 33])
    assert offs == [0, 16, 32, 48, 80, 96, 128, 160] and rounds == [(0, 8, 193)]


def test_a_cap_of_one_page_is_a_round_per_page(exe):
    lens = [700] * 9
    rounds, offs = plan(exe, 700, lens)
    assert rounds == [(i, 1, 700) for i in range(9)] and offs == [0] * 9
    rounds, _ = plan(exe, 1, [5, 900, 16, 1])   # a cap of 1: every page is longer than it
    assert rounds == [(0, 1, 5), (1, 1, 900), (2, 1, 16), (3, 1, 1)]
    # two pages of 700 fit 1404 (704 + 700) and not 1403
    assert [r[1] for r in plan(exe, 1404, lens)[0]] == [2, 2, 2, 2, 1]
    assert [r[1] for r in plan(exe, 1403, lens)[0]] == [1] * 9


def test_cap_zero_is_the_default(exe):
    big = (1 << 32) - 1  # (a record length is 32 bits)
    assert plan(exe, 0, [big]) == ([(0, 1, big)], [0])
    lens = [DEFAULT_CAP // 2, DEFAULT_CAP // 2, 1]
    assert plan(exe, 0, lens) == ([(0, 2, DEFAULT_CAP), (2, 1, 1)], [0, DEFAULT_CAP // 2, 0])
    assert plan(exe, 0, lens) == plan(exe, DEFAULT_CAP, lens)


@pytest.mark.parametrize("seed", range(6))
def test_plan_properties(exe, seed):
    rng = random.Random(seed)
    lens = [rng.choice([0, 1, 6, 15, 16, 17, 100, 1000, 4096, 65_537]) + rng.randrange(3) for _ in range(rng.randrange(1, 60))]
    cap = rng.choice([1, 16, 17, 1000, 5000, 70_000, 1 << 20])
    rounds, offs = plan(exe, cap, lens)
    assert len(offs) == len(lens)
    nxt = 0
    for first, count, nbytes in rounds:
        assert first == nxt and count >= 1
        nxt = first + count
        end = 0
        for i in range(first, first + count):
            assert offs[i] % 16 == 0 and offs[i] >= end and offs[i] - end < 16   # packed, no overlap
            end = offs[i] + lens[i]
        assert offs[first] == 0 and nbytes == end
        assert count == 1 or nbytes <= cap
        if nxt < len(lens):   # maximal: the next page did not fit behind this round
            assert -(-end // 16) * 16 + lens[nxt] > cap
    assert nxt == len(lens)
