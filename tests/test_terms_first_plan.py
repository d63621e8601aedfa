"""The terms-first choice on the host (tempo_amd/csrc/terms_first.hpp), through
tests/terms_first_check.cpp, which includes the header the loader (block.cpp count_narrow_sets) and
the planner (pool.hip terms_first_choice) use:

* the per-set counts of a column equal numpy.bincount of it, the absent key's all-ones id and ids
  past the set count left out;
* the launch's p is the product of the terms' counted shares per block, weighted over the blocks by
  the entries each contributes, for hand-computed cases; the share of 256-entry steps holding a
  pass is 1 - (1 - p)^256;
* the choice: p one step either side of the threshold share, forced off and forced on whatever p
  is, and a launch with a block that has no counts (auto: off).

The GPU side of the choice (which instance ran) is tests/test_gpu_terms_first.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABSENT = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tf") / "terms_first_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tempo_amd", "csrc"),
                           os.path.join(ROOT, "tests", "terms_first_check.cpp"), "-o", out])
    return out


def bitmap(sets):
    w = [0] * 8
    for s in sets:
        w[s >> 5] |= 1 << (s & 31)
    return w


def plan(exe, mode, blocks):
    """blocks: (entries, scanned, [(counts or None, sets in the term's bitmap), ...])"""
    lines = []
    for entries, scanned, terms in blocks:
        f = [entries, scanned, len(terms)]
        for counts, sets in terms:
            f += [len(counts or [])] + list(counts or []) + bitmap(sets)
        lines.append(" ".join(str(x) for x in f))
    res = subprocess.run([exe, "plan", str(mode)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    p, share, pick, thr = res.stdout.split()
    return float(p), float(share), int(pick), float(thr)


@pytest.mark.parametrize("nsets", [1, 7, 254])
def test_counts_equal_bincount(exe, nsets):
    rng = np.random.default_rng(nsets)
    col = rng.integers(0, nsets, size=3000, dtype=np.uint32)
    col[rng.random(3000) < 0.1] = ABSENT       # key absent
    col[5] = nsets                             # (an id past the sets: never written by a loader, never counted)
    res = subprocess.run([exe, "count", str(nsets)] + [str(int(v)) for v in col], capture_output=True, text=True, check=True)
    got = np.array(res.stdout.split(), dtype=np.int64)
    assert (got == np.bincount(col[col < nsets], minlength=nsets)).all()


def test_estimate(exe):
    # one block: 1000 entries, term 0 passes sets {1, 3} = 20 + 30 entries, term 1 set {0} = 500
    b0 = (1000, 1000, [([100, 20, 850, 30], {1, 3}), ([500, 500], {0})])
    p, share, _, _ = plan(exe, 2, [b0])
    assert p == pytest.approx(0.05 * 0.5, rel=1e-12)
    assert share == pytest.approx(1 - (1 - 0.025) ** 256, rel=1e-12)
    # a second block, half of it scanned (a limit query's part): weights 1000 and 2000
    b1 = (4000, 2000, [([4000], {0}), ([3996, 4], {1})])
    p, _, _, _ = plan(exe, 2, [b0, b1])
    assert p == pytest.approx((0.025 * 1000 + 0.001 * 2000) / 3000, rel=1e-12)
    # a set outside the bitmap's counts, an empty bitmap
    assert plan(exe, 2, [(10, 10, [([5, 5], set())])])[:3] == (0.0, 0.0, 1)
    assert plan(exe, 2, [(10, 10, [([5, 5], {0, 1, 200})])])[0] == 1.0


def test_choice_both_sides_of_the_threshold(exe):
    thr = plan(exe, 2, [(10, 10, [([10], {0})])])[3]
    assert 0.0 < thr < 1.0
    n = 10_000_000
    p_thr = 1 - (1 - thr) ** (1 / 256)
    for k, want in ((int(p_thr * n * 0.98), 1), (int(p_thr * n * 1.02) + 1, 0)):
        blk = (n, n, [([n - k, k], {1})])
        p, share, pick, _ = plan(exe, 2, [blk])
        assert p == pytest.approx(k / n) and (share < thr) == bool(want) and pick == want
        assert plan(exe, 0, [blk])[2] == 0 and plan(exe, 1, [blk])[2] == 1
    # the issue's five conjunctions on the bench's blocks land where their shares say
    for p in (2e-2, 6e-3, 2.5e-3, 1e-3, 1.25e-4):
        k = round(p * n)
        share = 1 - (1 - k / n) ** 256
        assert plan(exe, 2, [(n, n, [([n - k, k], {1})])])[2] == int(share < thr)


def test_block_without_counts_votes_off(exe):
    sparse = (3000, 3000, [([2999, 1], {1})])
    assert plan(exe, 2, [sparse])[2] == 1
    bare = (500, 500, [(None, {1})])
    p, _, pick, _ = plan(exe, 2, [sparse, bare])
    assert p < 0 and pick == 0
    assert plan(exe, 1, [sparse, bare])[2] == 1 and plan(exe, 0, [sparse, bare])[2] == 0
    # a block nothing of which is scanned does not vote
    assert plan(exe, 2, [sparse, (500, 0, [(None, {1})])])[2] == 1
