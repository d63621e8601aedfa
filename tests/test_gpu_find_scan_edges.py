"""findOne's object scan and gather (find_scan_kernel, find_gather_kernel; tempo_amd/csrc/find.hip steps
4 and 5) on the constructed pages of tests/find_scan_cases.py. Every find call's (id_idx, block_idx,
status, object) list equals the Python model's for the lookup's hits, in the lookup's order; the
model is held to the oracle, and the cases to their aim, in tests/test_find_scan_cases.py.

  family       what it pins
  windows      an object 0..24 bytes before the end of the first and of the second 64 KiB LDS window, the
               wanted id at it and behind it: the slides at next >= wl (0), at a header astride the end
               (1..7), at an id astride it (8..23), none (24); objects longer than one and two windows;
               a pending id that equals a straddling object's id only in the bytes inside the window
  tails        0..9 bytes behind the last object, in the open and alone in a second window: the clean
               ends at 0, 4 and 8 (whatever the 8 bytes hold), the errors at the rest; an empty page
  malformed    total 0, 7, R + 1, R, 2^32 - 1; an id length past the object; id lengths 0, 15, 17, 32
               around a pending id's bytes; empty objects: the id before the damage is found, the ids
               behind it get the page's error, or are found where the walk goes on
  duplicates   an id twice in a page (the first wins), twice in a call, in two blocks
  pending      1 .. 513 ids of one page: one, two and three passes of 256, lanes with 1..4 ids; every 7th
               absent; an error behind every found id, and an error for the absent ids of a three-pass page
               (which pass an id falls into is the host's grouping order, not the page's to choose)
  gather       objects of 0, 1, 255, 256, 257 and 70 000 bytes behind each other in the result, with a
               not-found and a corrupt hit between them
  snappy       windows and tails through find_decode_kernel (stored chunks of <= 64 KiB): the scan reads
               what the decoder wrote, at arena offsets other than 0
  mixed        every block in one call, the ids shuffled: pages of several blocks in one launch"""
import os
import random

import pytest

import tempo_amd as T
from tests import find_scan_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("find_scan"))
    fams = {f.name: f for f in S.all_families()}
    paths = {}

    def path(fam, enc=T.ENC_NONE):
        """The family's blocks at that encoding, written on first use."""
        if (fam, enc) not in paths:
            paths[fam, enc] = [S.write_block(os.path.join(root, "%s%d_%d" % (fam, k, enc)), cases, enc)
                               for k, cases in enumerate(fams[fam].blocks)]
        return paths[fam, enc]
    return fams, path


def check(engine, paths, blocks, ask):
    handles = [engine.open_v2block(p) for p in paths]
    try:
        got, _ = engine.find(handles, S.as_ids(ask))
        lk, _ = engine.lookup(handles, S.as_ids(ask))
    finally:
        for h in handles:
            h.close()
    hits = [(int(r[0]), int(r[1])) for r in lk]
    assert [(g[0], g[1]) for g in got] == hits  # one entry per lookup hit, in the lookup's order
    # every pending id reaches its own page
    own = {(i, b) for i, tid in enumerate(ask) for b, cases in enumerate(blocks) if any(tid in c.pending for c in cases)}
    assert own <= set(hits) and len(own) >= len(ask)
    want = S.expected(blocks, ask, hits)
    bad = [(S.page_of(blocks[w[1]], ask[w[0]]).name, ask[w[0]].hex(), g[2], w[2]) for g, w in zip(got, want) if g != w]
    assert not bad, bad[:8]
    return got


@pytest.mark.parametrize("fam", ["windows", "tails", "malformed", "duplicates", "pending", "gather"])
def test_family(engine, corpus, fam):
    fams, path = corpus
    f = fams[fam]
    got = check(engine, path(fam), f.blocks, f.ask)
    assert {g[2] for g in got} >= ({T.TSG_OK} if fam == "duplicates" else {T.TSG_OK, T.TSG_E_NOT_FOUND})


@pytest.mark.parametrize("fam", ["windows", "tails"])
def test_family_through_snappy_decode(engine, corpus, fam):
    fams, path = corpus
    f = fams[fam]
    check(engine, path(fam, T.ENC_SNAPPY), f.blocks, f.ask)


def test_mixed_call(engine, corpus):
    fams, path = corpus
    blocks, paths, ask = [], [], []
    for name, f in fams.items():
        blocks += f.blocks
        paths += path(name)
        ask += f.ask
    random.Random(5).shuffle(ask)
    got = check(engine, paths, blocks, ask)
    assert {g[1] for g in got} == set(range(len(blocks)))
