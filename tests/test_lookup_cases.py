"""The lookup corpus of tests/lookup_cases.py on the CPU: the C oracle against the pure-Python model on
all five hit columns for every case, and the conditions that keep the corpus from being vacuous (they
are statements about the oracle alone; densities and seeds in lookup_cases.py are chosen to meet them)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import lookup_cases as L


def oracle_hits(paths, ids, **kw):
    rc, hits = O.lookup([O.V2Block(p) for p in paths], ids, **kw)
    assert rc == 0
    return np.array(hits, dtype=np.int64).reshape(-1, 5)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("lookup_cases"))
    fam = L.slab_family(root)
    return dict(fam=fam, slab=L.slab_cases(fam), size=L.size_cases(fam), param=L.param_cases(root, fam),
                mixed=L.mixed_cases(root, fam), index=L.index_cases(root))


def test_model_hashes():
    """The model's hashes against the oracle's (themselves pinned to the reference's vectors)."""
    rng = np.random.default_rng(5)
    for n in (0, 1, 8, 15, 16, 17, 31, 33):
        b = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        assert L.murmur3_128(b) == O.murmur3_128(b)
        assert L.fnv1_32(b) == O.fnv1_32(b)


def check_nonvacuous(case, hits):
    nb, nids = len(case.paths), len(case.ids)
    share = len(hits) / float(nb * nids)
    assert 0.02 <= share <= 0.60, (case.name, share)
    per_block = [frozenset(hits[hits[:, 1] == b, 0].tolist()) for b in range(nb)]
    assert len(set(per_block)) == nb, case.name  # no two blocks answer alike: a swapped column shows
    if nb >= 8:  # the write pass copies up to kHitK = 4 kept hits and probes again above that
        cnt = np.bincount(hits[:, 0], minlength=nids)
        assert (cnt == 0).sum() >= 50 and ((cnt >= 1) & (cnt <= 4)).sum() >= 50 and (cnt > 4).sum() >= 50, \
            (case.name, (cnt == 0).sum(), ((cnt >= 1) & (cnt <= 4)).sum(), (cnt > 4).sum())


def test_slab_family(corpus):
    fam = corpus["fam"]
    model = L.model_lookup([L.ModelBlock(p) for p in fam.paths], fam.ids)  # (a block's hits do not depend on the others)
    for case in corpus["slab"]:
        hits = oracle_hits(case.paths, case.ids)
        np.testing.assert_array_equal(hits, model[model[:, 1] < len(case.paths)], err_msg=case.name)
        check_nonvacuous(case, hits)


def test_param_family(corpus):
    for case in corpus["param"]:
        hits = oracle_hits(case.paths, case.ids)
        np.testing.assert_array_equal(hits, L.model_lookup([L.ModelBlock(p) for p in case.paths], case.ids), err_msg=case.name)
        check_nonvacuous(case, hits)


def test_mixed_call(corpus):
    blocks = [L.ModelBlock(p) for p in corpus["mixed"][0].paths]
    for case in corpus["mixed"]:
        hits = oracle_hits(case.paths, case.ids, **case.kw)
        np.testing.assert_array_equal(hits, L.model_lookup(blocks, case.ids, **case.kw), err_msg=case.name)
        if case.kw:  # the window drops blocks at both ends: block_idx stays the caller's ordinal
            assert sorted(set(hits[:, 1].tolist())) == list(range(2, 9))
        else:
            assert sorted(set(hits[:, 1].tolist())) == list(range(11))
        cnt = np.bincount(hits[:, 0], minlength=len(case.ids))
        assert ((cnt >= 1) & (cnt <= 4)).sum() >= 50 and (cnt > 4).sum() >= 50, case.name


def test_call_sizes(corpus):
    for case in corpus["size"]:
        hits = oracle_hits(case.paths, case.ids)
        np.testing.assert_array_equal(hits, L.model_lookup([L.ModelBlock(p) for p in case.paths], case.ids), err_msg=case.name)
        if case.name in ("size/nohits", "size/noblocks"):
            assert len(hits) == 0
        elif len(case.ids) >= 63:
            assert len(hits) > 0, case.name
    assert [len(c.ids) for c in corpus["size"][:len(L.CALL_SIZES)]] == list(L.CALL_SIZES)


def test_index_family(corpus):
    """Oracle == model; and per directory block whose meta range reaches past its records the oracle
    returns record 0 for an id below every record, nothing for an id above every record, and a record
    that is not the id's own. (meta_own and meta_emptymax cannot: their range check rejects those ids,
    which is what they are there for, and is asserted instead.)"""
    directories = 0
    for case in corpus["index"]:
        blocks = [L.ModelBlock(p) for p in case.paths]
        hits = oracle_hits(case.paths, case.ids)
        np.testing.assert_array_equal(hits, L.model_lookup(blocks, case.ids), err_msg=case.name)
        if case.name == "index/all":
            assert len(set(hits[:, 1].tolist())) >= len(case.paths) - 1  # (all but meta_emptymax)
            continue
        recs = blocks[0].rec_ids
        ids = [r.tobytes() for r in case.ids]
        rec_of = dict(zip(hits[:, 0].tolist(), hits[:, 2].tolist()))
        below = [i for i, x in enumerate(ids) if x < recs[0]]
        above = [i for i, x in enumerate(ids) if x > recs[-1]]
        assert below and above, case.name
        assert all(i not in rec_of for i in above), case.name
        if case.name == "index/meta_emptymax":
            assert len(hits) == 0
            continue
        if case.name == "index/meta_own":
            assert all(i not in rec_of for i in below)
            continue
        if L.dir_shape(recs):
            directories += 1
            assert any(rec_of.get(i) == 0 for i in below), case.name
            assert any(i in rec_of and recs[rec_of[i]] != ids[i] for i in range(len(ids))), case.name
            cp = L.dir_shape(recs)[0]
            if cp:  # the prefix branches: ids off the prefix, below and above, in the meta range
                lo = [i for i in below if ids[i][:cp] != recs[0][:cp] and rec_of.get(i) == 0]
                hi = [i for i in above if ids[i][:cp] != recs[0][:cp]]
                assert lo and hi, case.name
                if cp > 8:  # ... in the low half too
                    assert any(ids[i][:8] == recs[0][:8] for i in lo) and any(ids[i][:8] == recs[0][:8] for i in hi), case.name
    assert directories >= 12
