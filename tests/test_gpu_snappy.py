"""The device snappy decoder (find_decode_kernel) on the hand-built frames of
tests/snappy_frames.py, one frame per page: every tag form, chunk type and boundary of ACCEPTED
comes back byte-exact through findOne, and every damage of REJECTED reports TSG_E_CORRUPT for its
page's hit while the intact pages between them are untouched. The oracle's verdict on the same
frames: tests/test_snappy_frames.py."""
import os

import pytest

import tempo_amd as T
from tests import snappy_frames as F
from tests.test_gpu_lz4 import check_pages, seq_ids

pytestmark = pytest.mark.gpu


def write_pages(path, cases):
    """Page k = cases[k] built for id k; returns the objects the pages hold."""
    ids = seq_ids(len(cases))
    built = [c.build(bytes(ids[k])) for k, c in enumerate(cases)]
    assert all(bytes(ids[k]) == F.frame_id(k) for k in range(len(cases)))
    objs = [page[F.HDR:] for _, page in built]
    T.write_v2_block_pages(path, ids, objs, list(range(len(cases))), [payload for payload, _ in built], T.ENC_SNAPPY)
    return objs


def test_decoder_edges(engine, tmp_path):
    path = os.path.join(str(tmp_path), "a")
    objs = write_pages(path, F.ACCEPTED)
    check_pages(engine, path, objs)


def test_damaged_pages(engine, tmp_path):
    cases = []
    for c in F.REJECTED:  # intact, damaged, intact, damaged, ..., intact
        cases += [F.INTACT, c]
    cases.append(F.INTACT)
    path = os.path.join(str(tmp_path), "r")
    objs = write_pages(path, cases)
    check_pages(engine, path, objs, bad=set(range(1, len(cases), 2)))
