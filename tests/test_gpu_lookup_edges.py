"""The lookup kernels against the oracle at the shapes that select their paths (the corpus of
tests/lookup_cases.py; tests/test_lookup_cases.py holds the oracle itself to a Python model of it).
Every comparison is assert_array_equal on all five hit columns, in the oracle's (id, block) order.

  case                              path it pins (tempo_amd/csrc/lookup.hip)
  slab/J1                           a lone block: the per-block direct probe (d_probe)
  slab/J2, J31, J32                 slab probe W = 1; J % 32 tail mask of the last column; a full column
  slab/J33, J63, J64                W = 2 (uint2 loads)
  slab/J65, J128                    W = 4 (uint4)
  slab/J129, J255, J256             W = 8 (two uint4); 256 = a full slab
  slab/J257                         a group split after 256 members: slab + one direct block
  slab/* (m = bitlen = 1000)        the transposes' partial last word (nq = 40 < 64); distinct blooms and
                                    records per member: a swapped member column changes the hits
  param/m37k1, m1k3                 d_mod for tiny m, m = 1; k = 1; a 1-bit table
  param/m64k2s3, m1024k8s2          several shards, even k, power-of-two m
  param/m1000b900k7                 loc >= bitlen rejects (slab and direct)
  param/m4099k13legacy              bloomShards absent: 10 shards; odd k > 8
  param/writer1shard, 3shards       the default writer's m = 819200, k = 7
  param/* under TSG_LK_SLAB=1 / 0   each parameter set through the slab (J = 2) and through d_probe
  mixed/slab=None, 1, 0             several slabs and direct blocks interleaved in block order: the write
                                    pass's insertion sorts (<= 4 kept hits, > 4 re-probed) across sources;
                                    =1 makes the singleton a slab of J = 1
  mixed/window/*                    a time window drops members of a slab: block_idx stays the caller's
  index/n1 .. n63                   plain binary search (no directory below 64 records)
  index/n64, n65, n600, cp*         the directory: bucket bounds, empty buckets, the record after an absent
                                    id, past the last record; prefix of 0 / 1 / 7 / 8 / 9 / 12 bytes: the
                                    below / above branches of the prefix test in the high and the low half
  index/cp15                        dir_cp capped at 12, every record in one bucket
  index/onebucket                   64 buckets, all but two records in one
  index/meta_*, cp12_min8           min / max ids of 16, 8, 1 and 0 bytes in the range check
  index/all                         the same blocks as one slab (d_post behind the slab probe)
  size/n1 .. n33281                 calls of 1, 63 .. 257 ids (wave and tile edges) and of 131 tiles (the
                                    look-back walks past one 64-tile window); no hits at all; no blocks
  test_pass_switches                TSG_LK_PAIR=1 (odd and even k), TSG_LK_OCC=8 / 17, TSG_LK_DIR=0,
                                    TSG_LK_TR=1 (bit-at-a-time transpose) with forced slabs, id-major hits
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lookup_cases as L
from tests.test_lookup_cases import oracle_hits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("lookup_edges"))
    fam = L.slab_family(root)
    return dict(root=root, slab=L.slab_cases(fam), size=L.size_cases(fam), param=L.param_cases(root, fam),
                mixed=L.mixed_cases(root, fam), index=L.index_cases(root), expected={})


def expected(corpus, case):
    """The oracle's hits of a case, computed once (the slab setting does not change them)."""
    key = case.name.split("/slab=")[0]
    if key not in corpus["expected"]:
        corpus["expected"][key] = oracle_hits(case.paths, case.ids, **case.kw)
    return corpus["expected"][key]


def run_cases(engine, monkeypatch, corpus, cases, find=False):
    paths = sorted({p for c in cases for p in c.paths})
    blocks = {}
    try:
        for p in paths:
            blocks[p] = engine.open_v2block(p)
        for c in cases:
            if c.slab is None:
                monkeypatch.delenv("TSG_LK_SLAB", raising=False)
            else:
                monkeypatch.setenv("TSG_LK_SLAB", c.slab)
            kw = dict(time_start=c.kw.get("ts", 0), time_end=c.kw.get("te", 0))
            got, _ = engine.lookup([blocks[p] for p in c.paths], c.ids, **kw)
            np.testing.assert_array_equal(got, expected(corpus, c), err_msg=c.name)
            if find:
                fgot, _ = engine.find([blocks[p] for p in c.paths], c.ids, **kw)
                assert [(g[0], g[1]) for g in fgot] == [(int(r[0]), int(r[1])) for r in got], c.name
    finally:
        for b in blocks.values():
            b.close()


def test_slab_family(engine, monkeypatch, corpus):
    run_cases(engine, monkeypatch, corpus, corpus["slab"])
    forced = [c._replace(name=c.name + "/slab=1", slab="1") for c in corpus["slab"] if len(c.paths) in (1, 257)]
    run_cases(engine, monkeypatch, corpus, forced)  # (J = 1 as a slab; the 257th member as a slab of its own)


def test_param_family(engine, monkeypatch, corpus):
    cases = [c._replace(name="%s/slab=%s" % (c.name, s), slab=s) for c in corpus["param"] for s in (None, "1", "0")]
    run_cases(engine, monkeypatch, corpus, cases)


def test_mixed_call(engine, monkeypatch, corpus):
    run_cases(engine, monkeypatch, corpus, corpus["mixed"])


def test_index_family(engine, monkeypatch, corpus):
    run_cases(engine, monkeypatch, corpus, corpus["index"], find=True)


def test_call_sizes(engine, monkeypatch, corpus):
    run_cases(engine, monkeypatch, corpus, corpus["size"])


_CHILD = r"""
import json
import os
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import tempo_amd as T
plan = json.load(open(sys.argv[2]))
ids = np.load(sys.argv[3])
base = os.environ.get("TSG_LK_SLAB")
eng = T.Engine(devices=[0])
blocks, out = {}, {}
try:
    for c in plan:
        for p in c["paths"]:
            if p not in blocks:
                blocks[p] = eng.open_v2block(p)
        slab = c["slab"] if c["slab"] is not None else base
        if slab is None:
            os.environ.pop("TSG_LK_SLAB", None)
        else:
            os.environ["TSG_LK_SLAB"] = slab
        key = c["name"].replace("/", "__")
        out[key], _ = eng.lookup([blocks[p] for p in c["paths"]], ids[key])
finally:
    for b in blocks.values():
        b.close()
    eng.close()
np.savez(sys.argv[4], **out)
"""

SWITCHES = [{"TSG_LK_PAIR": "1"}, {"TSG_LK_OCC": "8"}, {"TSG_LK_OCC": "17"}, {"TSG_LK_DIR": "0"},
            {"TSG_LK_TR": "1", "TSG_LK_SLAB": "1"}, {"TSG_LK_SLOTMAJOR": "0"}]


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_pass_switches(corpus, env):
    """The switches the library reads once per process, each in a fresh child (one at a time): the slab
    cases J = 33 / 129 / 257, the parameter family (odd and even k) and the index family return the
    oracle's hits under every one of them."""
    cases = ([c for c in corpus["slab"] if len(c.paths) in (33, 129, 257)] + corpus["param"] + corpus["index"])
    tag = "_".join("%s%s" % kv for kv in env.items())
    plan, idp, outp = (os.path.join(corpus["root"], "%s_%s" % (tag, n)) for n in ("plan.json", "ids.npz", "got.npz"))
    with open(plan, "w") as f:
        json.dump([dict(name=c.name, paths=c.paths, slab=c.slab) for c in cases], f)
    np.savez(idp, **{c.name.replace("/", "__"): c.ids for c in cases})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ)
    e.pop("TSG_LK_SLAB", None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD, root, plan, idp, outp], env=e, timeout=120, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(outp)
    for c in cases:
        np.testing.assert_array_equal(got[c.name.replace("/", "__")], expected(corpus, c), err_msg="%s under %s" % (c.name, env))
