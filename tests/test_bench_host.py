"""Host-side helpers of bench.py (no GPU): CPU placement picks whole cores."""
import os

import bench


def _core(c):
    try:
        return open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
    except OSError:
        return str(c)


def test_idlest_picks_distinct_cores():
    cpus = sorted(os.sched_getaffinity(0))
    k = min(4, len(cpus))
    got = bench.idlest(cpus, k, window=0.05)
    assert len(got) == k and len(set(got)) == k and set(got) <= set(cpus)
    ncores = len({_core(c) for c in cpus})
    if ncores >= k:  # one CPU per core whenever there are enough cores
        assert len({_core(c) for c in got}) == k


def test_idlest_fills_when_cores_are_few():
    cpus = sorted(os.sched_getaffinity(0))[:2]
    got = bench.idlest(cpus, 2, window=0.01)
    assert sorted(got) == sorted(cpus)


def _args(*argv):
    import sys
    old = sys.argv
    sys.argv = ["bench.py", *argv]
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_rank_env_from_torchrun():
    """Under torchrun the environment names the rank; --gpus must agree with the world."""
    a = _args("--gpus", "4")
    assert bench.rank_env(a, {"WORLD_SIZE": "4", "RANK": "2", "LOCAL_RANK": "2"}) == (2, 4, 2)
    assert bench.rank_env(_args(), {"WORLD_SIZE": "8", "RANK": "7", "LOCAL_RANK": "7"}) == (7, 8, 7)
    import pytest
    with pytest.raises(SystemExit):
        bench.rank_env(a, {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})


def test_rank_env_single_and_launcher():
    assert bench.rank_env(_args(), {}) == (0, 1, 0)
    assert bench.rank_env(_args("--gpus", "1"), {}) == (0, 1, 0)
    assert bench.rank_env(_args("--gpus", "2"), {}) is None  # this process starts the ranks


def test_launch_fails_without_enough_gpus(capsys):
    """`bench.py --gpus 2` on a box with fewer GPUs exits non-zero with a clear message,
    before anything is started."""
    rc = bench.launch_ranks(_args("--gpus", "2"), ["--gpus", "2"], device_count=1)
    assert rc == 2
    assert "needs 2 visible GPUs, found 1" in capsys.readouterr().err


def test_launch_cmd_is_torchrun_on_loopback():
    cmd = bench.launch_cmd(["--gpus", "8", "--steps", "20"], 8, 29511)
    i = cmd.index("torch.distributed.run")
    assert cmd[i - 1] == "-m" and "--nproc-per-node=8" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and "--master-port=29511" in cmd
    assert cmd[-5:] == [os.path.abspath(bench.__file__), "--gpus", "8", "--steps", "20"]


def test_launch_runs_ranks_with_rank_environment(tmp_path):
    """The launcher's children see torchrun's rank environment (gloo world of 2 on the CPU:
    a stand-in script that reports what bench.rank_env reads)."""
    import subprocess
    import sys
    script = tmp_path / "probe.py"
    script.write_text(
        "import os, sys\n"
        f"sys.path.insert(0, {os.path.dirname(os.path.abspath(bench.__file__))!r})\n"
        "import bench\n"
        "a = bench.parse()\n"
        "r = bench.rank_env(a)\n"
        f"open(os.path.join({str(tmp_path)!r}, 'rank%d' % r[0]), 'w').write('%d %d %d' % r)\n")
    cmd = bench.launch_cmd(["--gpus", "2"], 2, bench.free_port())
    cmd[cmd.index(os.path.abspath(bench.__file__))] = str(script)
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    assert subprocess.call(cmd, env=env, timeout=120) == 0
    got = sorted((tmp_path / f).read_text() for f in ("rank0", "rank1"))
    assert got == ["0 2 0", "1 2 1"]


def test_plain_run_is_the_main_line_only():
    """Without --full every leg beside the main line is off, whatever its own option says;
    with --full the legs' options stand as given."""
    a = bench.main_line_only(_args("--gpus", "1", "--steps", "7", "--warmup", "2", "--cfg4", "1", "--shim-steps", "9"))
    assert all(getattr(a, k) == 0 for k in bench.FULL_ONLY)
    assert (a.steps, a.warmup, a.sets, a.events, a.dump_outputs) == (7, 2, 4, 4, None)
    f = bench.main_line_only(_args("--full", "--shim-steps", "9"))
    assert (f.shim_steps, f.mall_steps, f.cfg3, f.cfg4, f.cfg5, f.parity, f.cpu_baseline) == (9, 100, None, None, 1, 1, 1)


def _result(n, rng):
    """A tsg_result over numpy columns (kept alive beside it)."""
    import ctypes as C

    import numpy as np
    from tempo_amd import tsg
    names = [b"svc-07", b"GET /carts", b"", b"svc-01"]
    arena = b"".join(names)
    offs = np.cumsum([0] + [len(s) for s in names[:-1]]).astype(np.uint64)
    lens = np.array([len(s) for s in names], np.uint32)
    pick_s, pick_n = rng.integers(0, len(names), n), rng.integers(0, len(names), n)
    cols = dict(trace_id=rng.integers(0, 256, (n, 16), dtype=np.uint8), trace_id_len=np.full(n, 16, np.uint8),
                start_ns=rng.integers(2**60, 2**61, n, dtype=np.uint64), end_ns=rng.integers(2**60, 2**61, n, dtype=np.uint64),
                duration_ms=rng.integers(0, 2**32, n, dtype=np.uint32), block_idx=rng.integers(0, 10, n, dtype=np.uint32),
                entry_idx=np.sort(rng.integers(0, 2**40, n, dtype=np.uint64)),
                root_service_off=offs[pick_s], root_service_len=lens[pick_s],
                root_name_off=offs[pick_n], root_name_len=lens[pick_n])
    r = tsg._Result()
    r.n = n
    for k, v in cols.items():
        cols[k] = v = np.ascontiguousarray(v)
        setattr(r, k, v.ctypes.data_as(type(getattr(r, k))))
    buf = C.create_string_buffer(arena, len(arena))
    r.names, r.names_len = C.cast(buf, C.c_void_p), len(arena)
    r.metrics.traces_inspected, r.metrics.bytes_inspected, r.metrics.scan_bytes = 12345, 2**40 + 1, 2**33 + 3
    want = dict(cols, root_service=[names[i] for i in pick_s], root_name=[names[i] for i in pick_n])
    return r, want, buf


def test_result_arrays_hold_every_value_exactly(tmp_path):
    """--dump-outputs: float arrays from which every integer of the result reads back
    exactly (u64 nanoseconds split into seconds + the rest), names resolved."""
    import numpy as np
    r, want, _keep = _result(300, np.random.default_rng(3))
    out = bench.result_arrays(r)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    u = lambda a: a.astype(np.uint64)  # noqa: E731
    assert (out["row"] == np.arange(300)).all()
    assert (out["trace_id"].astype(np.uint8) == want["trace_id"]).all()
    for k in ("start", "end"):
        assert (u(out[k + "_s"]) * np.uint64(10**9) + u(out[k + "_subsec_ns"]) == want[k + "_ns"]).all()
    for k in ("trace_id_len", "duration_ms", "block_idx", "entry_idx"):
        assert (u(out[k]) == want[k]).all()
    names = bytes(out["names"].astype(np.uint8)).split(b"\0")
    assert names == sorted(set(names))
    for k in ("root_service", "root_name"):
        assert [names[int(i)] for i in out[k]] == want[k]
    assert out["metrics"].tolist() == [300, 12345, 0, 0, 2**40 + 1, 2**33 + 3]
    bench.dump_outputs(str(tmp_path / "d"), out, 0)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == sorted(k + ".npy" for k in out)
    assert (np.load(tmp_path / "d" / "entry_idx.npy") == out["entry_idx"]).all()


def test_result_arrays_sample_a_large_result_and_take_an_empty_one():
    """More rows than the byte cap holds: the same seeded rows every time, in order, within
    the cap; an empty result gives empty columns."""
    import numpy as np
    r, want, _keep = _result(5000, np.random.default_rng(4))
    cap = 2**21 + 1000 * 152
    a, b = bench.result_arrays(r, cap=cap), bench.result_arrays(r, cap=cap)
    rows = a["row"].astype(np.int64)
    assert len(rows) == 1000 and (np.diff(rows) > 0).all() and all((a[k] == b[k]).all() for k in a)
    assert (a["entry_idx"].astype(np.uint64) == want["entry_idx"][rows]).all()
    assert sum(x.nbytes for x in a.values()) <= cap
    r0, _, _keep0 = _result(0, np.random.default_rng(5))
    e = bench.result_arrays(r0)
    assert e["trace_id"].shape == (0, 16) and len(e["root_name"]) == 0 and e["metrics"][0] == 0
