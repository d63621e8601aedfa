"""The host half of tsg_wal_block_refresh, without a GPU: the tail replay and the refresh plan
(tempo_amd/csrc/block.cpp) in a stand-alone program under AddressSanitizer + UBSan
(tests/sanitize/san_wal_refresh.cpp: hand-built files grown in stages, the plan applied as the
merge kernel applies it and compared with a fresh decode; the prefix-changed and shorter-file
checks; a damaged appended page), and the new ABI pieces against the compiled header."""
import ctypes as C
import os
import subprocess

import pytest

import tempo_amd as T
from tempo_amd import tsg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"
CSRC = os.path.join(ROOT, "tempo_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang++ with the sanitizer runtimes")
def test_plan_and_tail_replay_under_asan(tmp_path):
    exe = str(tmp_path / "san_wal_refresh")
    srcs = [os.path.join(ROOT, "tests", "sanitize", "san_wal_refresh.cpp")] + \
        [os.path.join(CSRC, f) for f in ("block.cpp", "common.cpp", "writer.cpp", "zstd_host.cpp")]
    subprocess.check_call([CLANG, "-O1", "-g", "-fno-omit-frame-pointer", "-std=c++17", "-pthread",
                           "-I", os.path.join(ROOT, "include"), "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined"] + srcs + ["-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-6000:]
    for bad in ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "FAIL"):
        assert bad not in p.stdout, p.stdout[-6000:]
    assert "san_wal_refresh: ok" in p.stdout


def test_refresh_entry_points_and_stats_layout(tmp_path):
    L = T.lib()
    assert hasattr(L, "tsg_wal_block_refresh") and hasattr(L, "tsg_wal_block_refresh_mem")
    assert L.tsg_abi_version() == 7
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tsg.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   ' sizeof(tsg_wal_refresh_stats), offsetof(tsg_wal_refresh_stats, upload_bytes),'
                   ' offsetof(tsg_wal_refresh_stats, kernel_ns), offsetof(tsg_wal_refresh_stats, mode));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = tsg._WalRefreshStats
    assert got == [C.sizeof(S), S.upload_bytes.offset, S.kernel_ns.offset, S.mode.offset]


def test_refresh_rejects_null_arguments():
    st = tsg._WalRefreshStats()
    out = C.c_void_p()
    assert T.lib().tsg_wal_block_refresh(None, None, b"x", C.byref(out), C.byref(st)) == tsg.TSG_E_INVALID
    assert T.lib().tsg_wal_block_refresh_mem(None, None, None, 0, C.byref(out), C.byref(st)) == tsg.TSG_E_INVALID
