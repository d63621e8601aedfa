"""The narrow kernels' short predicate forms (tempo_amd/csrc/ds_word.hpp) on the host:
tests/scan_pred_check.cpp includes the header the kernels (pool_kernels.hpp unit_mask) use and
checks each form against the header's own decode-and-compare, which stays the definition:

* duration as one unsigned compare: every D16, every (lo, hi) from {0, 1, 2, 19, 20, 21, 1999,
  2000, 2001, 65534, 65535, 2^32 - 1}, lo > hi included;
* the time range on the packed word: every D16 x carry, rel in {0, 1, 16383, 0x7ffd, 0x7ffe,
  0x7fff}, base in {0, 1, 16383, 1 700 000 000, 2^32 - 0x8000, 2^32 - 0x7fff, 2^32 - 1}, query
  start and end at 0, at each decoded start and end second and one either side, and at 2^32 - 1,
  escaped words falling back to exact columns and late bases to the decode;
* the term table: every x, ns in {0, 1, 2, 31, 32, 33, 254, 255}, the all-zero, all-one,
  single-bit (0, 31, 32, 255) and seeded random bitmaps;
* the validity mask: every n - e0 in 0..520, every lane and step;
* floor(q / 1000) by the 24-bit multiply, every q <= 32767.

The same forms are checked against the oracle on the GPU in tests/test_gpu_scan_pred.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_short_forms_equal_the_decode(tmp_path):
    exe = str(tmp_path / "scan_pred_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tempo_amd", "csrc"),
                           os.path.join(ROOT, "tests", "scan_pred_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 1000000
