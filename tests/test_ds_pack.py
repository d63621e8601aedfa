"""The narrow kernels' packed scan word (tempo_amd/csrc/ds_word.hpp: duration code | carry |
block-relative start second in one uint32) on the host: tests/ds_pack_check.cpp includes the
header the packer (devctx.hip) and the kernels (pool_kernels.hpp) share, and checks

* the multiply-shift that replaces / 1000, for every q in 0..32767;
* decoded start / end seconds == uint32(start / 1e9) / uint32(end / 1e9) whenever neither escape
  is flagged; the end escape exactly when the duration code is saturated, the start escape
  exactly when start_s - base is outside [0, 0x7ffe];

over sub-second parts and durations either side of whole seconds, whole ms +- 1 ns up to and
past the code's 32767 ms, end = 0 and end = start - 1, starts at base - 1, base, base + 0x7ffe,
base + 0x7fff and base + 100000, base = 0, starts near 2^32 - 1 s, and 400 000 seeded random
entries. The same word is checked against the oracle on the GPU in tests/test_gpu_ds_start.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ds_word_pack_and_decode(tmp_path):
    exe = str(tmp_path / "ds_pack_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tempo_amd", "csrc"),
                           os.path.join(ROOT, "tests", "ds_pack_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-2000:]
    last = res.stdout.strip().splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 400000
