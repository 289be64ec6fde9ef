"""ASan + UBSan CPU build of the socket table (csrc/gcl_sock.c with the probe
of csrc/gcl_sock.h that the GPU kernel shares), driven by the stand-alone
program tests/fuzz/sock_fuzz.c: random entry sets, invalid ones among them,
frames of every length in [0, 80] and verdict bytes of every width in heap
blocks of exactly their size, every answer compared with a linear search.
The program is run on its own; nothing is loaded into Python.  Any sanitizer
report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def sock_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_sock(str(tmp_path_factory.mktemp("san_sock")))


@pytest.mark.parametrize("seed", [1, 2])
def test_sock_table_random_sets_frames_and_verdicts(sock_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sock_exe, str(seed), "400"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["sock", "ok"], r.stdout
    # HIT5, HIT3, HIT3_ANY, MULTI, MISS and NA all seen; sets refused; placements refused by the knob
    assert all(int(x) > 0 for x in out[2:10]), r.stdout
