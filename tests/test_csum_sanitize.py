"""ASan + UBSan CPU build of the checksum rule for one frame
(gcl_rx_csum_flags, csrc/gcl_host.c), driven by the stand-alone program
tests/fuzz/csum_fuzz.c: random frames of every length in [0, 80] in heap
blocks of exactly that size, compared with the rule written out over a
zero-padded copy.  The program is run on its own; nothing is loaded into
Python.  Any sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def csum_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_csum(str(tmp_path_factory.mktemp("san_csum")))


@pytest.mark.parametrize("seed", [1, 2])
def test_csum_flags_random_frames(csum_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([csum_exe, str(seed), "300"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["csum", "ok"], r.stdout
    # frames marked GOOD, marked BAD, and left as they were
    assert int(out[2]) > 0 and int(out[3]) > 0 and int(out[4]) > 0, r.stdout
