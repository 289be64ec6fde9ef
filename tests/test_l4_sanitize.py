"""ASan + UBSan CPU build of the TCP/UDP checksum verify and fill on the CPU
(gcl_l4_csum_host, csrc/gcl_host.c), driven by the stand-alone program
tests/fuzz/l4_fuzz.c: batches with hostile offsets, pkt_len and tot over heap
regions of exactly frames_len bytes, so that any read or write out of bounds
traps.  The program is run on its own; nothing is loaded into Python.  Any
sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def l4_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_l4(str(tmp_path_factory.mktemp("san_l4")))


@pytest.mark.parametrize("seed", [1, 2])
def test_l4_host_hostile_batches(l4_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([l4_exe, str(seed), "3000"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["l4", "ok"], r.stdout
    # packets GOOD after a fill, BAD, NA, and filled
    assert all(int(x) > 1000 for x in out[2:6]), r.stdout
