"""ASan + UBSan CPU build of the post-pass over a list's packed records
(gcl_host_deliver_packed, csrc/gcl_host.c), driven by the stand-alone program
tests/fuzz/pack_fuzz.c: random records with garbage verdict bytes, index
lists with entries at or above n, rings that fill, NULL optional pointers.
The program is run on its own; nothing is loaded into Python.  Any sanitizer
report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def pack_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_pack(str(tmp_path_factory.mktemp("san_pack")))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_deliver_packed_random_records(pack_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([pack_exe, str(seed), "400"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["pack", "ok"], r.stdout
    # packets delivered, callbacks made, entries outside the batch skipped
    assert int(out[2]) > 0 and int(out[3]) > 0 and int(out[4]) > 0, r.stdout
