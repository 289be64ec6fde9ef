"""ASan + UBSan CPU build of the loopback frame copy on the host
(gcl_copy_batch_host, csrc/gcl_host.c), driven by the stand-alone program
tests/fuzz/copy_fuzz.c: random batches whose source, destination and
per-packet arrays live in heap blocks of exactly their size, with offsets and
lengths near 0, src_len, dst_len, 2^63 and UINT64_MAX, compared with the rule
written out byte by byte.  The program is run on its own; nothing is loaded
into Python.  Any sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def copy_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_copy(str(tmp_path_factory.mktemp("san_copy")))


@pytest.mark.parametrize("seed", [1, 2])
def test_copy_batch_host_random_batches(copy_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([copy_exe, str(seed), "20000"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["copy", "ok"], r.stdout
    # packets copied, packets refused, bytes copied, bytes read as 0 past src_len
    assert all(int(x) > 1000 for x in out[2:6]), r.stdout
