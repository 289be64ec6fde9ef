"""ASan + UBSan CPU build of the payload descriptors and the packed layout on
the CPU (gcl_l4_payload_host, csrc/gcl_host.c, with the rule of csrc/gcl_pay.h
that the GPU kernel shares), driven by the stand-alone program
tests/fuzz/pay_fuzz.c: batches with hostile offsets, pkt_len, tot, data
offsets, orders and segment starts over heap arrays of their exact size, so
that any read or write out of bounds traps.  The program is run on its own;
nothing is loaded into Python.  Any sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def pay_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_pay(str(tmp_path_factory.mktemp("san_pay")))


@pytest.mark.parametrize("seed", [1, 2])
def test_pay_host_hostile_batches(pay_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([pay_exe, str(seed), "3000"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["pay", "ok"], r.stdout
    # entries kept, NA, dropped by a filter, and out of range
    assert all(int(x) > 1000 for x in out[2:6]), r.stdout
