"""ASan + UBSan CPU build of gcl_tcp_shut_host (csrc/gcl_host.c with the rule of
csrc/gcl_tcpshut.h that the GPU shares), driven by the stand-alone program
tests/fuzz/tcpshut_fuzz.c: random and garbage ops, how, states, flags and caps
over heap arrays of their exact size, so that a read or write past any of them
traps.  The program is run on its own; nothing is loaded into Python.  Any
sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def tcpshut_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_tcpshut(str(tmp_path_factory.mktemp("san_tcpshut")))


@pytest.mark.parametrize("seed", [1, 2])
def test_tcpshut_host_random_and_garbage_requests(tcpshut_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([tcpshut_exe, str(seed), "400"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["tcpshut", "ok"] and len(out) == 14, r.stdout
    counts = [int(x) for x in out[2:]]
    # every status was reached, FINs and RSTs written, connections failed, put and warned
    assert all(x > 100 for x in counts), r.stdout
