"""ASan + UBSan CPU build of tcp_rx_conn's fast path on the CPU
(gcl_tcp_rx_host, csrc/gcl_host.c, with the rule of csrc/gcl_tcprx.h that the
GPU kernels share), driven by the stand-alone program tests/fuzz/tcprx_fuzz.c:
garbage frames, offsets, cookies, connection words and orders over heap arrays
of their exact size, so that a read or write past any of them traps.  The
program is run on its own; nothing is loaded into Python.  Any sanitizer
report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def tcprx_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_tcprx(str(tmp_path_factory.mktemp("san_tcprx")))


@pytest.mark.parametrize("seed", [1, 2])
def test_tcprx_host_hostile_lists(tcprx_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([tcprx_exe, str(seed), "2000"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["tcprx", "ok"], r.stdout
    # FAST, SLOW and DROP were each reached: no branch went unexercised
    assert all(int(x) > 1000 for x in out[2:5]), r.stdout
