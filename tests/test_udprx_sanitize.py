"""ASan + UBSan CPU build of gcl_udp_rx_host (csrc/gcl_host.c with the rule of
csrc/gcl_udprx.h that the GPU shares), driven by the stand-alone program
tests/fuzz/udprx_fuzz.c: random frames, cookies, socket words and caps over
heap arrays of their exact size, so that a read or write past any of them
traps.  The program is run on its own; nothing is loaded into Python.  Any
sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def udprx_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_udprx(str(tmp_path_factory.mktemp("san_udprx")))


@pytest.mark.parametrize("seed", [1, 2])
def test_udprx_host_random_frames_cookies_and_caps(udprx_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([udprx_exe, str(seed), "1500"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["udprx", "ok"] and len(out) == 10, r.stdout
    counts = [int(x) for x in out[2:]]
    # every verdict was reached, bytes were taken and POLLIN was set
    assert all(x > 100 for x in counts[:6]), r.stdout
    assert counts[6] > 1000 and counts[7] > 20, r.stdout
