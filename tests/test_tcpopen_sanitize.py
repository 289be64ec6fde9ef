"""ASan + UBSan CPU build of gcl_tcp_rx_open_host (csrc/gcl_host.c with the rule
and the option walk of csrc/gcl_tcpopen.h that the GPU shares), driven by the
stand-alone program tests/fuzz/tcpopen_fuzz.c: random frames, options, cookies,
backlogs and caps over heap arrays of their exact size, so that a read or write
past any of them traps.  The program is run on its own; nothing is loaded into
Python.  Any sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def tcpopen_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_tcpopen(str(tmp_path_factory.mktemp("san_tcpopen")))


@pytest.mark.parametrize("seed", [1, 2])
def test_tcpopen_host_random_frames_options_and_caps(tcpopen_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([tcpopen_exe, str(seed), "1500"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["tcpopen", "ok"] and out[18] == ":", r.stdout
    counts, words = [int(x) for x in out[2:18]], [int(x) for x in out[19:]]
    # every verdict was reached, segments were written and skipped, records ran out of room
    assert all(x > 20 for x in counts[:12]), r.stdout
    assert counts[12] > 100 and counts[13] > 0 and counts[14] > 0, r.stdout
    # and both option words were written into SYN|ACKs
    assert len(words) == 2 and all(x > 20 for x in words), r.stdout
