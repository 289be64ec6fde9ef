"""ASan + UBSan CPU build of the TCP timer sweep and the control segments on
the CPU (gcl_tcp_tick_host and gcl_tcp_rx_acks_host, csrc/gcl_host.c, with the
rules of csrc/gcl_tcptmr.h that the GPU kernels share), driven by the
stand-alone program tests/fuzz/tcptmr_fuzz.c: garbage timer words, connection
words, addresses, orders, cookies, verdicts and caps over heap arrays of their
exact size, so that a read or write past any of them traps.  The program is
run on its own; nothing is loaded into Python.  Any sanitizer report fails the
run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def tcptmr_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_tcptmr(str(tmp_path_factory.mktemp("san_tcptmr")))


@pytest.mark.parametrize("seed", [1, 2])
def test_tcptmr_host_hostile_sweeps_and_lists(tcptmr_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([tcptmr_exe, str(seed), "1500"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["tcptmr", "ok"] and len(out) == 15, r.stdout
    # FIRED, ACK, PROBE, RETRANSMIT, FAIL, CLOSE, NOSPACE and SEGS of the sweeps, then the ACKs WANTED
    # and WRITTEN, the entries SKIPPED, and each of the two guards: no branch went unexercised
    assert all(int(x) > 1000 for x in out[2:15]), r.stdout
