"""ASan + UBSan CPU build of gcl_tcp_rx_states_host and gcl_tcp_rx_ctl_host
(csrc/gcl_host.c with the rules of csrc/gcl_tcprxs.h and csrc/gcl_tcptmr.h that
the GPU shares), driven by the stand-alone program tests/fuzz/tcprxs_fuzz.c:
random states, flags, queue ranges and seg_cap over heap arrays of their exact
size, so that a read or write past any of them traps.  The program is run on
its own; nothing is loaded into Python.  Any sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def tcprxs_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_tcprxs(str(tmp_path_factory.mktemp("san_tcprxs")))


@pytest.mark.parametrize("seed", [1, 2])
def test_tcprxs_host_random_states_flags_and_queues(tcprxs_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([tcprxs_exe, str(seed), "2000"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["tcprxs", "ok"] and out[25] == ":", r.stdout
    counts, branches = [int(x) for x in out[2:25]], [int(x) for x in out[26:]]
    # the four new counters moved: RSTS, FAILS, FINS, STATE_CHANGES
    assert all(x > 20 for x in counts[19:23]), r.stdout
    # and every new branch was reached: RST, RST_ACK, FAIL, STATE, FIN and PUT in ev, both kinds of RST segment
    assert len(branches) == 19 and all(x > 0 for x in branches[11:]), r.stdout
