"""ASan + UBSan CPU build of tcp_rx_conn with its established slow path and the
out-of-order queue on the CPU (gcl_tcp_rx_ooo_host, csrc/gcl_host.c, with the
rule of csrc/gcl_tcprxo.h that the GPU walk shares), driven by the stand-alone
program tests/fuzz/tcprxo_fuzz.c: hostile q_off, queue entries and orders over
heap arrays of their exact size, so that a read or write past any of them
traps.  The program is run on its own; nothing is loaded into Python.  Any
sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def tcprxo_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_tcprxo(str(tmp_path_factory.mktemp("san_tcprxo")))


@pytest.mark.parametrize("seed", [1, 2])
def test_tcprxo_host_hostile_queues(tcprxo_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([tcprxo_exe, str(seed), "2000"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["tcprxo", "ok"] and out[21] == ":", r.stdout
    counts, branches = [int(x) for x in out[2:21]], [int(x) for x in out[22:]]
    # every new counter moved: OOO, QUEUED, DRAINED, FREED, HEADCLIP, HELD
    assert all(x > 100 for x in counts[13:19]), r.stdout
    # and every new branch was reached: KEPT, FREED and DRAINED input entries, a refused segment, a head clip,
    # LATE_DRAINED, LATE_FREED, HELD, a drain of zero bytes, QSKIP, a stop at a full queue
    assert len(branches) == 11 and all(x > 0 for x in branches), r.stdout
