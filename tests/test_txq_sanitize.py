"""ASan + UBSan CPU build of the retransmit queues on the CPU
(gcl_tcp_txq_host, csrc/gcl_host.c, with the rule of csrc/gcl_txq.h that the GPU
kernels share), driven by the stand-alone program tests/fuzz/txq_fuzz.c:
garbage queue offsets, entries, connection words, wants and caps over heap
arrays of their exact size, so that a read or write past any of them traps.
The program is run on its own; nothing is loaded into Python.  Any sanitizer
report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def txq_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_txq(str(tmp_path_factory.mktemp("san_txq")))


@pytest.mark.parametrize("seed", [1, 2])
def test_txq_host_hostile_queues(txq_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([txq_exe, str(seed), "1500"], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["txq", "ok"] and len(out) == 14, r.stdout
    # ACKED, RETX, COPIED, TRIMMED, REFUSED, NOSPACE, DEFERRED and BYTES, then the connections flagged EMPTY,
    # BATCH and BADRANGE and the entries left NOSPACE: no branch went unexercised
    assert all(int(x) > 100 for x in out[2:14]), r.stdout
