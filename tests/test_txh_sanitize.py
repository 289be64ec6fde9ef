"""ASan + UBSan CPU build of the transmit headers on the CPU (gcl_tx_hdr_host,
csrc/gcl_host.c, with the rule of csrc/gcl_txh.h that the GPU kernel shares)
and of the neighbour table (csrc/gcl_neigh.c, with the probe of
csrc/gcl_neigh.h), driven by the stand-alone program tests/fuzz/txh_fuzz.c:
hostile descriptors, offsets, caps and min_pkt_size over heap regions of their
exact size, random tables under truncated hashes, and table images overwritten
with random bytes, so that any read or write out of bounds traps.  The program
is run on its own; nothing is loaded into Python.  Any sanitizer report fails
the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def txh_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_txh(str(tmp_path_factory.mktemp("san_txh")))


@pytest.mark.parametrize("seed", [1, 2])
def test_txh_host_hostile_batches(txh_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([txh_exe, str(seed), "3000"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["txh", "ok"], r.stdout
    # OK, SELF, NONEIGH and REFUSED entries: no branch went unexercised
    assert all(int(x) > 1000 for x in out[2:6]), r.stdout
