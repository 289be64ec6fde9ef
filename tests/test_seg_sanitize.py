"""ASan + UBSan CPU build of the tx segmenter on the CPU (gcl_tx_seg_host,
csrc/gcl_host.c, with the rule of csrc/gcl_seg.h that the GPU kernels share),
driven by the stand-alone program tests/fuzz/seg_fuzz.c: hostile writes (any
proto and mss, lengths and windows up to 2^32 - 1, sequence numbers and source
offsets at their wrap), any cap, layout, lead, frame_base and frames_len, over
heap arrays of their exact size, so that a segment written past seg_cap or a
write read past m traps.  The program is run on its own; nothing is loaded
into Python.  Any sanitizer report fails the run."""
import os
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def seg_exe(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    from caladan_amd import build
    return build.build_sanitized_seg(str(tmp_path_factory.mktemp("san_seg")))


@pytest.mark.parametrize("seed", [1, 2])
def test_seg_host_hostile_batches(seg_exe, seed):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([seg_exe, str(seed), "3000"], capture_output=True, text=True, timeout=240,
                       env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[-4000:]
    out = r.stdout.split()
    assert out[:2] == ["seg", "ok"], r.stdout
    # OK, REFUSED and NOSPACE writes: no branch went unexercised
    assert all(int(x) > 1000 for x in out[2:5]), r.stdout
