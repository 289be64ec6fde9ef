"""CPU: gcl_rx_csum_flags (include/gcl_host.h), the rule of gcl_rx_csum for
one frame, against the numpy definition (tests/csumcases.py); the guarantee
of include/gclassify.h as an acceptance model of the receiving runtime; and
the definition itself pinned to the reference's chksum_internet where the
reference tree is present."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.csumcases import (BAD, GOOD, HDR, MASK, entry_flags, expected, fold, header_set,
                             header_sums)

REF_INC = "/root/reference/inc"


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def headers():
    return header_set()


def test_header_set_is_what_it_says(headers):
    frames, kinds = headers
    assert len(frames) == 253 and {"good", "bad", "skip"} == set(kinds)
    offs = np.arange(len(frames)) * HDR
    out, counts = expected(frames.reshape(-1), frames.size, offs, 0x00)
    want = {"good": GOOD, "bad": BAD, "skip": 0x00}
    assert [int(o) for o in out] == [want[k] for k in kinds]
    assert counts.tolist() == [len(kinds) - kinds.count("skip"), kinds.count("good"),
                               kinds.count("bad"), kinds.count("skip")]
    assert kinds.count("bad") >= 160 + 10  # every single-bit flip, every IHL 6-15 header


def test_flags_match_definition_over_header_set(g, headers):
    frames, kinds = headers
    rng = np.random.default_rng(71)
    for i, f in enumerate(frames):
        for fl in entry_flags(rng, 16):
            want, _ = expected(f, HDR, [0], fl)
            got = g.rx_csum_flags(f.tobytes(), int(fl))
            assert got == want[0], f"header {i} ({kinds[i]}) flags {fl:#x}: {got:#x} != {want[0]:#x}"
            assert got & 0xF3 == int(fl) & 0xF3


def test_flags_match_definition_at_every_length(g, headers):
    """A frame cut at every len in [0, 80]: bytes at or past len read 0."""
    frames, _ = headers
    rng = np.random.default_rng(72)
    for f in (frames[0], frames[40], frames[-1], frames[226]):
        long = np.concatenate([f, rng.integers(0, 256, size=16, dtype=np.uint8)])
        for ln in range(81):
            for fl in (0x00, 0x04, 0x08, 0x0C, 0xF3):
                want, _ = expected(long, ln, [0], fl)
                assert g.rx_csum_flags(long[:ln].tobytes(), fl) == want[0], (ln, fl)
    assert g.lib.gcl_rx_csum_flags(None, 0, 0x04) == 0x04


def test_runtime_accepts_the_same_packets(g, headers):
    """The guarantee: the runtime accepts a packet iff csum_type is
    CHECKSUM_TYPE_UNNECESSARY (bit 48 of cmd) or its own 20-byte check
    passes.  Fed the output flags it must accept exactly the packets it
    accepts when fed the entry flags, for every entry flag value."""
    frames, _ = headers
    n = len(frames)
    offs = np.arange(n) * HDR
    _, s = header_sums(frames.reshape(-1), frames.size, offs)
    check_passes = s == 0xFFFF  # chksum_internet(iphdr, 20) == 0

    def accepts(flags):
        cmd = np.array([g.lib.gcl_rx_make_cmd(64, int(f)) for f in flags], dtype=np.uint64)
        return ((cmd >> np.uint64(48)) & np.uint64(1)).astype(bool) | check_passes

    skipped_check = 0
    for fl in range(16):
        entry = np.full(n, fl | 0xA0, dtype=np.uint8)
        out = np.array([g.rx_csum_flags(f.tobytes(), int(e)) for f, e in zip(frames, entry)],
                       dtype=np.uint8)
        assert (accepts(entry) == accepts(out)).all(), f"entry flags {fl:#x}"
        # the check is skipped only where it would have passed, or was skipped before
        unnecessary = (out & MASK) == GOOD
        assert (check_passes | ((entry & MASK) == GOOD))[unnecessary].all()
        skipped_check += int((unnecessary & ((entry & MASK) != GOOD)).sum())
    assert skipped_check > 0


def test_definition_is_the_reference_chksum(tmp_path):
    """chksum_internet of the reference returns 0 exactly where the numpy
    definition's folded sum is 0xFFFF."""
    if not os.path.isdir(REF_INC):
        pytest.skip("reference tree not present")
    if shutil.which("gcc") is None:
        pytest.skip("gcc missing")
    src = tmp_path / "shim.c"
    src.write_text('#include <stdint.h>\n#include <asm/chksum.h>\n'
                   'uint16_t shim_chksum(const void *b, int n) { return chksum_internet(b, n); }\n')
    so = tmp_path / "shim.so"
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-I", REF_INC, "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    lib.shim_chksum.restype = ctypes.c_uint16
    lib.shim_chksum.argtypes = [ctypes.c_char_p, ctypes.c_int]

    rng = np.random.default_rng(73)
    bufs = rng.integers(0, 256, size=(10000, 20), dtype=np.uint8)
    # half of them valid: the checksum field (header bytes 10-11) set
    for b in bufs[::2]:
        b[10:12] = 0
        c = ~int(fold((b[0::2].astype(np.uint64) << 8 | b[1::2]).sum())) & 0xFFFF
        b[10], b[11] = c >> 8, c & 0xFF
    carries = [np.full(20, 0xFF, np.uint8), np.zeros(20, np.uint8)]
    for k in range(64):
        w = np.where(rng.random(10) < 0.7, 0xFFFF, 0x0001)
        b = np.zeros(20, np.uint8)
        b[0::2], b[1::2] = w >> 8, w & 0xFF
        carries.append(b)
    bufs = np.concatenate([bufs, np.stack(carries)])
    frames = np.zeros((len(bufs), HDR), dtype=np.uint8)
    frames[:, 12] = 0x08
    frames[:, 14:34] = bufs
    _, s = header_sums(frames.reshape(-1), frames.size, np.arange(len(bufs)) * HDR)
    ref = np.array([lib.shim_chksum(b.tobytes(), 20) for b in bufs])
    assert ((ref == 0) == (s == 0xFFFF)).all()
    assert (ref == 0).sum() >= 5000 and (ref != 0).sum() >= 4000
    # and the complement of the folded sum is the value it returns
    assert (ref == (~s.astype(np.uint32) & 0xFFFF)).all()
