"""CPU: gcl_copy_batch_host (include/gcl_host.h), the loopback frame copy on
the host, against the numpy definition (tests/copycases.py) on every case set
the GPU test uses; its error returns; and gcl_loopback_olflags for every
tx_olflags value.  Every comparison is of the whole destination, guard bytes
included."""
import ctypes

import numpy as np
import pytest

from tests.copycases import (FILL, GUARD, NR, SIZES, dense_case, edge_cases, expected, grid_case,
                             ingress_case, loopback_olflags, mixed_case)

EINVAL = 22
CANARY = 64


def copy_batch_host(*a, **kw):
    """the binding's new name, looked up when called: the library is loaded
    by the first test that needs it, not while the suite is collected"""
    from caladan_amd import gclassify
    return gclassify.copy_batch_host(*a, **kw)


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def run_host(case, counts=None, olflags=None, rss=None, use_flags=True, use_hash=True):
    """One gcl_copy_batch_host over @case; returns (the destination with its
    guards, pkt_len, olflags, rss with their canary tails)."""
    n = len(case["len"])
    buf = np.full(case["dst_len"] + 2 * GUARD, FILL, dtype=np.uint8)
    dst = buf[GUARD:GUARD + case["dst_len"]]
    pl = np.full(n + CANARY, 0x5A5A, dtype=np.uint16)
    ol = np.full(n + CANARY, 0x5A, dtype=np.uint8) if olflags is None else olflags
    rs = np.full(n + CANARY, 0x5A5A5A5A, dtype=np.uint32) if rss is None else rss
    src = case["src"]
    if case["src_len"] == 0:
        src = np.zeros(1, dtype=np.uint8)
    pl, ol, rs = copy_batch_host(src, case["src_off"], case["len"], dst, dst_off=case["dst_off"],
                    dst_stride=case["dst_stride"], tx_olflags=case["tx_olflags"] if use_flags else None,
                    hash=case["hash"] if use_hash else None, n=n, src_len=case["src_len"],
                    dst_cap=case["dst_cap"], counts=counts, pkt_len=pl, olflags=ol, rss=rs)
    return buf, pl, ol, rs


def check_host(case, what):
    want, wpl, wol, wrs, wcnt = expected(case)
    n = len(case["len"])
    cnt = np.zeros(NR, dtype=np.uint64)
    buf, pl, ol, rs = run_host(case, counts=cnt)
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + case["dst_len"]:] == FILL).all(), what
    bad = np.nonzero(buf[GUARD:GUARD + case["dst_len"]] != want)[0]
    assert not len(bad), f"{what}: {len(bad)} destination bytes differ, first at {bad[0]}"
    assert (pl[:n] == wpl).all() and (ol[:n] == wol).all() and (rs[:n] == wrs).all(), what
    assert (pl[n:] == 0x5A5A).all() and (ol[n:] == 0x5A).all() and (rs[n:] == 0x5A5A5A5A).all(), what
    assert cnt.tolist() == wcnt.tolist() and cnt[0] + cnt[1] == n, what
    return wcnt


def test_length_alignment_grid():
    cnt = check_host(grid_case(), "grid")
    assert cnt[1] == 0 and cnt[0] > 26 * 49


@pytest.mark.parametrize("n", SIZES)
def test_dense_slots_and_ingress_geometry(n):
    check_host(dense_case(n), f"dense n={n}")
    check_host(ingress_case(n), f"ingress n={n}")


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_edges(name):
    cnt = check_host(edge_cases()[name], name)
    assert cnt[0] > 0
    if "src_len" not in name and "source" not in name:
        assert cnt[1] > 0


def test_mixed_lengths():
    check_host(mixed_case(), "mixed")


def test_optional_arrays_and_accumulated_counts():
    case = dense_case(257)
    n = 257
    want, wpl, wol, wrs, wcnt = expected(case)
    for use_flags in (True, False):
        for use_hash in (True, False):
            buf, pl, ol, rs = run_host(case, use_flags=use_flags, use_hash=use_hash)
            assert (buf[GUARD:-GUARD] == want).all()
            assert (ol[:n] == (wol if use_flags else 0x08)).all()
            assert (rs[:n] == (wrs if use_hash else 0)).all()
    # outputs left out: nothing else changes
    buf, pl, ol, rs = run_host(case, olflags=False, rss=False)
    assert ol is None and rs is None and (buf[GUARD:-GUARD] == want).all() and (pl[:n] == wpl).all()
    # allocated by the binding
    dst = np.full(case["dst_len"], FILL, dtype=np.uint8)
    pl, ol, rs = copy_batch_host(case["src"], case["src_off"], case["len"], dst, dst_stride=64,
                                 tx_olflags=case["tx_olflags"], hash=case["hash"])
    assert pl.dtype == np.uint16 and ol.dtype == np.uint8 and rs.dtype == np.uint32
    assert (dst == want).all() and (pl == wpl).all() and (ol == wol).all() and (rs == wrs).all()
    # two calls into the same counts
    cnt = np.zeros(NR, dtype=np.uint64)
    run_host(case, counts=cnt)
    run_host(case, counts=cnt)
    assert cnt.tolist() == (2 * wcnt).tolist()


def test_loopback_olflags_for_every_tx_value(g):
    tx = np.arange(256, dtype=np.uint8)
    want = loopback_olflags(tx)
    assert [g.lib.gcl_loopback_olflags(int(t)) for t in tx] == want.tolist()
    src = np.zeros(256 * 16, dtype=np.uint8)
    dst = np.zeros(256 * 16, dtype=np.uint8)
    _, ol, _ = copy_batch_host(src, np.arange(256, dtype=np.uint64) * 16, np.full(256, 16, dtype=np.uint16),
                               dst, dst_stride=16, tx_olflags=tx)
    assert (ol == want).all()
    assert set(want.tolist()) == {g.F_IP_CKSUM_GOOD, g.F_IP_CKSUM_GOOD | g.F_RSS_HASH}


def test_error_returns(g):
    n = 100
    src = np.zeros(n * 64, dtype=np.uint8)
    dst = np.full(n * 64, FILL, dtype=np.uint8)
    off = np.arange(n, dtype=np.uint64) * 64
    ln = np.full(n, 64, dtype=np.uint16)
    pl = np.full(n, 0x5A5A, dtype=np.uint16)
    cnt = np.full(NR, 7, dtype=np.uint64)

    def call(size=ctypes.sizeof(g.GclCopyIn), s=src.ctypes.data, src_len=n * 64, so=off.ctypes.data,
             le=ln.ctypes.data, nn=n, d=dst.ctypes.data, dst_len=n * 64, doff=None, stride=64,
             p=pl.ctypes.data, cin=True, cout=True):
        i = g.GclCopyIn(size=size, src=s, src_len=src_len, src_off=so, len=le, n=nn)
        o = g.GclCopyOut(dst=d, dst_len=dst_len, dst_off=doff, dst_stride=stride, pkt_len=p)
        return g.lib.gcl_copy_batch_host(ctypes.byref(i) if cin else None,
                                         ctypes.byref(o) if cout else None, cnt.ctypes.data)

    assert call(cin=False) == -EINVAL and call(cout=False) == -EINVAL
    assert call(size=ctypes.sizeof(g.GclCopyIn) - 8) == -EINVAL and call(size=0) == -EINVAL
    for kw in ({"s": None}, {"so": None}, {"le": None}, {"d": None}, {"p": None}):
        assert call(**kw) == -EINVAL, kw
    assert call(src_len=(1 << 64) - 1) == -EINVAL and call(dst_len=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1) == -EINVAL
    for stride in (0, 8, 15, 24, 72, (1 << 20) + 16):
        assert call(stride=stride) == -EINVAL, stride
    assert (dst == FILL).all() and (pl == 0x5A5A).all() and (cnt == 7).all()
    # a stride is not looked at when offsets are given; n == 0 needs no array
    assert call(stride=3, doff=off.ctypes.data) == 0
    assert call(nn=0, s=None, d=None) == 0
    assert cnt.tolist() == [7 + n, 7, 7 + 64 * n, 7]
    with pytest.raises(ValueError):
        copy_batch_host(src, off, ln, dst, dst_stride=64, pkt_len=pl[:n - 1])
    with pytest.raises(ValueError):
        copy_batch_host(src, off, ln, dst, dst_stride=64, src_len=n * 64 + 1)
    with pytest.raises(ValueError):
        copy_batch_host(src, off, ln, dst, dst_stride=64, counts=cnt[:3])
