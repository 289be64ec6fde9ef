"""CPU: gcl_tcp_rx_full_host (csrc/gcl_host.c with the rule of
csrc/gcl_tcprxf.h that the GPU walk shares) against the line-by-line
transcription of tcp_rx_conn and __tcp_rx_conn in tests/tcprxfcases.py: the
hand-derived values of the named cases, every output byte of the named cases
and of random streams over sentinel-filled outputs with guards, the counters,
rep_acks == NULL, the prefix that gcl_tcp_rx_host also handles, and every
-EINVAL."""
import ctypes
import errno

import numpy as np
import pytest

from tests import tcprxcases as rc
from tests import tcprxfcases as fc



@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def check(g, case, what):
    want = fc.model(case)
    got, cnt = fc.run_host(g, case)
    m, nconn = fc.dims(case)
    fc.compare(got, want, m, nconn, what)
    assert cnt.tolist() == want["counts"].tolist(), what
    return want


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_model_gives_the_hand_derived_values(name):
    case, exp = fc.cases()[name]
    fc.check_expected(fc.model(case), exp, name)


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_named_cases(g, name):
    case, exp = fc.cases()[name]
    check(g, case, name)
    got, cnt = fc.run_host(g, case)
    fc.check_expected(dict(got, counts=cnt), exp, name)


@pytest.fixture(scope="module")
def streams():
    return [fc.stream(k) for k in range(len(fc.STREAMS))]


def test_random_streams_meet_the_mix(streams):
    for k, case in enumerate(streams):
        fc.check_mix(fc.model(case), len(case["conn"]))


def test_random_streams(g, streams):
    for k, case in enumerate(streams):
        if k == 1:                                # a plan-like order: a permutation with repeats and strays
            rng = np.random.default_rng(5)
            n = len(case["pkt_len"])
            plan = np.argsort(case["sock"] % 3, kind="stable")
            case = dict(case, order=np.concatenate([plan, rng.integers(0, n + 9, size=300)]).astype(np.uint32))
        check(g, case, f"stream {k}")


def test_rep_acks_null_is_zeros(g):
    for name in ("dupacks_1_2_3_4", "two_interleaved", "rep_acks_2_on_entry"):
        case = fc.case_of(name)
        m, nconn = fc.dims(case)
        zero = dict(case, rep_acks=np.zeros(nconn, dtype=np.uint8))
        a, ca = fc.run_host(g, zero)
        b, cb = fc.run_host(g, case, rep_acks=None)
        fc.compare(b, a, m, nconn, name)
        assert ca.tolist() == cb.tolist()
        fc.compare(b, fc.model(zero), m, nconn, name)


def test_counts_accumulate_and_may_be_null(g):
    case = fc.case_of("two_interleaved")
    want = fc.model(case)
    got, _ = fc.run_host(g, case, counts=False)
    fc.compare(got, want, 6, 2, "no counts")
    cnt = np.zeros(fc.NR, dtype=np.uint64)
    for _ in range(2):
        g.tcp_rx_full_host(case["frames"], case["pkt_len"], case["sock"], case["conn"], offs=case["offs"],
                           rep_acks=case["rep_acks"], align=16, counts=cnt)
    assert cnt.tolist() == (2 * want["counts"]).tolist()


def all_cases(streams):
    return [(n, c) for n, (c, _) in sorted(fc.cases().items())] + [(f"stream {k}", c) for k, c in enumerate(streams)]


def test_prefix_agrees_with_gcl_tcp_rx(g, streams):
    """entry by entry up to each connection's gcl_tcp_rx first_slow the two calls agree"""
    seen = 0
    for name, case in all_cases(streams):
        full, _ = fc.run_host(g, case)
        old, _ = rc.run_host(g, case)
        m, nconn = fc.dims(case)
        order = case.get("order")
        idx = np.arange(m) if order is None else order.astype(np.int64)
        for j in range(m):
            v = int(old["verdict"][j])
            if v in (rc.NA, rc.NOCONN, rc.DROP):
                assert int(full["verdict"][j]) == v, (name, j)
                continue
            ck = int(case["sock"][int(idx[j])])
            fs = int(old["out_conn"]["first_slow"][ck])
            if fs == rc.NONE or j < fs:
                assert v == rc.FAST and int(full["verdict"][j]) == rc.FAST, (name, j)
                assert int(full["copy_len"][j]) == int(old["copy_len"][j]), (name, j)
                assert int(full["sflags"][j]) & 0x0F == int(old["sflags"][j]), (name, j)
                assert int(full["dst_off"][j]) - int(full["conn_off"][ck]) == \
                       int(old["dst_off"][j]) - int(old["conn_off"][ck]), (name, j)
                seen += 1
    # not vacuous: about half of the 600 connections of streams 0 and 3 begin with text
    assert seen > 200


def test_error_returns(g):
    case = fc.case_of("two_interleaved")
    m, nconn = 6, 2
    out = fc.blank(m, nconn)
    ok = dict(frames=case["frames"], pkt_len=case["pkt_len"], sock=case["sock"], conn=case["conn"],
              offs=case["offs"], out=out)
    g.tcp_rx_full_host(**ok)

    def refused(**kw):
        with pytest.raises(OSError) as e:
            g.tcp_rx_full_host(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(align=3)
    refused(align=512)
    refused(m=5)                                  # order NULL and m != n
    refused(blocks=rc.MAX_BLOCKS + 1)
    for f in fc.blank(m, nconn):                  # every output, out_ext among them
        refused(out=dict(out, **{f: None}))
    odd = np.zeros(8 * m + 16, dtype=np.uint8)
    refused(out=dict(out, dst_off=odd[1:]))
    refused(out=dict(out, rcv_nxt_after=odd[2:]))
    refused(out=dict(out, copy_len=odd[1:]))
    refused(out=dict(out, conn_off=odd[4:]))
    refused(out=dict(out, out_conn=np.zeros(48 * nconn + 16, dtype=np.uint8)[8:]))
    refused(out=dict(out, out_ext=np.zeros(16 * nconn + 16, dtype=np.uint8)[8:]))
    refused(conn=np.frombuffer(bytes(48 * nconn + 16), dtype=np.uint8)[8:], nconn=nconn)
    refused(pkt_len=None, n=m)
    refused(counts=np.zeros(14, dtype=np.uint64).view(np.uint8)[4:108])
    with pytest.raises(ValueError):
        g.tcp_rx_full_host(**dict(ok, sock=None))
    b = g.GclBatch(frames=case["frames"].ctypes.data, frames_len=case["frames_len"], n=m,
                   pkt_len=case["pkt_len"].ctypes.data, offs=case["offs"].ctypes.data)
    rin = g.GclTcprxfIn(size=ctypes.sizeof(g.GclTcprxfIn), m=m, sock=None, conn=case["conn"].ctypes.data,
                        nconn=nconn)
    rout = g.GclTcprxOut(**{f: out[f].ctypes.data for f in g.TCPRX_OUT_FIELDS})
    ext = out["out_ext"].ctypes.data

    def raw(bp=True, e=ext):
        return g.lib.gcl_tcp_rx_full_host(ctypes.byref(b) if bp else None, ctypes.byref(rin), ctypes.byref(rout), e,
                                          None)

    assert raw() == -errno.EINVAL                 # a NULL sock
    rin.sock, rin.size = case["sock"].ctypes.data, ctypes.sizeof(g.GclTcprxIn)
    assert raw() == -errno.EINVAL                 # gcl_tcprx_in's size is not this struct's
    rin.size, rin.nconn = ctypes.sizeof(g.GclTcprxfIn), rc.MAX_CONN + 1
    assert raw() == -errno.EINVAL
    order = np.arange(m, dtype=np.uint32)
    rin.nconn, rin.order = nconn, order.ctypes.data
    assert raw() == 0
    rin.m = (1 << 31) + 1
    assert raw() == -errno.EINVAL
    rin.m = m
    odd4 = np.zeros(4 * m + 8, dtype=np.uint8)
    rin.order = odd4.ctypes.data + 2
    assert raw() == -errno.EINVAL
    rin.order, rin.sock = order.ctypes.data, odd4.ctypes.data + 1
    assert raw() == -errno.EINVAL
    rin.sock = case["sock"].ctypes.data
    assert raw() == 0
    assert raw(bp=False) == -errno.EINVAL
    assert raw(e=None) == -errno.EINVAL
    rin.nconn = 0                                 # no connection: out_ext may be NULL
    assert raw(e=None) == 0
    need = ctypes.c_size_t()
    assert g.lib.gcl_tcp_rx_full_workspace((1 << 31) + 1, 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_full_workspace(1, rc.MAX_CONN + 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_full_workspace(1, 1, rc.MAX_BLOCKS + 1, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_full_workspace(1, 1, 0, None) == -errno.EINVAL
    assert g.tcp_rx_full_workspace(1 << 16, 4096) == g.tcp_rx_workspace(1 << 16, 4096) + 16 * 4096
