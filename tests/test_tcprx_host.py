"""CPU: gcl_tcp_rx_host (csrc/gcl_host.c with the rule of csrc/gcl_tcprx.h that
the GPU kernels share) against the line-by-line transcription of
tcp_rx_conn's fast path in tests/tcprxcases.py: every output byte of the named
cases and of random streams, sentinel-filled outputs with guards, the
counters, and every -EINVAL."""
import ctypes
import errno

import numpy as np
import pytest

from tests import tcprxcases as rc


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def check(g, case, what):
    want = rc.model(case)
    got, cnt = rc.run_host(g, case)
    m, nconn = len(want["verdict"]), len(case["conn"])
    rc.compare(got, want, m, nconn, what)
    assert cnt.tolist() == want["counts"].tolist(), what
    return want


@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_named_cases(g, name):
    check(g, rc.cases()[name], name)


def test_named_cases_say_what_their_names_say():
    """the model's own verdicts for the named cases: the cases test what they claim"""
    w = {k: rc.model(c) for k, c in rc.cases().items()}
    assert w["clean_chain"]["verdict"].tolist() == [rc.FAST] * 5
    for what in ("fin", "rst", "urg", "len0", "ack_gt", "seq_ne", "wnd_small"):
        assert w[f"{what}_at0"]["verdict"].tolist() == [rc.SLOW] * 5, what
        assert w[f"{what}_at2"]["verdict"].tolist() == [rc.FAST] * 2 + [rc.SLOW] * 3, what
        assert w[f"{what}_at2"]["out_conn"]["first_slow"][0] == 2
    assert w["too_long_at2"]["verdict"].tolist() == [rc.FAST, rc.FAST, rc.DROP, rc.SLOW, rc.SLOW]
    assert w["not_eligible"]["verdict"].tolist() == [rc.SLOW] * 3
    assert w["snd_full_at0"]["verdict"].tolist() == [rc.SLOW] * 3
    assert w["snd_full_at2"]["verdict"].tolist() == [rc.FAST] * 2 + [rc.SLOW] * 3
    assert w["drop_before_and_after_stop"]["verdict"].tolist() == [rc.DROP, rc.FAST, rc.SLOW, rc.DROP, rc.SLOW]
    assert w["rcv_wnd_exact"]["verdict"].tolist() == [rc.FAST, rc.FAST, rc.SLOW]
    assert w["rcv_wnd_exact"]["out_conn"]["rcv_wnd"][0] == 0
    assert w["wrap_seq_and_snd"]["verdict"].tolist() == [rc.FAST] * 4
    assert w["wrap_seq_and_snd"]["out_conn"]["rcv_nxt"][0] == 0x18A
    assert w["wrap_snd_full"]["verdict"].tolist() == [rc.SLOW]
    assert w["ack_eq_una"]["sflags"][0] & rc.SF_ACKED == 0 and w["ack_eq_snd_nxt"]["sflags"][0] & rc.SF_ACKED
    assert w["ack_older"]["sflags"].tolist() == [0, rc.SF_WAKE | rc.SF_ACK_NOW]
    assert w["wl1_tie_wl2_lte"]["sflags"][0] & rc.SF_WND and not w["wl1_tie_wl2_gt"]["sflags"][0] & rc.SF_WND
    assert w["wscale14"]["out_conn"]["snd_wnd"][0] == 0xFFFF << 14 and w["wscale0"]["out_conn"]["snd_wnd"][0] == 0xFFFF
    assert w["delack_cnt0_ad0"]["sflags"].tolist()[1] & rc.SF_ACK_NOW
    assert w["delack_cnt0_ad0"]["out_conn"]["flags"][0] & rc.TIMER_ARMED
    assert not w["delack_cnt0_ad4"]["out_conn"]["flags"][0] & rc.TIMER_ARMED
    assert w["delack_cnt1_ad4"]["sflags"].tolist()[0] & rc.SF_ACK_NOW
    assert [x & rc.SF_WAKE for x in w["wake_psh0_rxq0"]["sflags"].tolist()] == [0, rc.SF_WAKE]
    assert w["wake_psh8_rxq0"]["sflags"][0] & rc.SF_WAKE and w["wake_psh0_rxq2"]["sflags"][0] & rc.SF_WAKE
    assert w["syn_data_is_fast"]["verdict"].tolist() == [rc.FAST] * 2
    assert w["two_interleaved"]["verdict"].tolist() == [rc.FAST] * 6
    assert w["two_interleaved"]["conn_off"].tolist() == [0, 608, 640]
    assert w["cookie_ge_nconn"]["verdict"].tolist() == [rc.NOCONN, rc.FAST, rc.NOCONN, rc.NA]
    assert w["duplicate_order"]["verdict"].tolist() == [rc.FAST, rc.SLOW, rc.SLOW, rc.SLOW, rc.SLOW, rc.NA, rc.NA,
                                                        rc.SLOW]


@pytest.fixture(scope="module")
def streams(g):
    return [rc.random_case(s, m, nc, align=a) for s, m, nc, a in ((1, 4096, 300, 0), (2, 3000, 37, 64),
                                                                   (3, 4096, 1, 0), (4, 2000, 300, 256))]


def test_random_streams(g, streams):
    seen_v, seen_sf, seen_of = set(), 0, 0
    for k, case in enumerate(streams):
        # a plan-like order for one of them: a permutation with repeats and strays
        if k == 1:
            rng = np.random.default_rng(5)
            n = len(case["pkt_len"])
            plan = np.argsort(case["sock"] % 3, kind="stable")   # arrival order kept inside a bucket
            case = dict(case, order=np.concatenate([plan, rng.integers(0, n + 9, size=300)]).astype(np.uint32))
        want = check(g, case, f"stream {k}")
        seen_v |= set(want["verdict"].tolist())
        seen_sf |= int(np.bitwise_or.reduce(want["sflags"]))
        seen_of |= int(np.bitwise_or.reduce(want["out_conn"]["flags"]))
        # one connection stops at its first fault: its stream has a short FAST prefix by nature
        assert (want["verdict"] == rc.FAST).sum() > (50 if k == 2 else len(want["verdict"]) // 8), k
    assert seen_v == {rc.FAST, rc.SLOW, rc.DROP, rc.NOCONN, rc.NA}
    assert seen_sf == 0xF and seen_of == 0x7E


def test_counts_accumulate_and_may_be_null(g):
    case = rc.cases()["two_interleaved"]
    want = rc.model(case)
    got, _ = rc.run_host(g, case, counts=False)
    rc.compare(got, want, 6, 2, "no counts")


def test_error_returns(g):
    case = rc.cases()["two_interleaved"]
    m, nconn = 6, 2
    out = rc.blank(m, nconn)
    ok = dict(frames=case["frames"], pkt_len=case["pkt_len"], sock=case["sock"], conn=case["conn"],
              offs=case["offs"], out=out)
    g.tcp_rx_host(**ok)

    def refused(**kw):
        with pytest.raises(OSError) as e:
            g.tcp_rx_host(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(align=3)
    refused(align=512)
    refused(m=5)                                  # order NULL and m != n
    refused(blocks=rc.MAX_BLOCKS + 1)
    for f in rc.blank(m, nconn):
        refused(out=dict(out, **{f: None}))
    odd = np.zeros(8 * m + 16, dtype=np.uint8)
    refused(out=dict(out, dst_off=odd[1:]))
    refused(out=dict(out, rcv_nxt_after=odd[2:]))
    refused(out=dict(out, copy_len=odd[1:]))
    refused(out=dict(out, conn_off=odd[4:]))
    refused(out=dict(out, out_conn=np.zeros(48 * nconn + 16, dtype=np.uint8)[8:]))
    refused(conn=np.frombuffer(bytes(48 * nconn + 16), dtype=np.uint8)[8:], nconn=nconn)
    refused(pkt_len=None, n=m)
    refused(counts=np.zeros(9, dtype=np.uint64).view(np.uint8)[4:68])
    with pytest.raises(ValueError):
        g.tcp_rx_host(**dict(ok, sock=None))
    b = g.GclBatch(frames=case["frames"].ctypes.data, frames_len=case["frames_len"], n=m,
                   pkt_len=case["pkt_len"].ctypes.data, offs=case["offs"].ctypes.data)
    rin = g.GclTcprxIn(size=ctypes.sizeof(g.GclTcprxIn), m=m, sock=None, conn=case["conn"].ctypes.data, nconn=nconn)
    rout = g.GclTcprxOut(**{f: out[f].ctypes.data for f in g.TCPRX_OUT_FIELDS})
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    rin.sock, rin.size = case["sock"].ctypes.data, 48
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    rin.size, rin.nconn = ctypes.sizeof(g.GclTcprxIn), rc.MAX_CONN + 1
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    # m > 2^31 with an order given, so that only the limit can refuse it (it returns before reading order)
    order = np.arange(m, dtype=np.uint32)
    rin.nconn, rin.order = nconn, order.ctypes.data
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == 0
    rin.m = (1 << 31) + 1
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    rin.m = m
    # order and sock that are not 4-B aligned
    odd4 = np.zeros(4 * m + 8, dtype=np.uint8)
    rin.order = odd4.ctypes.data + 2
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    rin.order, rin.sock = order.ctypes.data, odd4.ctypes.data + 1
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    rin.sock = case["sock"].ctypes.data
    assert g.lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None) == 0
    assert g.lib.gcl_tcp_rx_host(None, ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    need = ctypes.c_size_t()
    assert g.lib.gcl_tcp_rx_workspace((1 << 31) + 1, 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_workspace(1, rc.MAX_CONN + 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_workspace(1, 1, rc.MAX_BLOCKS + 1, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_workspace(1, 1, 0, None) == -errno.EINVAL
    assert g.tcp_rx_workspace(1 << 20, 1 << 20) > g.tcp_rx_workspace(1 << 20, 2048) > 0
