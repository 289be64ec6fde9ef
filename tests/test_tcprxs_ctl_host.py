"""CPU: gcl_tcp_rx_ctl_host (csrc/gcl_host.c with gcl_rxctl_kind and
gcl_ctl_rst_desc of csrc/gcl_tcptmr.h): equal to gcl_tcp_rx_acks_host on lists
without RSTs, the segments the reference sent (tests/golden/tcprxs_ref.json) on
every recorded case, the 20 TCP header bytes gcl_tx_hdr_host writes from a RST
descriptor against runtime/net/tcp_out.c:112-118 and :154-160, seg_cap of 0,
one below wanted and wanted, and the -EINVAL list."""
import ctypes
import errno

import numpy as np
import pytest

from tests import tcprxocases as oc
from tests import tcprxscases as sc
from tests import tcprxsctlcases as cc
from tests import tcprxsrefcases as sr
from tests import tcptmrcases as tc


@pytest.fixture(scope="module")
def g():
    import caladan_amd.gclassify as g
    return g


def test_layout(g):
    assert ctypes.sizeof(g.GclRxctlIn) == 120 and g.GclRxctlIn.ev.offset == 104 and g.GclRxctlIn.rst_seq.offset == 112
    assert (g.CTL_ACK, g.CTL_PROBE, g.CTL_RST, g.CTL_RST_ACK) == (0, 1, 2, 3)


def test_equals_tcp_rx_acks_on_lists_without_rsts(g):
    """every case, its ev taken away, and the out-of-order streams, which hold none: byte for byte, counts too"""
    cases = [(n, sr.case_of(n)) for n in sr.names()] + [(n, sc.stream(n)) for n in sorted(sc.STREAMS)] + \
            [(k, oc.stream(k)) for k in range(len(oc.STREAMS))]
    acks = 0
    for name, case in cases:
        rx, _ = sc.run_host(g, case)
        m = len(case["sock"])
        for cap in (m + 1, 3):
            want, wcnt = cc.run_host(g, case, rx, cap, acks=True)
            got, cnt = cc.run_host(g, case, rx, cap, ev=np.zeros(m + 1, dtype=np.uint8))
            cc.same(got, want, min(cap, int(want["totals"][0])), name)
            assert cnt.tolist() == wcnt.tolist(), name
        acks += int(want["totals"][0])
    assert acks > 1000


def test_segments_are_what_the_reference_sent(g):
    rsts = 0
    for name in sr.names():
        case = sr.case_of(name)
        rx, _ = sc.run_host(g, case)
        got, cnt = cc.run_host(g, case, rx, len(case["sock"]) + 1)
        n = cc.check_against_reference(got, name, "host")
        assert cnt[:3].tolist() == [n, n, 0], name
        rsts += int((got["seg_kind"][:n] >= cc.K_RST).sum())
    assert rsts > 20


@pytest.mark.parametrize("short", [None, 1, 0])
def test_seg_cap(g, short):
    """seg_cap of wanted, one below and 0: the first seg_cap segments, nothing behind, totals[0] what was wanted"""
    name = "stream:lifetimes"
    case = sr.case_of(name)
    rx, _ = sc.run_host(g, case)
    full, _ = cc.run_host(g, case, rx, len(case["sock"]))
    wanted = int(full["totals"][0])
    cap = wanted if short is None else (wanted - 1) * short
    got, cnt = cc.run_host(g, case, rx, cap)
    assert got["totals"][:2].tolist() == [wanted, cap] and cnt[:2].tolist() == [wanted, cap]
    for f, _ in cc.SEG:
        assert got[f][:cap].tobytes() == full[f][:cap].tobytes(), f
        assert (got[f][cap:].view(np.uint8) == cc.SENTINEL).all(), f


def test_rst_descriptors_give_the_header_bytes_of_tcp_out(g):
    """tcp_tx_raw_rst (:112-118): sport, dport, seq = hton32(seq), ack 0, off 5, flags RST, win 0;
    tcp_tx_raw_rst_ack (:154-160): seq = hton32(0), ack = hton32(ack), off 5, flags RST|ACK, win 0"""
    net = g.txh_net(tc.NET["addr"], tc.NET["netmask"], tc.NET["gateway"], tc.NET["mac"])
    seen = set()
    for name in ("closed_ack_rst_neither", "syn_in_window_with_ack", "synrcvd_ack_above_snd_nxt",
                 "syn_fin_without_ack"):
        case = sr.case_of(name)
        rx, _ = sc.run_host(g, case)
        got, _ = cc.run_host(g, case, rx, len(case["sock"]))
        k = int(got["totals"][1])
        frames = np.full(k * cc.STRIDE, cc.SENTINEL, dtype=np.uint8)
        out = g.tx_hdr_host(got["desc"][:k].copy(), np.arange(k, dtype=np.uint64) * np.uint64(cc.STRIDE), frames, net)
        assert (out["status"][:k] != g.TXH_REFUSED).all() and (out["pkt_len"][:k] == 54).all(), name
        for x, (j, kind, seq, ack) in enumerate(cc.wanted(name)):
            t = frames[x * cc.STRIDE + 34:x * cc.STRIDE + 54]
            a = tc.addr1(int(case["sock"][j]))
            be = lambda lo, hi: int.from_bytes(t[lo:hi].tobytes(), "big")
            assert (be(0, 2), be(2, 4)) == (a["lport"], a["rport"]), (name, x)
            assert (be(4, 8), be(8, 12)) == (seq, ack), (name, x, "seq, ack")
            assert t[12] >> 4 == 5, (name, x, "off")
            assert t[13] == {cc.K_RST: 0x04, cc.K_RST_ACK: 0x14}[kind], (name, x, "flags")
            assert be(14, 16) == 0, (name, x, "win")
            seen.add(kind)
    assert seen == {cc.K_RST, cc.K_RST_ACK}


def test_einval(g):
    case = sr.case_of("closed_ack_rst_neither")
    rx, _ = sc.run_host(g, case)
    m, nconn = len(case["sock"]), len(case["conn"])
    base = dict(verdict=rx["verdict"], sflags=rx["sflags"], rcv_nxt_after=rx["rcv_nxt_after"], ev=rx["ev"],
                rst_seq=rx["rst_seq"], sock=case["sock"], conn=case["conn"], addr=cc.addrs(nconn), seg_cap=m, m=m,
                n=m, nconn=nconn)

    def refused(out=None, **kw):
        o = cc.blank(m)
        o.update(out or {})
        with pytest.raises(OSError) as e:
            g.tcp_rx_ctl_host(**dict(base, out=o, **kw))
        assert e.value.errno == errno.EINVAL, kw

    g.tcp_rx_ctl_host(**dict(base, out=cc.blank(m)))
    for f in ("verdict", "sflags", "rcv_nxt_after", "ev", "rst_seq", "sock", "conn", "addr"):
        refused(**{f: None})
    for f in ("desc", "frame_off", "seg_conn", "seg_kind", "seg_src", "totals"):
        refused(out={f: None})
    odd = np.zeros(4 * m + 8, dtype=np.uint8)
    refused(rst_seq=odd[1:])
    refused(frame_stride=53)
    refused(blocks=tc.MAX_BLOCKS + 1)
    big = (1 << 20) + 1
    refused(nconn=big, conn=np.zeros(big, dtype=case["conn"].dtype), addr=np.zeros(big, dtype=tc.ADDR))
