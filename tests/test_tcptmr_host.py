"""CPU: gcl_tcp_tick_host and gcl_tcp_rx_acks_host (csrc/gcl_host.c with the
rules of csrc/gcl_tcptmr.h that the GPU kernels share) against the line-by-line
transcription of tcp_handle_timeouts, tcp_timer_update, tcp_tx_ack and
tcp_tx_probe_window in tests/tcptmrcases.py: every output byte of the named
cases and of random sweeps, sentinel-filled outputs with guards, the counters,
the struct layouts, every -EINVAL, and the header bytes gcl_tx_hdr_host writes
from the descriptors against the reference's own tcp_push_tcphdr
(tests/golden/tcpctl_ref.json)."""
import ctypes
import errno
import importlib.util
import os

import numpy as np
import pytest

from tests import tcprxcases as rc
from tests import tcptmrcases as tm


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def check(g, case, what):
    want = tm.model(case)
    got, cnt = tm.run_host(g, case)
    tm.compare(got, want, len(case["tmr"]), case["seg_cap"], what)
    assert cnt.tolist() == want["counts"].tolist(), what
    return want


@pytest.mark.parametrize("name", sorted(tm.cases()))
def test_named_cases(g, name):
    check(g, tm.cases()[name], name)


def test_named_cases_say_what_their_names_say():
    """the model's own answers for the named cases: the cases test what they claim"""
    w = {k: tm.model(c) for k, c in tm.cases().items()}
    act = {k: v["out_tmr"]["action"].tolist() for k, v in w.items()}
    nt = {k: v["out_tmr"]["next_timeout"].tolist() for k, v in w.items()}
    F, NOW = tm.A_FIRED, tm.NOW
    for k in ("not_live", "not_due", "next_timeout_max"):
        assert act[k] == [0] and w[k]["out_tmr"]["flags"][0] == tm.cases()[k]["tmr"]["flags"][0], k
        assert nt[k] == tm.cases()[k]["tmr"]["next_timeout"].tolist(), k
    assert act["due_exactly"] == [F | tm.A_ACK]
    assert act["closed"] == [F] and nt["closed"] == [NOW] and w["closed"]["out_tmr"]["state"][0] == tm.CLOSED
    assert act["connect_fail"] == [F | tm.A_FAIL] and w["connect_fail"]["out_tmr"]["state"][0] == tm.CLOSED
    assert nt["connect_fail"] == [NOW] and w["connect_fail"]["out_tmr"]["flags"][0] & tm.ACK_DELAYED
    assert act["time_wait_close"] == [F | tm.A_CLOSE] and w["time_wait_close"]["out_tmr"]["state"][0] == tm.CLOSED
    assert act["nothing_to_do"] == [F] and nt["nothing_to_do"] == [tm.M64]
    assert act["ack_at"] == [F | tm.A_ACK] and act["ack_before"] == [F]
    assert nt["ack_at"] == [tm.M64] and nt["ack_before"] == [NOW + 1]
    assert act["zero_wnd_at"] == [F | tm.A_PROBE] and act["zero_wnd_before"] == [F]
    assert nt["zero_wnd_at"] == [NOW + tm.TCP_ZERO_WND_TIMEOUT] and nt["zero_wnd_before"] == [NOW + 1]
    assert w["zero_wnd_at"]["out_tmr"]["zero_wnd_ts"][0] == NOW
    assert act["retransmit_at"] == [F | tm.A_RETRANSMIT] and act["retransmit_before"] == [F]
    assert act["connect_at"] == [F | tm.A_FAIL] and act["connect_before"] == [F] and nt["connect_before"] == [NOW + 1]
    assert act["time_wait_at"] == [F | tm.A_CLOSE] and act["time_wait_before"] == [F]
    assert nt["time_wait_before"] == [NOW + 1]
    assert act["ack_ts_ahead"] == [F | tm.A_ACK] and act["zero_wnd_ts_ahead"] == [F | tm.A_PROBE]
    assert act["txq_ts_ahead"] == [F | tm.A_RETRANSMIT] and act["attach_ts_ahead"] == [F | tm.A_FAIL]
    assert act["time_wait_ts_ahead"] == [F | tm.A_CLOSE]
    assert act["now_max"] == [F | tm.A_ACK] and nt["now_max"] == [tm.TCP_OOQ_ACK_TIMEOUT - 1]     # now + T wraps
    assert nt["syn_sent_override"] == [NOW - 1000 + tm.TCP_CONNECT_TIMEOUT]
    assert nt["syn_received_override_min"] == [NOW - 3 + tm.TCP_ACK_TIMEOUT]
    assert nt["time_wait_timer"] == [NOW - 1000 + tm.TCP_TIME_WAIT_TIMEOUT]
    assert act["tx_exclusive_masks"] == [F, F | tm.A_RETRANSMIT]
    assert nt["tx_exclusive_masks"] == [tm.M64, NOW - 9]
    assert nt["txq_clear_ignores_ts"] == [tm.M64]
    assert act["ooo_forces_ack"] == [F | tm.A_ACK] and nt["ooo_forces_ack"] == [NOW + tm.TCP_OOQ_ACK_TIMEOUT]
    assert nt["ooo_and_later_terms"] == [NOW - 10 + tm.TCP_ZERO_WND_TIMEOUT, NOW + tm.TCP_OOQ_ACK_TIMEOUT]
    assert act["ack_and_probe"] == [F | tm.A_ACK | tm.A_PROBE]
    assert w["ack_and_probe"]["seg_kind"].tolist() == [tm.K_ACK, tm.K_PROBE]
    assert act["all_at_once"] == [F | tm.A_ACK | tm.A_PROBE | tm.A_RETRANSMIT]
    assert w["unknown_flag_bits_kept"]["out_tmr"]["flags"][0] == 0xC0 | tm.LIVE
    assert w["win_over_16_bits"]["desc"]["win"][0] == (0x12345678 >> 3) & 0xFFFF != 0x12345678 >> 3
    assert w["wscale0"]["desc"]["win"].tolist() == [0xFFFF] * 2 and w["wscale14"]["desc"]["win"].tolist() == [0xFFFF] * 2
    assert w["probe_seq_una0"]["desc"]["seq"].tolist() == [tm.M32]
    assert w["seq_wraps"]["desc"]["seq"].tolist() == [tm.M32] and w["seq_wraps"]["desc"]["ack"][0] == 0x80000000
    N = tm.A_NOSPACE
    both = F | tm.A_ACK | tm.A_PROBE
    assert act["cap_between_ack_and_probe"] == [both, both | N, both | N]
    assert w["cap_between_ack_and_probe"]["seg_kind"].tolist() == [0, 1, 0]
    assert w["cap_between_ack_and_probe"]["totals"].tolist() == [6, 3]
    assert w["cap_between_ack_and_probe"]["out_tmr"]["flags"].tolist() == [tm.LIVE | tm.ZERO_WND] * 3
    assert act["cap_zero"] == [both | N] * 3 and w["cap_zero"]["totals"].tolist() == [6, 0]
    assert act["cap_total_minus_1"] == [both, both, both | N] and act["cap_total"] == [both] * 3
    assert w["mixed"]["seg_conn"].tolist() == [1, 4, 6, 6] and w["mixed"]["seg_kind"].tolist() == [0, 1, 0, 1]
    assert w["mixed"]["counts"].tolist() == [5, 2, 2, 1, 1, 0, 0, 4]
    assert w["nconn_zero"]["totals"].tolist() == [0, 0]
    d = w["ack_and_probe"]["desc"]
    assert d["proto"].tolist() == [6, 6] and d["tcp_flags"].tolist() == [0x10] * 2 and d["tcp_off"].tolist() == [5] * 2
    assert d["seq"].tolist() == [5000, 999] and d["ack"].tolist() == [100, 100] and d["paylen"].tolist() == [0, 0]


@pytest.fixture(scope="module")
def sweeps():
    return [tm.random_case(1, 3000), tm.random_case(2, 777, due=0.1, seg_cap=40), tm.random_case(3, 1, due=1.0),
            tm.random_case(4, 2000, due=1.0, seg_cap=1500)]


def test_random_sweeps(g, sweeps):
    seen = 0
    for k, case in enumerate(sweeps):
        want = check(g, case, f"sweep {k}")
        seen |= int(np.bitwise_or.reduce(want["out_tmr"]["action"]))
    assert seen == 0x7F


def test_counts_accumulate_and_may_be_null(g):
    case = tm.cases()["mixed"]
    got, _ = tm.run_host(g, case, counts=False)
    tm.compare(got, tm.model(case), 7, case["seg_cap"], "no counts")
    cnt = np.zeros(tm.NR, dtype=np.uint64)
    for _ in range(2):
        g.tcp_tick_host(case["now"], case["tmr"], case["conn"], case["addr"], case["seg_cap"], counts=cnt)
    assert cnt.tolist() == (2 * tm.model(case)["counts"]).tolist()


def test_struct_sizes_and_offsets(g):
    assert ctypes.sizeof(g.GclTickIn) == 64 and ctypes.sizeof(g.GclTickOut) == 56
    assert ctypes.sizeof(g.GclRxackIn) == 104 and ctypes.sizeof(g.GclCtlsegOut) == 48
    assert [getattr(g.GclTickIn, f).offset for f in ("size", "blocks", "now", "tmr", "conn", "addr", "nconn",
                                                     "frame_stride", "seg_cap", "frame_base")] == \
        [0, 4, 8, 16, 24, 32, 40, 44, 48, 56]
    assert [getattr(g.GclRxackIn, f).offset for f in ("order", "m", "n", "sock", "verdict", "sflags",
                                                      "rcv_nxt_after", "conn", "addr", "nconn", "frame_stride",
                                                      "seg_cap", "frame_base")] == \
        [8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88, 96]
    assert g.GclTickOut.seg.offset == 8 and g.GclCtlsegOut.totals.offset == 40
    for mine, theirs in ((tm.TMR, g.TCP_TMR_DTYPE), (tm.TMR_OUT, g.TCP_TMR_OUT_DTYPE), (tm.ADDR, g.TCP_ADDR_DTYPE),
                         (tm.DESC, g.TXH_DESC_DTYPE)):
        assert mine == theirs
    assert tm.TMR.itemsize == 64 and [tm.TMR.fields[f][1] for f in ("txq_ts", "state", "flags", "pad")] == \
        [40, 48, 49, 50]
    assert tm.TMR_OUT.itemsize == 32 and [tm.TMR_OUT.fields[f][1] for f in ("zero_wnd_ts", "state", "flags", "action",
                                                                            "pad")] == [8, 16, 17, 18, 19]
    assert tm.ADDR.itemsize == 16 and [tm.ADDR.fields[f][1] for f in ("rip", "lport", "rport", "rcv_wscale")] == \
        [4, 8, 10, 12]
    for k, v in (("TMR_LIVE", tm.LIVE), ("TMR_OOO", tm.OOO), ("TMRA_NOSPACE", tm.A_NOSPACE), ("CTL_PROBE", tm.K_PROBE),
                 ("TICKC_SEGS", tm.C_SEGS), ("RXACKC_SKIPPED", tm.C_SKIPPED), ("TICK_MAX_BLOCKS", tm.MAX_BLOCKS),
                 ("TICK_MAX_CONN", tm.MAX_CONN), ("CTL_MIN_STRIDE", tm.MIN_STRIDE), ("TICK_TILE", tm.TILE),
                 ("TCP_STATE_TIME_WAIT", tm.TIME_WAIT), ("TCP_STATE_CLOSED", tm.CLOSED)):
        assert getattr(g, k) == v, k


def test_error_returns(g):
    case = tm.cases()["mixed"]
    nconn, cap = 7, case["seg_cap"]
    out = tm.blank(nconn, cap)
    ok = dict(now=case["now"], tmr=case["tmr"], conn=case["conn"], addr=case["addr"], seg_cap=cap, out=out)
    g.tcp_tick_host(**ok)

    def refused(**kw):
        with pytest.raises(OSError) as e:
            g.tcp_tick_host(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(frame_stride=53)
    g.tcp_tick_host(**dict(ok, frame_stride=54))
    refused(blocks=tm.MAX_BLOCKS + 1)
    refused(seg_cap=(1 << 31) + 1, out=dict(out, **{f: None for f in g.CTLSEG_SEG_FIELDS}))
    for f in out:
        refused(out=dict(out, **{f: None}))
    for f in ("tmr", "conn", "addr"):
        refused(**{f: None, "nconn": nconn})
    odd = np.zeros(4096, dtype=np.uint8)
    for f in ("tmr", "conn", "addr"):
        refused(**{f: odd[8:], "nconn": nconn})
    refused(out=dict(out, out_tmr=odd[8:]))
    refused(out=dict(out, desc=odd[8:]))
    refused(out=dict(out, frame_off=odd[4:]))
    refused(out=dict(out, seg_conn=odd[2:]))
    refused(out=dict(out, seg_src=odd[1:]))
    refused(out=dict(out, totals=odd[4:]))
    refused(counts=np.zeros(9, dtype=np.uint64).view(np.uint8)[4:68])
    # the per-segment arrays may be NULL when there is nothing to write to them
    none = dict(out, **{f: None for f in g.CTLSEG_SEG_FIELDS})
    g.tcp_tick_host(**dict(ok, seg_cap=0, out=none))
    g.tcp_tick_host(**dict(ok, nconn=0, tmr=None, conn=None, addr=None, out=dict(none, out_tmr=None)))
    tin, tout = g._tick_structs(case["now"], case["tmr"], case["conn"], case["addr"], nconn, cap, 0, 64, 0, out, None)
    assert g.lib.gcl_tcp_tick_host(ctypes.byref(tin), ctypes.byref(tout), None) == 0
    assert g.lib.gcl_tcp_tick_host(None, ctypes.byref(tout), None) == -errno.EINVAL
    assert g.lib.gcl_tcp_tick_host(ctypes.byref(tin), None, None) == -errno.EINVAL
    tin.size = 56
    assert g.lib.gcl_tcp_tick_host(ctypes.byref(tin), ctypes.byref(tout), None) == -errno.EINVAL
    tin.size, tin.nconn = ctypes.sizeof(g.GclTickIn), tm.MAX_CONN + 1
    assert g.lib.gcl_tcp_tick_host(ctypes.byref(tin), ctypes.byref(tout), None) == -errno.EINVAL
    need = ctypes.c_size_t()
    assert g.lib.gcl_tcp_tick_workspace(tm.MAX_CONN + 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_tick_workspace(1, tm.MAX_BLOCKS + 1, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_tick_workspace(1, 0, None) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_acks_workspace((1 << 31) + 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_acks_workspace(1, tm.MAX_BLOCKS + 1, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_acks_workspace(1, 0, None) == -errno.EINVAL
    assert g.tcp_tick_workspace(tm.MAX_CONN) == 4 * tm.MAX_BLOCKS and g.tcp_tick_workspace(5, 3) == 16
    assert g.tcp_rx_acks_workspace(1 << 31) == 4 * tm.MAX_BLOCKS


# ---------------------------------------------------------------- the ACKs of a gcl_tcp_rx call
def rx_outputs(g, rx):
    """gcl_tcp_rx_host's outputs for the tests/tcprxcases.py case @rx, cut to their m entries"""
    got, _ = rc.run_host(g, rx)
    m = len(rx["pkt_len"]) if rx.get("order") is None else len(rx["order"])
    return {f: got[f][:m].copy() for f, _ in rc.ENTRY}


def check_rxack(g, rx, rxout, addr, seg_cap, what, **kw):
    want = tm.rxack_model(rx, rxout, addr, seg_cap, kw.get("frame_base", 0), kw.get("frame_stride", 64))
    got, cnt = tm.run_rxack_host(g, rx, rxout, addr, seg_cap, **kw)
    tm.compare(got, want, 0, seg_cap, what)
    assert cnt.tolist() == want["counts"].tolist(), what
    return want


@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_rx_acks_of_the_named_rx_cases(g, name):
    rx = rc.cases()[name]
    rxout = rx_outputs(g, rx)
    want = check_rxack(g, rx, rxout, tm.random_addr(5, len(rx["conn"])), len(rxout["verdict"]) + 2, name)
    assert int(want["totals"][0]) == int((rxout["sflags"] & rc.SF_ACK_NOW != 0).sum())


def test_rx_acks_of_random_streams(g):
    for k, (seed, m, nconn) in enumerate(((1, 4096, 300), (2, 3000, 37), (3, 4096, 1))):
        rx = rc.random_case(seed, m, nconn)
        if k == 1:
            plan = np.argsort(rx["sock"] % 3, kind="stable")
            rx = dict(rx, order=np.concatenate([plan, np.arange(100)]).astype(np.uint32))
        rxout = rx_outputs(g, rx)
        addr = tm.random_addr(seed, nconn)
        want = check_rxack(g, rx, rxout, addr, len(rxout["verdict"]), f"stream {k}", frame_base=12345,
                           frame_stride=54)
        total = int(want["totals"][0])
        # one connection stops at its first fault: its stream carries few ACKs by nature
        assert total > (20 if k == 2 else 200) and want["counts"][tm.C_SKIPPED] == 0
        # the ack numbers are the model of gcl_tcp_rx's own, in list order
        acks = rc.model(rx)["rcv_nxt_after"][rxout["sflags"] & rc.SF_ACK_NOW != 0]
        assert want["desc"]["ack"].tolist() == acks.tolist()
        for cap in (0, 1, total - 1):
            check_rxack(g, rx, rxout, addr, cap, f"stream {k} cap {cap}")


def test_rx_acks_guards_emit_nothing(g):
    """verdict and sflags that ask for an ACK everywhere over an order and a
    sock that point outside: no segment, nothing read or written out of bounds"""
    rx = rc.random_case(6, 500, 9)
    m, n = 700, 500
    rng = np.random.default_rng(7)
    rx = dict(rx, order=rng.integers(0, n + 50, size=m).astype(np.uint32), sock=rx["sock"].copy())
    rx["sock"][::3] = rng.integers(9, 1 << 32, size=len(rx["sock"][::3]), dtype=np.uint64)
    rxout = dict(verdict=np.full(m, rc.FAST, dtype=np.uint8), sflags=np.full(m, 0xFF, dtype=np.uint8),
                 rcv_nxt_after=rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32),
                 copy_len=rng.integers(0, 1460, size=m).astype(np.uint16))
    # where an entry does name a connection, rcv_nxt_after continues that connection's chain, as gcl_tcp_rx's does
    nxt = rx["conn"]["rcv_nxt"].astype(np.uint64)
    for j in range(m):
        i = int(rx["order"][j])
        if i < n and rx["sock"][i] < 9:
            c = int(rx["sock"][i])
            nxt[c] = (nxt[c] + np.uint64(rxout["copy_len"][j])) & np.uint64(tm.M32)
            rxout["rcv_nxt_after"][j] = nxt[c]
    want = check_rxack(g, rx, rxout, tm.random_addr(8, 9), m, "hostile")
    assert 0 < want["counts"][tm.C_SKIPPED] < m and want["counts"][tm.C_WANTED] + want["counts"][tm.C_SKIPPED] == m
    rx["sock"][:] = 9
    want = check_rxack(g, rx, rxout, tm.random_addr(8, 9), m, "all skipped")
    assert want["totals"].tolist() == [0, 0] and want["counts"][tm.C_SKIPPED] == m
    rxout["sflags"][:] = 0xFF & ~rc.SF_ACK_NOW
    assert check_rxack(g, rx, rxout, tm.random_addr(8, 9), m, "none asked")["counts"].tolist() == [0] * tm.NR


def test_rx_acks_error_returns(g):
    rx = rc.cases()["two_interleaved"]
    rxout = rx_outputs(g, rx)
    addr = tm.random_addr(5, 2)
    out = tm.blank(0, 8, tick=False)
    ok = dict(verdict=rxout["verdict"], sflags=rxout["sflags"], rcv_nxt_after=rxout["rcv_nxt_after"], sock=rx["sock"],
              conn=rx["conn"], addr=addr, seg_cap=8, out=out)
    g.tcp_rx_acks_host(**ok)

    def refused(**kw):
        with pytest.raises(OSError) as e:
            g.tcp_rx_acks_host(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(frame_stride=0)
    refused(blocks=tm.MAX_BLOCKS + 1)
    refused(seg_cap=(1 << 31) + 1, out=dict(out, **{f: None for f in g.CTLSEG_SEG_FIELDS}))
    for f in out:
        refused(out=dict(out, **{f: None}))
    for f in ("verdict", "sflags", "rcv_nxt_after"):
        refused(**{f: None, "m": 6})
    refused(sock=None, n=6)
    refused(conn=None, nconn=2)
    refused(addr=None, nconn=2)
    odd = np.zeros(4096, dtype=np.uint8)
    refused(order=odd[2:], m=6)
    refused(sock=odd[1:], n=6)
    refused(rcv_nxt_after=odd[2:], m=6)
    refused(conn=odd[8:], nconn=2)
    refused(addr=odd[8:], nconn=2)
    refused(out=dict(out, desc=odd[8:]))
    refused(counts=np.zeros(9, dtype=np.uint64).view(np.uint8)[4:68])
    rin, rout = g._rxack_structs(rxout["verdict"], rxout["sflags"], rxout["rcv_nxt_after"], rx["sock"], rx["conn"],
                                 addr, 6, 6, 2, None, 8, 0, 64, 0, out, None)
    assert g.lib.gcl_tcp_rx_acks_host(ctypes.byref(rin), ctypes.byref(rout), None) == 0
    assert g.lib.gcl_tcp_rx_acks_host(None, ctypes.byref(rout), None) == -errno.EINVAL
    assert g.lib.gcl_tcp_rx_acks_host(ctypes.byref(rin), None, None) == -errno.EINVAL
    rin.size = 96
    assert g.lib.gcl_tcp_rx_acks_host(ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    rin.size, rin.nconn = ctypes.sizeof(g.GclRxackIn), tm.MAX_CONN + 1
    assert g.lib.gcl_tcp_rx_acks_host(ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    rin.nconn, rin.m = 2, (1 << 31) + 1
    assert g.lib.gcl_tcp_rx_acks_host(ctypes.byref(rin), ctypes.byref(rout), None) == -errno.EINVAL
    # m == 0 still writes totals, and needs no array
    out = tm.blank(0, 0, tick=False)
    g.tcp_rx_acks_host(None, None, None, None, None, None, 0, m=0, n=0, nconn=0,
                       out=dict(out, **{f: None for f in g.CTLSEG_SEG_FIELDS}))
    assert out["totals"][:2].tolist() == [0, 0]


# ---------------------------------------------------------------- the reference's own header bytes
def _generator():
    path = os.path.join(os.path.dirname(tm.GOLDEN), "make_tcpctl_ref.py")
    spec = importlib.util.spec_from_file_location("make_tcpctl_ref", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_headers_are_what_the_reference_gives():
    """Where oracle/_ref is built, the generator's result in memory equals the
    committed file, text and all."""
    from oracle import orc
    if orc.ref_tcpout() is None:
        pytest.skip("oracle/_ref/libtcpout_ref.so not built (no reference tree)")
    gen = _generator()
    fresh = gen.build()
    assert fresh == tm.load_golden()
    with open(tm.GOLDEN) as f:
        assert f.read() == gen.dumps(fresh)


def test_golden_holds_every_edge():
    d = tm.load_golden()
    assert os.path.getsize(tm.GOLDEN) <= 64 * 1024
    segs = d["segs"]
    assert [{k: v for k, v in r.items() if k != "tcphdr"} for r in segs] == tm.golden_inputs()
    assert {r["kind"] for r in segs} == {tm.K_ACK, tm.K_PROBE}
    assert any(r["rcv_wnd"] >> r["wscale"] > 0xFFFF for r in segs)
    assert {0, 14} <= {r["wscale"] for r in segs}
    assert any(r["kind"] == tm.K_PROBE and r["seq"] == tm.M32 for r in segs)
    for r in segs:
        h = bytes.fromhex(r["tcphdr"])
        assert len(h) == 20 and h[12] == 0x50 and h[13] == 0x10


def test_descriptors_give_the_references_header_bytes(g):
    """gcl_tx_hdr_host over the sweep's descriptors writes, as bytes 34-53 of
    each frame, what the reference's tcp_push_tcphdr wrote for that ACK or
    probe."""
    segs = tm.load_golden()["segs"]
    at = 0
    net = g.txh_net(tm.NET["addr"], tm.NET["netmask"], tm.NET["gateway"], tm.NET["mac"])
    for name in sorted(tm.cases()):
        case = tm.cases()[name]
        got, _ = tm.run_host(g, case)
        k = int(got["totals"][1])
        if k == 0:
            continue
        stride = case["frame_stride"]
        frames = np.full(k * stride, tm.SENTINEL, dtype=np.uint8)
        off = np.arange(k, dtype=np.uint64) * np.uint64(stride)
        out = g.tx_hdr_host(got["desc"][:k].copy(), off, frames, net)
        assert (out["status"][:k] != g.TXH_REFUSED).all() and (out["pkt_len"][:k] == 54).all(), name
        for j in range(k):
            r = segs[at + j]
            assert (r["case"], r["k"]) == (name, j)
            assert frames[j * stride + 34:j * stride + 54].tobytes().hex() == r["tcphdr"], (name, j)
        at += k
    assert at == len(segs) > 30
