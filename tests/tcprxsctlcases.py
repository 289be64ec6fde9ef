"""What the CPU and GPU tests of gcl_tcp_rx_ctl (include/gclassify.h) share:
the connections' addresses, the segments a gcl_tcp_rx_states call asks for as
read off the reference's trace (tests/golden/tcprxs_ref.json: tcp_tx_ack,
tcp_tx_raw_rst, tcp_tx_raw_rst_ack), and sentinel-filled outputs."""
import numpy as np

from tests import tcprxrefcases as rr
from tests import tcprxscases as sc
from tests import tcprxsrefcases as sr
from tests import tcptmrcases as tc
from tests.tcprxcases import M32

K_ACK, K_RST, K_RST_ACK = 0, 2, 3
SENTINEL, GUARD = sc.SENTINEL, sc.GUARD
SEG = (("desc", tc.DESC), ("frame_off", np.uint64), ("seg_conn", np.uint32), ("seg_kind", np.uint8),
       ("seg_src", np.uint32))
STRIDE, BASE = 64, 4096


def addrs(nconn):
    return tc.records([tc.addr1(k) for k in range(nconn)], tc.ADDR, M32)


def blank(seg_cap):
    b = {f: np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (seg_cap + GUARD)), dtype=dt).copy()
         for f, dt in SEG}
    b["totals"] = np.frombuffer(bytes([SENTINEL]) * (8 * (2 + GUARD)), dtype=np.uint64).copy()
    return b


def same(got, want, wrote, what):
    """two sentinel-filled output sets: the first @wrote segments and totals equal, everything behind untouched"""
    for f, dt in SEG:
        assert got[f][:wrote].tobytes() == want[f][:wrote].tobytes(), (what, f)
        assert (got[f][wrote:].view(np.uint8) == SENTINEL).all(), (what, f, "written past the segments")
    assert got["totals"][:2].tolist() == want["totals"][:2].tolist(), (what, "totals")
    assert (got["totals"][2:].view(np.uint8) == SENTINEL).all(), (what, "totals guard")


def run_host(g, case, rx, seg_cap, ev=None, counts=True, acks=False):
    """gcl_tcp_rx_ctl_host (or with @acks gcl_tcp_rx_acks_host) over the outputs @rx of a gcl_tcp_rx_states call"""
    m, nconn = len(case["sock"]), len(case["conn"])
    out = blank(seg_cap)
    cnt = np.full(8, 5, dtype=np.uint64) if counts else None
    args = dict(frame_stride=STRIDE, frame_base=BASE, order=case.get("order"), m=m, n=len(case["pkt_len"]),
                nconn=nconn, out=out, counts=cnt)
    if acks:
        g.tcp_rx_acks_host(rx["verdict"], rx["sflags"], rx["rcv_nxt_after"], case["sock"], case["conn"],
                           addrs(nconn), seg_cap, **args)
    else:
        g.tcp_rx_ctl_host(rx["verdict"], rx["sflags"], rx["rcv_nxt_after"], rx["ev"] if ev is None else ev,
                          rx["rst_seq"], case["sock"], case["conn"], addrs(nconn), seg_cap, **args)
    return out, None if cnt is None else cnt - np.uint64(5)


def wanted(name):
    """(j, kind, seq, ack) of the segments the reference sent for the recorded case @name, in list order, up to
    and with each connection's first FAIL or PUT; seq of an ACK is the connection's snd_nxt"""
    case, tr = sr.case_of(name), sr.traces(name)
    segs = rr.segments(case)
    res = []
    for k, rows in tr.items():
        for sg, t in zip(segs[k], rows):
            if t["tx_ack"]:
                res.append((sg["j"], K_ACK, int(case["conn"][k]["snd_nxt"]), t["rcv_nxt"]))
            elif t["rst_kind"] == 1:
                res.append((sg["j"], K_RST, t["rst_seq"], 0))
            elif t["rst_kind"] == 2:
                res.append((sg["j"], K_RST_ACK, 0, t["rst_ack"]))
            if t["fail_err"] or (t["new_state"] and t["new_state"] - 1 == sc.CLOSED):
                break
    return sorted(res)


def check_against_reference(got, name, what):
    want = wanted(name)
    assert int(got["totals"][0]) == len(want), (what, name, int(got["totals"][0]), len(want))
    case = sr.case_of(name)
    for k, (j, kind, seq, ack) in enumerate(want[:int(got["totals"][1])]):
        d, c = got["desc"][k], int(case["sock"][j])
        assert (int(got["seg_src"][k]), int(got["seg_kind"][k]), int(d["seq"]), int(d["ack"])) == (j, kind, seq, ack), \
            (what, name, k)
        assert int(got["seg_conn"][k]) == c and int(got["frame_off"][k]) == BASE + k * STRIDE, (what, name, k)
        a = tc.addr1(c)
        assert (int(d["lip"]), int(d["rip"]), int(d["lport"]), int(d["rport"]), int(d["proto"]), int(d["tcp_off"])) == \
            (a["lip"], a["rip"], a["lport"], a["rport"], 6, 5), (what, name, k)
        assert int(d["tcp_flags"]) == {K_ACK: 0x10, K_RST: 0x04, K_RST_ACK: 0x14}[kind], (what, name, k)
    return len(want)
