"""CPU: what gcl_tcp_rx_full_host writes, fed to the calls behind it.
gcl_tcp_rx_acks_host takes verdict, sflags and rcv_nxt_after unchanged and
must send one ACK per ACK_NOW entry with the model's rcv_nxt and window;
gcl_copy_batch_host takes copy_len and dst_off and must leave in every
connection's region the bytes the model appended to rxq."""
import numpy as np
import pytest

from tests import paycases as pc
from tests import tcprxfcases as fc
from tests import tcptmrcases as tc


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def expected_acks(case, want, addr):
    """(list position, ack, win) of every ACK the model's do_ack sends: tcp_tx_ack with the PCB as it
    stands after the segment, the window being what is left of rcv_wnd after the accepted bytes"""
    order, conn, res = case.get("order"), case["conn"], []
    for j in np.nonzero((want["verdict"] == fc.FAST) & (want["sflags"] & fc.SF_ACK_NOW != 0))[0]:
        c = int(case["sock"][j if order is None else int(order[j])])
        after = int(want["rcv_nxt_after"][j])
        wnd = (int(conn[c]["rcv_wnd"]) - ((after - int(conn[c]["rcv_nxt"])) & fc.M32)) & fc.M32
        res.append((int(j), after, (wnd >> int(addr[c]["rcv_wscale"])) & 0xFFFF, c))
    return res


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_acks_of_the_call(g, name):
    case = fc.case_of(name)
    m, nconn = fc.dims(case)
    want = fc.model(case)
    got, _ = fc.run_host(g, case)
    addr = tc.random_addr(3, max(nconn, 1))[:nconn]
    rxout = {f: got[f][:m] for f in ("verdict", "sflags", "rcv_nxt_after", "copy_len")}
    acks, cnt = tc.run_rxack_host(g, case, rxout, addr, m + 1)
    exp = expected_acks(case, want, addr)
    assert int(acks["totals"][1]) == len(exp) == int(want["counts"][fc.C_ACKS])
    for k, (j, ack, win, c) in enumerate(exp):
        d = acks["desc"][k]
        assert (int(acks["seg_src"][k]), int(d["ack"]), int(d["win"]), int(acks["seg_conn"][k])) == (j, ack, win, c)
        assert int(d["seq"]) == int(case["conn"][c]["snd_nxt"])
    # and the whole segments, as the model of gcl_tcp_rx_acks builds them from the MODEL's outputs
    ref = tc.rxack_model(case, {f: want[f] for f in rxout}, addr, m + 1, 0, 64)
    tc.compare(acks, ref, nconn, m + 1, name)


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_copy_of_the_call(g, name):
    case = fc.case_of(name)
    m, nconn = fc.dims(case)
    want = fc.model(case, with_rxq=True)
    got, _ = fc.run_host(g, case)
    pay = pc.model(case, case.get("order"), case["sock"], case.get("st"))
    total = int(want["conn_off"][nconn])
    rx = np.full(total + 64, fc.SENTINEL, dtype=np.uint8)
    if m:
        g.copy_batch_host(case["frames"], pay["src_off"].astype(np.uint64), got["copy_len"][:m].copy(), rx[:total],
                          dst_off=got["dst_off"][:m].copy(), n=m, src_len=case["frames_len"], dst_len=total,
                          olflags=False, rss=False)
    for c in range(nconn):
        o = int(want["conn_off"][c])
        assert rx[o:o + len(want["rxq"][c])].tobytes() == want["rxq"][c], (name, c)
    assert (rx[total:] == fc.SENTINEL).all()
    assert sum(len(s) for s in want["rxq"]) == int(want["counts"][fc.C_BYTES])
