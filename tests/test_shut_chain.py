"""gcl_tcp_shut_host chained with the host twins of the calls around it: the
state, the timer flags, snd_nxt and the FIN's queue record it writes go into
gcl_tcp_txq_host, gcl_tcp_rx_states_host and gcl_tcp_tick_host as they are.

Active close: shutdown(SHUT_WR) on an ESTABLISHED connection -> FIN_WAIT1 and a
FIN record; the record is retransmitted at now + RTO with the same seq and
flags 0x11; the peer's ACK of snd_nxt -> FIN_WAIT2; the peer's FIN -> TIME_WAIT;
the timer sweep expires it.  Passive close: tcp_close from CLOSE_WAIT ->
LAST_ACK; the peer's ACK -> CLOSED with GCL_TCPS_PUT.  tcp_abort: CLOSED at
once, and the sweep and the receive side leave the connection alone."""
import numpy as np

from caladan_amd import gclassify as G
from tests import shutcases as T
from tests import tcprxcases as rc
from tests import tcprxscases as sc

RTO = 300000
A, F = sc.A, sc.F


def one(op, how, state, c, **kw):
    """the batch of one connection whose PCB words are the dict @c, and its out_conn after the call"""
    s, t, _, a = T.conn(op=op, how=how, state=state, **kw)
    b = T.Batch(arrays=[np.array([s]), np.array([t]), rc.conns([c]), np.array([a])])
    got = b.run_host(1)
    T.check(b, got, b.expect(1))
    oc = np.frombuffer(T.raw(got["out_conn"], 48), dtype=G.SHUT_CONN_OUT_DTYPE)[0]
    return b, got, oc


def rx(c, state, segs):
    """gcl_tcp_rx_states_host over @segs for the one connection @c entering in @state"""
    case = sc.build([c], segs, state=np.array([state], dtype=np.uint8))
    out, _ = sc.run_host(G, case)
    return out


def fin_record(got):
    ent = np.frombuffer(T.raw(got["txq_ent"], 16), dtype=G.TXQ_ENT_DTYPE).copy()
    cold = np.frombuffer(T.raw(got["txq_cold"], 16), dtype=G.TXQ_COLD_DTYPE).copy()
    return ent, cold


def retransmit(b, c, ent, cold, when):
    cold = cold.copy()
    cold["flags"] &= 0xFF ^ G.TXQE_INFLIGHT       # the NIC is done with the first transmission
    return G.tcp_txq_host(when, np.array([0, 1], dtype=np.uint32), ent, cold, rc.conns([c]), b.addr, 4,
                          want=np.array([G.TXQ_W_RTO], dtype=np.uint8))


def test_active_close():
    rng = np.random.default_rng(1)
    c = rc.conn1(snd_una=5000, snd_nxt=5000)
    b, got, oc = one(G.SHUT_OP_SHUTDOWN, 1, T.ESTABLISHED, c, snd_nxt=5000, rcv_nxt=100)
    assert (oc["status"], oc["state"], oc["snd_nxt"], oc["nseg"]) == (G.SHUTS_DONE, T.FIN_WAIT1, 5001, 1)
    assert oc["tmr_flags"] & G.TMR_TXQ and oc["txq_ts"] == T.NOW and oc["next_timeout"] == T.NOW + RTO
    ent, cold = fin_record(got)
    assert (ent["seg_seq"][0], ent["seg_end"][0], ent["ts"][0]) == (5000, 5001, T.NOW)
    assert (cold["tcp_flags"][0], cold["tcp_off"][0], cold["flags"][0]) == (0x11, 5, G.TXQE_INFLIGHT)

    c = dict(c, snd_nxt=int(oc["snd_nxt"]))
    q = retransmit(b, c, ent, cold, int(oc["next_timeout"]))
    assert q["totals"][:2].tolist() == [1, 1] and q["state"][0] & 0x7F == G.TXQS_RETX
    assert (q["desc"][0]["seq"], q["desc"][0]["tcp_flags"], q["desc"][0]["paylen"]) == (5000, 0x11, 0)
    assert q["frame_off"][0] == cold["frame_off"][0]
    early = retransmit(b, c, ent, cold, int(oc["next_timeout"]) - 1)
    assert early["totals"][0] == 0                                # not before the timeout this call armed

    out = rx(c, int(oc["state"]), [sc.seg(rng, 0, 100, 0, ack=5001)])
    assert out["state_out"][0] == T.FIN_WAIT2 and out["ev"][0] & sc.EV_STATE
    c = dict(c, snd_una=5001)
    out = rx(c, int(out["state_out"][0]), [sc.seg(rng, 0, 100, 0, ack=5001, flags=A | F)])
    assert out["state_out"][0] == T.TIME_WAIT and out["ev"][0] & sc.EV_FIN
    assert out["out_ext"][0]["xflags"] & sc.X_TIMEWAIT

    tmr = b.tmr.copy()
    tmr["state"], tmr["flags"] = out["state_out"][0], oc["tmr_flags"] & (0xFF ^ G.TMR_TXQ)     # the FIN was acked
    tmr["time_wait_ts"], tmr["next_timeout"] = T.NOW + 5, T.NOW + 5 + 1000000
    conn = rc.conns([dict(c, rcv_nxt=101)])
    tick = G.tcp_tick_host(T.NOW + 5 + 999999, tmr, conn, b.addr, 2)
    assert tick["out_tmr"][0]["action"] == 0
    tick = G.tcp_tick_host(T.NOW + 5 + 1000000, tmr, conn, b.addr, 2)
    assert tick["out_tmr"][0]["action"] == G.TMRA_FIRED | G.TMRA_CLOSE and tick["out_tmr"][0]["state"] == T.CLOSED


def test_passive_close():
    rng = np.random.default_rng(2)
    c = rc.conn1(snd_una=5000, snd_nxt=5000, rcv_nxt=101)
    b, got, oc = one(G.SHUT_OP_CLOSE, 0, T.CLOSE_WAIT, c, sflags=G.SHUT_RX_CLOSED, snd_nxt=5000, rcv_nxt=101)
    assert (oc["status"], oc["state"], oc["snd_nxt"], oc["nseg"], oc["nput"]) == (G.SHUTS_DONE, T.LAST_ACK, 5001, 1, 1)
    assert oc["flags"] == G.SHO_POLLHUP | G.SHO_TX_CLOSED_SET | G.SHO_TXWAKE | G.SHO_DETACH_POLL
    assert np.ascontiguousarray(got["seg_kind"]).view(np.uint8)[0] == G.CTL_FIN
    ent, cold = fin_record(got)
    c = dict(c, snd_nxt=int(oc["snd_nxt"]))
    q = retransmit(b, c, ent, cold, int(oc["next_timeout"]))
    assert (q["desc"][0]["seq"], q["desc"][0]["tcp_flags"]) == (5000, 0x11)

    out = rx(c, int(oc["state"]), [sc.seg(rng, 0, 101, 0, ack=5001)])
    assert out["state_out"][0] == T.CLOSED and out["ev"][0] & sc.EV_PUT == G.TCPS_PUT
    assert out["out_ext"][0]["xflags"] & sc.X_PUT


def test_close_of_a_connection_not_yet_established_and_abort():
    rng = np.random.default_rng(3)
    c = rc.conn1(snd_una=5000, snd_nxt=5001)
    for op, state, nput in ((G.SHUT_OP_CLOSE, T.SYN_RECEIVED, 2), (G.SHUT_OP_ABORT, T.ESTABLISHED, 1)):
        b, got, oc = one(op, 0, state, c, snd_nxt=5001, tflags=G.TMR_LIVE | G.TMR_TXQ | G.TMR_OOO)
        assert (oc["status"], oc["state"], oc["err"], oc["nput"], oc["nseg"]) == (G.SHUTS_DONE, T.CLOSED, 103, nput, 1)
        d = np.frombuffer(T.raw(got["desc"], 32), dtype=G.TXH_DESC_DTYPE)[0]
        assert (d["tcp_flags"], d["seq"], d["ack"]) == (0x04, 5001, 0)
        assert np.ascontiguousarray(got["seg_kind"]).view(np.uint8)[0] == G.CTL_RST
        assert not oc["tmr_flags"] & (G.TMR_TXQ | G.TMR_OOO)
        # the sweep at the timeout the fail left: a closed connection fires and does nothing
        tmr = b.tmr.copy()
        tmr["state"], tmr["flags"], tmr["next_timeout"] = oc["state"], oc["tmr_flags"], oc["next_timeout"]
        tick = G.tcp_tick_host(int(oc["next_timeout"]), tmr, b.conn, b.addr, 2)
        assert tick["out_tmr"][0]["action"] == G.TMRA_FIRED and tick["totals"][0] == 0
        # the receive side in CLOSED: the segment changes nothing
        out = rx(c, int(oc["state"]), [sc.seg(rng, 0, 100, 10, ack=5001)])
        assert out["state_out"][0] == T.CLOSED and out["copy_len"][0] == 0


def test_blocked_close_changes_nothing_downstream():
    c = rc.conn1(snd_una=5000, snd_nxt=5000)
    b, got, oc = one(G.SHUT_OP_CLOSE, 0, T.ESTABLISHED, c, snd_nxt=5000, tflags=G.TMR_LIVE | G.TMR_TX_EXCLUSIVE)
    assert (oc["status"], oc["state"], oc["snd_nxt"], oc["nseg"], oc["nput"], oc["flags"]) == \
        (G.SHUTS_BLOCK, T.ESTABLISHED, 5000, 0, 0, 0)
    assert got["totals"][:2].tolist() == [0, 0]
