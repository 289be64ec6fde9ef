"""The definition of gcl_tcp_tick and gcl_tcp_rx_acks (include/gclassify.h) in
Python, and the cases the CPU and GPU tests share.  The model transcribes
tcp_worker's test (runtime/net/tcp.c:166), tcp_handle_timeouts (:80-140),
tcp_timer_update (:46-77), tcp_tx_ack and tcp_tx_probe_window
(runtime/net/tcp_out.c:178-228) and __tcp_add_tcphdr's window line (:74) line
by line over a dict of tcpconn_t fields; it knows nothing of
csrc/gcl_tcptmr.h.  The one departure from the text is the issue's: the
microtime() of tcp.c:74 is the sweep's @now.

A sweep case is a dict: now, tmr (TMR records), conn (tests/tcprxcases.py's CONN
records), addr (ADDR records), all indexed by cookie, seg_cap, frame_base,
frame_stride and optionally blocks.
"""
import functools
import json
import os

import numpy as np

from tests import tcprxcases as rc

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
ENOMEM = 12
# runtime/net/tcp.h:21-26, ONE_MS = 1000, ONE_SECOND = 1000000 (us)
TCP_ACK_TIMEOUT, TCP_CONNECT_TIMEOUT, TCP_OOQ_ACK_TIMEOUT = 10 * 1000, 5 * 1000000, 300 * 1000
TCP_TIME_WAIT_TIMEOUT, TCP_ZERO_WND_TIMEOUT, TCP_RETRANSMIT_TIMEOUT = 1 * 1000000, 300 * 1000, 300 * 1000
# runtime/net/tcp.h:41-52
(SYN_SENT, SYN_RECEIVED, ESTABLISHED, FIN_WAIT1, FIN_WAIT2, CLOSE_WAIT, CLOSING, LAST_ACK, TIME_WAIT,
 CLOSED) = range(10)
TCP_ACK = 0x10
LIVE, ACK_DELAYED, ZERO_WND, TX_EXCLUSIVE, TXQ, OOO = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
A_FIRED, A_ACK, A_PROBE, A_RETRANSMIT, A_FAIL, A_CLOSE, A_NOSPACE = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
K_ACK, K_PROBE = 0, 1
C_SEGS, NR = 7, 8
C_WANTED, C_WRITTEN, C_SKIPPED = 0, 1, 2
MAX_BLOCKS, MAX_CONN, TILE, MIN_STRIDE = 1024, 1 << 20, 256, 54
TMR = np.dtype([("next_timeout", "<u8"), ("attach_ts", "<u8"), ("time_wait_ts", "<u8"), ("ack_ts", "<u8"),
                ("zero_wnd_ts", "<u8"), ("txq_ts", "<u8"), ("state", "u1"), ("flags", "u1"), ("pad", "u1", (14,))])
TMR_OUT = np.dtype([("next_timeout", "<u8"), ("zero_wnd_ts", "<u8"), ("state", "u1"), ("flags", "u1"),
                    ("action", "u1"), ("pad", "u1", (13,))])
ADDR = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"), ("rcv_wscale", "u1"),
                 ("pad", "u1", (3,))])
DESC = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"), ("proto", "u1"),
                 ("tcp_flags", "u1"), ("tcp_off", "u1"), ("ecn", "u1"), ("seq", "<u4"), ("ack", "<u4"),
                 ("win", "<u2"), ("paylen", "<u2"), ("pad", "<u4")])
SEG = (("desc", DESC), ("frame_off", np.uint64), ("seg_conn", np.uint32), ("seg_kind", np.uint8),
       ("seg_src", np.uint32))
SENTINEL, GUARD = 0xA7, 16
NOW = 10_000_000_000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcpctl_ref.json")


# ---------------------------------------------------------------- the model
class Tx:
    """net_tx_alloc_mbuf_sz and net_tx_ip as a call sees them: the k-th
    allocation of the call succeeds exactly when k < seg_cap, and a segment
    that was sent is recorded in order."""

    def __init__(self, cap):
        self.cap, self.asked, self.segs = cap, 0, []

    def alloc(self):
        k, self.asked = self.asked, self.asked + 1
        return None if k >= self.cap else {}


def tcp_push_tcphdr(m, c, flags, off, l4len):
    # tcp_out.c:59-61
    ack, win = c["rcv_nxt"], c["rcv_wnd"]
    # :69-75; hton16 takes a uint16_t: the shifted window is truncated
    m.update(sport=c["lport"], dport=c["rport"], ack=ack, off=off, flags=flags,
             win=(win >> c["rcv_wscale"]) & 0xFFFF, seq=m["seg_seq"], l4len=l4len)


def tcp_tx_ack(c, tx, src, kind=K_ACK):
    # tcp_out.c:183-185
    m = tx.alloc()
    if m is None:
        return -ENOMEM
    # :188
    m["seg_seq"] = c["snd_nxt"]
    tcp_push_tcphdr(m, c, TCP_ACK, 5, 0)
    # :193: net_tx_ip(m, IPPROTO_TCP, raddr.ip, laddr.ip, NULL)
    m.update(proto=6, rip=c["rip"], lip=c["lip"], aux=None, cookie=c["cookie"], kind=kind, src=src)
    tx.segs.append(m)
    return 0


def tcp_tx_probe_window(c, tx, src):
    # tcp_out.c:214-216
    m = tx.alloc()
    if m is None:
        return -ENOMEM
    # :219
    m["seg_seq"] = (c["snd_una"] - 1) & M32
    tcp_push_tcphdr(m, c, TCP_ACK, 5, 0)
    m.update(proto=6, rip=c["rip"], lip=c["lip"], aux=None, cookie=c["cookie"], kind=K_PROBE, src=src)
    tx.segs.append(m)
    return 0


def tcp_timer_update(c, microtime):
    # tcp.c:48
    next_timeout = M64
    # :52-56
    if c["state"] == TIME_WAIT:
        next_timeout = (c["time_wait_ts"] + TCP_TIME_WAIT_TIMEOUT) & M64
    if c["state"] < ESTABLISHED:
        next_timeout = (c["attach_ts"] + TCP_CONNECT_TIMEOUT) & M64
    # :58-62
    if c["ack_delayed"]:
        next_timeout = min(next_timeout, (c["ack_ts"] + TCP_ACK_TIMEOUT) & M64)
    if c["zero_wnd"]:
        next_timeout = min(next_timeout, (c["zero_wnd_ts"] + TCP_ZERO_WND_TIMEOUT) & M64)
    # :64-70
    if not c["tx_exclusive"]:
        if c["txq"] is not None:
            next_timeout = min(next_timeout, (c["txq"] + TCP_RETRANSMIT_TIMEOUT) & M64)
    # :72-74
    if c["rxq_ooo"]:
        next_timeout = min(next_timeout, (microtime + TCP_OOQ_ACK_TIMEOUT) & M64)
    # :76
    c["next_timeout"] = next_timeout


def tcp_handle_timeouts(c, now, tx):
    """returns the action bits; @c is changed as the reference changes it"""
    do_ack = do_probe = do_retransmit = False
    act = A_FIRED
    # tcp.c:85-88
    if c["state"] == CLOSED:
        return act
    # :90-95
    if c["state"] < ESTABLISHED and (now - c["attach_ts"]) & M64 >= TCP_CONNECT_TIMEOUT:
        c["state"] = CLOSED                 # tcp_conn_fail -> tcp_conn_set_state(c, TCP_STATE_CLOSED)
        return act | A_FAIL
    # :97-104
    if c["state"] == TIME_WAIT and (now - c["time_wait_ts"]) & M64 >= TCP_TIME_WAIT_TIMEOUT:
        c["state"] = CLOSED
        return act | A_CLOSE
    # :106-110
    if c["ack_delayed"] and (now - c["ack_ts"]) & M64 >= TCP_ACK_TIMEOUT:
        c["ack_delayed"] = False
        do_ack = True
    # :112-116
    if c["zero_wnd"] and (now - c["zero_wnd_ts"]) & M64 >= TCP_ZERO_WND_TIMEOUT:
        c["zero_wnd_ts"] = now
        do_probe = True
    # :118-126
    if not c["tx_exclusive"] and c["txq"] is not None:
        if (now - c["txq"]) & M64 >= TCP_RETRANSMIT_TIMEOUT:
            do_retransmit = True
    # :128
    do_ack |= c["rxq_ooo"]
    # :130
    tcp_timer_update(c, now)
    # :134-139
    lost = False
    if do_ack:
        lost |= tcp_tx_ack(c, tx, c["cookie"]) != 0
        act |= A_ACK
    if do_probe:
        lost |= tcp_tx_probe_window(c, tx, c["cookie"]) != 0
        act |= A_PROBE
    if do_retransmit:
        act |= A_RETRANSMIT
    return act | (A_NOSPACE if lost else 0)


def _conn_of(case, k):
    t, p, a = case["tmr"][k], case["conn"][k], case["addr"][k]
    f = int(t["flags"])
    return dict(cookie=k, state=int(t["state"]), next_timeout=int(t["next_timeout"]), attach_ts=int(t["attach_ts"]),
                time_wait_ts=int(t["time_wait_ts"]), ack_ts=int(t["ack_ts"]), zero_wnd_ts=int(t["zero_wnd_ts"]),
                txq=int(t["txq_ts"]) if f & TXQ else None, live=bool(f & LIVE), ack_delayed=bool(f & ACK_DELAYED),
                zero_wnd=bool(f & ZERO_WND), tx_exclusive=bool(f & TX_EXCLUSIVE), rxq_ooo=bool(f & OOO),
                **_pcb_of(p, a))


def _pcb_of(p, a):
    return dict(snd_una=int(p["snd_una"]), snd_nxt=int(p["snd_nxt"]), rcv_nxt=int(p["rcv_nxt"]),
                rcv_wnd=int(p["rcv_wnd"]), rcv_wscale=int(a["rcv_wscale"]), lip=int(a["lip"]), rip=int(a["rip"]),
                lport=int(a["lport"]), rport=int(a["rport"]))


def _segs_out(tx, cap, base, stride):
    k = len(tx.segs)
    assert k == min(tx.asked, cap)
    out = {f: np.zeros(k, dtype=dt) for f, dt in SEG}
    for i, m in enumerate(tx.segs):
        assert m["aux"] is None and m["l4len"] == 0
        out["desc"][i] = (m["lip"], m["rip"], m["sport"], m["dport"], m["proto"], m["flags"], m["off"], 0, m["seq"],
                          m["ack"], m["win"], 0, 0)
        out["frame_off"][i] = (base + i * stride) & M64
        out["seg_conn"][i], out["seg_kind"][i], out["seg_src"][i] = m["cookie"], m["kind"], m["src"]
    out["totals"] = np.array([tx.asked, k], dtype=np.uint64)
    return out


def model(case):
    """every output of one sweep as a dict: out_tmr, the per-segment arrays
    (as long as the segments written), totals, counts"""
    now, nconn = case["now"], len(case["tmr"])
    tx = Tx(case["seg_cap"])
    ot = np.zeros(nconn, dtype=TMR_OUT)
    counts = [0] * NR
    for k in range(nconn):
        c = _conn_of(case, k)
        act = 0
        # tcp.c:160-167: on tcp_conns, and load_acquire(&c->next_timeout) <= now
        if c["live"] and c["next_timeout"] <= now:
            act = tcp_handle_timeouts(c, now, tx)
        f = int(case["tmr"][k]["flags"])
        f = (f & ~ACK_DELAYED) | (ACK_DELAYED if c["ack_delayed"] else 0)
        ot[k] = (c["next_timeout"], c["zero_wnd_ts"], c["state"], f, act, 0)
        for b in range(7):
            counts[b] += act >> b & 1
    out = _segs_out(tx, case["seg_cap"], case["frame_base"], case["frame_stride"])
    counts[C_SEGS] = len(tx.segs)
    return dict(out, out_tmr=ot, counts=np.array(counts, dtype=np.uint64))


def rxack_model(rx, rxout, addr, seg_cap, frame_base, frame_stride):
    """The ACKs of a gcl_tcp_rx call: @rx the tests/tcprxcases.py case, @rxout
    its outputs (verdict, sflags, rcv_nxt_after, copy_len).  Every connection's
    window is carried along its FAST segments as tcp_in.c:266-268 moves it, and
    tcp_tx_ack runs where the fast path says do_ack (tcp_in.c:289-290)."""
    order, sock, conn = rx.get("order"), rx["sock"], rx["conn"]
    n, nconn, m = len(sock), len(conn), len(rxout["verdict"])
    tx, skipped = Tx(seg_cap), 0
    wnd = [int(conn[c]["rcv_wnd"]) for c in range(nconn)]
    for j in range(m):
        if rxout["verdict"][j] != rc.FAST:
            continue
        i = j if order is None else int(order[j])
        c = int(sock[i]) if i < n else None
        if c is None or c >= nconn:                 # the issue's guards: real gcl_tcp_rx outputs never get here
            skipped += bool(rxout["sflags"][j] & rc.SF_ACK_NOW)
            continue
        wnd[c] = (wnd[c] - int(rxout["copy_len"][j])) & M32
        if rxout["sflags"][j] & rc.SF_ACK_NOW:
            pcb = dict(_pcb_of(conn[c], addr[c]), cookie=c, rcv_nxt=int(rxout["rcv_nxt_after"][j]), rcv_wnd=wnd[c])
            tcp_tx_ack(pcb, tx, j)
    out = _segs_out(tx, seg_cap, frame_base, frame_stride)
    counts = [0] * NR
    counts[C_WANTED], counts[C_WRITTEN], counts[C_SKIPPED] = tx.asked, len(tx.segs), skipped
    return dict(out, counts=np.array(counts, dtype=np.uint64))


# ---------------------------------------------------------------- builders
def tmr1(**kw):
    """an established connection on tcp_conns whose timer is due at NOW and has nothing to do"""
    d = dict(next_timeout=NOW, attach_ts=NOW - 100, time_wait_ts=NOW - 100, ack_ts=NOW - 1, zero_wnd_ts=NOW - 1,
             txq_ts=NOW - 1, state=ESTABLISHED, flags=LIVE)
    d.update(kw)
    return d


def addr1(k=0, **kw):
    d = dict(lip=0x0A000005, rip=0x0A000014 + k % 3, lport=(8000 + k) & 0xFFFF, rport=(40000 + 7 * k) & 0xFFFF,
             rcv_wscale=7)
    d.update(kw)
    return d


def records(ds, dt, mask):
    a = np.zeros(len(ds), dtype=dt)
    for k, d in enumerate(ds):
        for f, v in d.items():
            a[k][f] = v & mask
    return a


def build(ts, cs=None, ads=None, now=NOW, seg_cap=None, frame_base=4096, frame_stride=64, **kw):
    """a sweep case of the timer dicts @ts (connection and address dicts default)"""
    n = len(ts)
    cs = cs or [rc.conn1(snd_una=1000 + 16 * k, snd_nxt=5000 + 32 * k, rcv_nxt=100 + 8 * k) for k in range(n)]
    ads = ads or [addr1(k) for k in range(n)]
    case = dict(now=now, tmr=records(ts, TMR, M64), conn=rc.conns(cs), addr=records(ads, ADDR, M32),
                seg_cap=2 * n + 3 if seg_cap is None else seg_cap, frame_base=frame_base,
                frame_stride=frame_stride)
    case.update(kw)
    return case


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: the named cases of the issue"""
    res = {}
    # every early return
    res["not_live"] = build([tmr1(flags=ACK_DELAYED | ZERO_WND | OOO, ack_ts=0, zero_wnd_ts=0)])
    res["not_due"] = build([tmr1(next_timeout=NOW + 1, flags=LIVE | ACK_DELAYED | OOO, ack_ts=0)])
    res["due_exactly"] = build([tmr1(next_timeout=NOW, flags=LIVE | ACK_DELAYED, ack_ts=0)])
    res["closed"] = build([tmr1(state=CLOSED, flags=LIVE | ACK_DELAYED | ZERO_WND | OOO, ack_ts=0, zero_wnd_ts=0)])
    res["connect_fail"] = build([tmr1(state=SYN_SENT, attach_ts=NOW - TCP_CONNECT_TIMEOUT - 5,
                                      flags=LIVE | ACK_DELAYED | OOO, ack_ts=0)])
    res["time_wait_close"] = build([tmr1(state=TIME_WAIT, time_wait_ts=NOW - TCP_TIME_WAIT_TIMEOUT - 5,
                                         flags=LIVE | ZERO_WND, zero_wnd_ts=0)])
    res["nothing_to_do"] = build([tmr1()])
    # each timeout exactly at its threshold, one us before it, and with a timestamp ahead of now
    for nm, d in (("at", 0), ("before", -1)):
        res[f"ack_{nm}"] = build([tmr1(flags=LIVE | ACK_DELAYED, ack_ts=NOW - TCP_ACK_TIMEOUT - d)])
        res[f"zero_wnd_{nm}"] = build([tmr1(flags=LIVE | ZERO_WND, zero_wnd_ts=NOW - TCP_ZERO_WND_TIMEOUT - d)])
        res[f"retransmit_{nm}"] = build([tmr1(flags=LIVE | TXQ, txq_ts=NOW - TCP_RETRANSMIT_TIMEOUT - d)])
        res[f"connect_{nm}"] = build([tmr1(state=SYN_RECEIVED, attach_ts=NOW - TCP_CONNECT_TIMEOUT - d)])
        res[f"time_wait_{nm}"] = build([tmr1(state=TIME_WAIT, time_wait_ts=NOW - TCP_TIME_WAIT_TIMEOUT - d)])
    res["ack_ts_ahead"] = build([tmr1(flags=LIVE | ACK_DELAYED, ack_ts=NOW + 5)])
    res["zero_wnd_ts_ahead"] = build([tmr1(flags=LIVE | ZERO_WND, zero_wnd_ts=NOW + 5)])
    res["txq_ts_ahead"] = build([tmr1(flags=LIVE | TXQ, txq_ts=NOW + 5)])
    res["attach_ts_ahead"] = build([tmr1(state=SYN_SENT, attach_ts=NOW + 5)])
    res["time_wait_ts_ahead"] = build([tmr1(state=TIME_WAIT, time_wait_ts=NOW + 5)])
    res["next_timeout_max"] = build([tmr1(next_timeout=M64, flags=LIVE | ACK_DELAYED, ack_ts=0)])
    res["now_max"] = build([tmr1(next_timeout=M64, flags=LIVE | ACK_DELAYED | OOO, ack_ts=5)], now=M64)
    # the timer of a connection that is still connecting: attach_ts + CONNECT overrides the
    # TIME_WAIT line, whatever time_wait_ts holds, and the later terms only lower it
    res["syn_sent_override"] = build([tmr1(state=SYN_SENT, attach_ts=NOW - 1000, time_wait_ts=NOW - 999999)])
    res["syn_received_override_min"] = build([tmr1(state=SYN_RECEIVED, attach_ts=NOW - 1000, time_wait_ts=7,
                                                   flags=LIVE | ACK_DELAYED, ack_ts=NOW - 3)])
    res["time_wait_timer"] = build([tmr1(state=TIME_WAIT, time_wait_ts=NOW - 1000)])
    res["tx_exclusive_masks"] = build([tmr1(flags=LIVE | TX_EXCLUSIVE | TXQ, txq_ts=NOW - TCP_RETRANSMIT_TIMEOUT - 9),
                                       tmr1(flags=LIVE | TXQ, txq_ts=NOW - TCP_RETRANSMIT_TIMEOUT - 9)])
    res["txq_clear_ignores_ts"] = build([tmr1(flags=LIVE, txq_ts=0)])
    res["ooo_forces_ack"] = build([tmr1(flags=LIVE | OOO)])
    res["ooo_and_later_terms"] = build([tmr1(flags=LIVE | OOO | ZERO_WND, zero_wnd_ts=NOW - 10),
                                        tmr1(flags=LIVE | OOO | ZERO_WND, zero_wnd_ts=NOW + 10)])
    res["ack_and_probe"] = build([tmr1(flags=LIVE | ACK_DELAYED | ZERO_WND, ack_ts=NOW - TCP_ACK_TIMEOUT,
                                       zero_wnd_ts=NOW - TCP_ZERO_WND_TIMEOUT)])
    res["all_at_once"] = build([tmr1(flags=LIVE | ACK_DELAYED | ZERO_WND | TXQ | OOO, ack_ts=0, zero_wnd_ts=0,
                                     txq_ts=0)])
    res["unknown_flag_bits_kept"] = build([tmr1(flags=0xC0 | LIVE | ACK_DELAYED, ack_ts=0)])
    # the window line
    res["win_over_16_bits"] = build([tmr1(flags=LIVE | OOO)], [rc.conn1(rcv_wnd=0x12345678)], [addr1(rcv_wscale=3)])
    for ws in (0, 14):
        res[f"wscale{ws}"] = build([tmr1(flags=LIVE | OOO | ZERO_WND, zero_wnd_ts=0)],
                                   [rc.conn1(rcv_wnd=0x3FFFC000 if ws else 0xFFFF)], [addr1(rcv_wscale=ws)])
    res["probe_seq_una0"] = build([tmr1(flags=LIVE | ZERO_WND, zero_wnd_ts=0)], [rc.conn1(snd_una=0, snd_nxt=77)])
    res["seq_wraps"] = build([tmr1(flags=LIVE | OOO)], [rc.conn1(snd_nxt=M32, rcv_nxt=0x80000000)])
    # seg_cap: between a connection's ACK and its probe, and none at all
    three = [tmr1(flags=LIVE | ACK_DELAYED | ZERO_WND, ack_ts=0, zero_wnd_ts=0)] * 3
    res["cap_between_ack_and_probe"] = build(three, seg_cap=3)
    res["cap_zero"] = build(three, seg_cap=0)
    res["cap_total_minus_1"] = build(three, seg_cap=5)
    res["cap_total"] = build(three, seg_cap=6)
    res["mixed"] = build([tmr1(flags=0), tmr1(flags=LIVE | OOO), tmr1(next_timeout=NOW + 9), tmr1(state=CLOSED),
                          tmr1(flags=LIVE | ZERO_WND, zero_wnd_ts=0), tmr1(state=SYN_SENT, attach_ts=0),
                          tmr1(flags=LIVE | ACK_DELAYED | ZERO_WND | TXQ, ack_ts=0, zero_wnd_ts=0, txq_ts=0)],
                         frame_base=M64 - 100, frame_stride=1 << 20)
    res["nconn_zero"] = build([])
    return res


def random_case(seed, nconn, due=0.5, seg_cap=None, blocks=0, segs=None):
    """@nconn random connections, about @due of them due; timestamps crowd the
    thresholds.  @segs(k) in (0, 1, 2, 3) forces connection k's segments: bit 0
    the ACK, bit 1 the probe."""
    rng = np.random.default_rng(seed)
    T = (TCP_ACK_TIMEOUT, TCP_CONNECT_TIMEOUT, TCP_TIME_WAIT_TIMEOUT, TCP_ZERO_WND_TIMEOUT)

    def ts():
        w = int(rng.integers(0, 6))
        if w == 0:
            return int(rng.integers(0, 1 << 62))
        if w == 1:
            return NOW + int(rng.integers(0, 1000))
        return NOW - int(rng.choice(T)) + int(rng.integers(-2, 3))

    t = np.zeros(nconn, dtype=TMR)
    for f in ("attach_ts", "time_wait_ts", "ack_ts", "zero_wnd_ts", "txq_ts"):
        t[f] = [ts() for _ in range(nconn)]
    t["next_timeout"] = np.where(rng.random(nconn) < due, NOW - rng.integers(0, 3, nconn), NOW + rng.integers(1, 99, nconn))
    t["state"] = rng.choice([SYN_SENT, SYN_RECEIVED, ESTABLISHED, ESTABLISHED, ESTABLISHED, CLOSE_WAIT, TIME_WAIT,
                             CLOSED], size=nconn)
    t["flags"] = rng.integers(0, 64, nconn) | np.where(rng.random(nconn) < 0.9, LIVE, 0)
    if segs is not None:
        for k in range(nconn):
            s = segs(k)
            t[k] = (NOW, NOW, NOW, 0, 0, NOW, ESTABLISHED, LIVE | (ACK_DELAYED if s & 1 else 0) |
                    (ZERO_WND if s & 2 else 0), 0)
    c = np.zeros(nconn, dtype=rc.CONN)
    for f in ("snd_una", "snd_nxt", "rcv_nxt", "rcv_wnd"):
        c[f] = rng.integers(0, 1 << 32, nconn, dtype=np.uint64)
    c["snd_una"][rng.random(nconn) < 0.02] = 0
    a = np.zeros(nconn, dtype=ADDR)
    a["lip"], a["rip"] = rng.integers(0, 1 << 32, nconn, dtype=np.uint64), rng.integers(0, 1 << 32, nconn, dtype=np.uint64)
    a["lport"], a["rport"] = rng.integers(0, 1 << 16, nconn), rng.integers(0, 1 << 16, nconn)
    a["rcv_wscale"] = rng.integers(0, 15, nconn)
    return dict(now=NOW, tmr=t, conn=c, addr=a, seg_cap=2 * nconn if seg_cap is None else seg_cap,
                frame_base=int(rng.integers(0, 1 << 40)), frame_stride=int(rng.choice([54, 64, 128, 1536])),
                blocks=blocks)


def random_addr(seed, nconn):
    return random_case(seed, nconn)["addr"]


# ---------------------------------------------------------------- harness
def _arr(k, dt):
    return np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (k + GUARD)), dtype=dt).copy()


def blank(nconn, seg_cap, tick=True):
    """every output buffer of a call filled with SENTINEL, GUARD entries longer than the call may write"""
    b = {f: _arr(seg_cap, dt) for f, dt in SEG}
    b["totals"] = _arr(2, np.uint64)
    if tick:
        b["out_tmr"] = _arr(nconn, TMR_OUT)
    return b


def compare(got, want, nconn, seg_cap, what):
    """@got (blank() after a call) against @want: the written part equal byte
    for byte, everything past the segments written (the rest of seg_cap and the
    guard) untouched"""
    k = int(want["totals"][1])
    assert k <= seg_cap and len(want["desc"]) == k
    fields = [(f, k, seg_cap) for f, _ in SEG] + [("totals", 2, 2)]
    if "out_tmr" in got:
        fields.append(("out_tmr", nconn, nconn))
    for f, used, size in fields:
        g = got[f]
        assert len(g) == size + GUARD and (g[used:].view(np.uint8) == SENTINEL).all(), \
            f"{what}: {f} written past its {used} entries"
        bad = np.nonzero(g[:used].view(np.uint8) != want[f][:used].view(np.uint8))[0]
        if len(bad):
            e = bad[0] // g.dtype.itemsize
            raise AssertionError(f"{what}: {f}[{e}] = {g[e]} != {want[f][e]} ({len(bad)} bytes differ)")


def run_host(g, case, counts=True):
    """gcl_tcp_tick_host over sentinel-filled outputs: (outputs, counts)"""
    nconn = len(case["tmr"])
    out = blank(nconn, case["seg_cap"])
    cnt = np.full(NR, 5, dtype=np.uint64) if counts else None
    g.tcp_tick_host(case["now"], case["tmr"], case["conn"], case["addr"], case["seg_cap"],
                    frame_stride=case["frame_stride"], frame_base=case["frame_base"], nconn=nconn,
                    blocks=case.get("blocks", 0), out=out, counts=cnt)
    return out, None if cnt is None else cnt - np.uint64(5)


def run_rxack_host(g, rx, rxout, addr, seg_cap, frame_base=0, frame_stride=64, counts=True, blocks=0):
    """gcl_tcp_rx_acks_host over sentinel-filled outputs: (outputs, counts)"""
    out = blank(0, seg_cap, tick=False)
    cnt = np.full(NR, 5, dtype=np.uint64) if counts else None
    m = len(rxout["verdict"])
    g.tcp_rx_acks_host(rxout["verdict"], rxout["sflags"], rxout["rcv_nxt_after"], rx["sock"], rx["conn"], addr,
                       seg_cap, frame_stride=frame_stride, frame_base=frame_base, order=rx.get("order"), m=m,
                       n=len(rx["sock"]), nconn=len(rx["conn"]), blocks=blocks, out=out, counts=cnt)
    return out, None if cnt is None else cnt - np.uint64(5)


# ---------------------------------------------------------------- the reference's header bytes
NET = dict(addr=0x0A000005, netmask=0xFFFFFF00, gateway=0x0A000001, mac=bytes([2, 0, 0, 0, 0, 5]))


def golden_inputs():
    """The segments of the named cases, in name order, as the inputs of the
    reference's tcp_push_tcphdr: what tests/golden/make_tcpctl_ref.py records
    the header bytes of.  rcv_wnd is the 32-bit window before the shift."""
    recs = []
    for name in sorted(cases()):
        case = cases()[name]
        want = model(case)
        for k in range(int(want["totals"][1])):
            c = int(want["seg_conn"][k])
            p, a = case["conn"][c], case["addr"][c]
            kind = int(want["seg_kind"][k])
            recs.append(dict(case=name, k=k, kind=kind, lip=int(a["lip"]), lport=int(a["lport"]), rip=int(a["rip"]),
                             rport=int(a["rport"]),
                             seq=int(p["snd_nxt"]) if kind == K_ACK else (int(p["snd_una"]) - 1) & M32,
                             ack=int(p["rcv_nxt"]), rcv_wnd=int(p["rcv_wnd"]), wscale=int(a["rcv_wscale"])))
    return recs


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
