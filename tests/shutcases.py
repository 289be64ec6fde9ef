"""Cases and an independent model for gcl_tcp_shut (include/gclassify.h).

The model is written from the reference's runtime/net/tcp.c, not from the C rule
of csrc/gcl_tcpshut.h: a small connection object with the fields tcp_shutdown,
tcp_close, tcp_abort, tcp_conn_shutdown_tx, tcp_conn_shutdown_rx, tcp_conn_fail,
tcp_conn_set_state, tcp_timer_update and tcp_tx_ctl touch, the functions run
line by line on it, and what they did read back as the output record.  A call
that would sleep raises Sleep; a call whose segment has no room is run on a
copy that is thrown away.

Also here: the enumeration of every op x state x flag x how, whole and LIVE, with
the not-LIVE and bad-state connections behind it, three cases called out by name, the random batch generator, and the helpers the CPU and GPU tests
share."""
import itertools
import json
import os

import numpy as np

from caladan_amd import gclassify as G

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
NOW = (1 << 40) + 12345
(SYN_SENT, SYN_RECEIVED, ESTABLISHED, FIN_WAIT1, FIN_WAIT2, CLOSE_WAIT, CLOSING, LAST_ACK, TIME_WAIT,
 CLOSED) = range(10)
ECONNABORTED, EINVAL, ENOBUFS = 103, 22, 105
TCP_FIN, TCP_RST, TCP_ACK = 0x01, 0x04, 0x10
T_ACK, T_CONNECT, T_OOQ_ACK, T_TIME_WAIT, T_ZERO_WND, T_RETRANSMIT = 10000, 5000000, 300000, 1000000, 300000, 300000


class Sleep(Exception):
    """waitq_wait on tx_wq: the call does not come back within this instant"""


class Conn:
    """the fields of tcpconn_t the calls touch, as the snapshot gives them"""

    def __init__(self, sh, tm, cn, ad):
        fl = int(tm["flags"])
        self.state, self.err = int(tm["state"]), 0
        self.tx_closed = bool(sh["flags"] & G.SHUT_TX_CLOSED)
        self.rx_closed = bool(sh["flags"] & G.SHUT_RX_CLOSED)
        self.rx_exclusive = bool(sh["flags"] & G.SHUT_RX_EXCL)
        self.tx_exclusive = bool(fl & G.TMR_TX_EXCLUSIVE)
        self.ack_delayed, self.zero_wnd = bool(fl & G.TMR_ACK_DELAYED), bool(fl & G.TMR_ZERO_WND)
        self.txq = [int(tm["txq_ts"])] if fl & G.TMR_TXQ else []    # the timestamps of c->txq
        self.rxq_ooo = bool(fl & G.TMR_OOO)
        self.next_timeout = int(tm["next_timeout"])
        self.attach_ts, self.time_wait_ts = int(tm["attach_ts"]), int(tm["time_wait_ts"])
        self.ack_ts, self.zero_wnd_ts = int(tm["ack_ts"]), int(tm["zero_wnd_ts"])
        self.snd_nxt, self.rcv_nxt, self.rcv_wnd = int(cn["snd_nxt"]), int(cn["rcv_nxt"]), int(cn["rcv_wnd"])
        self.rcv_wscale = int(ad["rcv_wscale"]) & 31
        self.ev = 0          # G.SHO_*
        self.puts = 0
        self.sent = []       # (flags, seq, ack, win, queued)


def timer_update(c, now):                                       # tcp.c:46-77
    nt = M64
    if c.state == TIME_WAIT:
        nt = (c.time_wait_ts + T_TIME_WAIT) & M64
    if c.state < ESTABLISHED:
        nt = (c.attach_ts + T_CONNECT) & M64
    if c.ack_delayed:
        nt = min(nt, (c.ack_ts + T_ACK) & M64)
    if c.zero_wnd:
        nt = min(nt, (c.zero_wnd_ts + T_ZERO_WND) & M64)
    if not c.tx_exclusive and c.txq:
        nt = min(nt, (c.txq[0] + T_RETRANSMIT) & M64)
    if c.rxq_ooo:
        nt = min(nt, (now + T_OOQ_ACK) & M64)                   # microtime(): the call's one reading
    c.next_timeout = nt


def set_state(c, new, now):                                     # tcp.c:248-263
    if c.state < ESTABLISHED and new >= ESTABLISHED:
        c.ev |= G.SHO_POLLOUT
    c.state = new
    timer_update(c, now)


def shutdown_rx(c):                                             # tcp.c:1492-1502
    if c.rx_closed:
        return
    c.ev |= G.SHO_POLLRDHUP_IN | G.SHO_RXWAKE | G.SHO_RX_CLOSED_SET
    c.rx_closed = True


def conn_fail(c, err, now):                                     # tcp.c:1453-1484
    was_closed = c.state == CLOSED
    c.err = err
    set_state(c, CLOSED, now)
    shutdown_rx(c)
    if not c.tx_closed:
        c.tx_closed = True
        c.ev |= G.SHO_TX_CLOSED_SET | G.SHO_TXWAKE | G.SHO_POLLHUP
    if not c.tx_exclusive:
        c.txq = []
        c.ev |= G.SHO_FREE_TXQ | G.SHO_FREE_PEND
    if not c.rx_exclusive:
        c.ev |= G.SHO_FREE_RXQ
    c.rxq_ooo = False
    c.ev |= G.SHO_FREE_OOO
    if not was_closed:
        c.puts += 1


def tx_ctl(c, flags, now):                                      # tcp_out.c:264-295, :54-81
    c.sent.append((flags, c.snd_nxt, c.rcv_nxt, (c.rcv_wnd >> c.rcv_wscale) & 0xFFFF, True))
    c.snd_nxt = (c.snd_nxt + 1) & M32
    c.txq.append(now)


def tx_raw_rst(c, seq):                                         # tcp_out.c:98-128
    c.sent.append((TCP_RST, seq, 0, 0, False))


def shutdown_tx(c, now):                                        # tcp.c:1504-1546
    if c.tx_closed:
        return
    if c.state < ESTABLISHED:
        conn_fail(c, ECONNABORTED, now)
        tx_raw_rst(c, c.snd_nxt)
        return
    if c.tx_exclusive:
        raise Sleep
    tx_ctl(c, TCP_FIN | TCP_ACK, now)
    if c.state == ESTABLISHED:
        set_state(c, FIN_WAIT1, now)
    elif c.state == CLOSE_WAIT:
        set_state(c, LAST_ACK, now)
    else:
        c.ev |= G.SHO_WARN
    c.ev |= G.SHO_POLLHUP | G.SHO_TXWAKE | G.SHO_TX_CLOSED_SET
    c.tx_closed = True


def tcp_shutdown(c, how, now):                                  # tcp.c:1555-1579
    if how not in (0, 1, 2):
        return -EINVAL
    if how in (1, 2):
        shutdown_tx(c, now)
    if how in (0, 2):
        shutdown_rx(c)
    return 0


def tcp_abort(c, now):                                          # tcp.c:1585-1606
    if c.state == CLOSED:
        return
    conn_fail(c, ECONNABORTED, now)
    if c.tx_exclusive:
        raise Sleep
    tx_raw_rst(c, c.snd_nxt)


def tcp_close(c, now):                                          # tcp.c:1616-1633
    shutdown_tx(c, now)
    shutdown_rx(c)
    c.ev |= G.SHO_DETACH_POLL
    c.puts += 1


def model_conn(sh, tm, cn, ad, now, room):
    """One connection: (the fields of its out_conn less first_seg and nseg, its segment or None).
    @room: a segment of it would have a slot."""
    op, fl = int(sh["op"]), int(tm["flags"])
    echo = dict(next_timeout=int(tm["next_timeout"]), txq_ts=int(tm["txq_ts"]), ret=0, err=0,
                snd_nxt=int(cn["snd_nxt"]), flags=0, status=G.SHUTS_NONE, state=int(tm["state"]), tmr_flags=fl, nput=0)
    if op == G.SHUT_OP_NONE or not fl & G.TMR_LIVE:
        return echo, None
    if op > G.SHUT_OP_ABORT or int(tm["state"]) > CLOSED:
        return dict(echo, status=G.SHUTS_REFUSED), None
    c = Conn(sh, tm, cn, ad)
    status, ret = G.SHUTS_DONE, 0
    try:
        if op == G.SHUT_OP_SHUTDOWN:
            ret = tcp_shutdown(c, int(sh["how"]), now)
            if ret:
                return dict(echo, status=G.SHUTS_EINVAL, ret=ret), None
        elif op == G.SHUT_OP_CLOSE:
            tcp_close(c, now)
        else:
            tcp_abort(c, now)
    except Sleep:
        if op != G.SHUT_OP_ABORT:
            return dict(echo, status=G.SHUTS_BLOCK), None       # slept before anything happened
        status = G.SHUTS_ABORT_WAIT                             # slept after the fail
    assert len(c.sent) <= 1
    seg = c.sent[0] if c.sent else None
    if seg and not room:
        return dict(echo, status=G.SHUTS_NOSPACE, ret=-ENOBUFS), "lost"
    tf = fl & ~(G.TMR_TXQ | G.TMR_OOO) | (G.TMR_TXQ if c.txq else 0) | (G.TMR_OOO if c.rxq_ooo else 0)
    return dict(next_timeout=c.next_timeout, txq_ts=c.txq[0] if c.txq else int(tm["txq_ts"]), ret=ret, err=c.err,
                snd_nxt=c.snd_nxt, flags=c.ev, status=status, state=c.state, tmr_flags=tf, nput=c.puts), seg


def rec(dtype, **kw):
    r = np.zeros((), dtype=dtype)
    for k, v in kw.items():
        r[k] = v
    return r


def conn(op=G.SHUT_OP_NONE, how=0, state=ESTABLISHED, sflags=0, tflags=G.TMR_LIVE, snd_nxt=1000, rcv_nxt=5000,
         rcv_wnd=65535, wscale=0, next_timeout=M64, attach_ts=NOW - 100, time_wait_ts=NOW - 200, ack_ts=NOW - 300,
         zero_wnd_ts=NOW - 400, txq_ts=NOW - 500, lip=0x0A000001, rip=0x0A000002, lport=80, rport=40000):
    """one connection of a batch: (shut, tmr, conn, addr) records"""
    return (rec(G.TCP_SHUT_DTYPE, how=how, op=op, flags=sflags),
            rec(G.TCP_TMR_DTYPE, next_timeout=next_timeout, attach_ts=attach_ts, time_wait_ts=time_wait_ts,
                ack_ts=ack_ts, zero_wnd_ts=zero_wnd_ts, txq_ts=txq_ts, state=state, flags=tflags),
            rec(G.TCP_CONN_DTYPE, snd_una=(snd_nxt - 10) & M32, snd_nxt=snd_nxt, snd_wnd=65535, rcv_nxt=rcv_nxt,
                rcv_wnd=rcv_wnd, rcv_mss=1460),
            rec(G.TCP_ADDR_DTYPE, lip=lip, rip=rip, lport=lport, rport=rport, rcv_wscale=wscale))


def raw(a, nbytes):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:nbytes].tobytes()


class Batch:
    def __init__(self, conns=None, arrays=None):
        if arrays is None:
            arrays = [np.array([c[i] for c in conns], dtype=dt) if conns else np.zeros(0, dtype=dt)
                      for i, dt in enumerate((G.TCP_SHUT_DTYPE, G.TCP_TMR_DTYPE, G.TCP_CONN_DTYPE, G.TCP_ADDR_DTYPE))]
        self.shut, self.tmr, self.conn, self.addr = arrays
        self.nconn = len(self.shut)

    def expect(self, seg_cap, frame_base=0, frame_stride=64, frames_len=0, now=NOW):
        """the model's out_conn, segments, totals and counts"""
        cap = seg_cap
        if frames_len:
            cap = min(cap, 0 if frames_len < frame_base else (frames_len - frame_base) // frame_stride)
        oc = np.zeros(self.nconn, dtype=G.SHUT_CONN_OUT_DTYPE)
        segs = {f: [] for f in G.SHUT_SEG_FIELDS}
        cnt, wanted, k = [0] * G.SHUTC_NR, 0, 0
        for c in range(self.nconn):
            o, seg = model_conn(self.shut[c], self.tmr[c], self.conn[c], self.addr[c], now, k < cap)
            for f, v in o.items():
                oc[c][f] = v
            cnt[o["status"]] += 1
            cnt[G.SHUTC_FAIL] += o["err"] != 0
            cnt[G.SHUTC_PUT] += o["nput"]
            cnt[G.SHUTC_WARN] += bool(o["flags"] & G.SHO_WARN)
            if seg is None:
                continue
            wanted += 1
            if seg == "lost":
                continue
            flags, seq, ack, win, queued = seg
            a, off = self.addr[c], (frame_base + k * frame_stride) & M64
            oc[c]["first_seg"], oc[c]["nseg"] = k, 1
            segs["desc"].append(rec(G.TXH_DESC_DTYPE, lip=a["lip"], rip=a["rip"], lport=a["lport"], rport=a["rport"],
                                    proto=6, tcp_flags=flags, tcp_off=5, seq=seq, ack=ack, win=win))
            segs["frame_off"].append(off)
            segs["seg_conn"].append(c)
            segs["seg_src"].append(c)
            segs["seg_kind"].append(G.CTL_FIN if queued else G.CTL_RST)
            segs["txq_ent"].append(rec(G.TXQ_ENT_DTYPE, seg_seq=seq, seg_end=(seq + 1) & M32, ts=now) if queued
                                   else rec(G.TXQ_ENT_DTYPE))
            segs["txq_cold"].append(rec(G.TXQ_COLD_DTYPE, frame_off=off, tcp_flags=flags, tcp_off=5,
                                        flags=G.TXQE_INFLIGHT) if queued else rec(G.TXQ_COLD_DTYPE))
            cnt[G.SHUTC_FIN if queued else G.SHUTC_RST] += 1
            k += 1
        dts = dict(desc=G.TXH_DESC_DTYPE, frame_off=np.uint64, seg_conn=np.uint32, seg_kind=np.uint8,
                   seg_src=np.uint32, txq_ent=G.TXQ_ENT_DTYPE, txq_cold=G.TXQ_COLD_DTYPE)
        exp = {f: np.array(v, dtype=dts[f]) if v else np.zeros(0, dtype=dts[f]) for f, v in segs.items()}
        exp.update(out_conn=oc, totals=np.array([wanted, k], dtype=np.uint64), counts=cnt)
        return exp

    def run_host(self, seg_cap, frame_base=0, frame_stride=64, frames_len=0, counts=None, now=NOW, blocks=0,
                 guard=0):
        """the host twin over 0xFF-filled outputs with @guard elements behind each"""
        out = {}
        for f in G.SHUT_SEG_FIELDS:
            out[f] = np.full((seg_cap + guard) * G.SHUT_OUT_WIDTH[f] + (16 if not seg_cap + guard else 0), 0xFF,
                             dtype=np.uint8)
        out["out_conn"] = np.full((self.nconn + guard) * 48 + (48 if not self.nconn + guard else 0), 0xFF,
                                  dtype=np.uint8)
        out["totals"] = np.full(2 + guard, M64, dtype=np.uint64)
        return G.tcp_shut_host(now, self.shut, self.tmr, self.conn, self.addr, seg_cap, frame_stride=frame_stride,
                               frame_base=frame_base, frames_len=frames_len, nconn=self.nconn, blocks=blocks, out=out,
                               counts=counts)


def check(b, got, exp, counts=None, seg_cap=None, guard=0):
    """@got (the twin's or the device's arrays) is the model's answer @exp byte for byte, and nothing
    behind what the call may write was touched"""
    assert raw(got["out_conn"], 48 * b.nconn) == exp["out_conn"].tobytes(), first_diff(b, got, exp)
    assert raw(got["totals"], 16) == exp["totals"].tobytes()
    n = int(exp["totals"][1])
    for f in G.SHUT_SEG_FIELDS:
        w = G.SHUT_OUT_WIDTH[f]
        assert raw(got[f], n * w) == exp[f].tobytes(), f
        if seg_cap is not None:
            tail = np.ascontiguousarray(got[f]).view(np.uint8).reshape(-1)[n * w:(seg_cap + guard) * w]
            assert (tail == 0xFF).all(), f
    if guard:
        tail = np.ascontiguousarray(got["out_conn"]).view(np.uint8).reshape(-1)[48 * b.nconn:48 * (b.nconn + guard)]
        assert (tail == 0xFF).all()
        assert (np.ascontiguousarray(got["totals"]).view(np.uint64)[2:2 + guard] == M64).all()
    if counts is not None:
        assert [int(x) for x in counts] == [int(x) for x in exp["counts"]]


def first_diff(b, got, exp):
    g = np.frombuffer(raw(got["out_conn"], 48 * b.nconn), dtype=G.SHUT_CONN_OUT_DTYPE)
    for c in range(b.nconn):
        if g[c].tobytes() != exp["out_conn"][c].tobytes():
            return f"connection {c}: {b.shut[c]} {b.tmr[c]} got {g[c]} expected {exp['out_conn'][c]}"
    return ""


OPS = (G.SHUT_OP_NONE, G.SHUT_OP_SHUTDOWN, G.SHUT_OP_CLOSE, G.SHUT_OP_ABORT, 4)
HOWS = (-1, 0, 1, 2, 3)


ENUM_LIVE = len(OPS) * 10 * 16 * len(HOWS)      # the whole product, every one of them LIVE
BAD_STATES = (10, 11, 16, 255)


def _enum_conn(i, op, state, x, txc, rxc, rxe, how, live):
    """connection @i of the enumeration: the other timer flags and the timestamps turn with the index,
    so that every term of the timer update is the least one somewhere"""
    extra = (G.TMR_ACK_DELAYED, G.TMR_ZERO_WND, G.TMR_TXQ, G.TMR_OOO)
    tf = sum(f for j, f in enumerate(extra) if (i * 7 + i // 5) >> j & 1)
    tf |= (G.TMR_TX_EXCLUSIVE if x else 0) | (G.TMR_LIVE if live else 0)
    ts = [NOW - 1000 * ((i * (j + 3)) % 11) - j for j in range(5)]
    return conn(op=op, how=how, state=state,
                sflags=(G.SHUT_TX_CLOSED if txc else 0) | (G.SHUT_RX_CLOSED if rxc else 0) |
                (G.SHUT_RX_EXCL if rxe else 0), tflags=tf, snd_nxt=(M32 - 20 + i) & M32,
                rcv_nxt=(7 * i) & M32, rcv_wnd=(i * 977) & M32, wscale=i % 15,
                next_timeout=NOW + i, attach_ts=ts[0] - T_CONNECT + T_OOQ_ACK,
                time_wait_ts=ts[1] - T_TIME_WAIT + T_OOQ_ACK, ack_ts=ts[2] - T_ACK + T_OOQ_ACK,
                zero_wnd_ts=ts[3], txq_ts=ts[4], lport=1 + i % 60000, rport=2 + i % 50000, rip=0x0A000100 + i)


def enumeration():
    """Connections [0, ENUM_LIVE): every op (and one unknown) x state 0..9 x X x TX_CLOSED x RX_CLOSED
    x RX_EXCL x how, 4 000 of them, every one LIVE and in its own state; combination (op, state, x,
    txc, rxc, rxe, how) has the index of itertools.product over those ranges.  Behind them, as
    further connections and not as substitutions: the same 4 000 without GCL_TMR_LIVE, and every op x
    X x how in each state of BAD_STATES, LIVE."""
    combos = list(itertools.product(OPS, range(10), (0, 1), (0, 1), (0, 1), (0, 1), HOWS))
    conns = [_enum_conn(i, *c, live=True) for i, c in enumerate(combos)]
    conns += [_enum_conn(len(conns) + i, *c, live=False) for i, c in enumerate(combos)]
    bad = list(itertools.product(OPS, BAD_STATES, (0, 1), HOWS))
    conns += [_enum_conn(len(conns) + i, op, state, x, i & 1, i >> 1 & 1, i >> 2 & 1, how, live=True)
              for i, (op, state, x, how) in enumerate(bad)]
    return Batch(conns)


def enum_index(op, state, x=0, txc=0, rxc=0, rxe=0, how=0):
    """where the LIVE combination lies in enumeration()"""
    return (((((OPS.index(op) * 10 + state) * 2 + x) * 2 + txc) * 2 + rxc) * 2 + rxe) * len(HOWS) + HOWS.index(how)


def case_fail_keeps_txq_term():
    """tcp_abort of an ESTABLISHED connection with a queue: tcp_conn_fail's timer update (tcp.c:1459)
    runs before mbuf_list_free(&c->txq) (:1471), so next_timeout is the queue head's deadline although
    TXQ is clear in the output flags"""
    return (conn(op=G.SHUT_OP_ABORT, state=ESTABLISHED, tflags=G.TMR_LIVE | G.TMR_TXQ, txq_ts=NOW - 777),
            dict(status=G.SHUTS_DONE, state=CLOSED, err=ECONNABORTED, next_timeout=NOW - 777 + T_RETRANSMIT,
                 tmr_flags=G.TMR_LIVE, nput=1, nseg=1, txq_ts=NOW - 777))


def case_warn_leaves_timer():
    """SHUT_WR in FIN_WAIT2 without tx_closed: the reference's WARN().  The FIN goes out and joins the
    queue, but no tcp_conn_set_state runs, so next_timeout stays although the queue has a head now"""
    return (conn(op=G.SHUT_OP_SHUTDOWN, how=1, state=FIN_WAIT2, next_timeout=NOW + 4242),
            dict(status=G.SHUTS_DONE, state=FIN_WAIT2, err=0, next_timeout=NOW + 4242, txq_ts=NOW,
                 tmr_flags=G.TMR_LIVE | G.TMR_TXQ, nput=0, nseg=1, snd_nxt=1001,
                 flags=G.SHO_WARN | G.SHO_POLLHUP | G.SHO_TX_CLOSED_SET | G.SHO_TXWAKE))


def case_rdwr_on_syn_received():
    """SHUT_RDWR on SYN_RECEIVED: the tx part fails the connection (one put, one RST with seq =
    snd_nxt) and closes rx inside the fail; the rx part then finds rx_closed set: RX_CLOSED_SET once"""
    return (conn(op=G.SHUT_OP_SHUTDOWN, how=2, state=SYN_RECEIVED),
            dict(status=G.SHUTS_DONE, state=CLOSED, err=ECONNABORTED, nput=1, nseg=1, snd_nxt=1000,
                 flags=G.SHO_POLLOUT | G.SHO_POLLRDHUP_IN | G.SHO_RX_CLOSED_SET | G.SHO_RXWAKE | G.SHO_TX_CLOSED_SET |
                 G.SHO_TXWAKE | G.SHO_POLLHUP | G.SHO_FREE_TXQ | G.SHO_FREE_PEND | G.SHO_FREE_RXQ | G.SHO_FREE_OOO))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcpfin_ref.json")
NET = dict(addr=0x0A000005, netmask=0xFFFFFF00, gateway=0x0A000001, mac=bytes([2, 0, 0, 0, 0, 5]))


NEIGH = [(0x0A000014 + k, bytes([2, 0, 0, 0, 1, k])) for k in range(3)]


def golden_inputs():
    """the tuples tests/golden/make_tcpfin_ref.py gives to the reference's tcp_push_tcphdr with flags
    FIN | ACK: window scales 0 and 7, windows that the shift and hton16 truncate, and sequence numbers
    around the wrap at 2^32 (seq 2^32 - 1: the FIN's seg_end is 0)"""
    seqs = (0, 1, M32, (1 << 31) - 1, 1 << 31, M32 - 1, 1000, 0x12345678, 0xFFFF0000)
    wins = (0, 1, 65535, 65536, 0x7FFFFF, 0x800000, M32, 1 << 20, 127)
    rows = []
    for i, (seq, win) in enumerate(itertools.product(seqs[:6], wins[:6])):
        rows.append(dict(lip=NET["addr"], lport=1024 + 37 * i, rip=0x0A000014 + i % 3, rport=(50000 + 811 * i) & 0xFFFF,
                         seq=seqs[(i + seq) % 9] if i % 5 == 4 else seq, ack=(seq * 3 + 0xFFFFFFF0 + i) & M32,
                         rcv_wnd=wins[(i * 2) % 9] if i % 4 == 3 else win, wscale=7 if i % 2 else 0))
    return rows


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_batch():
    """one connection per tuple of golden_inputs(), alternately closed from ESTABLISHED and shut down
    for writing from CLOSE_WAIT: every one sends a FIN"""
    return Batch([conn(op=G.SHUT_OP_CLOSE if i % 2 else G.SHUT_OP_SHUTDOWN, how=1 + i % 3 % 2,
                       state=ESTABLISHED if i % 2 else CLOSE_WAIT, snd_nxt=r["seq"], rcv_nxt=r["ack"],
                       rcv_wnd=r["rcv_wnd"], wscale=r["wscale"], lip=r["lip"], rip=r["rip"], lport=r["lport"],
                       rport=r["rport"]) for i, r in enumerate(golden_inputs())])


NAMED = (case_fail_keeps_txq_term, case_warn_leaves_timer, case_rdwr_on_syn_received)


def random_batch(seed, nconn, mix="mixed", garbage=False):
    """@mix: "mixed" (about half act), "all" (every connection wants a segment), "none" (nobody
    wants one), "last" (only the last connection wants one).  @garbage: states up to 255, random op
    bytes and flag bytes."""
    r = np.random.default_rng(seed)
    shut, tmr = np.zeros(nconn, dtype=G.TCP_SHUT_DTYPE), np.zeros(nconn, dtype=G.TCP_TMR_DTYPE)
    cn, ad = np.zeros(nconn, dtype=G.TCP_CONN_DTYPE), np.zeros(nconn, dtype=G.TCP_ADDR_DTYPE)
    for f in ("next_timeout", "attach_ts", "time_wait_ts", "ack_ts", "zero_wnd_ts", "txq_ts"):
        tmr[f] = NOW - r.integers(0, 2 * T_CONNECT, nconn).astype(np.uint64) + np.uint64(T_CONNECT)
    tmr["next_timeout"][r.random(nconn) < 0.3] = M64
    tmr["state"] = r.integers(0, 10, nconn)
    tmr["flags"] = r.integers(0, 64, nconn) | np.where(r.random(nconn) < 0.9, G.TMR_LIVE, 0)
    shut["op"] = r.choice([0, 1, 2, 3], nconn, p=[0.4, 0.3, 0.15, 0.15])
    shut["how"] = r.choice([-1, 0, 1, 2, 3, 1 << 30, -(1 << 31)], nconn, p=[0.03, 0.25, 0.3, 0.3, 0.06, 0.03, 0.03])
    shut["flags"] = r.integers(0, 8, nconn) & r.integers(0, 8, nconn)
    shut["pad"] = r.integers(0, 256, (nconn, 10))
    for f in ("snd_una", "snd_nxt", "snd_wnd", "rcv_nxt", "rcv_wnd"):
        cn[f] = r.integers(0, 1 << 32, nconn)
    cn["snd_nxt"][::17] = M32
    for f in ("lip", "rip"):
        ad[f] = r.integers(0, 1 << 32, nconn)
    for f in ("lport", "rport"):
        ad[f] = r.integers(0, 1 << 16, nconn)
    ad["rcv_wscale"] = r.integers(0, 256, nconn)
    if garbage:
        tmr["state"] = r.integers(0, 256, nconn)
        tmr["flags"] = r.integers(0, 256, nconn)
        tmr["pad"] = r.integers(0, 256, (nconn, 14))
        shut["op"] = np.where(r.random(nconn) < 0.5, r.integers(0, 256, nconn), r.integers(0, 4, nconn))
        shut["flags"] = r.integers(0, 256, nconn)
        shut["how"] = np.where(r.random(nconn) < 0.5, r.integers(-(1 << 31), 1 << 31, nconn), shut["how"])
    if mix in ("all", "none", "last"):
        tmr["flags"] = (tmr["flags"] | G.TMR_LIVE) & (0xFF ^ G.TMR_TX_EXCLUSIVE)
        tmr["state"] = r.choice([ESTABLISHED, CLOSE_WAIT, SYN_RECEIVED, FIN_WAIT2], nconn)
        shut["flags"] &= 0xFF ^ G.SHUT_TX_CLOSED
        shut["op"], shut["how"] = r.choice([1, 2, 3], nconn), r.choice([1, 2], nconn)
        if mix != "all":
            quiet = slice(0, nconn - 1 if mix == "last" else nconn)
            shut["op"][quiet] = r.choice([0, 1], nconn)[quiet]
            shut["how"][quiet] = 0
    return Batch(arrays=[shut, tmr, cn, ad])
