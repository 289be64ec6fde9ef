"""The reference model and the cases of gcl_tcp_txq (include/gclassify.h).

The model is a line-by-line transcription of the reference's walks over a
connection's queue of sent but unacknowledged segments, run in the order the
reference runs them: tcp_retransmit calls tcp_tx_retransmit over the whole
queue and only then does tcp_write_finish pop and start the fast retransmit
(runtime/net/tcp.c:1425-1444, :1309-1349).  The reference lines stand beside
each statement.  It works on mbuf objects whose timestamps and seg_seq it
changes as the reference does; the states, head_ts and the counters are read
off those objects afterwards, not computed the way the C rule computes them.

What is not the reference's, as include/gclassify.h says: a segment that does
not fit seg_cap stands for the -ENOMEM of tcp_out.c:410; the refusals; the fast
retransmit leaves an entry alone that the walk of the same call already sent;
and the two departures (the trimmed l4len, and no pull of option bytes).
"""
import copy
import json
import os

import numpy as np

M32, M64 = 0xFFFFFFFF, (1 << 64) - 1
TCP_RETRANSMIT_TIMEOUT = 300000  # runtime/net/tcp.h
TCP_RETRANSMIT_BATCH = 16
TCP_FIN, TCP_SYN, TCP_PSH, TCP_ACK = 0x01, 0x02, 0x08, 0x10
HDR = 54

W_RTO, W_FAST, W_EXCL = 0x01, 0x02, 0x04
INFLIGHT = 0x01
KEPT, ACKED, RETX, RETX_COPY, NOSPACE, REFUSED = range(6)
TRIMMED = 0x80
O_EMPTY, O_DEFERRED, O_NOSPACE, O_BATCH, O_BADRANGE = 0x01, 0x02, 0x04, 0x08, 0x10
C_ACKED, C_RETX, C_COPIED, C_TRIMMED, C_REFUSED, C_NOSPACE, C_DEFERRED, C_BYTES = range(8)
NR, TILE, LONG, MAX_BLOCKS, MAX_CONN = 8, 256, 64, 1024, 1 << 20

ENT = np.dtype([("seg_seq", "<u4"), ("seg_end", "<u4"), ("ts", "<u8")])
COLD = np.dtype([("frame_off", "<u8"), ("tcp_flags", "u1"), ("tcp_off", "u1"), ("flags", "u1"), ("pad", "u1", (5,))])
CONN_OUT = np.dtype([("head_ts", "<u8"), ("nacked", "<u4"), ("nretx", "<u4"), ("first", "<u4"), ("flags", "u1"),
                     ("pad", "u1", (11,))])
DESC = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"), ("proto", "u1"),
                 ("tcp_flags", "u1"), ("tcp_off", "u1"), ("ecn", "u1"), ("seq", "<u4"), ("ack", "<u4"),
                 ("win", "<u2"), ("paylen", "<u2"), ("pad", "<u4")])
CONN = np.dtype([("snd_una", "<u4"), ("snd_nxt", "<u4"), ("snd_wnd", "<u4"), ("snd_wl1", "<u4"), ("snd_wl2", "<u4"),
                 ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("rcv_mss", "<u2"), ("snd_wscale", "u1"), ("flags", "u1"),
                 ("acks_delayed_cnt", "u1"), ("pad", "u1", (15,))])
ADDR = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"), ("rcv_wscale", "u1"),
                 ("pad", "u1", (3,))])
SEG = (("desc", DESC), ("frame_off", np.uint64), ("src_off", np.uint64), ("len", np.uint16),
       ("dst_off", np.uint64), ("seg_conn", np.uint32), ("seg_ent", np.uint32))
SENTINEL, GUARD = 0xA7, 16
NOW = 1 << 40


# ---------------------------------------------------------------- inc/base/stddef.h:144-178
def s32(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def wraps_lt(a, b):
    return s32(a - b) < 0


def wraps_lte(a, b):
    return s32(a - b) <= 0


def wraps_gt(a, b):
    return s32(b - a) < 0


def wraps_gte(a, b):
    return s32(b - a) <= 0


# ---------------------------------------------------------------- the model
class Mbuf:
    def __init__(self, e, h, q):
        self.e = e                                  # its index in ent: seg_ent
        self.seg_seq, self.seg_end, self.timestamp = int(h["seg_seq"]), int(h["seg_end"]), int(h["ts"])
        self.frame_off, self.flags, self.off = int(q["frame_off"]), int(q["tcp_flags"]), int(q["tcp_off"])
        self.ref = 2 if int(q["flags"]) & INFLIGHT else 1
        self.event = KEPT                           # what became of it in this call
        self.trimmed = False


class Conn:
    def __init__(self, c, p, a, want, txq):
        self.c, self.txq = c, txq
        self.snd_una, self.rcv_nxt, self.rcv_wnd = int(p["snd_una"]), int(p["rcv_nxt"]), int(p["rcv_wnd"])
        self.a = a
        self.tx_exclusive = bool(want & W_EXCL)
        self.want = want
        self.flags = 0
        self.refused = 0


class Tx:
    """the segments of a call: net_tx_ip's side of it"""
    def __init__(self, cap, frame_base, frame_stride):
        self.cap, self.frame_base, self.frame_stride = cap, frame_base, frame_stride
        self.segs = []


def tcp_tx_retransmit_one(c, m, tx, now):
    """tcp_out.c:388-444; returns (ret, sent)"""
    opts_len = m.off - 5                                            # :399
    copy_it = m.ref != 1                                            # :407
    una = c.snd_una                                                 # :426
    trim = (una - m.seg_seq) & M32 if wraps_lt(m.seg_seq, una) else 0   # :430-431
    seq = (m.seg_seq + trim) & M32                                  # :432
    l4len = (m.seg_end - seq) & M32                                 # :395, of the trimmed segment (departure 1)
    if m.flags & (TCP_SYN | TCP_FIN):                               # :396
        l4len = (l4len - 1) & M32                                   # :397
    sz = 4 * opts_len + l4len                                       # :408
    refused = not 5 <= m.off <= 15 or l4len > 0xFFFF or (trim > 0 and opts_len > 0)   # (departure 2)
    if not refused and copy_it:
        refused = sz > 0xFFFF or HDR + sz > tx.frame_stride
    if refused:                                                     # like the mbuf_free; return 0 of :428
        if m.event != REFUSED:
            c.refused += 1
        m.event = REFUSED
        return 0, False
    k = len(tx.segs)
    if k >= tx.cap:                                                 # net_tx_alloc_mbuf_sz fails
        m.event = NOSPACE
        c.flags |= O_NOSPACE
        return -12, False                                           # :411 -ENOMEM
    if trim:
        m.seg_seq = una                                             # :432
        m.trimmed = True
    if copy_it:                                                     # :408-418
        frame_off = (tx.frame_base + k * tx.frame_stride) & M64
        length = sz
    else:                                                           # :421: strip headers; :431 mbuf_pull
        frame_off = (m.frame_off + trim) & M64
        length = 0
    a = c.a
    win = (c.rcv_wnd >> (int(a["rcv_wscale"]) & 31)) & 0xFFFF        # :436 tcp_push_tcphdr, tcp_out.c:74
    tx.segs.append(dict(                                            # :440 net_tx_ip
        desc=(int(a["lip"]), int(a["rip"]), int(a["lport"]), int(a["rport"]), 6, m.flags, m.off, 0, seq,
              c.rcv_nxt, win, l4len, 0),
        frame_off=frame_off, src_off=(m.frame_off + HDR + trim) & M64, len=length,
        dst_off=(frame_off + HDR) & M64, seg_conn=c.c, seg_ent=m.e, trim=trim, copy=copy_it))
    m.event = RETX_COPY if copy_it else RETX
    return 0, True


def tcp_tx_retransmit(c, tx, now):
    """tcp_out.c:480-506"""
    count = 0                                                       # :489
    for m in c.txq:                                                 # :490
        if (now - m.timestamp) & M64 < TCP_RETRANSMIT_TIMEOUT:      # :492
            break                                                   # :493
        if wraps_gte(c.snd_una, m.seg_end):                         # :495
            continue                                                # :496
        m.timestamp = now                                           # :498
        ret, sent = tcp_tx_retransmit_one(c, m, tx, now)            # :499
        if ret:                                                     # :500
            break                                                   # :501
        if sent:                                                    # a refused entry does not count
            count += 1                                              # :503
            if count >= TCP_RETRANSMIT_BATCH:
                c.flags |= O_BATCH
                break                                               # :504


def tcp_conn_ack(c, freeq):
    """tcp.c:217-238"""
    if c.tx_exclusive:                                              # :224
        return                                                      # :225
    while True:                                                     # :228
        m = c.txq[0] if c.txq else None                             # :229
        if m is None:                                               # :230
            break
        if wraps_gt(m.seg_end, c.snd_una):                          # :232
            break
        freeq.append(c.txq.pop(0))                                  # :235-236


def tcp_tx_fast_retransmit_start(c, now):
    """tcp_out.c:450-466"""
    if c.tx_exclusive:                                              # :456
        return None
    m = c.txq[0] if c.txq else None                                 # :459
    if m is not None and m.event in (RETX, RETX_COPY):              # the walk of this call sent it already
        return None
    if m is not None:
        m.timestamp = now                                           # :461
        m.ref += 1                                                  # :462
    return m


def run_conn(c, tx, now):
    """one connection, as tcp_retransmit and tcp_write_finish order it"""
    freeq = []
    if c.tx_exclusive:                                              # tcp.c:1431 waits; :224; tcp_out.c:456
        c.flags |= O_DEFERRED
        return freeq
    if c.want & W_RTO:
        tcp_tx_retransmit(c, tx, now)                               # tcp.c:1437
    tcp_conn_ack(c, freeq)                                          # tcp.c:1321
    if c.want & W_FAST:                                             # tcp.c:1332-1335: the caller decided
        m = tcp_tx_fast_retransmit_start(c, now)
        if m is not None:
            tcp_tx_retransmit_one(c, m, tx, now)                    # tcp_out.c:471
    return freeq


def _queue(case, c):
    lo, hi = int(case["qoff"][c]), int(case["qoff"][c + 1])
    if lo > hi or hi > len(case["ent"]):
        return None
    return [Mbuf(e, case["ent"][e], case["cold"][e]) for e in range(lo, hi)]


def model(case):
    """every output of gcl_tcp_txq for @case, with the counters"""
    nconn, nent, cap, now = len(case["conn"]), len(case["ent"]), case["seg_cap"], case["now"]
    tx = Tx(cap, case["frame_base"], case["frame_stride"])
    out_conn = np.zeros(nconn, dtype=CONN_OUT)
    state = np.full(nent, SENTINEL, dtype=np.uint8)
    counts = np.zeros(NR, dtype=np.uint64)
    wanted = 0
    for k in range(nconn):
        want = int(case["want"][k]) if case.get("want") is not None else 0
        q = _queue(case, k)
        bad = q is None
        q = q or []
        # what the connection asks for when nothing limits it: its share of totals[0] and of `first`
        free = Conn(k, case["conn"][k], case["addr"][k], want, copy.deepcopy(q))
        unbounded = Tx(1 << 62, 0, case["frame_stride"])
        run_conn(free, unbounded, now)
        first = min(wanted, cap)
        wanted += len(unbounded.segs)
        c = Conn(k, case["conn"][k], case["addr"][k], want, list(q))
        before = len(tx.segs)
        freeq = run_conn(c, tx, now)
        for m in q:
            st = ACKED if m in freeq else m.event
            if st in (RETX, RETX_COPY) and m.trimmed:
                st |= TRIMMED
            state[m.e] = st
        o = out_conn[k]
        o["nacked"], o["nretx"], o["first"] = len(freeq), len(tx.segs) - before, first
        o["head_ts"] = c.txq[0].timestamp if c.txq else 0          # the head that is left, as the calls left it
        o["flags"] = c.flags | (O_EMPTY if not c.txq else 0) | (O_BADRANGE if bad else 0)
        mine = tx.segs[before:]
        counts[C_ACKED] += len(freeq)
        counts[C_RETX] += len(mine)
        counts[C_COPIED] += sum(1 for s in mine if s["copy"])
        counts[C_TRIMMED] += sum(1 for s in mine if s["trim"])
        counts[C_REFUSED] += c.refused
        counts[C_NOSPACE] += 1 if c.flags & O_NOSPACE else 0
        counts[C_DEFERRED] += 1 if c.flags & O_DEFERRED else 0
        counts[C_BYTES] += sum(s["len"] for s in mine)
    res = {f: np.zeros(len(tx.segs), dtype=dt) for f, dt in SEG}
    for k, s in enumerate(tx.segs):
        res["desc"][k] = s["desc"]
        for f in ("frame_off", "src_off", "len", "dst_off", "seg_conn", "seg_ent"):
            res[f][k] = s[f]
    res.update(out_conn=out_conn, state=state, counts=counts,
               totals=np.array([wanted, min(wanted, cap), counts[C_BYTES]], dtype=np.uint64))
    return res


# ---------------------------------------------------------------- building cases
DUE = NOW - TCP_RETRANSMIT_TIMEOUT - 7


def ent(seq, end, ts=DUE, flags=TCP_ACK, off=5, inflight=False, frame_off=None):
    return dict(seg_seq=seq & M32, seg_end=end & M32, ts=ts & M64, tcp_flags=flags, tcp_off=off,
                flags=INFLIGHT if inflight else 0, frame_off=frame_off)


def conn(q, una=1000, want=W_RTO, rcv_nxt=0x11223344, rcv_wnd=0x00654321, wscale=3, k=0):
    return dict(q=q, snd_una=una & M32, want=want, rcv_nxt=rcv_nxt, rcv_wnd=rcv_wnd, wscale=wscale)


FRAME_SLOT = 2048  # where entry e's original frame lies: 256 + e * FRAME_SLOT


def build(conns, now=NOW, seg_cap=None, frame_base=1 << 20, frame_stride=1600, want=True, qoff=None, **kw):
    """a case of @conns (conn() dicts); @qoff overrides the CSR (hostile ranges)"""
    ents = [e for c in conns for e in c["q"]]
    h, q = np.zeros(len(ents), dtype=ENT), np.zeros(len(ents), dtype=COLD)
    for i, e in enumerate(ents):
        h[i] = (e["seg_seq"], e["seg_end"], e["ts"])
        q[i]["frame_off"] = 256 + i * FRAME_SLOT if e["frame_off"] is None else e["frame_off"]
        q[i]["tcp_flags"], q[i]["tcp_off"], q[i]["flags"] = e["tcp_flags"], e["tcp_off"], e["flags"]
    off = np.zeros(len(conns) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c["q"]) for c in conns])
    p, a = np.zeros(len(conns), dtype=CONN), np.zeros(len(conns), dtype=ADDR)
    for k, c in enumerate(conns):
        p[k]["snd_una"], p[k]["rcv_nxt"], p[k]["rcv_wnd"] = c["snd_una"], c["rcv_nxt"], c["rcv_wnd"]
        p[k]["snd_nxt"] = (c["snd_una"] + 5000) & M32
        a[k] = (0x0A000005, 0x0A000100 + k, 8000 + k, 40000 + 7 * k, c["wscale"], (0, 0, 0))
    case = dict(now=now, qoff=off if qoff is None else np.asarray(qoff, dtype=np.uint32), ent=h, cold=q, conn=p,
                addr=a, want=np.array([c["want"] for c in conns], dtype=np.uint8) if want else None,
                seg_cap=17 * len(conns) + 3 if seg_cap is None else seg_cap, frame_base=frame_base,
                frame_stride=frame_stride)
    case.update(kw)
    return case


def run_of(n, seq=1000, size=100, **kw):
    """@n back-to-back segments of @size bytes from @seq"""
    return [ent(seq + i * size, seq + (i + 1) * size, **kw) for i in range(n)]


_CASES = None


def cases():
    """name -> case: every edge of the rule once"""
    global _CASES
    if _CASES is not None:
        return _CASES
    res = {}
    young = NOW - TCP_RETRANSMIT_TIMEOUT + 1
    # wraps_gt against wraps_gte: seg_end == snd_una is popped and passed over, snd_una + 1 is neither
    res["end_eq_una"] = build([conn([ent(900, 1000), ent(1000, 1001), ent(1001, 1100)])])
    res["end_eq_una_plus_1"] = build([conn([ent(900, 1001), ent(1001, 1100)])])
    res["end_eq_una_wrap"] = build([conn([ent(0xFFFFFF00, 4), ent(4, 5), ent(5, 90)], una=4)])
    res["end_eq_una_plus_1_wrap"] = build([conn([ent(0xFFFFFFF0, 0), ent(0, 50)], una=0xFFFFFFFF)])
    res["una_behind_the_wrap"] = build([conn([ent(0xFFFFFF00, 0xFFFFFFF0), ent(0xFFFFFFF0, 0x20)], una=0xFFFFFFF8)])
    # the 300 ms test
    res["age_299999"] = build([conn([ent(1000, 1100, ts=NOW - 299999)])])
    res["age_300000"] = build([conn([ent(1000, 1100, ts=NOW - 300000)])])
    res["ts_ahead_of_now"] = build([conn([ent(1000, 1100, ts=NOW + 5)])])
    res["young_then_due"] = build([conn([ent(1000, 1100, ts=young), ent(1100, 1200)])])
    # TCP_RETRANSMIT_BATCH
    res["seventeen_due"] = build([conn(run_of(17))])
    res["sixteen_due"] = build([conn(run_of(16))])
    res["seventeen_due_and_fast"] = build([conn(run_of(17), want=W_RTO | W_FAST)])
    # continue, no pop
    res["acked_behind_unacked"] = build([conn([ent(1000, 1100), ent(800, 900), ent(1100, 1200)])])
    # the walk breaks at a young acknowledged head; the pops still happen
    res["young_acked_head"] = build([conn([ent(900, 1000, ts=young), ent(1000, 1100)])])
    res["all_acked"] = build([conn(run_of(3, seq=700))])
    # the partial ACK
    res["trim_1"] = build([conn([ent(1000, 1100)], una=1001)])
    res["trim_all_but_one"] = build([conn([ent(1000, 1100)], una=1099)])
    res["trim_inflight"] = build([conn([ent(1000, 1100, inflight=True)], una=1040)])
    res["trim_fin"] = build([conn([ent(1000, 1101, flags=TCP_FIN | TCP_ACK)], una=1050)])
    res["fin_paylen_0"] = build([conn([ent(1000, 1001, flags=TCP_FIN | TCP_ACK)])])
    res["syn_with_options"] = build([conn([ent(1000, 1001, flags=TCP_SYN, off=10)])])
    res["syn_with_options_inflight"] = build([conn([ent(1000, 1001, flags=TCP_SYN | TCP_ACK, off=10, inflight=True)])])
    res["inflight"] = build([conn([ent(1000, 1100, inflight=True), ent(1100, 1200)])])
    # the fast retransmit
    res["fast_alone"] = build([conn([ent(900, 1000), ent(1000, 1100, ts=young), ent(1100, 1200)], want=W_FAST)])
    res["fast_and_rto_same_head"] = build([conn([ent(1000, 1100), ent(1100, 1200)], want=W_RTO | W_FAST)])
    res["fast_and_rto_young_head"] = build([conn([ent(1000, 1100, ts=young), ent(1100, 1200)], want=W_RTO | W_FAST)])
    res["fast_empty_queue"] = build([conn([], want=W_FAST)])
    res["fast_all_acked"] = build([conn(run_of(2, seq=700), want=W_FAST)])
    res["fast_trim"] = build([conn([ent(1000, 1100)], una=1030, want=W_FAST)])
    res["excl_with_everything"] = build([conn([ent(900, 1000), ent(1000, 1100)], want=W_EXCL | W_RTO | W_FAST)])
    res["excl_empty"] = build([conn([], want=W_EXCL)])
    res["want_null"] = build([conn([ent(900, 1000), ent(1000, 1100)])], want=False)
    res["want_zero"] = build([conn([ent(900, 1000), ent(1000, 1100)], want=0)])
    # each refusal; the walk goes on behind it
    res["refuse_off_4"] = build([conn([ent(1000, 1100, off=4), ent(1100, 1200)])])
    res["refuse_off_16"] = build([conn([ent(1000, 1100, off=16), ent(1100, 1200)])])
    res["refuse_paylen"] = build([conn([ent(1000, 1000 + 65536), ent(1000 + 65536, 1000 + 65636)])])
    res["paylen_65535"] = build([conn([ent(1000, 1000 + 65535)])])
    res["refuse_fin_without_sequence"] = build([conn([ent(1000, 1000, flags=TCP_FIN, ts=DUE), ent(1000, 1100)],
                                                     una=999)])
    res["refuse_trim_with_options"] = build([conn([ent(1000, 1100, off=6), ent(1100, 1200)], una=1010)])
    res["refuse_copy_past_stride"] = build([conn([ent(1000, 1100, inflight=True), ent(1100, 1146, inflight=True),
                                                  ent(1146, 1193, inflight=True)])], frame_stride=100)
    res["refuse_fast_past_stride"] = build([conn([ent(1000, 1100)], want=W_RTO | W_FAST),
                                            conn([ent(1000, 1100)], want=W_FAST)], frame_stride=100)
    res["seventeen_refused_then_sixteen"] = build([conn(run_of(17, off=3) + run_of(17, seq=2700))])
    # seg_cap
    for name, cap in (("nospace_first", 0), ("nospace_middle", 1), ("nospace_last", 2), ("space_for_all", 3)):
        res[name] = build([conn(run_of(3) + [ent(1300, 1400, ts=young)])], seg_cap=cap)
    res["nospace_fast"] = build([conn(run_of(2), want=W_RTO), conn([ent(1000, 1100, ts=young)], want=W_FAST)],
                                seg_cap=2)
    res["nospace_fast_after_walk"] = build([conn([ent(1000, 1100)], want=W_RTO | W_FAST)], seg_cap=0)
    res["nospace_then_refused_kept"] = build([conn([ent(1000, 1100), ent(1100, 1200), ent(1200, 1300, off=4)]),
                                              conn(run_of(2)), conn([ent(1000, 1100, off=4)])], seg_cap=1)
    res["seg_cap_0"] = build([conn(run_of(2)), conn(run_of(2, seq=700)), conn(run_of(1), want=W_FAST)], seg_cap=0)
    res["cap_at_a_connection_end"] = build([conn(run_of(2)), conn(run_of(3)), conn(run_of(1))], seg_cap=5)
    res["empty_queue"] = build([conn([])])
    res["no_connections_with_entries"] = build([conn([]), conn([]), conn([])])
    # garbage qoff: an inverted range, one past nent, one that is fine, one that starts past nent
    res["bad_qoff"] = build([conn(run_of(2)), conn(run_of(2)), conn(run_of(2)), conn([]), conn([])],
                            qoff=[0, 5, 3, 9, 6, 6])
    res["qoff_moved_boundary"] = build([conn(run_of(3)), conn(run_of(3), want=W_RTO | W_FAST)], qoff=[0, 4, 6])
    _CASES = res
    return res


def concat(cs, seg_cap=None):
    """several cases as one batch of connections (the call's own inputs from the first)"""
    off, ents, colds = [0], [], []
    for c in cs:
        base = off[-1] if len(off) else 0
        q = c["qoff"].astype(np.int64)
        # a hostile CSR cannot be shifted meaningfully: keep only cases whose ranges are in order
        assert (np.diff(q) >= 0).all() and q[-1] == len(c["ent"])
        off.extend((q[1:] + base).tolist())
        ents.append(c["ent"])
        k = c["cold"].copy()
        colds.append(k)
    res = dict(cs[0])
    res.update(qoff=np.array(off, dtype=np.uint32), ent=np.concatenate(ents), cold=np.concatenate(colds),
               conn=np.concatenate([c["conn"] for c in cs]), addr=np.concatenate([c["addr"] for c in cs]),
               want=np.concatenate([c["want"] if c["want"] is not None else np.zeros(len(c["conn"]), np.uint8)
                                    for c in cs]))
    res["cold"]["frame_off"] = 256 + np.arange(len(res["cold"]), dtype=np.uint64) * FRAME_SLOT
    res["seg_cap"] = 17 * len(res["conn"]) + 3 if seg_cap is None else seg_cap
    return res


def all_named(seg_cap=None, frame_stride=1600):
    """all named cases with an orderly CSR and the common stride as one batch"""
    cs = [c for _, c in sorted(cases().items())
          if c["frame_stride"] == frame_stride and (np.diff(c["qoff"].astype(np.int64)) >= 0).all()
          and c["qoff"][-1] == len(c["ent"])]
    return concat(cs, seg_cap)


def random_case(seed, nconn, qlen=None, due=0.5, hostile=0.1, seg_cap=None, blocks=0, want=None, bad_qoff=0.0,
                frame_stride=1600):
    """a seeded batch: mostly consistent queues (back-to-back segments around
    snd_una, timestamps that grow along the queue), with hostile entries,
    connections and ranges mixed in.  @qlen(k, rng) gives connection k's queue
    length; @want(k, rng) its want byte."""
    rng = np.random.default_rng(seed)
    lens = np.array([int(qlen(k, rng)) if qlen else int(rng.choice([0, 1, 1, 2, 3, 5, 8, 20])) for k in range(nconn)],
                    dtype=np.int64)
    off = np.zeros(nconn + 1, dtype=np.uint32)
    off[1:] = np.cumsum(lens)
    nent = int(off[-1])
    h, q = np.zeros(nent, dtype=ENT), np.zeros(nent, dtype=COLD)
    p, a = np.zeros(nconn, dtype=CONN), np.zeros(nconn, dtype=ADDR)
    w = np.zeros(nconn, dtype=np.uint8)
    for k in range(nconn):
        lo, n = int(off[k]), int(lens[k])
        una = int(rng.integers(0, 1 << 32)) if rng.random() < 0.7 else int(rng.choice([0, 1, M32, M32 - 50, 1 << 31]))
        sizes = rng.choice([1, 1, 40, 100, 536, 1460], size=n)
        acked = int(rng.integers(0, n + 1)) if n and rng.random() < 0.5 else 0
        start = una - int(sizes[:acked].sum()) - (int(rng.integers(0, int(sizes[acked]))) if acked < n and
                                                   rng.random() < 0.3 else 0)
        seq = start
        isdue = rng.random() < due
        ts = NOW - TCP_RETRANSMIT_TIMEOUT - int(rng.integers(0, 1000)) if isdue else NOW - int(rng.integers(0, 299999))
        for i in range(n):
            e = lo + i
            fl = TCP_ACK | (TCP_PSH if rng.random() < 0.3 else 0)
            ln = int(sizes[i])
            if i == n - 1 and rng.random() < 0.1:
                fl |= TCP_FIN
                ln += 1
            h[e] = (seq & M32, (seq + ln) & M32, ts & M64)
            q[e]["tcp_flags"], q[e]["tcp_off"] = fl, 5
            q[e]["flags"] = INFLIGHT if rng.random() < 0.2 else 0
            seq += ln
            ts += int(rng.integers(0, 400)) if rng.random() < 0.9 else TCP_RETRANSMIT_TIMEOUT
            if rng.random() < hostile:
                h[e] = (int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)),
                        int(rng.integers(0, 1 << 63)) * 2 if rng.random() < 0.5 else NOW - 300000 + int(rng.integers(-2, 3)))
                q[e]["tcp_off"] = int(rng.integers(0, 20))
                q[e]["tcp_flags"] = int(rng.integers(0, 256))
                q[e]["flags"] = int(rng.integers(0, 256))
        p[k]["snd_una"], p[k]["snd_nxt"] = una, seq & M32
        p[k]["rcv_nxt"], p[k]["rcv_wnd"] = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        a[k] = (0x0A000005, int(rng.integers(1, 1 << 32)), int(rng.integers(1, 65536)), int(rng.integers(1, 65536)),
                int(rng.integers(0, 256)) if rng.random() < hostile else int(rng.integers(0, 15)), (0, 0, 0))
        w[k] = int(want(k, rng)) if want else int(rng.choice([0, W_RTO, W_RTO, W_RTO, W_FAST, W_RTO | W_FAST, W_EXCL,
                                                              W_EXCL | W_RTO, 0xFF, 0xF8]))
    q["frame_off"] = 256 + np.arange(nent, dtype=np.uint64) * FRAME_SLOT
    if bad_qoff:
        for k in range(nconn + 1):
            if rng.random() < bad_qoff:
                # past nent: both neighbours become bad ranges; never a range that overlaps another one,
                # whose shared states would depend on which lane writes last
                off[k] = int(rng.choice([nent + 1, M32, nent + 1 + int(rng.integers(0, 1000))]))
    return dict(now=NOW, qoff=off, ent=h, cold=q, conn=p, addr=a, want=w, blocks=blocks,
                seg_cap=17 * nconn + 3 if seg_cap is None else seg_cap, frame_base=1 << 30, frame_stride=frame_stride)


# ---------------------------------------------------------------- harness
def _arr(k, dt):
    return np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (k + 2 * GUARD)), dtype=dt).copy()


def blank(nconn, nent, seg_cap):
    """every output buffer of a call filled with SENTINEL, with GUARD entries in front of what the call is given
    and GUARD entries behind what it may write; inner() gives the arrays to pass"""
    b = {f: _arr(seg_cap, dt) for f, dt in SEG}
    b.update(totals=_arr(3, np.uint64), out_conn=_arr(nconn, CONN_OUT), state=_arr(nent, np.uint8))
    return b


def inner(b):
    """the arrays of blank() (or their device copies, rows of records) as a call takes them: behind the front guard"""
    return {f: a[GUARD:] for f, a in b.items()}


def compare(got, want, case, what):
    """@got (blank() after a call over inner()) against @want: the written
    part equal byte for byte; the guard in front of every array, everything
    past the segments written (the rest of seg_cap and the guard behind) and
    every state no valid range covers untouched"""
    nconn, nent, seg_cap = len(case["conn"]), len(case["ent"]), case["seg_cap"]
    k = int(want["totals"][1])
    assert k <= seg_cap and len(want["desc"]) == k
    fields = [(f, k, seg_cap) for f, _ in SEG] + [("totals", 3, 3), ("out_conn", nconn, nconn), ("state", nent, nent)]
    for f, used, size in fields:
        assert len(got[f]) == size + 2 * GUARD
        assert (got[f][:GUARD].view(np.uint8) == SENTINEL).all(), f"{what}: {f} written in front of its first entry"
        g = got[f][GUARD:]
        assert (g[used:].view(np.uint8) == SENTINEL).all(), f"{what}: {f} written past its {used} entries"
        bad = np.nonzero(g[:used].view(np.uint8) != want[f][:used].view(np.uint8))[0]
        if len(bad):
            e = bad[0] // g.dtype.itemsize
            raise AssertionError(f"{what}: {f}[{e}] = {g[e]} != {want[f][e]} ({len(bad)} bytes differ)")


def run_host(g, case, counts=True):
    """gcl_tcp_txq_host over sentinel-filled outputs: (blank() as the call left it, counts)"""
    nconn, nent = len(case["conn"]), len(case["ent"])
    out = blank(nconn, nent, case["seg_cap"])
    cnt = np.full(NR, 5, dtype=np.uint64) if counts else None
    g.tcp_txq_host(case["now"], case["qoff"], case["ent"], case["cold"], case["conn"], case["addr"], case["seg_cap"],
                   want=case.get("want"), frame_stride=case["frame_stride"], frame_base=case["frame_base"],
                   nconn=nconn, nent=nent, blocks=case.get("blocks", 0), out=inner(out), counts=cnt)
    return out, None if cnt is None else cnt - np.uint64(5)


# ---------------------------------------------------------------- the reference's header bytes
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txq_ref.json")
NET = dict(addr=0x0A000005, netmask=0xFFFFFF00, gateway=0x0A000001, mac=bytes([2, 0, 0, 0, 0, 5]))
REF_L4LEN_MAX = 65535 - 20  # the longest payload an IPv4 packet carries behind a 20-byte TCP header


def region(size):
    """the tx region of a case before the chain: byte x is a fixed function of x with period 251 * 256, so that
    every offset of a frame slot, and neighbouring slots, hold different bytes"""
    x = np.arange(size, dtype=np.uint64)
    return ((x % np.uint64(251)) * np.uint64(7) + (x >> np.uint64(8)) * np.uint64(13) + np.uint64(3)).astype(np.uint8)


def region_size(case):
    """room for every original frame of @case and for seg_cap copied ones"""
    orig = int(case["cold"]["frame_off"].max()) + HDR + 60 + (1 << 16) if len(case["cold"]) else 0
    return max(orig, case["frame_base"] + (case["seg_cap"] + 1) * case["frame_stride"])


def sent_segments(case):
    """The segments @case retransmits, read off its inputs the way
    tcp_tx_retransmit_one reads them (which entries are sent, and which by
    copy, is the model's): per segment the frame it is sent from and the
    inputs of the reference's tcp_push_tcphdr at tcp_out.c:436."""
    want = model(case)
    recs = []
    for k in range(int(want["totals"][1])):
        c, e = int(want["seg_conn"][k]), int(want["seg_ent"][k])
        p, a, h, q = case["conn"][c], case["addr"][c], case["ent"][e], case["cold"][e]
        una, seq = int(p["snd_una"]), int(h["seg_seq"])
        trim = (una - seq) & M32 if wraps_lt(seq, una) else 0                   # :430-431
        seq = (seq + trim) & M32                                                # :432
        flags, off = int(q["tcp_flags"]), int(q["tcp_off"])
        paylen = (int(h["seg_end"]) - seq - (1 if flags & (TCP_SYN | TCP_FIN) else 0)) & M32
        by_copy = int(want["state"][e]) & 0x7F == RETX_COPY
        recs.append(dict(k=k, by_copy=by_copy, trim=trim, off=off, paylen=paylen,
                         old=int(q["frame_off"]),                               # the entry's frame
                         frame=case["frame_base"] + k * case["frame_stride"] if by_copy else int(q["frame_off"]) + trim,
                         lip=int(a["lip"]), lport=int(a["lport"]), rip=int(a["rip"]), rport=int(a["rport"]),
                         seq=seq, ack=int(p["rcv_nxt"]), rcv_wnd=int(p["rcv_wnd"]), wscale=int(a["rcv_wscale"]),
                         flags=flags))
    return recs


def in_golden(r):
    """tcp_push_tcphdr's struct has no room for options, and no IPv4 packet for more than REF_L4LEN_MAX bytes"""
    return r["off"] == 5 and r["paylen"] <= REF_L4LEN_MAX


GOLDEN_KEYS = ("k", "by_copy", "trim", "paylen", "lip", "lport", "rip", "rport", "seq", "ack", "rcv_wnd", "wscale",
               "flags")


def golden_inputs():
    """The retransmitted tcp_off 5 segments of the named cases, in name
    order: what tests/golden/make_txq_ref.py records the header bytes of.
    rcv_wnd is the 32-bit window before the shift."""
    recs = []
    for name in sorted(cases()):
        for r in sent_segments(cases()[name]):
            if in_golden(r):
                recs.append(dict(case=name, **{f: r[f] for f in GOLDEN_KEYS}))
    return recs


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def check_chain(name, case, got, reg, golden, refused):
    """@reg, region(region_size(case)) after gcl_tcp_txq -> gcl_copy_batch ->
    gcl_tx_hdr over it; @got the inner() outputs of the first call; @golden
    the records of @name; @refused[k]: gcl_tx_hdr refused segment k.  Every
    segment's frame lies where tcp_tx_retransmit_one sends from (the old frame
    moved up by the trim, or slot k), holds the reference's TCP header bytes
    and an IPv4 length of the trimmed segment in front of the options and the
    payload bytes that stay, and no other byte of the region changed."""
    segs = sent_segments(case)
    assert int(got["totals"][1]) == len(segs)
    before = region(len(reg))
    expect = before.copy()
    headers = np.zeros(len(reg), dtype=bool)
    at = 0
    for r in segs:
        f, k = r["frame"], r["k"]
        n = 4 * (r["off"] - 5) + r["paylen"]
        src = r["old"] + HDR + r["trim"]
        assert int(got["frame_off"][k]) == f, (name, k)
        if r["by_copy"]:
            expect[f + HDR:f + HDR + n] = before[src:src + n]
        else:
            assert f + HDR == src and int(got["len"][k]) == 0, (name, k)
        headers[f:f + HDR] = True
        assert (reg[f + HDR:f + HDR + n] == before[src:src + n]).all(), (name, k)
        if not in_golden(r):
            continue
        ref = golden[at]
        at += 1
        assert {x: ref[x] for x in GOLDEN_KEYS} == {x: r[x] for x in GOLDEN_KEYS} and not refused[k], (name, k)
        assert reg[f + 34:f + HDR].tobytes().hex() == ref["tcphdr"], (name, k)
        assert int(reg[f + 16]) << 8 | int(reg[f + 17]) == 40 + r["paylen"], (name, k)
        assert (reg[f + HDR:f + HDR + n] == before[src:src + n]).all(), (name, k)
    assert at == len(golden), name
    diff = np.nonzero((reg != expect) & ~headers)[0]
    assert len(diff) == 0, f"{name}: byte {diff[0]} of the region changed"
    return len(segs)
