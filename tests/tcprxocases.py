"""The definition of gcl_tcp_rx_ooo (include/gclassify.h) in Python, and the
cases the CPU and GPU tests share.  The model transcribes tcp_rx_conn,
__tcp_rx_conn, tcp_rx_text and tcp_rx_append_text (runtime/net/tcp_in.c) line
by line over a dict of PCB fields and a real doubly linked list of mbuf records
for c->rxq_ooo (list_for_each_rev, list_add_after, list_add, list_top,
list_del); it knows nothing of csrc/gcl_tcprxo.h.  The named cases below carry
expected values written out by hand from the reference's lines; the pin to
the reference's own code is tests/golden/tcprx_ref.json, what tcp_in.c,
compiled in place (oracle/ref_tcpin.c), did with every segment of these cases:
tests/tcprxrefcases.py holds this model, the host twin and the kernel to it.
What is the same as in gcl_tcp_rx_full (is_acceptable, the wraps_*
comparisons, the frame builders) comes from tests/tcprxfcases.py.

A case is tests/tcprxfcases.py's dict plus optionally q_off (u32[nconn + 1]),
q (ENT records) and q_out_cap (default: room for every entry).
"""
import functools

import numpy as np

from tests import l4cases as lc
from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests.tcprxcases import (ACK_DELAYED, DROP, ELIGIBLE, FAST, M32, NA, NOCONN, NONE, REP_ACKS_RESET, RXQ, SLOW,
                              STOPPED, TCP_ACK, TCP_FIN, TCP_PUSH, TCP_RST, TCP_SYN, TCP_URG, TIMER_ARMED, WOKEN,
                              wraps_gt, wraps_lt, wraps_lte)
from tests.tcprxfcases import (C_ACKS, C_BYTES, C_DROPPED, C_DUPACKS, C_FASTRTX, C_RULE2, C_TXWAKES, C_WAKES,
                               SF_ACK_NOW, SF_ACKED, SF_DROPPED, SF_FASTRTX, SF_RULE2, SF_TXWAKE, SF_WAKE, SF_WND,
                               X_FASTRTX, X_TXWAKE)

CAP, ESTABLISHED, X_QSKIP = 64, 0x80, 4
O_OOO, O_QUEUED, O_HEADCLIP, O_LATE_DRAINED, O_LATE_FREED, O_HELD = 1, 2, 4, 8, 0x10, 0x20
Q_UNTOUCHED, Q_KEPT, Q_FREED, Q_DRAINED = 0, 1, 2, 3
C_OOO, C_QUEUED, C_DRAINED, C_FREED, C_HEADCLIP, C_HELD, NR = 13, 14, 15, 16, 17, 18, 19
ENT = np.dtype([("seq", "<u4"), ("end", "<u4"), ("ref", "<u4"), ("flags", "<u2"), ("src", "<u2")])
EXT, CONN, CONN_OUT, SENTINEL, GUARD = fc.EXT, rc.CONN, rc.CONN_OUT, rc.SENTINEL, rc.GUARD
ENTRY = rc.ENTRY + (("oflags", np.uint8), ("skip", np.uint16))
QIN = (("qin_state", np.uint8), ("qin_skip", np.uint16), ("qin_len", np.uint16), ("qin_dst_off", np.uint64))


def wraps_gte(a, b):
    # inc/base/stddef.h
    return not wraps_lt(a, b)


# ---------------------------------------------------------------- base/list.h, as far as tcp_in.c uses it
class Node:
    __slots__ = ("m", "prev", "next")

    def __init__(self, m=None):
        self.m, self.prev, self.next = m, self, self


class List:
    def __init__(self):
        self.h = Node()

    def empty(self):
        return self.h.next is self.h

    def top(self):
        return None if self.empty() else self.h.next

    def add_after(self, pos, m):
        n = Node(m)
        n.prev, n.next = pos, pos.next
        pos.next.prev = n
        pos.next = n

    def add(self, m):
        self.add_after(self.h, m)

    def add_tail(self, m):
        self.add_after(self.h.prev, m)

    def delete(self, n):
        n.prev.next, n.next.prev = n.next, n.prev

    def rev(self):
        n = self.h.prev
        while n is not self.h:
            yield n
            n = n.prev

    def __iter__(self):
        n = self.h.next
        while n is not self.h:
            yield n.m
            n = n.next

    def __len__(self):
        return sum(1 for _ in self)


class Stop(Exception):
    """the segment leaves for the runtime's own __tcp_rx_conn"""


def tcp_rx_append_text(c, m):
    # :72-73
    assert wraps_lte(m["seg_seq"], c["rcv_nxt"]) and wraps_gt(m["seg_end"], c["rcv_nxt"])
    # :76-80
    if wraps_lt(m["seg_seq"], c["rcv_nxt"]):
        ln = (c["rcv_nxt"] - m["seg_seq"]) & M32
        m["pulled"] += ln                       # mbuf_pull
        m["len"] -= ln
        m["seg_seq"] = (m["seg_seq"] + ln) & M32
    # :83-87
    if wraps_lt((c["rcv_nxt"] + c["rcv_wnd"]) & M32, m["seg_end"]):
        ln = (m["seg_end"] - ((c["rcv_nxt"] + c["rcv_wnd"]) & M32)) & M32
        assert ln <= m["len"]                   # mbuf_trim: the windows of the tests stay below 2^31
        m["len"] -= ln
        m["seg_end"] = (c["rcv_nxt"] + c["rcv_wnd"]) & M32
    # :90-94
    got = (m["seg_end"] - m["seg_seq"]) & M32
    assert c["rcv_wnd"] >= got and got == m["len"]
    c["rcv_wnd"] = (c["rcv_wnd"] - got) & M32
    c["rcv_nxt"] = m["seg_end"]
    c["rxq"] = True
    c["rxq_list"].append(m)


def tcp_rx_text(c, m, out):
    # :105-106
    if c["rcv_wnd"] == 0:
        return False
    if wraps_lte(m["seg_seq"], c["rcv_nxt"]):
        # :111-116
        if (m["flags"] & (TCP_PUSH | TCP_FIN)) != 0 or c["rxq"]:
            out["wake"] = True
        tcp_rx_append_text(c, m)
    else:
        # :119-135.  TCP_OOO_MAX_SIZE (2048) is out of reach: the call's own cap is 64
        c["n_ooo"] += 1
        m["oflags"] |= O_OOO
        ooo = c["rxq_ooo"]
        for pos in ooo.rev():
            if wraps_gt(m["seg_end"], pos.m["seg_end"]):
                if len(ooo) >= CAP:
                    raise Stop                  # the call's own line: the 65th entry is the runtime's
                ooo.add_after(pos, m)
                break
            elif wraps_gte(m["seg_seq"], pos.m["seg_seq"]):
                return False
        else:
            if len(ooo) >= CAP:
                raise Stop
            ooo.add(m)
        m["oflags"] |= O_QUEUED
        c["n_queued"] += 1
    # drain, :140-163
    while True:
        pos = c["rxq_ooo"].top()
        if pos is None:
            break
        if wraps_lte(pos.m["seg_end"], c["rcv_nxt"]):
            c["rxq_ooo"].delete(pos)
            pos.m["fate"] = "freed"             # mbuf_free
            c["n_freed"] += 1
            continue
        if wraps_gt(pos.m["seg_seq"], c["rcv_nxt"]):
            break
        c["rxq_ooo"].delete(pos)
        out["wake"] = True
        pos.m["fate"] = "drained"
        c["n_drained"] += 1
        tcp_rx_append_text(c, pos.m)
    # :165-166
    if c["rcv_wnd"] == 0:
        out["wake"] = True
    return True


SCALARS = ("snd_una", "snd_wnd", "snd_wl1", "snd_wl2", "rcv_nxt", "rcv_wnd", "acks_delayed_cnt", "ack_delayed",
           "rxq", "woken", "armed", "rep_reset", "rep_acks", "fast_rtx_ack", "xflags", "dupacks", "n_ooo")


def slow_rx_conn(c, m, ack, snd_nxt, win):
    """__tcp_rx_conn (:352-611) for a connection in ESTABLISHED.  Returns the
    sflags of the segment; raises Stop, with nothing changed, for what the call
    leaves to the runtime."""
    sf = SF_RULE2
    do_ack, do_drop, ack_same, wnd_updated = False, True, False, False
    seq, ln = m["seg_seq"], m["len"]
    # the call's own line: the flags whose steps (:369, :444, :452, step 6) end, reset or mark the connection
    if m["flags"] & (TCP_FIN | TCP_RST | TCP_URG | TCP_SYN):
        raise Stop
    saved = {k: c[k] for k in SCALARS}
    try:
        while True:                              # 'break' is 'goto done'
            # :438-441
            if not fc.is_acceptable(c, ln, seq, m["flags"]):
                do_ack = (m["flags"] & TCP_RST) == 0
                break
            # :459-461
            if (m["flags"] & TCP_ACK) == 0:
                break
            # :476-501
            snd_was_full = fc.tcp_is_snd_full(c)
            if wraps_lte(c["snd_una"], ack) and wraps_lte(ack, snd_nxt):
                if c["snd_una"] != ack:
                    c["snd_una"] = ack
                    sf |= SF_ACKED
                else:
                    ack_same = True
                if wraps_lt(c["snd_wl1"], seq) or (c["snd_wl1"] == seq and wraps_lte(c["snd_wl2"], ack)):
                    if not ack_same or c["snd_wnd"] <= win:
                        if c["snd_wnd"] != win or c["snd_wl2"] != ack:
                            wnd_updated = True
                        c["snd_wnd"], c["snd_wl1"], c["snd_wl2"] = win, seq, ack
                        sf |= SF_WND
            elif wraps_gt(ack, snd_nxt):
                do_ack = True
                break
            # :502-505
            if snd_was_full and not fc.tcp_is_snd_full(c):
                sf |= SF_TXWAKE
                c["xflags"] |= X_TXWAKE
            # :514-528
            if ack_same and c["snd_una"] != c["snd_nxt"] and ln == 0 and not wnd_updated:
                c["rep_acks"] += 1
                c["dupacks"] += 1
                if c["rep_acks"] >= fc.TCP_FAST_RETRANSMIT_THRESH:
                    sf |= SF_FASTRTX
                    c["fast_rtx_ack"] = ack
                    c["xflags"] |= X_FASTRTX
                    c["rep_acks"] = 0
                    c["rep_reset"] = True
            elif c["snd_una"] == ack:
                c["rep_acks"] = 0
                c["rep_reset"] = True
            # :547-575
            if ln > 0:
                o = {"wake": False}
                do_drop = not tcp_rx_text(c, m, o)
                if o["wake"]:
                    assert c["rxq"] and not do_drop
                    sf |= SF_WAKE
                    c["woken"] = True
                c["acks_delayed_cnt"] += 1
                if c["acks_delayed_cnt"] >= 2:
                    do_ack = True
                elif not c["ack_delayed"]:
                    c["ack_delayed"] = True
                    c["armed"] = True
                # :574
                do_ack |= not c["rxq_ooo"].empty()
            break
    except Stop:
        c.update(saved)                          # the queue itself was not touched yet
        m["oflags"] = 0
        raise
    # done, :593-598
    if do_ack:
        c["ack_delayed"] = False
        c["acks_delayed_cnt"] = 0
        sf |= SF_ACK_NOW
    if do_drop:
        sf |= SF_DROPPED
    return sf


def queue_range(case, k):
    q_off, nq = case.get("q_off"), len(case["q"]) if case.get("q") is not None else 0
    if q_off is None:
        return 0, 0
    a, b = min(int(q_off[k]), nq), min(int(q_off[k + 1]), nq)
    return a, max(a, b)


def model(case, with_rxq=False):
    """Every output of one call as a dict; with @with_rxq also 'rxq': per
    connection the bytes of the mbufs appended to c->rxq, in order (list
    entries only)."""
    order, sock, st, conn = case.get("order"), case["sock"], case.get("st"), case["conn"]
    align = max(case.get("align", 0), 1)
    pay = pc.model(case, order, sock, st)
    n, nconn = len(case["pkt_len"]), len(conn)
    rep = case.get("rep_acks")
    q = case.get("q")
    nq = 0 if q is None else len(q)
    idx = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    m = len(idx)
    out = {f: np.zeros(m, dtype=dt) for f, dt in ENTRY}
    out.update({f: np.zeros(nq, dtype=dt) for f, dt in QIN})
    counts = [0] * NR
    pcb = [{k: int(conn[c][k]) for k in CONN.names if k != "pad"} for c in range(nconn)]
    mbufs = {}
    for k, c in enumerate(pcb):
        c.update(rxq=bool(c["flags"] & RXQ), ack_delayed=bool(c["flags"] & ACK_DELAYED), stopped=False, woken=False,
                 armed=False, rep_reset=False, nfast=0, nslow=0, nacks=0, first_slow=NONE, rxq_list=[],
                 rep_acks=0 if rep is None else int(rep[k]), fast_rtx_ack=0, xflags=0, dupacks=0, nrule2=0,
                 ndropped=0, rxq_ooo=List(), n_ooo=0, n_queued=0, n_drained=0, n_freed=0)
        a, b = queue_range(case, k)
        c["taken"] = bool(c["flags"] & (ELIGIBLE | ESTABLISHED)) and b - a <= CAP and \
            not any(int(q[i]["flags"]) & TCP_FIN for i in range(a, b))
        if c["taken"]:
            for i in range(a, b):
                mb = {"seg_seq": int(q[i]["seq"]), "seg_end": int(q[i]["end"]), "flags": int(q[i]["flags"]),
                      "len": (int(q[i]["end"]) - int(q[i]["seq"])) & M32, "pulled": 0, "qi": i, "fate": None,
                      "ref": int(q[i]["ref"]), "oflags": 0}
                c["rxq_ooo"].add_tail(mb)
                mbufs["q", i] = mb
        elif b > a:
            c["xflags"] |= X_QSKIP
    for j in range(m):
        if pay["kind"][j] != pc.K_TCP:
            out["verdict"][j] = NA
            counts[NA] += 1
            continue
        i = int(idx[j])
        ck = int(sock[i])
        if ck >= nconn:
            out["verdict"][j] = NOCONN
            counts[NOCONN] += 1
            continue
        c = pcb[ck]
        o = int(case["offs"][i]) if case["offs"] is not None else i * case["stride"]
        f = case["frames"][o:]
        snd_nxt = c["snd_nxt"]
        seq, ack = pc.be(f, 38, 4), pc.be(f, 42, 4)
        win = (pc.be(f, 48, 2) << (c["snd_wscale"] & 31)) & M32
        flags = int(f[47])
        ln = int(pay["len"][j])
        if ln > c["rcv_mss"]:
            out["verdict"][j] = DROP
            counts[DROP] += 1
            continue
        mb = {"seg_seq": seq, "seg_end": (seq + ln) & M32, "flags": flags, "len": ln, "pulled": 0, "j": j,
              "src": int(pay["src_off"][j]), "fate": None, "oflags": 0}
        stop = c["stopped"] or not c["taken"]
        dup0, sf = c["dupacks"], 0
        if not stop:
            # :221-239
            slow_path = (flags & rc.TCP_SLOWPATH_FLAGS) != 0 or ln == 0 or wraps_gt(ack, snd_nxt)
            slow_path |= fc.tcp_is_snd_full(c)
            slow_path |= seq != c["rcv_nxt"] or not c["rxq_ooo"].empty()
            slow_path |= c["rcv_wnd"] < ln
            if slow_path:
                try:
                    sf = slow_rx_conn(c, mb, ack, snd_nxt, win)
                except Stop:
                    stop = True
            else:
                # :247-287
                if wraps_lte(c["snd_una"], ack):
                    if c["snd_una"] != ack:
                        c["rep_acks"], c["rep_reset"], c["snd_una"] = 0, True, ack
                        sf |= SF_ACKED
                    if wraps_lt(c["snd_wl1"], seq) or (c["snd_wl1"] == seq and wraps_lte(c["snd_wl2"], ack)):
                        c["snd_wnd"], c["snd_wl1"], c["snd_wl2"] = win, seq, ack
                        c["rep_acks"], c["rep_reset"] = 0, True
                        sf |= SF_WND
                c["rcv_nxt"] = (seq + ln) & M32
                c["rcv_wnd"] = (c["rcv_wnd"] - ln) & M32
                if c["rxq"] or (flags & TCP_PUSH) > 0:
                    sf |= SF_WAKE
                    c["woken"] = True
                c["acks_delayed_cnt"] += 1
                if c["acks_delayed_cnt"] >= 2:
                    c["ack_delayed"] = False
                    sf |= SF_ACK_NOW
                    c["acks_delayed_cnt"] = 0
                elif not c["ack_delayed"]:
                    c["armed"] = True
                    c["ack_delayed"] = True
                c["rxq"] = True
                c["rxq_list"].append(mb)
        if stop:
            if not c["stopped"]:
                c["first_slow"] = j
            c["stopped"] = True
            c["nslow"] += 1
            out["verdict"][j] = SLOW
            counts[SLOW] += 1
            continue
        mbufs["j", j] = mb
        c["nfast"] += 1
        c["nacks"] += bool(sf & SF_ACK_NOW)
        c["nrule2"] += bool(sf & SF_RULE2)
        c["ndropped"] += bool(sf & SF_DROPPED)
        out["verdict"][j], out["sflags"][j], out["rcv_nxt_after"][j] = FAST, sf, c["rcv_nxt"]
        counts[FAST] += 1
        for slot, bit in ((C_ACKS, SF_ACK_NOW), (C_WAKES, SF_WAKE), (C_RULE2, SF_RULE2), (C_TXWAKES, SF_TXWAKE),
                          (C_FASTRTX, SF_FASTRTX), (C_DROPPED, SF_DROPPED)):
            counts[slot] += bool(sf & bit)
        counts[C_DUPACKS] += c["dupacks"] - dup0
    oc, ext = np.zeros(nconn, dtype=CONN_OUT), np.zeros(nconn, dtype=EXT)
    off, at = np.zeros(nconn + 1, dtype=np.uint64), 0
    qout, qout_off = [], np.zeros(nconn + 1, dtype=np.uint32)
    for k, c in enumerate(pcb):
        fl = (RXQ if c["rxq"] else 0) | (ACK_DELAYED if c["ack_delayed"] else 0) | \
             (STOPPED if c["stopped"] else 0) | (WOKEN if c["woken"] else 0) | \
             (TIMER_ARMED if c["armed"] else 0) | (REP_ACKS_RESET if c["rep_reset"] else 0)
        oc[k] = (c["snd_una"], c["snd_wnd"], c["snd_wl1"], c["snd_wl2"], c["rcv_nxt"], c["rcv_wnd"], c["nfast"],
                 c["nslow"], c["nacks"], c["first_slow"], c["acks_delayed_cnt"], fl, 0)
        ext[k] = (c["nrule2"], c["ndropped"], c["fast_rtx_ack"], c["rep_acks"] & 0xFF, c["xflags"], 0)
        off[k] = at
        pos = 0
        for mb in c["rxq_list"]:                  # the layout: rxq in order
            if "j" in mb:
                j = mb["j"]
                out["copy_len"][j], out["skip"][j] = mb["len"], mb["pulled"]
                out["dst_off"][j] = at + pos if mb["len"] else 0
                if mb["pulled"]:
                    mb["oflags"] |= O_HEADCLIP
                    counts[C_HEADCLIP] += 1
                if mb["fate"] == "drained":
                    mb["oflags"] |= O_LATE_DRAINED
            else:
                i = mb["qi"]
                out["qin_state"][i] = Q_DRAINED
                out["qin_skip"][i], out["qin_len"][i] = min(mb["pulled"], 0xFFFF), min(mb["len"], 0xFFFF)
                out["qin_dst_off"][i] = at + pos if mb["len"] else 0
                counts[C_HEADCLIP] += bool(mb["pulled"])
            pos += mb["len"]
        assert pos == (c["rcv_nxt"] - int(conn[k]["rcv_nxt"])) & M32
        counts[C_BYTES] += pos
        at += -(-pos // align) * align
        qout_off[k] = len(qout)
        for mb in c["rxq_ooo"]:
            if "j" in mb:
                mb["oflags"] |= O_HELD
                counts[C_HELD] += 1
                qout.append((mb["seg_seq"], mb["seg_end"], mb["j"], mb["flags"], 1))
            else:
                out["qin_state"][mb["qi"]] = Q_KEPT
                qout.append((mb["seg_seq"], mb["seg_end"], mb["ref"], mb["flags"], 0))
        counts[C_OOO] += c["n_ooo"]
        counts[C_QUEUED] += c["n_queued"]
        counts[C_DRAINED] += c["n_drained"]
        counts[C_FREED] += c["n_freed"]
    for key, mb in mbufs.items():
        if mb["fate"] == "freed":
            if key[0] == "j":
                mb["oflags"] |= O_LATE_FREED
            else:
                out["qin_state"][key[1]] = Q_FREED
        if key[0] == "j":
            out["oflags"][key[1]] = mb["oflags"]
    off[nconn] = at
    qout_off[nconn] = len(qout)
    assert sum(counts[:5]) == m
    res = dict(out, out_conn=oc, out_ext=ext, conn_off=off, counts=np.array(counts, dtype=np.uint64),
               qout_off=qout_off, qout=np.array(qout, dtype=ENT) if qout else np.zeros(0, dtype=ENT),
               totals=np.array([len(qout)], dtype=np.uint64))
    if with_rxq:
        assert all("j" in mb for c in pcb for mb in c["rxq_list"])
        res["rxq"] = [b"".join(case["frames"][mb["src"] + mb["pulled"]:mb["src"] + mb["pulled"] + mb["len"]].tobytes()
                               for mb in c["rxq_list"]) for c in pcb]
    return res


# ---------------------------------------------------------------- named cases
conn1, seg, build = rc.conn1, rc.seg, rc.build
R, D, A, W, K, N = SF_RULE2, SF_DROPPED, SF_ACK_NOW, SF_WAKE, SF_ACKED, SF_WND
QH = O_OOO | O_QUEUED | O_HELD
QD = O_OOO | O_QUEUED | O_LATE_DRAINED


def ents(rows):
    """ENT records of (seq, end[, ref[, flags]]) rows"""
    a = np.zeros(len(rows), dtype=ENT)
    for k, r in enumerate(rows):
        a[k] = (r[0] & M32, r[1] & M32, r[2] if len(r) > 2 else 1000 + k, r[3] if len(r) > 3 else TCP_ACK, 0)
    return a


def qcap(case):
    if "q_out_cap" in case:
        return case["q_out_cap"]
    m, _ = fc.dims(case)
    return m + (len(case["q"]) if case.get("q") is not None else 0)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (case, expected).  @expected holds values derived by hand from
    tcp_in.c for conn1(snd_wl1=50000): snd_una 1000 == every segment's ack, so
    ack_same holds, :487 never takes the window (50000 is past every seq used)
    and a slow text segment's sflags are RULE2 plus what the text step gives;
    rcv_nxt 100, rcv_wnd 2^20, acks_delayed_cnt 0, no ACK_DELAYED, no RXQ.
    S(k) is the 100-byte segment [100 + 100 k, 200 + 100 k).  Keys: 'verdict',
    'sflags', 'copy', 'after', 'skip', 'oflags', 'dst' per entry; 'oc' and
    'ext' fields of connection 0; 'counts'; 'qout' rows (seq, end, ref, src);
    'qout_off'; 'qin_state', 'qin_len', 'qin_skip', 'qin_dst'; 'totals'."""
    rng = np.random.default_rng(93)
    res = {}

    def add(name, cs, segs, exp, q_off=None, q=None, **kw):
        case = build(cs, segs, **kw)
        if q is not None:
            case["q_off"], case["q"] = np.array(q_off, dtype=np.uint32), q
        res[name] = (case, exp)

    c = conn1(snd_wl1=50000)

    def S(k, ln=100, **kw):
        return seg(rng, 0, 100 + 100 * k, ln, **kw)

    # S1 is queued at the head of an empty queue (:134); :568 counts 0 -> 1 and arms, :574 sends the ACK and
    # done clears both.  S0 is slow by :233's second half, appends 100 (no wake: no PSH, rxq empty), the drain
    # pops S1 (wake), the queue is empty: 0 -> 1, armed again, no ACK
    add("hole_filled_by_next", [c], [S(1), S(0)],
        dict(verdict=[FAST, FAST], sflags=[R | A, R | W], copy=[100, 100], after=[100, 300], dst=[100, 0],
             skip=[0, 0], oflags=[QD, 0], qout=[], totals=0,
             oc=dict(rcv_nxt=300, rcv_wnd=(1 << 20) - 200, nfast=2, nslow=0, nacks=1, acks_delayed_cnt=1,
                     flags=RXQ | ACK_DELAYED | WOKEN | TIMER_ARMED | REP_ACKS_RESET),
             ext=dict(nrule2=2, ndropped=0, xflags=0),
             counts={C_OOO: 1, C_QUEUED: 1, C_DRAINED: 1, C_FREED: 0, C_HELD: 0, C_BYTES: 200, C_ACKS: 1}))
    # S1 goes before S2 (:125 and :129 both fail against S2: the head, :134)
    add("three_in_reverse", [c], [S(2), S(1), S(0)],
        dict(verdict=[FAST] * 3, sflags=[R | A, R | A, R | W], copy=[100] * 3, after=[100, 100, 400],
             dst=[200, 100, 0], oflags=[QD, QD, 0], qout=[], oc=dict(rcv_nxt=400, nacks=2),
             counts={C_OOO: 2, C_QUEUED: 2, C_DRAINED: 2}))
    # S2 into the empty queue, S6 at the tail (:125 against S2), S4 in the middle (fails both against S6, :125
    # against S2), S1 at the head (fails both against all three)
    held4 = dict(verdict=[FAST] * 4, sflags=[R | A] * 4, copy=[0] * 4, oflags=[QH] * 4, after=[100] * 4,
                 qout=[(200, 300, 3, 1), (300, 400, 0, 1), (500, 600, 2, 1), (700, 800, 1, 1)], qout_off=[0, 4],
                 totals=4, oc=dict(rcv_nxt=100, nacks=4, acks_delayed_cnt=0, flags=TIMER_ARMED | REP_ACKS_RESET),
                 counts={C_OOO: 4, C_QUEUED: 4, C_HELD: 4, C_BYTES: 0})
    add("insert_head_middle_tail", [c], [S(2), S(6), S(4), S(1)], held4)
    add("q_out_cap_one_short", [c], [S(2), S(6), S(4), S(1)], dict(held4, qout=held4["qout"][:3]), q_out_cap=3)
    # against S2 = [300, 400): the duplicate, [320, 380) and [350, 400) all fail :125 and meet :129: refused,
    # no drain, and :568-574 still run: the queue is not empty, so each is ACKed
    add("duplicate_contained_same_end", [c], [S(2), S(2), seg(rng, 0, 320, 60), seg(rng, 0, 350, 50)],
        dict(verdict=[FAST] * 4, sflags=[R | A, R | A | D, R | A | D, R | A | D], copy=[0] * 4,
             oflags=[QH, O_OOO, O_OOO, O_OOO], qout=[(300, 400, 0, 1)],
             ext=dict(nrule2=4, ndropped=3), counts={C_OOO: 4, C_QUEUED: 1, C_DROPPED: 3, C_HELD: 1}))
    # [150, 180) is queued; [100, 200) passes it: :146 frees it, no wake
    add("freed_as_already_received", [c], [seg(rng, 0, 150, 30), S(0)],
        dict(verdict=[FAST] * 2, sflags=[R | A, R], copy=[0, 100], oflags=[O_OOO | O_QUEUED | O_LATE_FREED, 0],
             qout=[], oc=dict(rcv_nxt=200, acks_delayed_cnt=1), counts={C_FREED: 1, C_DRAINED: 0, C_BYTES: 100}))
    # [99, 199): its last byte is in the window (:49), :76 pulls one byte
    add("head_clip_by_one", [c], [seg(rng, 0, 99, 100)],
        dict(verdict=[FAST], sflags=[R], copy=[99], skip=[1], dst=[0], oflags=[O_HEADCLIP], after=[199],
             oc=dict(rcv_nxt=199, rcv_wnd=(1 << 20) - 99), counts={C_HEADCLIP: 1, C_OOO: 0}))
    # the window is [100, 350).  X = [150, 400) is queued (its first byte is inside).  S0 leaves rcv_nxt 200 and
    # a window of 150; the drain pulls 50 off X's head first, then trims its tail to 350: 150 bytes, window 0
    cw = conn1(snd_wl1=50000, rcv_wnd=250)
    add("head_and_tail_clip_on_one", [cw], [seg(rng, 0, 150, 250), S(0)],
        dict(verdict=[FAST] * 2, sflags=[R | A, R | W], copy=[150, 100], skip=[50, 0], dst=[100, 0],
             oflags=[QD | O_HEADCLIP, 0], after=[100, 350], oc=dict(rcv_nxt=350, rcv_wnd=0),
             counts={C_HEADCLIP: 1, C_DRAINED: 1, C_BYTES: 250}))
    # X = [200, 400) and Y = [345, 410) (after X by :125).  S0, then X trimmed to [200, 350): the window is 0;
    # Y is neither received (:146) nor ahead (:154): popped, 5 bytes pulled, trimmed to nothing, in rxq empty
    add("drain_to_window_0_then_zero_bytes", [cw], [seg(rng, 0, 200, 200), seg(rng, 0, 345, 65), S(0)],
        dict(verdict=[FAST] * 3, sflags=[R | A, R | A, R | W], copy=[150, 0, 100], skip=[0, 5, 0],
             dst=[100, 0, 0], oflags=[QD, QD | O_HEADCLIP, 0], qout=[], oc=dict(rcv_nxt=350, rcv_wnd=0),
             counts={C_DRAINED: 2, C_HEADCLIP: 1, C_BYTES: 250}))
    # :568 leaves the counter at 1 and would only arm; :574 alone gives the ACK
    add("dup_ack_line_574", [c], [S(2)],
        dict(sflags=[R | A], oc=dict(nacks=1, acks_delayed_cnt=0, flags=TIMER_ARMED | REP_ACKS_RESET),
             counts={C_ACKS: 1}))
    # after S0 the queue is empty again: S2 is gcl_tcp_rx's FAST (no RULE2): rxq holds bytes (WAKE), 1 -> 2: ACK
    add("drains_empty_then_fast", [c], [S(1), S(0), S(2)],
        dict(verdict=[FAST] * 3, sflags=[R | A, R | W, W | A], copy=[100] * 3, dst=[100, 0, 200],
             oc=dict(rcv_nxt=400, nacks=2, acks_delayed_cnt=0), ext=dict(nrule2=2)))
    # rcv_nxt 0xFFFFFF00.  P = [0x100, 0x164), Q = [0xFFFFFF80, 0xFFFFFFE4) goes before it, Z = [0xFFFFFFE4, 0x48)
    # between them; [0xFFFFFF00, 0xFFFFFF80) then drains Q and Z across 2^32 and stops at P
    cwr = conn1(snd_wl1=50000, rcv_nxt=0xFFFFFF00)
    add("wrap_inside_the_queue", [cwr], [seg(rng, 0, 0x100, 100), seg(rng, 0, 0xFFFFFF80, 100),
                                          seg(rng, 0, 0xFFFFFFE4, 100), seg(rng, 0, 0xFFFFFF00, 128)],
        dict(verdict=[FAST] * 4, sflags=[R | A, R | A, R | A, R | W | A], copy=[0, 100, 100, 128],
             dst=[0, 128, 228, 0], oflags=[QH, QD, QD, 0], after=[0xFFFFFF00] * 3 + [0x48],
             qout=[(0x100, 0x164, 0, 1)], oc=dict(rcv_nxt=0x48, nacks=4)))
    # 64 entries of 10 bytes, each at the tail; a duplicate of the first is refused by :129 and does not stop;
    # the 65th insert does, and what follows is SLOW
    full = [seg(rng, 0, 1000 + 20 * k, 10) for k in range(CAP)]
    add("insert_65_stops", [c], full + [seg(rng, 0, 1000, 10), seg(rng, 0, 5000, 10), S(0)],
        dict(verdict=[FAST] * 65 + [SLOW, SLOW], sflags=[R | A] * 64 + [R | A | D, 0, 0],
             oflags=[QH] * 64 + [O_OOO, 0, 0], qout=[(1000 + 20 * k, 1010 + 20 * k, k, 1) for k in range(CAP)],
             oc=dict(rcv_nxt=100, nfast=65, nslow=2, first_slow=65, nacks=65),
             counts={C_QUEUED: 64, C_OOO: 65, C_HELD: 64, SLOW: 2}))
    ce = conn1(snd_wl1=50000, flags=ESTABLISHED)
    # an input entry with FIN, and 65 input entries: not taken, the queue stays with the runtime
    add("input_queue_with_fin", [ce], [S(0)],
        dict(verdict=[SLOW], qout=[], qout_off=[0, 0], qin_state=[Q_UNTOUCHED] * 2, ext=dict(xflags=X_QSKIP),
             oc=dict(flags=STOPPED, first_slow=0, rcv_nxt=100)),
        q_off=[0, 2], q=ents([(300, 400), (400, 500, 7, TCP_ACK | TCP_FIN)]))
    add("input_queue_of_65", [ce], [S(0)],
        dict(verdict=[SLOW], qout=[], qin_state=[Q_UNTOUCHED] * 65, ext=dict(xflags=X_QSKIP), totals=0),
        q_off=[0, 65], q=ents([(1000 + 20 * k, 1010 + 20 * k) for k in range(65)]))
    # ESTABLISHED without ELIGIBLE, one input entry [200, 300): S0 is slow by :233, appends, and the drain takes
    # the input entry: its bytes land behind S0's
    add("input_entry_drained", [ce], [S(0)],
        dict(verdict=[FAST], sflags=[R | W], copy=[100], qin_state=[Q_DRAINED], qin_len=[100], qin_skip=[0],
             qin_dst=[100], qout=[], oc=dict(rcv_nxt=300, flags=RXQ | ACK_DELAYED | WOKEN | TIMER_ARMED | REP_ACKS_RESET),
             counts={C_DRAINED: 1, C_BYTES: 200}),
        q_off=[0, 1], q=ents([(200, 300, 77)]))
    # the reference's walk on a list that is not sorted: [500, 600) at the head hides [300, 400) from the drain
    # (:154 breaks at the head), and S3 = [400, 500) meets :125 against [300, 400) at the tail: after it
    add("unsorted_input_queue", [ce], [seg(rng, 0, 100, 200), S(3)],
        dict(verdict=[FAST] * 2, sflags=[R | A, R | A], copy=[200, 0], oflags=[0, QH],
             qin_state=[Q_KEPT, Q_KEPT], qout=[(500, 600, 1000, 0), (300, 400, 1001, 0), (400, 500, 1, 1)],
             oc=dict(rcv_nxt=300)),
        q_off=[0, 2], q=ents([(500, 600), (300, 400)]))
    # an entry whose end lies before its seq meets both :146 and :154 once S0 has moved rcv_nxt to 200: the
    # reference asks :146 first and frees it (no wake, and the queue is empty: no ACK)
    add("reversed_input_entry_is_freed", [ce], [S(0)],
        dict(verdict=[FAST], sflags=[R], copy=[100], qin_state=[Q_FREED], qout=[], totals=0,
             oc=dict(rcv_nxt=200, acks_delayed_cnt=1), counts={C_FREED: 1, C_DRAINED: 0}),
        q_off=[0, 1], q=ents([(500, 150)]))
    # q_off past nq, reversed and out of order: connection 0 owns q[2, 4), 1 nothing ([4, 0) is reversed),
    # 2 q[0, 2); nothing else is read
    add("garbage_q_off", [ce, ce, ce], [seg(rng, 1, 100, 100)],
        dict(verdict=[FAST], sflags=[0], qout_off=[0, 2, 2, 4], qin_state=[Q_KEPT] * 4,
             qout=[(700, 800, 1002, 0), (900, 1000, 1003, 0), (300, 400, 1000, 0), (500, 600, 1001, 0)], totals=4),
        q_off=[2, 0xFFFFFFFF, 0, 2], q=ents([(300, 400), (500, 600), (700, 800), (900, 1000)]))
    # the same q_off, and now both connections that own entries have a segment: [800, 900) goes between
    # connection 0's two entries (:125 against [700, 800)), [600, 700) behind connection 2's (:125 at the tail)
    add("q_off_out_of_order_with_runs", [ce, ce, ce], [seg(rng, 0, 800, 100), seg(rng, 2, 600, 100)],
        dict(verdict=[FAST, FAST], sflags=[R | A, R | A], oflags=[QH, QH], qout_off=[0, 3, 3, 6],
             qin_state=[Q_KEPT] * 4, totals=6,
             qout=[(700, 800, 1002, 0), (800, 900, 0, 1), (900, 1000, 1003, 0),
                   (300, 400, 1000, 0), (500, 600, 1001, 0), (600, 700, 1, 1)]),
        q_off=[2, 0xFFFFFFFF, 0, 2], q=ents([(300, 400), (500, 600), (700, 800), (900, 1000)]))
    return res


def case_of(name):
    return cases()[name][0]


def check_expected(got, exp, what):
    """@got (a model()-shaped dict) against the hand-derived @exp of a named case"""
    for key, f in (("verdict", "verdict"), ("sflags", "sflags"), ("copy", "copy_len"), ("after", "rcv_nxt_after"),
                   ("skip", "skip"), ("oflags", "oflags"), ("dst", "dst_off"), ("qin_state", "qin_state"),
                   ("qin_len", "qin_len"), ("qin_skip", "qin_skip"), ("qin_dst", "qin_dst_off"),
                   ("qout_off", "qout_off")):
        if key in exp:
            assert got[f][:len(exp[key])].tolist() == list(exp[key]), (what, key, got[f].tolist())
    for key, f in (("oc", "out_conn"), ("ext", "out_ext")):
        for k, v in exp.get(key, {}).items():
            assert int(got[f][0][k]) == v, (what, f, k, int(got[f][0][k]), v)
    for slot, v in exp.get("counts", {}).items():
        assert int(got["counts"][slot]) == v, (what, "counts", slot, int(got["counts"][slot]))
    if "qout" in exp:
        rows = [(int(e["seq"]), int(e["end"]), int(e["ref"]), int(e["src"])) for e in got["qout"][:len(exp["qout"])]]
        assert rows == [tuple(r) for r in exp["qout"]], (what, rows)
    if "totals" in exp:
        assert int(got["totals"][0]) == exp["totals"], (what, got["totals"])


# ---------------------------------------------------------------- random streams
def random_case(seed, m=3000, nconn=40, align=0, swap=0.1, loss=0.05, inq=0.3, stops=0.002, seglen=None,
                window=None):
    """A random stream of about @m entries over @nconn connections.  Every
    connection sends a chain of in-order text; a fraction @loss of the segments
    is held back and retransmitted later, some as a longer segment that
    overlaps its neighbours; a fraction @swap trades places with a neighbour;
    pure ACKs are mixed in and about @stops carry FIN.  A fraction @inq of the
    connections enters with a queue: pieces of its own near future."""
    rng = np.random.default_rng(seed)
    cs, sends, q, q_off = [], [], [], [0]
    per = max(m // nconn, 1)
    for k in range(nconn):
        una = int(rng.integers(0, 1 << 32))
        rn = int(rng.choice([int(rng.integers(0, 1 << 32)), 0xFFFFFFFF - int(rng.integers(0, 3000))]))
        mss = int(rng.choice([1460, 536]))
        has_q = rng.random() < inq
        c = conn1(snd_una=una, snd_nxt=una + 40000, snd_wnd=int(rng.integers(50000, 90000)),
                  snd_wl1=rn - int(rng.integers(0, 3)), snd_wl2=una, rcv_nxt=rn,
                  rcv_wnd=window or int(rng.choice([1 << 20, int(rng.integers(20000, 60000))])), rcv_mss=mss,
                  snd_wscale=int(rng.integers(0, 8)),
                  flags=(ESTABLISHED if has_q else int(rng.choice([ELIGIBLE, ELIGIBLE | ESTABLISHED]))) |
                  (RXQ if rng.random() < 0.3 else 0) | (ACK_DELAYED if rng.random() < 0.3 else 0),
                  acks_delayed_cnt=int(rng.integers(0, 2)))
        if rng.random() < 0.03:
            c["flags"] &= ~(ELIGIBLE | ESTABLISHED)
        cs.append(c)
        at, chain = rn, []
        for _ in range(per):
            ln = seglen or int(rng.integers(1, mss + 1))
            chain.append((at, ln))
            at = (at + ln) & M32
        mine = []
        if has_q:                                    # a few of the chain's segments are in the queue already
            pick = sorted(set(int(x) for x in rng.integers(1, min(per, 12), size=int(rng.integers(1, 5)))))
            for p in pick:
                s0, ln = chain[p]
                q.append((s0, s0 + ln, len(q) + 5000, TCP_ACK | (TCP_PUSH if rng.random() < 0.2 else 0)))
            chain = [x for p, x in enumerate(chain) if p not in pick or rng.random() < 0.3]
        late = []
        for p, (s0, ln) in enumerate(chain):
            r = rng.random()
            if r < loss:                             # lost: retransmitted a few segments later
                grow = int(rng.integers(0, 5))
                if grow == 1 and p + 1 < len(chain):
                    ln = min(mss, ln + int(rng.integers(1, 200)))      # overlaps the next segment
                elif grow == 2 and ln > 20:
                    s0, ln = (s0 + 10) & M32, ln - 10                  # a shorter one with the same end
                elif grow >= 3 and p + 1 < len(chain) and ln + chain[p + 1][1] <= mss:
                    ln += chain[p + 1][1]                              # covers the next segment whole: freed
                late.append((p + int(rng.integers(2, 9)), s0, ln))
                if rng.random() < 0.5:
                    continue                         # truly lost the first time
            mine.append((s0, ln))
            for x in [x for x in late if x[0] <= p]:
                late.remove(x)
                mine.append((x[1], x[2]))
        mine += [(x[1], x[2]) for x in late]
        for p in range(len(mine) - 1):
            if rng.random() < swap:
                mine[p], mine[p + 1] = mine[p + 1], mine[p]
        sends.append(mine)
        q_off.append(len(q))
    segs, st = [], []
    left = [list(reversed(s)) for s in sends]
    live = [k for k in range(nconn) if left[k]]
    una = [c["snd_una"] for c in cs]
    while live:
        k = live[int(rng.integers(0, len(live)))]
        c = cs[k]
        r = rng.random()
        if r < 0.08:
            una[k] = (una[k] + int(rng.integers(0, 300))) & M32
            segs.append(seg(rng, k, c["rcv_nxt"], 0, ack=una[k], win=int(rng.integers(0x4000, 1 << 16))))
        elif r < 0.08 + stops:
            segs.append(seg(rng, k, c["rcv_nxt"], 0, ack=una[k], flags=TCP_ACK | TCP_FIN))
        else:
            s0, ln = left[k].pop()
            segs.append(seg(rng, k, s0, ln, ack=una[k], win=int(rng.integers(0x4000, 1 << 16)),
                            flags=TCP_ACK | (TCP_PUSH if rng.random() < 0.2 else 0), doff=int(rng.choice([5, 8]))))
            if not left[k]:
                live.remove(k)
        st.append(lc.GOOD)
    case = build(cs, segs, align=align)
    case["st"] = np.array(st, dtype=np.uint8)
    case["rep_acks"] = rng.integers(0, 3, size=nconn).astype(np.uint8)
    case["q_off"], case["q"] = np.array(q_off, dtype=np.uint32), ents(q)
    return case


# seed, m, nconn, align, swap, loss: many short runs; an aligned layout and heavy loss; runs longer than a wave
STREAMS = ((1, 3000, 60, 0, 0.1, 0.05, 0.002), (2, 2500, 25, 64, 0.3, 0.15, 0.002),
           (3, 3000, 8, 0, 0.1, 0.08, 0.0002))


@functools.lru_cache(maxsize=None)
def stream(k):
    seed, m, nconn, align, swap, loss, stops = STREAMS[k]
    return random_case(seed, m, nconn, align=align, swap=swap, loss=loss, stops=stops)


def check_mix(want):
    """the conditions a random stream must meet, on the MODEL's output"""
    cnt = want["counts"]
    for slot in (C_OOO, C_QUEUED, C_DRAINED, C_FREED, C_HEADCLIP, C_HELD, C_DROPPED, C_RULE2, C_WAKES, C_ACKS):
        assert int(cnt[slot]) > 5, (slot, cnt)
    assert int(cnt[FAST]) - int(cnt[C_RULE2]) > 50                  # the fast path is taken again and again
    assert int(((want["oflags"] & O_OOO) != 0).sum() - ((want["oflags"] & O_QUEUED) != 0).sum()) > 3  # refused
    assert int((want["qin_state"] == Q_DRAINED).sum()) > 0


# ---------------------------------------------------------------- running the host twin
OOO_OUT = (("oflags", np.uint8, "m"), ("skip", np.uint16, "m"), ("qin_state", np.uint8, "nq"),
           ("qin_skip", np.uint16, "nq"), ("qin_len", np.uint16, "nq"), ("qin_dst_off", np.uint64, "nq"),
           ("qout_off", np.uint32, "nconn1"), ("qout", ENT, "cap"), ("totals", np.uint64, "one"))


def sizes(case):
    m, nconn = fc.dims(case)
    nq = len(case["q"]) if case.get("q") is not None else 0
    return {"m": m, "nconn": nconn, "nq": nq, "nconn1": nconn + 1, "cap": qcap(case), "one": 1}


def blank(case):
    z = sizes(case)
    b = fc.blank(z["m"], z["nconn"])
    for f, dt, by in OOO_OUT:
        b[f] = np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (z[by] + GUARD)), dtype=dt).copy()
    return b


def compare(got, want, case, what):
    """@got (blank() after a call) against @want: the written part equal byte for byte, the guards untouched;
    qout is written below min(wanted, q_out_cap) only"""
    z = sizes(case)
    fc.compare(got, want, z["m"], z["nconn"], what)
    for f, dt, by in OOO_OUT:
        k = z[by]
        wrote = min(k, len(want["qout"])) if f == "qout" else k
        g = got[f]
        assert len(g) == k + GUARD and (g[wrote:].view(np.uint8) == SENTINEL).all(), f"{what}: {f} written past its end"
        bad = np.nonzero(g[:wrote].view(np.uint8) != want[f][:wrote].view(np.uint8))[0]
        if len(bad):
            e = bad[0] // g.dtype.itemsize
            raise AssertionError(f"{what}: {f}[{e}] = {g[e]} != {want[f][e]} ({len(bad)} bytes differ)")


def run_host(g, case, counts=True):
    """gcl_tcp_rx_ooo_host over sentinel-filled outputs: (outputs, counts)"""
    z = sizes(case)
    out = blank(case)
    cnt = np.full(NR, 5, dtype=np.uint64) if counts else None
    g.tcp_rx_ooo_host(case["frames"], case["pkt_len"], case["sock"], case["conn"], stride=case["stride"],
                      offs=case["offs"], frames_len=case["frames_len"], order=case.get("order"), m=z["m"],
                      l4_status=case.get("st"), nconn=z["nconn"], align=case.get("align", 0),
                      blocks=case.get("blocks", 0), rep_acks=case.get("rep_acks"), q_off=case.get("q_off"),
                      q=case.get("q"), nq=z["nq"], q_out_cap=z["cap"], out=out, counts=cnt)
    return out, None if cnt is None else cnt - np.uint64(5)
