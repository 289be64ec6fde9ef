"""The cases of gcl_tcp_rx_states (include/gclassify.h) that the CPU and GPU
tests share, a plain Python transcription of the lines of __tcp_rx_conn
(runtime/net/tcp_in.c:352-611) the call adds to gcl_tcp_rx_ooo, and the
helpers that run the host twin.  The pin to the reference's own code is
tests/golden/tcprxs_ref.json (tests/golden/make_tcprxs_ref.py): what tcp_in.c,
compiled in place behind oracle/ref_tcpin.c, did with every segment of these
cases.

A case is tests/tcprxocases.py's dict plus 'state': u8[nconn] of enum tcp
state (runtime/net/tcp.h:41-52), or absent for state == NULL.
"""
import functools

import numpy as np

from tests import l4cases as lc
from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests import tcprxocases as oc
from tests.tcprxcases import (ACK_DELAYED, DROP, FAST, M32, NA, NOCONN, NONE, REP_ACKS_RESET, RXQ, SLOW, STOPPED,
                              TCP_ACK, TCP_FIN, TCP_PUSH, TCP_RST, TCP_SYN, TCP_URG, TIMER_ARMED, WOKEN, wraps_gt,
                              wraps_lt, wraps_lte)
from tests.tcprxfcases import (SF_ACK_NOW, SF_ACKED, SF_DROPPED, SF_FASTRTX, SF_RULE2, SF_TXWAKE, SF_WAKE, SF_WND,
                               X_FASTRTX, X_TXWAKE)
from tests.tcprxocases import (CAP, ENT, O_HEADCLIP, O_HELD, O_LATE_DRAINED, O_LATE_FREED, O_OOO, O_QUEUED,
                               Q_DRAINED, Q_FREED, Q_KEPT, X_QSKIP, List, wraps_gte)

(SYN_SENT, SYN_RECEIVED, ESTABLISHED, FIN_WAIT1, FIN_WAIT2, CLOSE_WAIT, CLOSING, LAST_ACK, TIME_WAIT,
 CLOSED) = range(10)
NOSTATE = 0xFF
EV_RST, EV_RST_ACK, EV_FAIL, EV_STATE, EV_FIN, EV_PUT = 1, 2, 4, 8, 0x10, 0x20
X_FAILED, X_PUT, X_TIMEWAIT, X_OPENED = 8, 0x10, 0x20, 0x40
C_RSTS, C_FAILS, C_FINS, C_STATE_CHANGES, NR = 19, 20, 21, 22, 23
TEXT_STATES = (ESTABLISHED, FIN_WAIT1, FIN_WAIT2)
ENTRY = oc.ENTRY + (("ev", np.uint8), ("rst_seq", np.uint32), ("state_after", np.uint8))
SENTINEL, GUARD = rc.SENTINEL, rc.GUARD


def state_in(case, k):
    """the state connection k enters with, as the header says"""
    if case.get("state") is not None:
        return int(case["state"][k])
    return ESTABLISHED if int(case["conn"][k]["flags"]) & (rc.ELIGIBLE | oc.ESTABLISHED) else NOSTATE


# ---------------------------------------------------------------- the transcription
class Stop(Exception):
    pass


def append_text(c, m):
    """tcp_rx_append_text, :64-95; m["len"] is the mbuf's length, seg_seq / seg_end sequence space"""
    assert wraps_lte(m["seg_seq"], c["rcv_nxt"]) and wraps_gt(m["seg_end"], c["rcv_nxt"])
    if wraps_lt(m["seg_seq"], c["rcv_nxt"]):
        ln = (c["rcv_nxt"] - m["seg_seq"]) & M32
        m["pulled"] += ln
        m["len"] -= ln
        m["seg_seq"] = (m["seg_seq"] + ln) & M32
    if wraps_lt((c["rcv_nxt"] + c["rcv_wnd"]) & M32, m["seg_end"]):
        ln = (m["seg_end"] - ((c["rcv_nxt"] + c["rcv_wnd"]) & M32)) & M32
        m["len"] = max(m["len"] - ln, 0)          # mbuf_trim; the FIN octet is counted in ln
        m["seg_end"] = (c["rcv_nxt"] + c["rcv_wnd"]) & M32
    got = (m["seg_end"] - m["seg_seq"]) & M32
    assert c["rcv_wnd"] >= got
    m["at"] = (m["seg_seq"] - c["rcv0"]) & M32
    c["rcv_wnd"] = (c["rcv_wnd"] - got) & M32
    c["rcv_nxt"] = m["seg_end"]
    c["rxq"] = True
    c["rxq_list"].append(m)


def rx_text(c, m, o):
    """tcp_rx_text, :98-169, with the call's own cap"""
    if c["rcv_wnd"] == 0:
        return False
    if wraps_lte(m["seg_seq"], c["rcv_nxt"]):
        if (m["flags"] & (TCP_PUSH | TCP_FIN)) != 0 or c["rxq"]:
            o["wake"] = True
            o["fin"] |= (m["flags"] & TCP_FIN) > 0
        append_text(c, m)
    else:
        ooo = c["rxq_ooo"]
        for pos in ooo.rev():
            if wraps_gt(m["seg_end"], pos.m["seg_end"]):
                if len(ooo) >= CAP:
                    raise Stop
                ooo.add_after(pos, m)
                break
            elif wraps_gte(m["seg_seq"], pos.m["seg_seq"]):
                m["oflags"] |= O_OOO
                c["n_ooo"] += 1
                return False
        else:
            if len(ooo) >= CAP:
                raise Stop
            ooo.add(m)
        m["oflags"] |= O_OOO | O_QUEUED
        c["n_ooo"] += 1
        c["n_queued"] += 1
    while True:
        pos = c["rxq_ooo"].top()
        if pos is None:
            break
        if wraps_lte(pos.m["seg_end"], c["rcv_nxt"]):
            c["rxq_ooo"].delete(pos)
            pos.m["fate"] = "freed"
            c["n_freed"] += 1
            continue
        if wraps_gt(pos.m["seg_seq"], c["rcv_nxt"]):
            break
        c["rxq_ooo"].delete(pos)
        o["wake"] = True
        o["fin"] |= (pos.m["flags"] & TCP_FIN) > 0
        pos.m["fate"] = "drained"
        c["n_drained"] += 1
        append_text(c, pos.m)
    if c["rcv_wnd"] == 0:
        o["wake"] = True
    return True


SCALARS = ("snd_una", "snd_wnd", "snd_wl1", "snd_wl2", "rcv_nxt", "rcv_wnd", "acks_delayed_cnt", "ack_delayed",
           "rxq", "woken", "armed", "rep_reset", "rep_acks", "fast_rtx_ack", "xflags", "dupacks", "state")


def slow_rx_conn(c, m, ack, snd_nxt, win):
    """__tcp_rx_conn, :352-611, without SYN_SENT.  Returns (sflags, ev, rst_seq)."""
    sf, ev, rst = SF_RULE2, 0, 0
    do_ack, do_drop, ack_same, wnd_updated = False, True, False, False
    seq, flags = m["seg_seq"], m["flags"]
    ln = m["len"] + (1 if flags & TCP_FIN else 0)                    # :367-370
    o = {"wake": False, "fin": False}
    saved = {k: c[k] for k in SCALARS}

    def set_state(s):
        nonlocal ev
        c["state"] = s
        ev |= EV_STATE

    def send_rst(acked):
        nonlocal ev, rst
        if acked:
            ev, rst = ev | EV_RST, ack
        else:
            ev, rst = ev | EV_RST_ACK, (seq + ln) & M32

    while True:                                                      # 'break' is 'goto done'
        if c["state"] == CLOSED:                                     # :372-376
            if not flags & TCP_RST:
                send_rst(False)
            break
        if not fc.is_acceptable(c, ln, seq, flags):                  # :438-441
            do_ack = (flags & TCP_RST) == 0
            break
        if flags & TCP_RST:                                          # :444-447
            ev |= EV_FAIL
            break
        if flags & TCP_SYN:                                          # :452-456
            send_rst((flags & TCP_ACK) > 0)
            ev |= EV_FAIL
            break
        if not flags & TCP_ACK:                                      # :459-461
            break
        if c["state"] == SYN_RECEIVED:                               # :462-473
            if not (wraps_lte(c["snd_una"], ack) and wraps_lte(ack, snd_nxt)):
                send_rst(True)
                break
            c["snd_wnd"], c["snd_wl1"], c["snd_wl2"] = win, seq, ack
            sf |= SF_WND
            set_state(ESTABLISHED)
            c["xflags"] |= X_OPENED
        snd_was_full = fc.tcp_is_snd_full(c)                         # :476-505
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
        if snd_was_full and not fc.tcp_is_snd_full(c):
            sf |= SF_TXWAKE
            c["xflags"] |= X_TXWAKE
        if ack_same and c["snd_una"] != snd_nxt and ln == 0 and not wnd_updated:     # :514-528
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
        if c["state"] == FIN_WAIT1 and c["snd_una"] == snd_nxt:      # :530-542
            set_state(FIN_WAIT2)
        elif c["state"] == CLOSING and c["snd_una"] == snd_nxt:
            c["xflags"] |= X_TIMEWAIT
            set_state(TIME_WAIT)
        elif c["state"] == LAST_ACK and c["snd_una"] == snd_nxt:
            set_state(CLOSED)
            ev |= EV_PUT
            c["xflags"] |= X_PUT
            break
        if ln > 0 and c["state"] in TEXT_STATES:                     # :547-575
            m["seg_end"] = (seq + ln) & M32
            try:
                do_drop = not rx_text(c, m, o)
            except Stop:
                c.update(saved)
                m["oflags"] = 0
                raise
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
            do_ack |= not c["rxq_ooo"].empty()
        if not o["fin"]:                                             # :578-590
            break
        ev |= EV_FIN
        if c["state"] == ESTABLISHED:
            set_state(CLOSE_WAIT)
        elif c["state"] == FIN_WAIT1:
            set_state(CLOSING)
        elif c["state"] == FIN_WAIT2:
            c["xflags"] |= X_TIMEWAIT
            do_ack = True
            set_state(TIME_WAIT)
        break
    if ev & EV_FAIL:
        c["xflags"] |= X_FAILED
    if do_ack:
        c["ack_delayed"] = False
        c["acks_delayed_cnt"] = 0
        sf |= SF_ACK_NOW
    if do_drop:
        sf |= SF_DROPPED
    return sf, ev, rst


def model(case, with_rxq=False):
    """Every output of one call as a dict; with @with_rxq also 'rxq': per
    connection (offset inside its region, bytes) of the mbufs appended to
    c->rxq, in order (list entries only)."""
    order, sock, st, conn = case.get("order"), case["sock"], case.get("st"), case["conn"]
    align = max(case.get("align", 0), 1)
    pay = pc.model(case, order, sock, st)
    n, nconn = len(case["pkt_len"]), len(conn)
    rep, q = case.get("rep_acks"), case.get("q")
    nq = 0 if q is None else len(q)
    idx = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    m = len(idx)
    out = {f: np.zeros(m, dtype=dt) for f, dt in ENTRY}
    out.update({f: np.zeros(nq, dtype=dt) for f, dt in oc.QIN})
    counts = [0] * NR
    pcb = [{k: int(conn[c][k]) for k in rc.CONN.names if k != "pad"} for c in range(nconn)]
    mbufs = {}
    for k, c in enumerate(pcb):
        c.update(rxq=bool(c["flags"] & RXQ), ack_delayed=bool(c["flags"] & ACK_DELAYED), stopped=False, woken=False,
                 armed=False, rep_reset=False, nfast=0, nslow=0, nacks=0, first_slow=NONE, rxq_list=[],
                 rep_acks=0 if rep is None else int(rep[k]), fast_rtx_ack=0, xflags=0, dupacks=0, nrule2=0,
                 ndropped=0, rxq_ooo=List(), n_ooo=0, n_queued=0, n_drained=0, n_freed=0, state=state_in(case, k),
                 dead=False, rcv0=c["rcv_nxt"])
        a, b = oc.queue_range(case, k)
        c["taken"] = 1 <= c["state"] <= 9 and b - a <= CAP
        if c["taken"]:
            for i in range(a, b):
                fl = int(q[i]["flags"])
                ln = (int(q[i]["end"]) - int(q[i]["seq"])) & M32
                mb = {"seg_seq": int(q[i]["seq"]), "seg_end": int(q[i]["end"]), "flags": fl,
                      "len": max(ln - (1 if fl & TCP_FIN else 0), 0), "pulled": 0, "qi": i, "fate": None,
                      "ref": int(q[i]["ref"]), "oflags": 0, "seq0": int(q[i]["seq"]), "end0": int(q[i]["end"])}
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
              "src": int(pay["src_off"][j]), "fate": None, "oflags": 0, "seq0": seq}
        stop = c["stopped"] or not c["taken"] or c["dead"]
        dup0, sf, ev, rst = c["dupacks"], 0, 0, 0
        if not stop:
            # :221-239
            slow_path = (flags & rc.TCP_SLOWPATH_FLAGS) != 0 or ln == 0 or wraps_gt(ack, snd_nxt)
            slow_path |= c["state"] != ESTABLISHED
            slow_path |= fc.tcp_is_snd_full(c)
            slow_path |= seq != c["rcv_nxt"] or not c["rxq_ooo"].empty()
            slow_path |= c["rcv_wnd"] < ln
            if slow_path:
                try:
                    sf, ev, rst = slow_rx_conn(c, mb, ack, snd_nxt, win)
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
                mb["at"] = (seq - c["rcv0"]) & M32
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
        c["dead"] = bool(ev & (EV_FAIL | EV_PUT))
        mbufs["j", j] = mb
        c["nfast"] += 1
        c["nacks"] += bool(sf & SF_ACK_NOW)
        c["nrule2"] += bool(sf & SF_RULE2)
        c["ndropped"] += bool(sf & SF_DROPPED)
        out["verdict"][j], out["sflags"][j], out["rcv_nxt_after"][j] = FAST, sf, c["rcv_nxt"]
        out["ev"][j], out["rst_seq"][j], out["state_after"][j] = ev, rst, c["state"]
        counts[FAST] += 1
        for slot, bit in ((fc.C_ACKS, SF_ACK_NOW), (fc.C_WAKES, SF_WAKE), (fc.C_RULE2, SF_RULE2),
                          (fc.C_TXWAKES, SF_TXWAKE), (fc.C_FASTRTX, SF_FASTRTX), (fc.C_DROPPED, SF_DROPPED)):
            counts[slot] += bool(sf & bit)
        counts[fc.C_DUPACKS] += c["dupacks"] - dup0
        counts[C_RSTS] += bool(ev & (EV_RST | EV_RST_ACK))
        counts[C_FAILS] += bool(ev & EV_FAIL)
        counts[C_FINS] += bool(ev & EV_FIN)
        counts[C_STATE_CHANGES] += bool(ev & EV_STATE)
    ocn, ext = np.zeros(nconn, dtype=rc.CONN_OUT), np.zeros(nconn, dtype=fc.EXT)
    off, at = np.zeros(nconn + 1, dtype=np.uint64), 0
    qout, qout_off = [], np.zeros(nconn + 1, dtype=np.uint32)
    state_out = np.zeros(nconn, dtype=np.uint8)
    for k, c in enumerate(pcb):
        fl = (RXQ if c["rxq"] else 0) | (ACK_DELAYED if c["ack_delayed"] else 0) | \
             (STOPPED if c["stopped"] else 0) | (WOKEN if c["woken"] else 0) | \
             (TIMER_ARMED if c["armed"] else 0) | (REP_ACKS_RESET if c["rep_reset"] else 0)
        ocn[k] = (c["snd_una"], c["snd_wnd"], c["snd_wl1"], c["snd_wl2"], c["rcv_nxt"], c["rcv_wnd"], c["nfast"],
                  c["nslow"], c["nacks"], c["first_slow"], c["acks_delayed_cnt"], fl, 0)
        ext[k] = (c["nrule2"], c["ndropped"], c["fast_rtx_ack"], c["rep_acks"] & 0xFF, c["xflags"], 0)
        state_out[k] = c["state"]
        off[k] = at
        for mb in c["rxq_list"]:                  # the layout: by sequence number
            if "j" in mb:
                j = mb["j"]
                out["copy_len"][j], out["skip"][j] = mb["len"], mb["pulled"]
                out["dst_off"][j] = at + mb["at"] if mb["len"] else 0
                if mb["pulled"]:
                    mb["oflags"] |= O_HEADCLIP
                    counts[oc.C_HEADCLIP] += 1
                if mb["fate"] == "drained":
                    mb["oflags"] |= O_LATE_DRAINED
            else:
                i = mb["qi"]
                out["qin_state"][i] = Q_DRAINED
                out["qin_skip"][i], out["qin_len"][i] = min(mb["pulled"], 0xFFFF), min(mb["len"], 0xFFFF)
                out["qin_dst_off"][i] = at + mb["at"] if mb["len"] else 0
                counts[oc.C_HEADCLIP] += bool(mb["pulled"])
        span = (c["rcv_nxt"] - c["rcv0"]) & M32
        counts[fc.C_BYTES] += span
        at += -(-span // align) * align
        qout_off[k] = len(qout)
        for mb in c["rxq_ooo"]:
            if "j" in mb:
                mb["oflags"] |= O_HELD
                counts[oc.C_HELD] += 1
                qout.append((mb["seg_seq"], mb["seg_end"], mb["j"], mb["flags"], 1))
            else:
                out["qin_state"][mb["qi"]] = Q_KEPT
                qout.append((mb["seg_seq"], mb["seg_end"], mb["ref"], mb["flags"], 0))
        counts[oc.C_OOO] += c["n_ooo"]
        counts[oc.C_QUEUED] += c["n_queued"]
        counts[oc.C_DRAINED] += c["n_drained"]
        counts[oc.C_FREED] += c["n_freed"]
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
    res = dict(out, out_conn=ocn, out_ext=ext, conn_off=off, counts=np.array(counts, dtype=np.uint64),
               qout_off=qout_off, qout=np.array(qout, dtype=ENT) if qout else np.zeros(0, dtype=ENT),
               totals=np.array([len(qout)], dtype=np.uint64), state_out=state_out)
    if with_rxq:
        res["rxq"] = [[(mb["at"], case["frames"][mb["src"] + mb["pulled"]:mb["src"] + mb["pulled"] + mb["len"]]
                        .tobytes()) for mb in c["rxq_list"] if "j" in mb] for c in pcb]
    return res


# ---------------------------------------------------------------- named cases
conn1, seg, build, ents = rc.conn1, rc.seg, rc.build, oc.ents
A, F, P, R, S, U = TCP_ACK, TCP_FIN, TCP_PUSH, TCP_RST, TCP_SYN, TCP_URG


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (case, expected): @expected is a dict of hand-derived values:
    'ev', 'rst', 'state' (state_after), 'copy', 'verdict' per entry, 'sout'
    state_out, 'xflags' of connection 0.  conn1(): snd_una 1000, snd_nxt 5000,
    rcv_nxt 100, rcv_wnd 2^20; every segment's default ack is 1000."""
    rng = np.random.default_rng(97)
    res = {}

    def add(name, cs, states, segs, exp=None, q_off=None, q=None, **kw):
        case = build(cs, segs, **kw)
        if states is not None:
            case["state"] = np.array(states, dtype=np.uint8)
        if q is not None:
            case["q_off"], case["q"] = np.array(q_off, dtype=np.uint32), q
        res[name] = (case, exp or {})

    c = conn1(snd_wl1=50000)
    cl = conn1(snd_wl1=50000, snd_una=5000)            # everything we sent is acknowledged: snd_una == snd_nxt
    sg = lambda seq, ln, **kw: seg(rng, 0, seq, ln, **kw)

    # ---- :462-473
    add("synrcvd_to_established_then_text", [c], [SYN_RECEIVED], [sg(100, 0), sg(100, 50), sg(150, 50)],
        dict(ev=[EV_STATE, 0, 0], state=[ESTABLISHED] * 3, copy=[0, 50, 50], xflags=X_OPENED, sout=[ESTABLISHED]))
    add("synrcvd_ack_below_snd_una", [c], [SYN_RECEIVED], [sg(100, 0, ack=999), sg(100, 10)],
        dict(ev=[EV_RST, EV_STATE], rst=[999, 0], state=[SYN_RECEIVED, ESTABLISHED], copy=[0, 10]))
    add("synrcvd_ack_above_snd_nxt", [c], [SYN_RECEIVED], [sg(100, 0, ack=5001)],
        dict(ev=[EV_RST], rst=[5001], state=[SYN_RECEIVED], sflags=[SF_RULE2 | SF_DROPPED]))
    add("synrcvd_with_text_and_fin", [c], [SYN_RECEIVED], [sg(100, 20, flags=A | F)],
        dict(ev=[EV_STATE | EV_FIN], state=[CLOSE_WAIT], copy=[20], after=[121]))
    # ---- FIN in ESTABLISHED, :581-582
    add("established_fin_with_text_then_text", [c], [ESTABLISHED], [sg(100, 30, flags=A | F), sg(131, 10)],
        dict(ev=[EV_STATE | EV_FIN, 0], state=[CLOSE_WAIT, CLOSE_WAIT], copy=[30, 0], after=[131, 131],
             sflags=[SF_RULE2 | SF_WAKE, SF_RULE2 | SF_DROPPED]))
    add("established_fin_without_text", [c], None, [sg(100, 0, flags=A | F)],
        dict(ev=[EV_STATE | EV_FIN], state=[CLOSE_WAIT], copy=[0], after=[101], sout=[CLOSE_WAIT]))
    add("fin_head_clipped", [c], [ESTABLISHED], [sg(100, 40), sg(120, 40, flags=A | F)],
        dict(ev=[0, EV_STATE | EV_FIN], copy=[40, 20], skip=[0, 20], after=[140, 161]))
    add("fin_head_clip_leaves_fin_only", [c], [ESTABLISHED], [sg(100, 40), sg(100, 40, flags=A | F)],
        dict(ev=[0, EV_STATE | EV_FIN], copy=[40, 0], skip=[0, 40], after=[140, 141]))
    # the reference's trim counts the FIN octet: 6 bytes into a window of 3 links 2, rcv_nxt moves by 3
    add("fin_tail_clip_6_into_3", [conn1(snd_wl1=50000, rcv_wnd=3)], [ESTABLISHED], [sg(100, 6, flags=A | F)],
        dict(ev=[EV_STATE | EV_FIN], copy=[2], after=[103], state=[CLOSE_WAIT]))
    add("fin_into_window_1", [conn1(snd_wl1=50000, rcv_wnd=1)], [ESTABLISHED],
        [sg(100, 1, flags=A | F), sg(101, 0, flags=A | F)],
        dict(ev=[EV_STATE | EV_FIN, 0], copy=[0, 0], after=[101, 101], state=[CLOSE_WAIT, CLOSE_WAIT]))
    add("fin_alone_into_window_1", [conn1(snd_wl1=50000, rcv_wnd=1)], [ESTABLISHED], [sg(100, 0, flags=A | F)],
        dict(ev=[EV_STATE | EV_FIN], copy=[0], after=[101]))
    add("fin_into_window_0", [conn1(snd_wl1=50000, rcv_wnd=0)], [ESTABLISHED],
        [sg(100, 0, flags=A | F), sg(100, 5, flags=A | F)],
        dict(ev=[0, 0], sflags=[SF_RULE2 | SF_ACK_NOW | SF_DROPPED] * 2, state=[ESTABLISHED] * 2))
    # ---- the queue
    add("fin_queued_then_drained", [c], [ESTABLISHED], [sg(150, 50, flags=A | F), sg(100, 50)],
        dict(ev=[0, EV_STATE | EV_FIN], state=[ESTABLISHED, CLOSE_WAIT], copy=[50, 50], after=[100, 201],
             oflags=[O_OOO | O_QUEUED | O_LATE_DRAINED, 0]))
    add("fin_entry_in_input_queue", [c], [ESTABLISHED], [sg(100, 100)],
        dict(ev=[EV_STATE | EV_FIN], state=[CLOSE_WAIT], after=[300], qin_state=[Q_DRAINED], qin_len=[99]),
        q_off=[0, 1], q=ents([(200, 300, 7, A | F)]))
    add("fin_entry_queue_by_flags", [conn1(snd_wl1=50000, flags=oc.ESTABLISHED)], None, [sg(100, 100)],
        dict(ev=[EV_STATE | EV_FIN], state=[CLOSE_WAIT], after=[300], qin_len=[99]),
        q_off=[0, 1], q=ents([(200, 300, 7, A | F)]))
    # an entry's end counts its FIN (:552).  The drain goes on behind the FIN entry: both land behind the FIN gap
    # at offset 150 of the region
    add("two_entries_behind_fin_entry", [c], [ESTABLISHED], [sg(100, 100)],
        dict(ev=[EV_STATE | EV_FIN], state=[CLOSE_WAIT], after=[401], qin_state=[Q_DRAINED] * 3,
             qin_len=[50, 100, 50], qin_skip=[0, 0, 50], qin_dst=[100, 151, 251]),
        q_off=[0, 3], q=ents([(200, 251, 7, A | F), (251, 351, 8), (301, 401, 9)]))
    add("fin_entry_tail_clipped", [conn1(snd_wl1=50000, rcv_wnd=130)], [ESTABLISHED], [sg(100, 100)],
        dict(ev=[EV_STATE | EV_FIN], after=[230], qin_len=[29]),
        q_off=[0, 1], q=ents([(200, 251, 7, A | F)]))
    # ---- FIN_WAIT1, :530-532 and :583-585
    fw = conn1(snd_wl1=50000, snd_una=4999)
    add("finwait1_fin_our_fin_acked", [fw], [FIN_WAIT1], [sg(100, 0, ack=5000, flags=A | F)],
        dict(ev=[EV_STATE | EV_FIN], state=[TIME_WAIT], xflags=X_TIMEWAIT, sflags_has=[SF_ACK_NOW]))
    add("finwait1_fin_our_fin_not_acked", [fw], [FIN_WAIT1], [sg(100, 0, ack=4999, flags=A | F), sg(101, 0, ack=5000)],
        dict(ev=[EV_STATE | EV_FIN, EV_STATE], state=[CLOSING, TIME_WAIT], xflags=X_TIMEWAIT))
    add("finwait1_to_finwait2", [fw], [FIN_WAIT1], [sg(100, 10, ack=5000)],
        dict(ev=[EV_STATE], state=[FIN_WAIT2], copy=[10]))
    # snd_una == snd_nxt already and the ack is an old one: :531 looks at snd_una, not at ack
    add("finwait1_old_ack", [cl], [FIN_WAIT1], [sg(100, 0, ack=4000)], dict(ev=[EV_STATE], state=[FIN_WAIT2]))
    add("closing_old_ack", [cl], [CLOSING], [sg(100, 0, ack=4000)], dict(ev=[EV_STATE], state=[TIME_WAIT]))
    add("lastack_old_ack", [cl], [LAST_ACK], [sg(100, 0, ack=4000)], dict(ev=[EV_STATE | EV_PUT], state=[CLOSED]))
    # ---- CLOSING -> TIME_WAIT, :533-536
    add("closing_to_timewait", [fw], [CLOSING], [sg(100, 0, ack=4999), sg(100, 0, ack=5000)],
        dict(ev=[0, EV_STATE], state=[CLOSING, TIME_WAIT], xflags=X_TIMEWAIT))
    # ---- FIN_WAIT2, :586-589
    add("finwait2_text_then_fin", [cl], [FIN_WAIT2], [sg(100, 20, ack=5000), sg(120, 0, ack=5000, flags=A | F)],
        dict(ev=[0, EV_STATE | EV_FIN], state=[FIN_WAIT2, TIME_WAIT], copy=[20, 0], xflags=X_TIMEWAIT,
             sflags=[SF_RULE2, SF_RULE2 | SF_WAKE | SF_ACK_NOW]))
    # ---- LAST_ACK -> CLOSED, :537-542, and the stop behind it
    add("lastack_to_closed_then_stop", [fw], [LAST_ACK], [sg(100, 0, ack=5000), sg(100, 0, ack=5000)],
        dict(ev=[EV_STATE | EV_PUT, 0], state=[CLOSED, 0], verdict=[FAST, SLOW], xflags=X_PUT, sout=[CLOSED],
             first_slow=1))
    add("lastack_put_skips_text", [fw], [LAST_ACK], [sg(100, 10, ack=5000, flags=A | F)],
        dict(ev=[EV_STATE | EV_PUT], copy=[0], after=[100]))
    add("lastack_not_yet", [fw], [LAST_ACK], [sg(100, 0, ack=4999)], dict(ev=[0], state=[LAST_ACK]))
    # ---- retransmitted FIN
    add("timewait_retransmitted_fin", [conn1(snd_wl1=50000, snd_una=5000, rcv_nxt=101)], [TIME_WAIT],
        [sg(100, 0, ack=5000, flags=A | F)],
        dict(ev=[0], state=[TIME_WAIT], sflags=[SF_RULE2 | SF_ACK_NOW | SF_DROPPED]))
    add("closewait_retransmitted_fin", [conn1(snd_wl1=50000, rcv_nxt=101)], [CLOSE_WAIT],
        [sg(100, 0, flags=A | F), sg(90, 10, flags=A | F)],
        dict(ev=[0, 0], state=[CLOSE_WAIT] * 2))
    # ---- RST, :439 and :444
    add("rst_in_window_then_stop", [c], [ESTABLISHED], [sg(100, 0, flags=A | R), sg(100, 10)],
        dict(ev=[EV_FAIL, 0], verdict=[FAST, SLOW], state=[ESTABLISHED, 0], xflags=X_FAILED, first_slow=1))
    add("rst_out_of_window", [c], [ESTABLISHED], [sg(50, 0, flags=A | R), sg(100, 10)],
        dict(ev=[0, 0], sflags=[SF_RULE2 | SF_DROPPED, 0], verdict=[FAST, FAST]))
    add("rst_with_window_0", [conn1(snd_wl1=50000, rcv_wnd=0)], [ESTABLISHED], [sg(7777, 0, flags=R)],
        dict(ev=[EV_FAIL], xflags=X_FAILED))
    add("rst_with_text_out_of_window", [c], [FIN_WAIT2], [sg(50, 10, flags=A | R)],
        dict(ev=[0], sflags=[SF_RULE2 | SF_DROPPED]))
    # ---- SYN, :452-456
    add("syn_in_window_with_ack", [c], [ESTABLISHED], [sg(100, 0, ack=1234, flags=A | S), sg(100, 0)],
        dict(ev=[EV_RST | EV_FAIL, 0], rst=[1234, 0], verdict=[FAST, SLOW]))
    add("syn_in_window_without_ack", [c], [CLOSE_WAIT], [sg(100, 7, flags=S)],
        dict(ev=[EV_RST_ACK | EV_FAIL], rst=[107]))
    add("syn_fin_without_ack", [c], [ESTABLISHED], [sg(100, 7, flags=S | F)],
        dict(ev=[EV_RST_ACK | EV_FAIL], rst=[108]))
    add("syn_out_of_window", [c], [ESTABLISHED], [sg(50, 0, flags=A | S)],
        dict(ev=[0], sflags=[SF_RULE2 | SF_ACK_NOW | SF_DROPPED]))
    # an in-order SYN with text and ACK is tcp_rx_conn's fast path: SYN is no slow-path flag (:20)
    add("syn_with_text_on_the_fast_path", [c], [ESTABLISHED], [sg(100, 10, flags=A | S)],
        dict(ev=[0], sflags=[0], copy=[10]))
    # ---- CLOSED, :372-376: walked to the end
    add("closed_ack_rst_neither", [c], [CLOSED],
        [sg(300, 0), sg(100, 10, flags=A | R), sg(400, 5, flags=0), sg(500, 5, flags=F), sg(1, 0, flags=S)],
        dict(ev=[EV_RST_ACK, 0, EV_RST_ACK, EV_RST_ACK, EV_RST_ACK], rst=[300, 0, 405, 506, 1],
             state=[CLOSED] * 5, verdict=[FAST] * 5, sflags=[SF_RULE2 | SF_DROPPED] * 5, sout=[CLOSED]))
    # ---- text in the states that take none
    for nm, s0 in (("closewait", CLOSE_WAIT), ("closing", CLOSING), ("lastack", LAST_ACK), ("timewait", TIME_WAIT)):
        add(f"text_in_{nm}", [conn1(snd_wl1=50000, acks_delayed_cnt=1)], [s0], [sg(100, 50), sg(100, 0)],
            dict(ev=[0, 0], state=[s0, s0], copy=[0, 0], after=[100, 100], sflags=[SF_RULE2 | SF_DROPPED] * 2))
    # ---- URG is not looked at
    add("urg_with_text", [c], [ESTABLISHED], [sg(100, 30, flags=A | U), sg(130, 30, flags=A | U | P)],
        dict(ev=[0, 0], copy=[30, 30], sflags=[SF_RULE2, SF_RULE2 | SF_WAKE | SF_ACK_NOW]))
    # ---- not taken
    add("syn_sent_and_state_10", [c, c, c], [SYN_SENT, 10, ESTABLISHED],
        [seg(rng, 0, 100, 10), seg(rng, 1, 100, 10), seg(rng, 2, 100, 10)],
        dict(verdict=[SLOW, SLOW, FAST], sout=[SYN_SENT, 10, ESTABLISHED]))
    add("state_overrides_flags", [conn1(flags=0), conn1()], [ESTABLISHED, SYN_SENT],
        [seg(rng, 0, 100, 10), seg(rng, 1, 100, 10)], dict(verdict=[FAST, SLOW]))
    add("no_state_no_flags", [conn1(flags=0)], None, [sg(100, 10)], dict(verdict=[SLOW], sout=[NOSTATE]))
    # ---- becomes ESTABLISHED and takes the fast path
    add("opened_then_fast_path", [c], [SYN_RECEIVED], [sg(100, 0), sg(100, 10), sg(110, 10)],
        dict(sflags=[SF_RULE2 | SF_WND | SF_DROPPED, SF_WND, SF_WND | SF_WAKE | SF_ACK_NOW]))
    # ---- a dup-ACK test that must count the FIN in len: ack_same, data pending, FIN: no rep_acks++
    add("fin_is_no_duplicate_ack", [c], [CLOSE_WAIT], [sg(101, 0, flags=A | F)] * 3, dict(ev=[0, 0, 0]),
        rep_acks=np.array([2], dtype=np.uint8))
    return res


def case_of(name):
    return cases()[name][0]


def check_expected(got, exp, what):
    for key, f in (("verdict", "verdict"), ("sflags", "sflags"), ("copy", "copy_len"), ("after", "rcv_nxt_after"),
                   ("skip", "skip"), ("oflags", "oflags"), ("ev", "ev"), ("rst", "rst_seq"), ("state", "state_after"),
                   ("qin_state", "qin_state"), ("qin_len", "qin_len"), ("qin_skip", "qin_skip"),
                   ("qin_dst", "qin_dst_off"), ("sout", "state_out")):
        if key in exp:
            assert np.asarray(got[f][:len(exp[key])]).tolist() == list(exp[key]), (what, key, got[f].tolist())
    for j, bit in enumerate(exp.get("sflags_has", [])):
        assert int(got["sflags"][j]) & bit, (what, "sflags", j)
    if "xflags" in exp:
        assert int(got["out_ext"][0]["xflags"]) == exp["xflags"], (what, "xflags", int(got["out_ext"][0]["xflags"]))
    if "first_slow" in exp:
        assert int(got["out_conn"][0]["first_slow"]) == exp["first_slow"], (what, "first_slow")


# ---------------------------------------------------------------- random lifetimes
def random_case(seed, nconn=40, align=0, garbage=0.15, data=(3, 10), window=None):
    """Random whole lifetimes: every connection opens passively (SYN_RECEIVED)
    or is found in some state, receives text with reordering and loss, and
    closes actively, passively or both at once, or is reset; a fraction
    @garbage of the segments is off-state garbage (old or future sequence
    numbers, bad ACKs, stray SYN, RST and FIN flags)."""
    rng = np.random.default_rng(seed)
    cs, states, lists, q, q_off = [], [], [], [], [0]
    for k in range(nconn):
        una = int(rng.integers(0, 1 << 32))
        rn = int(rng.choice([int(rng.integers(0, 1 << 32)), 0xFFFFFFFF - int(rng.integers(0, 2000))]))
        mss = int(rng.choice([1460, 536]))
        s0 = int(rng.choice([SYN_RECEIVED, SYN_RECEIVED, ESTABLISHED, ESTABLISHED, FIN_WAIT1, FIN_WAIT2, CLOSE_WAIT,
                             CLOSING, LAST_ACK, TIME_WAIT, CLOSED, SYN_SENT]))
        pend = int(rng.choice([0, 1, 1, 500]))               # what the peer has not acknowledged yet
        c = conn1(snd_una=una, snd_nxt=una + pend, snd_wnd=int(rng.integers(0, 90000)),
                  snd_wl1=rn - int(rng.integers(0, 3)), snd_wl2=una, rcv_nxt=rn,
                  rcv_wnd=window or int(rng.choice([1 << 20, int(rng.integers(1, 4000)), 0])), rcv_mss=mss,
                  snd_wscale=int(rng.integers(0, 8)),
                  flags=(RXQ if rng.random() < 0.3 else 0) | (ACK_DELAYED if rng.random() < 0.3 else 0),
                  acks_delayed_cnt=int(rng.integers(0, 2)))
        cs.append(c)
        states.append(s0)
        at, mine = rn, []
        for _ in range(int(rng.integers(*data))):
            ln = int(rng.integers(1, mss + 1))
            mine.append((at, ln, A | (P if rng.random() < 0.2 else 0), una + (pend if rng.random() < 0.6 else 0)))
            at = (at + ln) & M32
        how = rng.random()
        if how < 0.6:                                          # the peer's FIN, with or without a last piece of text
            ln = int(rng.choice([0, 0, int(rng.integers(1, mss + 1))]))
            mine.append((at, ln, A | F, una + (pend if rng.random() < 0.8 else 0)))
            at = (at + ln + 1) & M32
            mine.append((at, 0, A, una + pend))                # the ACK of our FIN
            if rng.random() < 0.3:
                mine.append(((at - 1) & M32, 0, A | F, una + pend))          # the FIN again
        elif how < 0.75:
            mine.append((at, 0, A | R, una))
            mine.append((at, 10, A, una))
        if rng.random() < 0.25 and len(mine) > 3:              # an input queue: pieces of its own near future
            for p in sorted(set(int(x) for x in rng.integers(1, len(mine) - 1, size=2))):
                s1, ln, fl, _ = mine[p]
                q.append((s1, s1 + ln + (1 if fl & F else 0), 9000 + len(q), fl))
        for p in range(len(mine) - 1):                         # reordering, loss with a retransmit
            r = rng.random()
            if r < 0.25:
                mine[p], mine[p + 1] = mine[p + 1], mine[p]
            elif r < 0.35:
                mine.append(mine[p])
        for p in range(len(mine)):
            if rng.random() < garbage:
                g = int(rng.integers(0, 6))
                s1, ln, fl, ak = mine[p]
                junk = [((s1 - 70000) & M32, ln, fl, ak), ((s1 + (1 << 21)) & M32, ln, fl, ak),
                        (s1, ln, fl, (ak + 100000) & M32), (s1, 0, S | (A if rng.random() < 0.5 else 0), ak),
                        (s1, ln, fl & ~A, ak), (s1, ln, fl | U, (ak - 5) & M32)][g]
                mine.insert(p, junk)
        lists.append(mine)
        q_off.append(len(q))
    segs, st = [], []
    left = [list(reversed(s)) for s in lists]
    live = [k for k in range(nconn) if left[k]]
    while live:
        k = live[int(rng.integers(0, len(live)))]
        s1, ln, fl, ak = left[k].pop()
        segs.append(seg(rng, k, s1, min(ln, cs[k]["rcv_mss"]), ack=ak, flags=fl, win=int(rng.integers(0, 1 << 16)),
                        doff=int(rng.choice([5, 8]))))
        st.append(lc.GOOD)
        if not left[k]:
            live.remove(k)
    case = build(cs, segs, align=align)
    case["st"] = np.array(st, dtype=np.uint8)
    case["rep_acks"] = rng.integers(0, 3, size=nconn).astype(np.uint8)
    case["q_off"], case["q"] = np.array(q_off, dtype=np.uint32), ents(q)
    case["state"] = np.array(states, dtype=np.uint8)
    return case


STREAMS = {"lifetimes": lambda: random_case(11, nconn=150), "lifetimes_aligned": lambda: random_case(12, nconn=150, align=64),
           "small_windows": lambda: random_case(13, nconn=150, window=700)}


@functools.lru_cache(maxsize=None)
def stream(name):
    return STREAMS[name]()


def check_mix(want):
    """the conditions the random lifetimes must meet, on the MODEL's output"""
    cnt = want["counts"]
    for slot in (C_RSTS, C_FAILS, C_FINS, C_STATE_CHANGES, oc.C_QUEUED, oc.C_DRAINED, fc.C_DROPPED, fc.C_ACKS):
        assert int(cnt[slot]) > 3, (slot, cnt)
    assert len(set(want["state_out"].tolist())) >= 6


# ---------------------------------------------------------------- running the host twin
S_OUT = (("ev", np.uint8, "m"), ("rst_seq", np.uint32, "m"), ("state_after", np.uint8, "m"),
         ("state_out", np.uint8, "nconn"))


def blank(case, fill=SENTINEL):
    z = oc.sizes(case)
    b = oc.blank(case)
    for f, dt, by in S_OUT:
        b[f] = np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (z[by] + GUARD)), dtype=dt).copy()
    if fill != SENTINEL:
        b = {f: np.full(a.nbytes, fill, dtype=np.uint8).view(a.dtype) for f, a in b.items()}
    return b


def compare(got, want, case, what):
    """@got (blank() after a call) against @want: the written part equal byte for byte, the guards untouched"""
    z = oc.sizes(case)
    oc.compare(got, want, case, what)
    for f, dt, by in S_OUT:
        k, g = z[by], got[f]
        assert len(g) == k + GUARD and (g[k:].view(np.uint8) == SENTINEL).all(), f"{what}: {f} written past its end"
        bad = np.nonzero(g[:k] != want[f][:k])[0]
        assert not len(bad), f"{what}: {f}[{bad[0]}] = {g[bad[0]]} != {want[f][bad[0]]} ({len(bad)} differ)"


def run_host(g, case, counts=True, fill=SENTINEL):
    """gcl_tcp_rx_states_host over sentinel-filled outputs: (outputs, counts)"""
    z = oc.sizes(case)
    out = blank(case, fill)
    cnt = np.full(NR, 5, dtype=np.uint64) if counts else None
    g.tcp_rx_states_host(case["frames"], case["pkt_len"], case["sock"], case["conn"], stride=case["stride"],
                         offs=case["offs"], frames_len=case["frames_len"], order=case.get("order"), m=z["m"],
                         l4_status=case.get("st"), nconn=z["nconn"], align=case.get("align", 0),
                         blocks=case.get("blocks", 0), rep_acks=case.get("rep_acks"), q_off=case.get("q_off"),
                         q=case.get("q"), nq=z["nq"], q_out_cap=z["cap"], state=case.get("state"), out=out,
                         counts=cnt)
    return out, None if cnt is None else cnt - np.uint64(5)
