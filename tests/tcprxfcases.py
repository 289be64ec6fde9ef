"""The definition of gcl_tcp_rx_full (include/gclassify.h) in Python, and the
cases the CPU and GPU tests share.  The model transcribes tcp_rx_conn,
__tcp_rx_conn, is_acceptable, tcp_rx_text and tcp_rx_append_text
(runtime/net/tcp_in.c) line by line over a dict of PCB fields, read for
state == ESTABLISHED and an empty out-of-order queue; it knows nothing of
csrc/gcl_tcprxf.h.  The named cases below carry expected values written out
by hand from the reference's lines; the pin to the reference's own code is
tests/golden/tcprx_ref.json (tests/tcprxrefcases.py), recorded from tcp_in.c
compiled in place by oracle/ref_tcpin.c.  What is the same as in
gcl_tcp_rx (the wraps_* comparisons, the records, the frame builders) comes
from tests/tcprxcases.py and tests/paycases.py.

A case is tests/tcprxcases.py's dict plus optionally rep_acks (u8[nconn]).
"""
import functools

import numpy as np

from tests import l4cases as lc
from tests import paycases as pc
from tests import tcprxcases as rc
from tests.tcprxcases import (ACK_DELAYED, DROP, ELIGIBLE, FAST, M32, NA, NOCONN, NONE, REP_ACKS_RESET, RXQ, SLOW,
                              STOPPED, TCP_ACK, TCP_FIN, TCP_PUSH, TCP_RST, TCP_SYN, TCP_URG, TIMER_ARMED, WOKEN,
                              wraps_gt, wraps_lt, wraps_lte)

C_BYTES, C_ACKS, C_WAKES, C_RULE2, C_TXWAKES, C_FASTRTX, C_DUPACKS, C_DROPPED, NR = 5, 6, 7, 8, 9, 10, 11, 12, 13
SF_WAKE, SF_ACK_NOW, SF_ACKED, SF_WND, SF_RULE2, SF_TXWAKE, SF_FASTRTX, SF_DROPPED = (1, 2, 4, 8, 0x10, 0x20, 0x40,
                                                                                      0x80)
X_TXWAKE, X_FASTRTX = 1, 2
TCP_FAST_RETRANSMIT_THRESH = 3
EXT = np.dtype([("nrule2", "<u4"), ("ndropped", "<u4"), ("fast_rtx_ack", "<u4"), ("rep_acks", "u1"),
                ("xflags", "u1"), ("pad", "u1", (2,))])
ENTRY, CONN, CONN_OUT, SENTINEL, GUARD = rc.ENTRY, rc.CONN, rc.CONN_OUT, rc.SENTINEL, rc.GUARD


class Stop(Exception):
    """the segment leaves for the runtime's own __tcp_rx_conn"""


def tcp_is_snd_full(c):
    # tcp.h:224
    return wraps_lte((c["snd_una"] + c["snd_wnd"]) & M32, c["snd_nxt"])


def is_acceptable(c, ln, seq, flags):
    # :32-50
    if ln == 0 and c["rcv_wnd"] == 0:
        if (flags & TCP_ACK) or (flags & TCP_URG) or (flags & TCP_RST):
            return True
        return seq == c["rcv_nxt"]
    elif ln == 0 and c["rcv_wnd"] > 0:
        return wraps_lte(c["rcv_nxt"], seq) and wraps_lt(seq, (c["rcv_nxt"] + c["rcv_wnd"]) & M32)
    elif ln > 0 and c["rcv_wnd"] == 0:
        return False
    end1 = (seq + ln - 1) & M32
    return (wraps_lte(c["rcv_nxt"], seq) and wraps_lt(seq, (c["rcv_nxt"] + c["rcv_wnd"]) & M32)) or \
           (wraps_lte(c["rcv_nxt"], end1) and wraps_lt(end1, (c["rcv_nxt"] + c["rcv_wnd"]) & M32))


def tcp_rx_append_text(c, m):
    # :72-73
    assert wraps_lte(m["seg_seq"], c["rcv_nxt"]) and wraps_gt(m["seg_end"], c["rcv_nxt"])
    # :76-80: a head clip never gets here (the call stops the connection first)
    assert not wraps_lt(m["seg_seq"], c["rcv_nxt"])
    # :83-87
    if wraps_lt((c["rcv_nxt"] + c["rcv_wnd"]) & M32, m["seg_end"]):
        ln = (m["seg_end"] - ((c["rcv_nxt"] + c["rcv_wnd"]) & M32)) & M32
        assert ln <= m["len"]            # mbuf_trim: the windows of the tests stay below 2^31
        m["len"] -= ln
        m["seg_end"] = (c["rcv_nxt"] + c["rcv_wnd"]) & M32
    # :90-94
    got = (m["seg_end"] - m["seg_seq"]) & M32
    assert c["rcv_wnd"] >= got
    c["rcv_wnd"] = (c["rcv_wnd"] - got) & M32
    c["rcv_nxt"] = m["seg_end"]
    c["rxq"] = True
    c["rxq_bytes"].append(m)


def tcp_rx_text(c, m, out):
    # :105-106
    if c["rcv_wnd"] == 0:
        return False
    # :108-116; the out-of-order branch of :117-136 is the runtime's
    assert wraps_lte(m["seg_seq"], c["rcv_nxt"])
    if (m["flags"] & (TCP_PUSH | TCP_FIN)) != 0 or c["rxq"]:
        out["wake"] = True
    tcp_rx_append_text(c, m)
    # :140-163: rxq_ooo is empty
    # :165-166
    if c["rcv_wnd"] == 0:
        out["wake"] = True
    return True


def slow_rx_conn(c, m, ack, snd_nxt, win):
    """__tcp_rx_conn (:352-611) for a connection in ESTABLISHED with an empty
    rxq_ooo.  Returns the sflags of the segment; raises Stop, before it has
    changed anything, for what the call leaves to the runtime."""
    sf = SF_RULE2
    do_ack, do_drop, ack_same, wnd_updated = False, True, False, False
    seq, ln = m["seg_seq"], m["len"]
    # the call's own lines: every other state, the out-of-order queue and the flags whose steps
    # (:369, :444, :452, step 6) end, reset or mark the connection
    if not c["state_ok"] or (m["flags"] & (TCP_FIN | TCP_RST | TCP_URG | TCP_SYN)):
        raise Stop
    while True:                                  # 'break' is 'goto done'
        # :438-441
        if not is_acceptable(c, ln, seq, m["flags"]):
            do_ack = (m["flags"] & TCP_RST) == 0
            break
        # the call's own line: acceptable text that tcp_rx_text would queue out of order (:117) or
        # tcp_rx_append_text would clip at the head (:76); taken here, before the ACK steps move anything
        if ln > 0 and seq != c["rcv_nxt"]:
            raise Stop
        # :459-461
        if (m["flags"] & TCP_ACK) == 0:
            break
        # :476-501
        snd_was_full = tcp_is_snd_full(c)
        if wraps_lte(c["snd_una"], ack) and wraps_lte(ack, snd_nxt):
            if c["snd_una"] != ack:
                c["snd_una"] = ack
                sf |= SF_ACKED                   # tcp_conn_ack
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
        if snd_was_full and not tcp_is_snd_full(c):
            sf |= SF_TXWAKE
            c["xflags"] |= X_TXWAKE
        # :514-528
        if ack_same and c["snd_una"] != c["snd_nxt"] and ln == 0 and not wnd_updated:
            c["rep_acks"] += 1
            c["dupacks"] += 1
            if c["rep_acks"] >= TCP_FAST_RETRANSMIT_THRESH:
                sf |= SF_FASTRTX
                c["fast_rtx_ack"] = ack          # fast_retransmit_last_ack, or tcp_tx_fast_retransmit_start
                c["xflags"] |= X_FASTRTX
                c["rep_acks"] = 0
                c["rep_reset"] = True
        elif c["snd_una"] == ack:
            c["rep_acks"] = 0
            c["rep_reset"] = True
        # :530-542: other states
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
                c["armed"] = True                # ack_ts = microtime()
            # :574: rxq_ooo is empty
        # :578: no FIN
        break
    # done, :593-598 (tcp_timer_update stays with the runtime)
    if do_ack:
        c["ack_delayed"] = False
        c["acks_delayed_cnt"] = 0
        sf |= SF_ACK_NOW
    if do_drop:
        sf |= SF_DROPPED
    return sf


def model(case, with_rxq=False):
    """Every output of one call as a dict (the per-entry arrays, out_conn,
    out_ext, conn_off, counts); with @with_rxq also 'rxq': per connection the
    bytes of the mbufs appended to c->rxq, in order."""
    order, sock, st, conn = case.get("order"), case["sock"], case.get("st"), case["conn"]
    align = max(case.get("align", 0), 1)
    pay = pc.model(case, order, sock, st)
    n, nconn = len(case["pkt_len"]), len(conn)
    rep = case.get("rep_acks")
    idx = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    m = len(idx)
    out = {f: np.zeros(m, dtype=dt) for f, dt in ENTRY}
    counts = [0] * NR
    pcb = [{k: int(conn[c][k]) for k in CONN.names if k != "pad"} for c in range(nconn)]
    for k, c in enumerate(pcb):
        c.update(state_ok=bool(c["flags"] & ELIGIBLE), rxq=bool(c["flags"] & RXQ),
                 ack_delayed=bool(c["flags"] & ACK_DELAYED), stopped=False, woken=False, armed=False,
                 rep_reset=False, nfast=0, nslow=0, nacks=0, first_slow=NONE, rxq_bytes=[], placed=[],
                 rep_acks=0 if rep is None else int(rep[k]), fast_rtx_ack=0, xflags=0, dupacks=0, nrule2=0,
                 ndropped=0)
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
        # :186
        snd_nxt = c["snd_nxt"]
        # :198-206
        seq, ack = pc.be(f, 38, 4), pc.be(f, 42, 4)
        win = (pc.be(f, 48, 2) << (c["snd_wscale"] & 31)) & M32
        flags = int(f[47])
        ln = int(pay["len"][j])
        # :207
        if ln > c["rcv_mss"]:
            out["verdict"][j] = DROP
            counts[DROP] += 1
            continue
        if c["stopped"]:
            c["nslow"] += 1
            out["verdict"][j] = SLOW
            counts[SLOW] += 1
            continue
        # :212-214
        src = int(pay["src_off"][j])
        mb = {"seg_seq": seq, "seg_end": (seq + ln) & M32, "flags": flags, "len": ln, "src": src, "j": j}
        # :221-239
        slow_path = (flags & rc.TCP_SLOWPATH_FLAGS) != 0 or ln == 0 or wraps_gt(ack, snd_nxt)
        slow_path |= not c["state_ok"]
        slow_path |= tcp_is_snd_full(c)
        slow_path |= seq != c["rcv_nxt"]
        slow_path |= c["rcv_wnd"] < ln
        slow_path |= wraps_gt(ack, snd_nxt)
        dup0 = c["dupacks"]
        if slow_path:
            # :241-242
            try:
                sf = slow_rx_conn(c, mb, ack, snd_nxt, win)
            except Stop:
                c["first_slow"] = j
                c["stopped"] = True
                c["nslow"] += 1
                out["verdict"][j] = SLOW
                counts[SLOW] += 1
                continue
        else:
            sf = 0
            # :247-264
            if wraps_lte(c["snd_una"], ack):
                if c["snd_una"] != ack:
                    c["rep_acks"] = 0
                    c["rep_reset"] = True
                    c["snd_una"] = ack
                    sf |= SF_ACKED
                if wraps_lt(c["snd_wl1"], seq) or (c["snd_wl1"] == seq and wraps_lte(c["snd_wl2"], ack)):
                    c["snd_wnd"], c["snd_wl1"], c["snd_wl2"] = win, seq, ack
                    c["rep_acks"] = 0
                    c["rep_reset"] = True
                    sf |= SF_WND
            # :266-268
            c["rcv_nxt"] = (seq + ln) & M32
            c["rcv_wnd"] = (c["rcv_wnd"] - ln) & M32
            # :271-274
            if c["rxq"] or (flags & TCP_PUSH) > 0:
                sf |= SF_WAKE
                c["woken"] = True
            # :277-285
            c["acks_delayed_cnt"] += 1
            if c["acks_delayed_cnt"] >= 2:
                c["ack_delayed"] = False
                sf |= SF_ACK_NOW
                c["acks_delayed_cnt"] = 0
            elif not c["ack_delayed"]:
                c["armed"] = True
                c["ack_delayed"] = True
            # :287
            c["rxq"] = True
            c["rxq_bytes"].append(mb)
        got = mb["len"] if not (sf & SF_DROPPED) else 0
        c["nfast"] += 1
        c["nacks"] += bool(sf & SF_ACK_NOW)
        c["nrule2"] += bool(sf & SF_RULE2)
        c["ndropped"] += bool(sf & SF_DROPPED)
        out["verdict"][j], out["sflags"][j] = FAST, sf
        out["rcv_nxt_after"][j], out["copy_len"][j] = c["rcv_nxt"], got
        counts[FAST] += 1
        counts[C_BYTES] += got
        for slot, bit in ((C_ACKS, SF_ACK_NOW), (C_WAKES, SF_WAKE), (C_RULE2, SF_RULE2), (C_TXWAKES, SF_TXWAKE),
                          (C_FASTRTX, SF_FASTRTX), (C_DROPPED, SF_DROPPED)):
            counts[slot] += bool(sf & bit)
        counts[C_DUPACKS] += c["dupacks"] - dup0
    oc, ext = np.zeros(nconn, dtype=CONN_OUT), np.zeros(nconn, dtype=EXT)
    off, at = np.zeros(nconn + 1, dtype=np.uint64), 0
    for k, c in enumerate(pcb):
        fl = (RXQ if c["rxq"] else 0) | (ACK_DELAYED if c["ack_delayed"] else 0) | \
             (STOPPED if c["stopped"] else 0) | (WOKEN if c["woken"] else 0) | \
             (TIMER_ARMED if c["armed"] else 0) | (REP_ACKS_RESET if c["rep_reset"] else 0)
        oc[k] = (c["snd_una"], c["snd_wnd"], c["snd_wl1"], c["snd_wl2"], c["rcv_nxt"], c["rcv_wnd"], c["nfast"],
                 c["nslow"], c["nacks"], c["first_slow"], c["acks_delayed_cnt"], fl, 0)
        ext[k] = (c["nrule2"], c["ndropped"], c["fast_rtx_ack"], c["rep_acks"], c["xflags"], 0)
        off[k] = at
        pos = 0
        for mb in c["rxq_bytes"]:
            out["dst_off"][mb["j"]] = at + pos
            pos += mb["len"]
        assert pos == (c["rcv_nxt"] - int(conn[k]["rcv_nxt"])) & M32
        at += -(-pos // align) * align
    off[nconn] = at
    assert sum(counts[:5]) == m
    res = dict(out, out_conn=oc, out_ext=ext, conn_off=off, counts=np.array(counts, dtype=np.uint64))
    if with_rxq:
        res["rxq"] = [b"".join(case["frames"][mb["src"]:mb["src"] + mb["len"]].tobytes() for mb in c["rxq_bytes"])
                      for c in pcb]
    return res


# ---------------------------------------------------------------- named cases
conn1, seg, build = rc.conn1, rc.seg, rc.build
R, D, A, W, K, N, T, F = SF_RULE2, SF_DROPPED, SF_ACK_NOW, SF_WAKE, SF_ACKED, SF_WND, SF_TXWAKE, SF_FASTRTX


def ack0(rng, seq=100, **kw):
    """a pure ACK of connection 0"""
    return seg(rng, 0, seq, 0, **kw)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (case, expected): the named cases of the issue.  @expected holds
    values derived by hand from tcp_in.c for conn1() (snd_una 1000, snd_nxt
    5000, snd_wnd 60000, snd_wl1 99, snd_wl2 1000, rcv_nxt 100, rcv_wnd 2^20;
    a segment's default ack 1000 and win 0xF000 = 61440): 'verdict', 'sflags'
    and 'copy' per entry, 'oc' and 'ext' fields of connection 0, 'counts'."""
    rng = np.random.default_rng(92)
    res = {}

    def add(name, cs, segs, exp, rep=None, **kw):
        case = build(cs, segs, **kw)
        if rep is not None:
            case["rep_acks"] = np.array(rep, dtype=np.uint8)
        res[name] = (case, exp)

    c = conn1()
    # ---- pure ACKs
    # :479-481 snd_una moves; :487 wl1 99 < 100 and !ack_same: the window is taken; :526 rep_acks = 0
    add("pure_ack_moves_una", [c], [ack0(rng, ack=2000)],
        dict(verdict=[FAST], sflags=[R | K | N | D], copy=[0],
             oc=dict(snd_una=2000, snd_wnd=61440, snd_wl1=100, snd_wl2=2000, rcv_nxt=100, nfast=1, nacks=0,
                     flags=REP_ACKS_RESET),
             ext=dict(nrule2=1, ndropped=1, rep_acks=0, xflags=0), counts={C_RULE2: 1, C_DROPPED: 1, FAST: 1}), rep=[2])
    # ack_same, 60000 <= 61441: the window grows, wnd_updated, so no duplicate; :526 resets
    add("pure_ack_window_only", [c], [ack0(rng, win=0xF001)],
        dict(verdict=[FAST], sflags=[R | N | D], oc=dict(snd_una=1000, snd_wnd=61441, snd_wl1=100, snd_wl2=1000),
             ext=dict(rep_acks=0), counts={C_DUPACKS: 0}), rep=[2])
    # ack_same and 60000 > 4096: the guard of :490 refuses, so it is a duplicate
    add("ack_same_smaller_window", [c], [ack0(rng, win=0x1000)],
        dict(verdict=[FAST], sflags=[R | D], oc=dict(snd_wnd=60000, snd_wl1=99, flags=0), ext=dict(rep_acks=1),
             counts={C_DUPACKS: 1, C_FASTRTX: 0}))
    add("dupacks_1_2_3_4", [c], [ack0(rng, win=0x1000) for _ in range(4)],
        dict(verdict=[FAST] * 4, sflags=[R | D, R | D, R | D | F, R | D],
             oc=dict(flags=REP_ACKS_RESET, nfast=4),
             ext=dict(rep_acks=1, fast_rtx_ack=1000, xflags=X_FASTRTX, nrule2=4, ndropped=4),
             counts={C_DUPACKS: 4, C_FASTRTX: 1}))
    add("rep_acks_2_on_entry", [c], [ack0(rng, win=0x1000)],
        dict(sflags=[R | D | F], ext=dict(rep_acks=0, fast_rtx_ack=1000, xflags=X_FASTRTX)), rep=[2])
    # the reference's int: 255 + 1 >= 3
    add("rep_acks_255_on_entry", [c], [ack0(rng, win=0x1000)],
        dict(sflags=[R | D | F], ext=dict(rep_acks=0, fast_rtx_ack=1000)), rep=[255])
    # :514 snd_una == snd_nxt: nothing in flight, no count; :526 resets
    cw = conn1(snd_una=5000, snd_wl2=5000)
    add("dup_with_nothing_in_flight", [cw], [ack0(rng, ack=5000, win=0x1000)],
        dict(sflags=[R | D], ext=dict(rep_acks=0), oc=dict(flags=REP_ACKS_RESET), counts={C_DUPACKS: 0}), rep=[1])
    # ack below snd_una: neither branch of :477-501, and :526 does not hold
    add("old_ack_keeps_rep_acks", [c], [ack0(rng, ack=999)],
        dict(verdict=[FAST], sflags=[R | D], oc=dict(snd_una=1000, snd_wl1=99, flags=0), ext=dict(rep_acks=2)),
        rep=[2])
    add("ack_one_past_una", [c], [ack0(rng, ack=1001)], dict(sflags=[R | K | N | D], oc=dict(snd_una=1001)))
    # wraps_lte(ack, snd_nxt) at ack == snd_nxt; wraps_gt one further
    add("ack_eq_snd_nxt", [c], [ack0(rng, ack=5000)], dict(sflags=[R | K | N | D], oc=dict(snd_una=5000)))
    cw = conn1(flags=ELIGIBLE | ACK_DELAYED, acks_delayed_cnt=1)
    add("ack_gt_snd_nxt_cancels_delayed_ack", [cw], [ack0(rng, ack=5001)],
        dict(verdict=[FAST], sflags=[R | A | D], copy=[0],
             oc=dict(snd_una=1000, snd_wl1=99, acks_delayed_cnt=0, flags=0, nacks=1), ext=dict(rep_acks=2)), rep=[2])
    # :487-489 at snd_wl1 == seq: wl2 <= ack takes it, wl2 > ack and wl1 > seq do not
    add("wl1_eq_seq_wl2_lte", [conn1(snd_wl1=100)], [ack0(rng, win=0xF001)],
        dict(sflags=[R | N | D], oc=dict(snd_wnd=61441)))
    add("wl1_eq_seq_wl2_gt", [conn1(snd_wl1=100, snd_wl2=1001)], [ack0(rng, win=0xF001)],
        dict(sflags=[R | D], oc=dict(snd_wnd=60000), ext=dict(rep_acks=1)))
    add("wl1_gt_seq", [conn1(snd_wl1=101)], [ack0(rng, win=0xF001)],
        dict(sflags=[R | D], oc=dict(snd_wnd=60000), ext=dict(rep_acks=1)))
    # ---- window and acceptability
    cf = conn1(snd_wnd=4000)                      # 1000 + 4000 == snd_nxt: full
    add("txwake_full_to_not_full", [cf], [ack0(rng, ack=2000)],
        dict(sflags=[R | K | N | T | D], ext=dict(xflags=X_TXWAKE), counts={C_TXWAKES: 1}))
    # the same window again: still full, nothing changed, a duplicate
    add("still_full_no_txwake", [cf], [ack0(rng, win=4000)],
        dict(sflags=[R | N | D], oc=dict(snd_wnd=4000, snd_wl1=100), ext=dict(xflags=0, rep_acks=1)))
    c0 = conn1(rcv_wnd=0)
    # :32-38: rcv_wnd == 0 and len == 0
    add("wnd0_pure_ack_any_seq", [c0], [ack0(rng, seq=5555, ack=2000)], dict(sflags=[R | K | N | D]))
    add("wnd0_no_ack_flag_seq_ne", [c0], [ack0(rng, seq=101, flags=0)], dict(sflags=[R | A | D]))
    add("wnd0_no_ack_flag_seq_eq", [c0], [ack0(rng, seq=100, flags=0)], dict(sflags=[R | D]))
    # :39-41: len == 0 into a window of 1000
    c1k = conn1(rcv_wnd=1000)
    add("len0_seq_window_edges", [c1k], [ack0(rng, seq=99), ack0(rng, seq=1100), ack0(rng, seq=1099, ack=2000)],
        dict(verdict=[FAST] * 3, sflags=[R | A | D, R | A | D, R | K | N | D], oc=dict(nacks=2, snd_wl1=1099)))
    # :42-43
    add("wnd0_text", [c0], [seg(rng, 0, 100, 100)], dict(verdict=[FAST], sflags=[R | A | D], copy=[0],
                                                         oc=dict(rcv_nxt=100, flags=0)))
    # :47-50: a whole duplicate (its last byte 99 < rcv_nxt), text past the window; the connection goes on
    add("whole_duplicate_then_fast", [c1k], [seg(rng, 0, 0, 100), seg(rng, 0, 1100, 10), seg(rng, 0, 100, 100)],
        dict(verdict=[FAST] * 3, sflags=[R | A | D, R | A | D, N], copy=[0, 0, 100],
             oc=dict(rcv_nxt=200, nfast=3, nslow=0, first_slow=NONE, nacks=2)))
    # the window holds one segment and a half: fast, then the tail clip and the wake at window 0 (:165),
    # the counter 1 -> 2 -> ACK; then the window is 0: text is not acceptable, a pure ACK is
    cw = conn1(rcv_wnd=150)
    add("tail_clip_then_window_0", [cw], [seg(rng, 0, 100, 100), seg(rng, 0, 200, 100), seg(rng, 0, 250, 10),
                                         ack0(rng, seq=250, ack=2000)],
        dict(verdict=[FAST] * 4, sflags=[N, R | N | W | A, R | A | D, R | K | N | D], copy=[100, 50, 0, 0],
             after=[200, 250, 250, 250],
             oc=dict(rcv_nxt=250, rcv_wnd=0, nacks=2, acks_delayed_cnt=0, snd_una=2000,
                     flags=RXQ | WOKEN | TIMER_ARMED | REP_ACKS_RESET)))
    add("wake_only_by_window_0", [conn1(rcv_wnd=50)], [seg(rng, 0, 100, 100)],
        dict(sflags=[R | N | W], copy=[50],
             oc=dict(rcv_nxt=150, rcv_wnd=0, acks_delayed_cnt=1,
                     flags=RXQ | ACK_DELAYED | WOKEN | TIMER_ARMED | REP_ACKS_RESET)))
    add("tail_clip_by_one", [conn1(rcv_wnd=99)], [seg(rng, 0, 100, 100)], dict(copy=[99], oc=dict(rcv_wnd=0)))
    # ---- text and ordering
    # slow only by :230; the slow rule's own counter: 0 -> 1 (armed) -> 2: ACK; the wake by rxq
    add("text_slow_by_full_send_window", [cf], [seg(rng, 0, 100, 100, win=4000), seg(rng, 0, 200, 100, win=4000)],
        dict(verdict=[FAST] * 2, sflags=[R | N, R | N | W | A], copy=[100, 100],
             oc=dict(rcv_nxt=300, acks_delayed_cnt=0, nacks=1, flags=RXQ | WOKEN | TIMER_ARMED | REP_ACKS_RESET),
             ext=dict(nrule2=2, ndropped=0)))
    add("text_slow_counter_1_on_entry", [conn1(snd_wnd=4000, acks_delayed_cnt=1, flags=ELIGIBLE | ACK_DELAYED)],
        [seg(rng, 0, 100, 100, win=4000)], dict(sflags=[R | N | A], oc=dict(acks_delayed_cnt=0, flags=RXQ | REP_ACKS_RESET)))
    add("no_ack_flag", [cf], [ack0(rng, flags=0), seg(rng, 0, 100, 100, flags=TCP_PUSH)],
        dict(verdict=[FAST] * 2, sflags=[R | D, R | D], copy=[0, 0], oc=dict(rcv_nxt=100, flags=0, snd_wl1=99)))
    add("fast_ack_fast", [c], [seg(rng, 0, 100, 100), ack0(rng, seq=200, ack=2000), seg(rng, 0, 200, 100, ack=2000)],
        dict(verdict=[FAST] * 3, sflags=[N, R | K | N | D, N | W | A], copy=[100, 0, 100],
             oc=dict(nfast=3, nslow=0, first_slow=NONE, rcv_nxt=300, snd_una=2000), ext=dict(nrule2=1)))
    add("fast_acked_resets_rep_acks", [c], [seg(rng, 0, 100, 100, ack=2000)],
        dict(sflags=[K | N], ext=dict(rep_acks=0, nrule2=0), oc=dict(flags=RXQ | ACK_DELAYED | TIMER_ARMED | REP_ACKS_RESET)),
        rep=[2])
    # a fast segment that moves nothing on the send side (wl1 > seq) keeps rep_acks
    add("fast_keeps_rep_acks", [conn1(snd_wl1=101)], [seg(rng, 0, 100, 100)], dict(sflags=[0], ext=dict(rep_acks=2)),
        rep=[2])
    # ---- the stops: a pure ACK handled, the stop, a pure ACK behind it
    stops = {"fin": ack0(rng, flags=TCP_ACK | TCP_FIN), "rst": ack0(rng, flags=TCP_RST),
             "urg": ack0(rng, flags=TCP_ACK | TCP_URG), "syn": ack0(rng, flags=TCP_ACK | TCP_SYN),
             "ooo_text": seg(rng, 0, 300, 100), "head_clipped_text": seg(rng, 0, 50, 100)}
    for what, s in stops.items():
        add(f"stop_{what}", [c], [ack0(rng, ack=2000), s, ack0(rng, ack=3000)],
            dict(verdict=[FAST, SLOW, SLOW], sflags=[R | K | N | D, 0, 0], copy=[0, 0, 0], after=[100, 0, 0],
                 oc=dict(snd_una=2000, nfast=1, nslow=2, first_slow=1, flags=STOPPED | REP_ACKS_RESET)))
    add("stop_not_eligible", [conn1(flags=RXQ)], [ack0(rng, ack=2000), seg(rng, 0, 100, 100)],
        dict(verdict=[SLOW, SLOW], oc=dict(snd_una=1000, nslow=2, first_slow=0, flags=RXQ | STOPPED)))
    # SYN on text that the fast path takes is gcl_tcp_rx's FAST (rule 1 comes first)
    add("syn_text_is_rule_1", [c], [seg(rng, 0, 100, 100, flags=TCP_ACK | TCP_SYN)], dict(verdict=[FAST], sflags=[N]))
    # ---- sequence numbers that wrap (the two refused ACKs clear the delayed-ACK counter: the last text arms it anew)
    cw = conn1(rcv_nxt=0xFFFFFFC0, rcv_wnd=0x100, snd_una=0xFFFFFF00, snd_nxt=0x100, snd_wnd=0x300,
               snd_wl1=0xFFFFFFBF, snd_wl2=0xFFFFFF00)
    add("wrap", [cw], [ack0(rng, seq=0xFFFFFFC0, ack=0x80), seg(rng, 0, 0xFFFFFFC0, 0x80, ack=0x80),
                       ack0(rng, seq=0x40, ack=0x100), ack0(rng, seq=0x40, ack=0x101),
                       ack0(rng, seq=0x140, ack=0x100), seg(rng, 0, 0x40, 0x100, ack=0x100)],
        dict(verdict=[FAST] * 6, sflags=[R | K | N | D, N, R | K | N | D, R | A | D, R | A | D, R | N | W],
             copy=[0, 0x80, 0, 0, 0, 0x80], after=[0xFFFFFFC0, 0x40, 0x40, 0x40, 0x40, 0xC0],
             oc=dict(snd_una=0x100, rcv_nxt=0xC0, rcv_wnd=0)))
    # ---- more than one connection, an order with repeats and strays, nothing at all
    c2 = conn1(rcv_nxt=50000, snd_una=7, snd_nxt=9, snd_wnd=100, snd_wl2=7)
    a = [seg(rng, 0, 100, 100), ack0(rng, seq=200, ack=1500), seg(rng, 0, 200, 300, ack=1500)]
    b = [seg(rng, 1, 50000, 5, ack=7), seg(rng, 1, 50005, 0, ack=8), seg(rng, 1, 50005, 6, ack=8)]
    add("two_interleaved", [c, c2], [a[0], b[0], b[1], a[1], a[2], b[2]],
        dict(verdict=[FAST] * 6, copy=[100, 5, 0, 0, 300, 6]), align=16, rep=[1, 2])
    s = [seg(rng, 0, 100, 100), ack0(rng, seq=200, win=0x1000), seg(rng, 0, 200, 100)]
    add("duplicate_order", [c], s,
        dict(verdict=[FAST, FAST, FAST, FAST, FAST, NA, NA, FAST],
             # the repeated text is a whole duplicate: its ACK clears the counter (:595-598), so the
             # next text counts 0 -> 1 again and sends none
             sflags=[N, R | A | D, R | D, R | D, N | W, 0, 0, R | A | D]),
        order=np.array([0, 0, 1, 1, 2, 7, 0xFFFFFFFF, 2], dtype=np.uint32))
    add("m_zero", [c, c2], [], dict(verdict=[]), rep=[3, 4])
    add("noconn_and_drop", [c], [seg(rng, 1, 100, 10), seg(rng, 0, 100, 1461), ack0(rng, ack=2000)],
        dict(verdict=[NOCONN, DROP, FAST], sflags=[0, 0, R | K | N | D]))
    return res


def case_of(name):
    return cases()[name][0]


def check_expected(got, exp, what):
    """@got (a model()-shaped dict) against the hand-derived @exp of a named case"""
    for key, f in (("verdict", "verdict"), ("sflags", "sflags"), ("copy", "copy_len"), ("after", "rcv_nxt_after")):
        if key in exp:
            assert got[f][:len(exp[key])].tolist() == list(exp[key]), (what, key, got[f].tolist())
    for key, f in (("oc", "out_conn"), ("ext", "out_ext")):
        for k, v in exp.get(key, {}).items():
            assert int(got[f][0][k]) == v, (what, f, k, int(got[f][0][k]), v)
    for slot, v in exp.get("counts", {}).items():
        assert int(got["counts"][slot]) == v, (what, "counts", slot, int(got["counts"][slot]))


# ---------------------------------------------------------------- random streams
def random_case(seed, m=4096, nconn=300, align=0, flow=None, stops=0.012, noise=0.03):
    """A random stream of @m entries over @nconn connections: receivers of
    in-order text, senders that get pure ACKs (new, window-only and runs of
    duplicates), connections that start with a full send window or a short
    receive window, and about @stops of the segments what stops a connection.
    @flow(k) overrides the connection of entry k."""
    rng = np.random.default_rng(seed)
    cs = []
    for _ in range(nconn):
        una = int(rng.integers(0, 1 << 32))
        rn = int(rng.choice([int(rng.integers(0, 1 << 32)), 0xFFFFFFFF - int(rng.integers(0, 3000))]))
        inflight = int(rng.integers(1, 50000))
        full = rng.random() < 0.15
        cs.append(conn1(snd_una=una, snd_nxt=una + inflight,
                        snd_wnd=inflight if full else int(rng.integers(50000, 90000)),
                        snd_wl1=rn - int(rng.integers(0, 3)), snd_wl2=una - int(rng.integers(0, 3)), rcv_nxt=rn,
                        rcv_wnd=int(rng.choice([1 << 20, int(rng.integers(500, 20000))])),
                        rcv_mss=int(rng.choice([1460, 536])), snd_wscale=int(rng.integers(0, 8)),
                        flags=(ELIGIBLE if rng.random() < 0.98 else 0) | (RXQ if rng.random() < 0.3 else 0) |
                        (ACK_DELAYED if rng.random() < 0.3 else 0), acks_delayed_cnt=int(rng.integers(0, 2))))
    nxt = [c["rcv_nxt"] for c in cs]
    una = [c["snd_una"] for c in cs]
    segs, st, pending = [], [], []
    for k in range(m):
        status = lc.GOOD
        if pending:
            segs.append(pending.pop())
            st.append(status)
            continue
        ck = int(rng.integers(0, nconn)) if flow is None else flow(k)
        c = cs[ck]
        left = (c["snd_nxt"] - una[ck]) & M32
        newack = (una[ck] + int(rng.integers(1, min(left, 2000) + 1))) & M32 if left else una[ck]
        win = int(rng.integers(0x4000, 1 << 16))
        r = rng.random()
        if r < stops:
            what = int(rng.integers(0, 6))
            s = [seg(rng, ck, nxt[ck], 0, ack=una[ck], flags=TCP_ACK | TCP_FIN),
                 seg(rng, ck, nxt[ck], 0, ack=una[ck], flags=TCP_RST),
                 seg(rng, ck, nxt[ck], 10, ack=una[ck], flags=TCP_ACK | TCP_URG),
                 seg(rng, ck, nxt[ck], 0, ack=una[ck], flags=TCP_ACK | TCP_SYN),
                 seg(rng, ck, nxt[ck] + 1460, 100, ack=una[ck]),
                 seg(rng, ck, nxt[ck] - 10, 100, ack=una[ck])][what]
        elif r < stops + noise:
            what = int(rng.integers(0, 8))
            if what == 0:
                s = seg(rng, ck, nxt[ck], c["rcv_mss"] + 1)
            elif what == 1:
                s = (ck, pc.udp_frame(rng, 100))
            elif what == 2:
                s = seg(rng, nconn + int(rng.integers(0, 5)), nxt[ck], 10)
            elif what == 3:
                s = seg(rng, int(rng.choice([pc.S_MISS, pc.S_NA, pc.S_MULTI])), nxt[ck], 10)
            elif what == 4:
                s, status = seg(rng, ck, nxt[ck], 10), lc.BAD
            elif what == 5:
                s = seg(rng, ck, nxt[ck] - 2000, 100, ack=una[ck])           # a whole duplicate
            elif what == 6:
                s = seg(rng, ck, nxt[ck], 0, ack=c["snd_nxt"] + 1 + int(rng.integers(0, 100)))
            else:
                s = seg(rng, ck, nxt[ck], int(rng.integers(0, 2)) * 10, ack=una[ck], flags=TCP_PUSH)   # no ACK flag
        elif r < 0.45:                                   # a pure ACK
            q = rng.random()
            if q < 0.55 and left:
                s = seg(rng, ck, nxt[ck], 0, ack=newack, win=win)
                una[ck] = newack
            elif q < 0.7:
                s = seg(rng, ck, nxt[ck], 0, ack=una[ck], win=0xFFFF)       # the window only
            elif q < 0.8:
                s = seg(rng, ck, nxt[ck], 0, ack=una[ck] - int(rng.integers(1, 1000)), win=win)
            else:                                        # duplicates: a window of 0 is never taken over a larger one
                s = seg(rng, ck, nxt[ck], 0, ack=una[ck], win=0)
                pending = [seg(rng, ck, nxt[ck], 0, ack=una[ck], win=0) for _ in range(int(rng.integers(0, 4)))]
        else:                                            # in-order text
            ln = int(rng.integers(1, c["rcv_mss"] + 1))
            ack = newack if rng.random() < 0.4 else una[ck]
            s = seg(rng, ck, nxt[ck], ln, ack=ack, win=win, doff=int(rng.choice([5, 8])),
                    flags=TCP_ACK | (TCP_PUSH if rng.random() < 0.2 else 0))
            nxt[ck] = (nxt[ck] + ln) & M32               # the generator's guess: good enough to keep chains going
            una[ck] = ack
        segs.append(s)
        st.append(status)
    case = build(cs, segs, align=align)
    case["st"] = np.array(st, dtype=np.uint8)
    case["rep_acks"] = rng.integers(0, 3, size=nconn).astype(np.uint8)
    return case


# seed, m, nconn, align, stops: many short runs, an aligned layout, runs longer than a wave, a wide align
STREAMS = ((1, 4096, 300, 0, 0.012), (2, 3000, 37, 64, 0.004), (3, 4096, 20, 0, 0.0007), (4, 2000, 300, 256, 0.012))


@functools.lru_cache(maxsize=None)
def stream(k):
    seed, m, nconn, align, stops = STREAMS[k]
    return random_case(seed, m, nconn, align=align, stops=stops)


def check_mix(want, nconn):
    """the conditions a random stream must meet, on the MODEL's output"""
    tcp = int((want["verdict"] <= DROP).sum())
    rule2 = int(want["counts"][C_RULE2])
    assert rule2 * 4 >= tcp, (rule2, tcp)
    assert (int(want["counts"][FAST]) - rule2) * 10 >= tcp
    assert int((want["out_conn"]["first_slow"] != NONE).sum()) * 20 >= nconn
    assert int(np.bitwise_or.reduce(want["sflags"])) == 0xFF
    assert (want["counts"] > 0).all(), want["counts"]


# ---------------------------------------------------------------- running the host twin
def blank(m, nconn):
    b = rc.blank(m, nconn)
    b["out_ext"] = np.frombuffer(bytes([SENTINEL]) * (EXT.itemsize * (nconn + GUARD)), dtype=EXT).copy()
    return b


def compare(got, want, m, nconn, what):
    """@got (blank() after a call) against @want: the written part equal byte for byte, the guard untouched"""
    rc.compare(got, want, m, nconn, what)
    g = got["out_ext"]
    assert len(g) == nconn + GUARD and (g[nconn:].view(np.uint8) == SENTINEL).all(), f"{what}: out_ext past its end"
    bad = np.nonzero(g[:nconn].view(np.uint8) != want["out_ext"][:nconn].view(np.uint8))[0]
    if len(bad):
        e = bad[0] // EXT.itemsize
        raise AssertionError(f"{what}: out_ext[{e}] = {g[e]} != {want['out_ext'][e]}")


def dims(case):
    order = case.get("order")
    return len(case["pkt_len"]) if order is None else len(order), len(case["conn"])


def run_host(g, case, counts=True, rep_acks="case"):
    """gcl_tcp_rx_full_host over sentinel-filled outputs: (outputs, counts)"""
    m, nconn = dims(case)
    out = blank(m, nconn)
    cnt = np.full(NR, 5, dtype=np.uint64) if counts else None
    g.tcp_rx_full_host(case["frames"], case["pkt_len"], case["sock"], case["conn"], stride=case["stride"],
                       offs=case["offs"], frames_len=case["frames_len"], order=case.get("order"), m=m,
                       l4_status=case.get("st"), nconn=nconn, align=case.get("align", 0),
                       blocks=case.get("blocks", 0),
                       rep_acks=case.get("rep_acks") if isinstance(rep_acks, str) else rep_acks, out=out, counts=cnt)
    return out, None if cnt is None else cnt - np.uint64(5)
