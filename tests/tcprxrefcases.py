"""The three TCP receive calls against what the REFERENCE's own tcp_rx_conn did
(tests/golden/tcprx_ref.json, recorded by tests/golden/make_tcprx_ref.py from
runtime/net/tcp_in.c compiled in place behind oracle/ref_tcpin.c): the recorded
cases, and the table that turns a connection's trace into the documented
outputs of gcl_tcp_rx ('rx'), gcl_tcp_rx_full ('full') and gcl_tcp_rx_ooo
('ooo') of include/gclassify.h.  The CPU and the GPU tests share it.

This is a table, not a model: whatever the reference shows is read off the
trace (the PCB words after each call, the calls of tcp_conn_ack, tcp_tx_ack,
tcp_timer_update and tcp_tx_fast_retransmit_start, the POLLIN and POLLOUT
wakes, the mbufs freed, the mbufs linked into c->rxq with the bytes pulled off
their front, rxq_ooo after each call).  A connection's segments are compared
one by one up to its first segment that meets a STOP REASON of the call's
header, evaluated on the trace's state before that segment and on the frame:
  'not taken'  the connection's flags (and for 'ooo' its input queue) say so;
  'slow path'  'rx': tcp_timer_update ran, which only __tcp_rx_conn calls;
  'flags'      'full', 'ooo': the slow path ran on FIN, RST, URG or SYN;
  'text'       'full': len > 0, seq != rcv_nxt and is_acceptable(tcp_in.c:27-51);
  'cap'        'ooo': the reference inserted the segment into an rxq_ooo of 64.
The expected first_slow is the first such segment, so a connection that does
not stop has none.  Three things the reference does leave no mark on its
state, and the table says so by name instead of guessing:
  WND_INVISIBLE    snd_wnd, snd_wl1 and snd_wl2 hold (win, seq, ack) before and
                   after: a rewrite cannot be seen, GCL_TCPRX_SF_WND may be
                   either (counted in Expected.loose);
  REP_INVISIBLE    rep_acks is 0 before and after every handled segment that
                   could have reset it: GCL_TCPO_REP_ACKS_RESET may be either
                   when reset_by_rule() (the header's own lines) says it is
                   set; that function is held to the trace wherever rep_acks
                   was not 0;
  took_ooo_branch  a refused duplicate (:129-130) and a segment that is not
                   acceptable are both freed and ACKed: GCL_OOOF_OOO of a
                   dropped segment is reached_ack_step() on the before-state.
"""
import functools
import json
import os

import numpy as np

from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests import tcprxocases as oc
from tests.tcprxcases import (ACK_DELAYED, DROP, ELIGIBLE, FAST, M32, NA, NOCONN, NONE, REP_ACKS_RESET, RXQ, SLOW,
                              STOPPED, TCP_ACK, TCP_FIN, TCP_RST, TCP_SYN, TCP_URG, TIMER_ARMED, WOKEN, wraps_gt,
                              wraps_lt, wraps_lte)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcprx_ref.json")
KINDS = ("rx", "full", "ooo")
TCP_STATE_ESTABLISHED, TCP_STATE_CLOSE_WAIT = 2, 5          # runtime/net/tcp.h:41-52
# the words of one stored trace record, in order; 'freed', 'linked' and 'q' follow by name where not empty
WORDS = ("snd_una", "snd_wnd", "snd_wl1", "snd_wl2", "rcv_nxt", "rcv_wnd", "acks_delayed_cnt", "ack_delayed",
         "rep_acks", "state", "ooo_len", "ack_ts", "slow", "conn_ack", "tx_ack", "pollin", "pollout", "fastrtx",
         "frees")
EXTRA = ("fail_err", "new_state", "rst_kind", "rst_seq", "rst_ack")

# the recorded random streams: small ones of the three files' own generators
STREAMS = {
    "rx:stream": lambda: rc.random_case(7, m=200, nconn=12),
    "full:stream": lambda: fc.random_case(8, m=260, nconn=10, stops=0.006),
    "ooo:reorder_and_loss": lambda: oc.random_case(9, m=200, nconn=5, swap=0.3, loss=0.15, stops=0.002),
    "ooo:overlapping_retransmits": lambda: oc.random_case(10, m=160, nconn=4, align=64, swap=0.05, loss=0.35,
                                                          stops=0.0),
}


@functools.lru_cache(maxsize=None)
def named():
    """name -> case: every named case of the three files"""
    res = {"rx:" + n: c for n, c in rc.cases().items()}
    res.update({"full:" + n: c for n, (c, _) in fc.cases().items()})
    res.update({"ooo:" + n: c for n, (c, _) in oc.cases().items()})
    return res


@functools.lru_cache(maxsize=None)
def case_of(name):
    return named()[name] if name in named() else STREAMS[name]()


def names():
    return sorted(named()) + sorted(STREAMS)


# ---------------------------------------------------------------- a case as the reference is fed it
def segments(case):
    """Per connection the list entries that reach tcp_rx_conn, in list order:
    dicts of j, the IPv4 header's offset and the mbuf's length, and the
    frame's seq, ack, flags, win (unscaled), len and src_off."""
    order, sock, conn = case.get("order"), case["sock"], case["conn"]
    pay = pc.model(case, order, sock, case.get("st"))
    n, flen = len(case["pkt_len"]), case["frames_len"]
    idx = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    res = [[] for _ in range(len(conn))]
    for j in range(len(idx)):
        if pay["kind"][j] != pc.K_TCP:
            continue
        i = int(idx[j])
        ck = int(sock[i])
        if ck >= len(conn):
            continue
        o = int(case["offs"][i]) if case["offs"] is not None else i * case["stride"]
        f = case["frames"][o:]
        res[ck].append(dict(j=j, ip=o + 14, mlen=min(int(case["pkt_len"][i]), flen - o) - 14, seq=pc.be(f, 38, 4),
                            ack=pc.be(f, 42, 4), flags=int(f[47]), win=pc.be(f, 48, 2), len=int(pay["len"][j]),
                            src=int(pay["src_off"][j])))
    return res


def conn_words(case, k):
    """connection k as oracle/ref_tcpin.c takes it"""
    c = case["conn"][k]
    fl = int(c["flags"])
    d = {f: int(c[f]) for f in ("snd_una", "snd_nxt", "snd_wnd", "snd_wl1", "snd_wl2", "rcv_nxt", "rcv_wnd", "rcv_mss",
                                "acks_delayed_cnt")}
    d.update(snd_wscale=int(c["snd_wscale"]) & 31, ack_delayed=int(bool(fl & ACK_DELAYED)), rxq=int(bool(fl & RXQ)),
             rep_acks=0 if case.get("rep_acks") is None else int(case["rep_acks"][k]),
             state=TCP_STATE_ESTABLISHED if fl & (ELIGIBLE | oc.ESTABLISHED) else TCP_STATE_CLOSE_WAIT)
    return d


def queue_of(case, k):
    """connection k's input queue: (first index into q, ENT records)"""
    a, b = oc.queue_range(case, k)
    return a, ([] if b == a else case["q"][a:b])


def record(ref, name):
    """the trace of every connection of case @name, as stored: one dict per
    connection that has segments or a queue"""
    case = case_of(name)
    conns = []
    for k, segs in enumerate(segments(case)):
        _, q = queue_of(case, k)
        if not segs and not len(q):
            continue
        cw = conn_words(case, k)
        trace, qfinal = ref.run(cw, [(int(e["seq"]), int(e["end"]), int(e["flags"])) for e in q], case["frames"],
                                [s["ip"] for s in segs], [s["mlen"] for s in segs])
        prev = dict(rcv_nxt=cw["rcv_nxt"], rcv_wnd=cw["rcv_wnd"], ooo_len=len(q), q=[-1 - i for i in range(len(q))])
        rows = []
        for t in trace:
            # the state before a call is the state after the one before: stored once
            assert (t["pre_rcv_nxt"], t["pre_rcv_wnd"], t["pre_ooo_len"]) == (prev["rcv_nxt"], prev["rcv_wnd"],
                                                                               prev["ooo_len"])
            assert t["ooo_len"] == len(t["q"]) and t["frees"] == len(t["freed"])
            row = {"t": [t[w] for w in WORDS]}
            if t["freed"]:
                row["f"] = t["freed"]
            if t["linked"]:
                row["l"] = [list(x) for x in t["linked"]]
            if t["q"] != prev["q"]:
                row["q"] = t["q"]
            if any(t[w] for w in EXTRA):
                row["x"] = [t[w] for w in EXTRA]
            rows.append(row)
            prev = t
        conns.append({"c": k, "segs": rows, "qfinal": [list(x) for x in qfinal]})
    return {"case": name, "conns": conns}


@functools.lru_cache(maxsize=None)
def load():
    with open(PATH) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def traces(name):
    """connection -> list of trace dicts (WORDS, pre_*, freed, linked, q, pre_q) of the stored case @name"""
    rec = next(r for r in load()["cases"] if r["case"] == name)
    case = case_of(name)
    res = {}
    for cr in rec["conns"]:
        k = cr["c"]
        cw = conn_words(case, k)
        nq = len(queue_of(case, k)[1])
        prev = dict(cw, ooo_len=nq, q=[-1 - i for i in range(nq)])
        rows = []
        for row in cr["segs"]:
            t = dict(zip(WORDS, row["t"]))
            t.update(freed=row.get("f", []), linked=[tuple(x) for x in row.get("l", [])], q=row.get("q", prev["q"]),
                     pre=prev)
            t.update(zip(EXTRA, row.get("x", [0] * len(EXTRA))))
            rows.append(t)
            prev = t
        res[k] = rows
    return res


# ---------------------------------------------------------------- the lines of the header the trace cannot show
def is_acceptable(pre, ln, seq, flags):
    """tcp_in.c:27-51 on the state before the segment"""
    nxt, wnd = pre["rcv_nxt"], pre["rcv_wnd"]
    def inside(x):
        return wraps_lte(nxt, x & M32) and wraps_lt(x & M32, (nxt + wnd) & M32)
    if ln == 0 and wnd == 0:
        return bool(flags & (TCP_ACK | TCP_URG | TCP_RST)) or seq == nxt
    if ln == 0:
        return inside(seq)
    if wnd == 0:
        return False
    return inside(seq) or inside(seq + ln - 1)


def reached_ack_step(pre, sg, snd_nxt):
    """the slow path got past :438, :459 and :498 to the duplicate-ACK lines (no FIN, RST, URG or SYN)"""
    return is_acceptable(pre, sg["len"], sg["seq"], sg["flags"]) and bool(sg["flags"] & TCP_ACK) and \
        not wraps_gt(sg["ack"], snd_nxt)


def reset_by_rule(t, sg, snd_nxt, win):
    """whether the header's lines set rep_acks = 0 in this call"""
    pre = t["pre"]
    if not t["slow"]:
        return bool(t["conn_ack"]) or (t["snd_wnd"], t["snd_wl1"], t["snd_wl2"]) != \
            (pre["snd_wnd"], pre["snd_wl1"], pre["snd_wl2"]) or \
            (wraps_lte(pre["snd_una"], sg["ack"]) and (pre["snd_wnd"], pre["snd_wl1"], pre["snd_wl2"]) ==
             (win, sg["seq"], sg["ack"]))
    if not reached_ack_step(pre, sg, snd_nxt):
        return False
    return bool(t["fastrtx"]) or (t["rep_acks"] != pre["rep_acks"] + 1 and t["snd_una"] == sg["ack"])


# ---------------------------------------------------------------- trace -> the documented outputs
class Expected:
    """What one call of @kind must leave for @case, by the stored traces.
    Arrays as the models': per entry verdict, sflags, rcv_nxt_after, copy_len,
    dst_off (and oflags, skip), out_conn, out_ext, conn_off, counts, and for
    'ooo' qin_*, qout_off, qout, totals.  wnd_loose[j]: GCL_TCPRX_SF_WND of
    entry j may be either; rep_loose[c]: REP_ACKS_RESET of connection c may be
    either; why[c]: the stop reason; compared: the handled segments; rxq[c]:
    (id, pulled, len) of the mbufs the reference linked into c->rxq up to the
    stop."""


def expected(kind, name):
    case, tr = case_of(name), traces(name)
    conn = case["conn"]
    nconn = len(conn)
    m, _ = fc.dims(case)
    segs = segments(case)
    align = max(case.get("align", 0), 1)
    pay = pc.model(case, case.get("order"), case["sock"], case.get("st"))
    q = case.get("q") if kind == "ooo" else None
    nq = 0 if q is None else len(q)
    nr = {"rx": rc.NR, "full": fc.NR, "ooo": oc.NR}[kind]
    e = Expected()
    e.kind, e.compared, e.loose, e.why, e.rxq = kind, 0, 0, {}, [[] for _ in range(nconn)]
    out = {f: np.zeros(m, dtype=dt) for f, dt in oc.ENTRY}
    out.update({f: np.zeros(nq, dtype=dt) for f, dt in oc.QIN})
    e.wnd_loose, e.rep_loose = np.zeros(m, dtype=bool), np.zeros(nconn, dtype=bool)
    counts = [0] * oc.NR
    # the verdicts that never reach tcp_rx_conn
    out["verdict"][:] = NA
    idx = np.arange(m, dtype=np.int64) if case.get("order") is None else np.asarray(case["order"]).astype(np.int64)
    for j in range(m):
        if pay["kind"][j] == pc.K_TCP:
            out["verdict"][j] = NOCONN          # overwritten below for the connections that exist
    ocn, ext = np.zeros(nconn, dtype=rc.CONN_OUT), np.zeros(nconn, dtype=fc.EXT)
    off, at = np.zeros(nconn + 1, dtype=np.uint64), 0
    qout, qout_off = [], np.zeros(nconn + 1, dtype=np.uint32)
    for k in range(nconn):
        cw = conn_words(case, k)
        fl = int(conn[k]["flags"])
        qa, qk = queue_of(case, k) if kind == "ooo" else (0, [])
        if kind == "ooo":
            taken = bool(fl & (ELIGIBLE | oc.ESTABLISHED)) and len(qk) <= oc.CAP and \
                not any(int(x["flags"]) & TCP_FIN for x in qk)
        else:
            taken = bool(fl & ELIGIBLE)
            # ELIGIBLE promises an empty rxq_ooo; the recorded trace had the case's queue
            assert not (taken and len(queue_of(case, k)[1])), (name, k)
        snd_nxt = cw["snd_nxt"]
        rows = tr.get(k, [])
        assert len(rows) == len(segs[k]), (name, k)
        last = dict(cw, q=[-1 - i for i in range(len(qk))] if taken else [])
        stopped, first_slow, nfast, nslow, nacks, nrule2, ndropped = False, NONE, 0, 0, 0, 0, 0
        woken, armed, txwake, fastrtx, fast_rtx_ack, rxq_any = False, False, False, False, 0, bool(cw["rxq"])
        rep_must, rep_may = False, False
        where, freed_at, handled = {}, {}, []        # id -> (pulled, len, position in rxq); id -> segment that freed it
        for s, (sg, t) in enumerate(zip(segs[k], rows)):
            j, pre = sg["j"], t["pre"]
            win = (sg["win"] << cw["snd_wscale"]) & M32
            if not t["slow"] and t["freed"] == [s]:
                # :207-210: freed before the lock, nothing read or changed
                assert not t["linked"] and sg["len"] > cw["rcv_mss"]
                out["verdict"][j] = DROP
                counts[DROP] += 1
                continue
            if not stopped:
                inserted = bool(t["slow"]) and sg["len"] > 0 and s not in t["freed"] and \
                    wraps_gt(sg["seq"], pre["rcv_nxt"])
                why = None
                if not taken:
                    why = "not taken"
                elif kind == "rx":
                    why = "slow path" if t["slow"] else None
                elif t["slow"] and sg["flags"] & (TCP_FIN | TCP_RST | TCP_URG | TCP_SYN):
                    why = "flags"
                elif kind == "full" and t["slow"] and sg["len"] > 0 and sg["seq"] != pre["rcv_nxt"] and \
                        is_acceptable(pre, sg["len"], sg["seq"], sg["flags"]):
                    why = "text"
                elif kind == "ooo" and inserted and pre["ooo_len"] >= oc.CAP:
                    why = "cap"
                if why:
                    stopped, first_slow, e.why[k] = True, j, why
            if stopped:
                out["verdict"][j] = SLOW
                counts[SLOW] += 1
                nslow += 1
                continue
            # ---- a handled segment: every field from the trace
            e.compared += 1
            handled.append(s)
            sf = (rc.SF_WAKE if t["pollin"] else 0) | (rc.SF_ACK_NOW if t["tx_ack"] else 0) | \
                 (rc.SF_ACKED if t["conn_ack"] else 0)
            triple = (t["snd_wnd"], t["snd_wl1"], t["snd_wl2"])
            if triple != (pre["snd_wnd"], pre["snd_wl1"], pre["snd_wl2"]):
                sf |= rc.SF_WND
            elif triple == (win, sg["seq"], sg["ack"]):
                e.wnd_loose[j] = True                # WND_INVISIBLE
                e.loose += 1
            dropped = bool(t["slow"]) and s in t["freed"]
            if kind != "rx":
                sf |= (fc.SF_RULE2 if t["slow"] else 0) | (fc.SF_TXWAKE if t["pollout"] else 0) | \
                      (fc.SF_FASTRTX if t["fastrtx"] else 0) | (fc.SF_DROPPED if dropped else 0)
            else:
                assert not t["slow"]
            out["verdict"][j], out["sflags"][j], out["rcv_nxt_after"][j] = FAST, sf, t["rcv_nxt"]
            counts[FAST] += 1
            nfast += 1
            nacks += bool(t["tx_ack"])
            nrule2 += bool(t["slow"])
            ndropped += dropped
            woken |= bool(t["pollin"])
            armed |= bool(t["ack_ts"])
            txwake |= bool(t["pollout"])
            if t["fastrtx"]:
                fastrtx, fast_rtx_ack = True, sg["ack"]
            if t["rep_acks"] == pre["rep_acks"] + 1 or t["fastrtx"]:
                counts[fc.C_DUPACKS] += 1                        # rep_acks++, also where the threshold zeroed it
            rule = reset_by_rule(t, sg, snd_nxt, win)
            if pre["rep_acks"] != 0 or t["rep_acks"] != 0:
                seen = t["rep_acks"] == 0                        # the reset is in the trace
                assert seen == rule, (name, k, s, "reset_by_rule disagrees with the reference")
                rep_must |= seen
            else:
                rep_may |= rule                                  # REP_INVISIBLE
            for slot, bit in ((rc.C_ACKS, rc.SF_ACK_NOW), (rc.C_WAKES, rc.SF_WAKE), (fc.C_RULE2, fc.SF_RULE2),
                              (fc.C_TXWAKES, fc.SF_TXWAKE), (fc.C_FASTRTX, fc.SF_FASTRTX),
                              (fc.C_DROPPED, fc.SF_DROPPED)):
                counts[slot] += bool(sf & bit)
            if kind == "ooo":
                ofl = 0
                if inserted:
                    ofl = oc.O_OOO | oc.O_QUEUED
                    counts[oc.C_QUEUED] += 1
                elif dropped and sg["len"] > 0 and wraps_gt(sg["seq"], pre["rcv_nxt"]) and \
                        reached_ack_step(pre, sg, snd_nxt):
                    ofl = oc.O_OOO                               # took_ooo_branch: refused by :129-130
                    assert pre["ooo_len"] > 0
                counts[oc.C_OOO] += bool(ofl)
                out["oflags"][j] = ofl
            for ident in t["freed"]:
                if ident != s:
                    freed_at[ident] = s
                    counts[oc.C_FREED] += 1
            for ident, pulled, ln in t["linked"]:
                where[ident] = (pulled, ln, len(e.rxq[k]), s)
                e.rxq[k].append((ident, pulled, ln))
                rxq_any = True
                if ident != s:
                    counts[oc.C_DRAINED] += 1
                counts[oc.C_HEADCLIP] += bool(pulled)
            last = t
        # ---- the connection after its last handled segment
        e.rep_loose[k] = rep_may and not rep_must
        flo = (RXQ if rxq_any else 0) | (ACK_DELAYED if last["ack_delayed"] else 0) | (STOPPED if stopped else 0) | \
              (WOKEN if woken else 0) | (TIMER_ARMED if armed else 0) | (REP_ACKS_RESET if rep_must or rep_may else 0)
        ocn[k] = (last["snd_una"], last["snd_wnd"], last["snd_wl1"], last["snd_wl2"], last["rcv_nxt"],
                  last["rcv_wnd"], nfast, nslow, nacks, first_slow, last["acks_delayed_cnt"], flo, 0)
        xfl = (fc.X_TXWAKE if txwake else 0) | (fc.X_FASTRTX if fastrtx else 0) | \
              (oc.X_QSKIP if kind == "ooo" and not taken and len(qk) else 0)
        ext[k] = (nrule2, ndropped, fast_rtx_ack, last["rep_acks"] & 0xFF, xfl, 0)
        off[k] = at
        pos = 0
        for ident, pulled, ln in e.rxq[k]:
            if ident >= 0:
                j = segs[k][ident]["j"]
                out["copy_len"][j], out["skip"][j] = ln, pulled
                out["dst_off"][j] = at + pos if ln else 0
                if pulled:
                    out["oflags"][j] |= oc.O_HEADCLIP
                if where[ident][3] != ident:
                    out["oflags"][j] |= oc.O_LATE_DRAINED
            else:
                i = qa + (-1 - ident)
                out["qin_state"][i] = oc.Q_DRAINED
                out["qin_skip"][i], out["qin_len"][i] = min(pulled, 0xFFFF), min(ln, 0xFFFF)
                out["qin_dst_off"][i] = at + pos if ln else 0
            pos += ln
        assert pos == (last["rcv_nxt"] - cw["rcv_nxt"]) & M32, (name, k)      # the layout's own premise
        counts[rc.C_BYTES] += pos
        at += -(-pos // align) * align
        for ident, s in freed_at.items():
            if ident >= 0:
                out["oflags"][segs[k][ident]["j"]] |= oc.O_LATE_FREED
            else:
                out["qin_state"][qa + (-1 - ident)] = oc.Q_FREED
        qout_off[k] = len(qout)
        for ident in (last["q"] if kind == "ooo" and taken else []):
            if ident >= 0:
                sg = segs[k][ident]
                out["oflags"][sg["j"]] |= oc.O_HELD
                counts[oc.C_HELD] += 1
                qout.append((sg["seq"], (sg["seq"] + sg["len"]) & M32, sg["j"], sg["flags"], 1))
            else:
                x = qk[-1 - ident]
                out["qin_state"][qa + (-1 - ident)] = oc.Q_KEPT
                qout.append((int(x["seq"]), int(x["end"]), int(x["ref"]), int(x["flags"]), 0))
    for j in range(m):
        v = int(out["verdict"][j])
        if v in (NA, NOCONN):
            counts[v] += 1
    off[nconn] = at
    qout_off[nconn] = len(qout)
    assert sum(counts[:5]) == m
    e.out = dict(out, out_conn=ocn, out_ext=ext, conn_off=off, counts=np.array(counts[:nr], dtype=np.uint64),
                 qout_off=qout_off, qout=np.array(qout, dtype=oc.ENT) if qout else np.zeros(0, dtype=oc.ENT),
                 totals=np.array([len(qout)], dtype=np.uint64))
    e.m, e.nconn, e.nq, e.q_out_cap = m, nconn, nq, oc.qcap(case)
    return e


ENTRY_FIELDS = {"rx": ("verdict", "sflags", "rcv_nxt_after", "copy_len", "dst_off"),
                "full": ("verdict", "sflags", "rcv_nxt_after", "copy_len", "dst_off"),
                "ooo": ("verdict", "sflags", "rcv_nxt_after", "copy_len", "dst_off", "oflags", "skip")}


def check(e, got, counts, what):
    """@got (a model()-shaped dict, or sentinel-filled buffers after a call:
    only the documented elements are read) and @counts against Expected @e.
    Returns the number of handled segments compared."""
    w, kind = e.out, e.kind
    for f in ENTRY_FIELDS[kind]:
        g, x = np.asarray(got[f][:e.m]), w[f]
        if f == "sflags":
            g = np.where(e.wnd_loose, g & ~np.uint8(rc.SF_WND), g)
            if kind == "rx":
                assert not (g & 0xF0).any(), (what, "rx sflags has a slow-rule bit")
        bad = np.nonzero(g != x)[0]
        assert not len(bad), f"{what}: {f}[{bad[0]}] = {g[bad[0]]}, the reference gives {x[bad[0]]} ({len(bad)} differ)"
    for f in rc.CONN_OUT.names:
        if f == "pad":
            continue
        g, x = np.asarray(got["out_conn"][f][:e.nconn]), w["out_conn"][f]
        if f == "flags":
            lo = np.where(e.rep_loose, np.uint8(REP_ACKS_RESET), np.uint8(0))
            g, x = g | lo, x | lo
        bad = np.nonzero(g != x)[0]
        assert not len(bad), f"{what}: out_conn[{bad[0]}].{f} = {g[bad[0]]}, the reference gives {x[bad[0]]}"
    assert np.asarray(got["conn_off"][:e.nconn + 1]).tolist() == w["conn_off"].tolist(), (what, "conn_off")
    if kind != "rx":
        for f in fc.EXT.names:
            if f == "pad":
                continue
            g, x = np.asarray(got["out_ext"][f][:e.nconn]), w["out_ext"][f]
            bad = np.nonzero(g != x)[0]
            assert not len(bad), f"{what}: out_ext[{bad[0]}].{f} = {g[bad[0]]}, the reference gives {x[bad[0]]}"
    if kind == "ooo":
        for f, _ in oc.QIN:
            assert np.asarray(got[f][:e.nq]).tolist() == w[f].tolist(), (what, f)
        assert np.asarray(got["qout_off"][:e.nconn + 1]).tolist() == w["qout_off"].tolist(), (what, "qout_off")
        assert int(got["totals"][0]) == len(w["qout"]), (what, "totals")
        k = min(len(w["qout"]), e.q_out_cap)
        for f in ("seq", "end", "ref", "flags", "src"):
            assert np.asarray(got["qout"][f][:k]).tolist() == w["qout"][f][:k].tolist(), (what, "qout", f)
    if counts is not None:
        assert [int(x) for x in counts] == w["counts"].tolist(), (what, "counts", list(counts), w["counts"].tolist())
    # nothing else was skipped: every entry the call handled was compared
    handled = int((np.asarray(got["verdict"][:e.m]) == FAST).sum())
    assert handled == e.compared, (what, handled, e.compared)
    return e.compared


def rxq_bytes(e, name, k):
    """the bytes of the mbufs the reference linked into connection k's rxq up
    to the stop, in its order (list entries only: an input queue entry has no
    bytes behind it)"""
    case = case_of(name)
    sg = segments(case)[k]
    res = b""
    for ident, pulled, ln in e.rxq[k]:
        assert ident >= 0
        a = sg[ident]["src"] + pulled
        res += case["frames"][a:a + ln].tobytes()
    return res


def copy_cases():
    """the recorded cases whose linked mbufs are all list entries (the whole rxq has bytes)"""
    return [n for n in names() if case_of(n).get("q") is None or not len(case_of(n)["q"])]
