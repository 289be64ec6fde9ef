"""gcl_tcp_rx_states against what the REFERENCE's own tcp_rx_conn did
(tests/golden/tcprxs_ref.json, recorded by tests/golden/make_tcprxs_ref.py from
runtime/net/tcp_in.c compiled in place behind oracle/ref_tcpin.c, each
connection started in the case's state word): the recorded cases and the check
that holds a call's outputs to a connection's trace.  The CPU and the GPU tests
share it.

Whatever the reference shows is read off the trace.  A connection's segments
are compared one by one up to and with its first segment that called
tcp_conn_fail (fail_err != 0) or closed from LAST_ACK: the driver's
tcp_conn_fail is a stub and leaves the state alone, and the call stops there.
Named exceptions, because the driver leaves no mark:
  OPENED_WAKE    tcp_conn_set_state is a stub: GCL_TCPX_OPENED's POLLOUT is
                 held to tcp.c:254-258 by the rule header, not to the trace;
  TIMEWAIT_TS    time_wait_ts is not in the trace: GCL_TCPX_TIMEWAIT is held
                 to new_state == TIME_WAIT;
  LAST_STATE     new_state records only the last transition of a segment:
                 state_after is compared with the trace's state, and
                 GCL_TCPS_STATE with 'new_state was set';
  QUEUE_ENTRY    the driver gives an input queue entry end - seq bytes, its
                 FIN octet counted: qin_len is held to that length less one
                 for an entry with FIN, not below 0;
  NOT_TAKEN      a connection in SYN_SENT, or in no state the header takes, is
                 not recorded: the call does not walk it.
No named case is left out.
"""
import functools
import json
import os

import numpy as np

from tests import tcprxrefcases as rr
from tests import tcprxscases as sc
from tests.tcprxcases import ACK_DELAYED, FAST, M32, SLOW, TCP_FIN, TIMER_ARMED
from tests.tcprxfcases import SF_ACK_NOW, SF_ACKED, SF_DROPPED, SF_FASTRTX, SF_RULE2, SF_TXWAKE, SF_WAKE

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcprxs_ref.json")
WORDS, EXTRA = rr.WORDS, rr.EXTRA
ECONNRESET = 104

# the recorded random stream: a thinned one of tests/tcprxscases.py's generator
STREAMS = {"stream:lifetimes": lambda: sc.random_case(21, nconn=36, garbage=0.2)}


@functools.lru_cache(maxsize=None)
def case_of(name):
    return sc.case_of(name) if name in sc.cases() else STREAMS[name]()


def names():
    return sorted(sc.cases()) + sorted(STREAMS)


def recorded(case, k):
    return 1 <= sc.state_in(case, k) <= 9


def conn_words(case, k):
    d = rr.conn_words(case, k)
    d["state"] = sc.state_in(case, k)
    return d


def record(ref, name):
    """the trace of every recorded connection of case @name, as stored"""
    case = case_of(name)
    conns = []
    for k, segs in enumerate(rr.segments(case)):
        _, q = rr.queue_of(case, k)
        if (not segs and not len(q)) or not recorded(case, k):
            continue
        cw = conn_words(case, k)
        trace, qfinal = ref.run(cw, [(int(e["seq"]), int(e["end"]), int(e["flags"])) for e in q], case["frames"],
                                [s["ip"] for s in segs], [s["mlen"] for s in segs])
        prev_q = [-1 - i for i in range(len(q))]
        rows = []
        for t in trace:
            assert t["ooo_len"] == len(t["q"]) and t["frees"] == len(t["freed"])
            row = {"t": [t[w] for w in WORDS]}
            if t["freed"]:
                row["f"] = t["freed"]
            if t["linked"]:
                row["l"] = [list(x) for x in t["linked"]]
            if t["q"] != prev_q:
                row["q"] = t["q"]
            if any(t[w] for w in EXTRA):
                row["x"] = [t[w] for w in EXTRA]
            rows.append(row)
            prev_q = t["q"]
        conns.append({"c": k, "segs": rows})
    return {"case": name, "conns": conns}


@functools.lru_cache(maxsize=None)
def load():
    with open(PATH) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def traces(name):
    """connection -> list of trace dicts of the stored case @name"""
    rec = next(r for r in load()["cases"] if r["case"] == name)
    case = case_of(name)
    res = {}
    for cr in rec["conns"]:
        k = cr["c"]
        nq = len(rr.queue_of(case, k)[1])
        prev_q, rows = [-1 - i for i in range(nq)], []
        for row in cr["segs"]:
            t = dict(zip(WORDS, row["t"]))
            t.update(freed=row.get("f", []), linked=[tuple(x) for x in row.get("l", [])], q=row.get("q", prev_q))
            t.update(zip(EXTRA, row.get("x", [0] * len(EXTRA))))
            rows.append(t)
            prev_q = t["q"]
        res[k] = rows
    return res


def comparable():
    """the recorded segments up to and with each connection's first FAIL or PUT: what check() must have compared"""
    total = 0
    for name in names():
        for rows in traces(name).values():
            for t in rows:
                total += 1
                if t["fail_err"] or (t["new_state"] and t["new_state"] - 1 == sc.CLOSED):
                    break
    return total


def check(got, name, what):
    """@got (the outputs of one call on case @name, sentinel-filled or not)
    against the stored traces.  Returns the number of segments compared."""
    case, tr = case_of(name), traces(name)
    segs = rr.segments(case)
    compared = 0
    for k in range(len(case["conn"])):
        if not recorded(case, k):
            for sg in segs[k]:
                assert got["verdict"][sg["j"]] == SLOW, (what, k, "a connection that is not taken was walked")
            continue
        rows = tr.get(k, [])
        assert len(rows) == len(segs[k]), (what, k)
        qa, qk = rr.queue_of(case, k)
        ended, last, armed, woken = False, None, False, False
        for s, (sg, t) in enumerate(zip(segs[k], rows)):
            j = sg["j"]
            w = (what, name, k, s)
            if ended:
                assert got["verdict"][j] == SLOW, (w, "handled behind FAIL or PUT")
                continue
            assert got["verdict"][j] == FAST, (w, "verdict", got["verdict"][j])
            compared += 1
            sf, ev = int(got["sflags"][j]), int(got["ev"][j])
            assert int(got["rcv_nxt_after"][j]) == t["rcv_nxt"], (w, "rcv_nxt", int(got["rcv_nxt_after"][j]), t["rcv_nxt"])
            assert int(got["state_after"][j]) == t["state"], (w, "state", int(got["state_after"][j]), t["state"])
            assert bool(sf & SF_ACK_NOW) == bool(t["tx_ack"]), (w, "ACK_NOW")
            assert bool(sf & SF_WAKE) == bool(t["pollin"]), (w, "WAKE")
            assert bool(sf & SF_TXWAKE) == bool(t["pollout"]), (w, "TXWAKE")
            assert bool(sf & SF_ACKED) == bool(t["conn_ack"]), (w, "ACKED")
            assert bool(sf & SF_FASTRTX) == bool(t["fastrtx"]), (w, "FASTRTX")
            assert bool(sf & SF_RULE2) == bool(t["slow"]), (w, "RULE2")
            assert bool(sf & SF_DROPPED) == (bool(t["slow"]) and s in t["freed"]), (w, "DROPPED")
            kind = 1 if ev & sc.EV_RST else 2 if ev & sc.EV_RST_ACK else 0
            assert kind == t["rst_kind"], (w, "rst_kind", kind, t["rst_kind"])
            assert int(got["rst_seq"][j]) == (t["rst_seq"] if kind == 1 else t["rst_ack"] if kind == 2 else 0), \
                (w, "rst_seq")
            assert bool(ev & sc.EV_FAIL) == (t["fail_err"] != 0) and t["fail_err"] in (0, ECONNRESET), (w, "FAIL")
            assert bool(ev & sc.EV_STATE) == bool(t["new_state"]), (w, "STATE")             # LAST_STATE
            put = bool(t["new_state"]) and t["new_state"] - 1 == sc.CLOSED
            assert bool(ev & sc.EV_PUT) == put, (w, "PUT")
            for ident, pulled, ln in t["linked"]:
                if ident >= 0:
                    jj = segs[k][ident]["j"]
                    assert (int(got["copy_len"][jj]), int(got["skip"][jj])) == (ln, pulled), \
                        (w, "linked", ident, int(got["copy_len"][jj]), int(got["skip"][jj]), ln, pulled)
                else:
                    i = qa + (-1 - ident)
                    want = max(ln - 1, 0) if int(qk[-1 - ident]["flags"]) & TCP_FIN else ln     # QUEUE_ENTRY
                    assert (int(got["qin_len"][i]), int(got["qin_skip"][i])) == (min(want, 0xFFFF), min(pulled, 0xFFFF)), \
                        (w, "linked entry", ident)
            armed |= bool(t["ack_ts"])
            woken |= bool(t["pollin"])
            last = t
            ended = t["fail_err"] != 0 or put
        done = rows[:rows.index(last) + 1] if last is not None else []
        ever = {x[0] for t in done for x in t["linked"]}
        for s in range(len(done)):                 # what the reference never linked carries no bytes
            if s not in ever:
                assert int(got["copy_len"][segs[k][s]["j"]]) == 0, (what, name, k, s, "copy_len")
        oc_, ex = got["out_conn"][k], got["out_ext"][k]
        if last is not None:
            for f in ("snd_una", "snd_wnd", "snd_wl1", "snd_wl2", "rcv_nxt", "rcv_wnd", "acks_delayed_cnt"):
                assert int(oc_[f]) == last[f], (what, name, k, f, int(oc_[f]), last[f])
            assert bool(int(oc_["flags"]) & ACK_DELAYED) == bool(last["ack_delayed"]), (what, name, k, "ack_delayed")
            assert bool(int(oc_["flags"]) & TIMER_ARMED) == armed, (what, name, k, "TIMER_ARMED")
            assert int(ex["rep_acks"]) == last["rep_acks"] & 0xFF, (what, name, k, "rep_acks")
            assert int(got["state_out"][k]) == last["state"], (what, name, k, "state_out")
            tw = any(t["new_state"] - 1 == sc.TIME_WAIT for t in rows[:rows.index(last) + 1] if t["new_state"])
            assert bool(int(ex["xflags"]) & sc.X_TIMEWAIT) == tw, (what, name, k, "TIMEWAIT")          # TIMEWAIT_TS
            # the queue as it stood after the last handled segment
            a, b = int(got["qout_off"][k]), int(got["qout_off"][k + 1])
            ids = [int(e["ref"]) if int(e["src"]) else None for e in got["qout"][a:b]]
            want = [segs[k][i]["j"] if i >= 0 else None for i in last["q"]]
            assert ids == want, (what, name, k, "queue", ids, want)
            refs = [int(e["ref"]) for e in got["qout"][a:b] if not int(e["src"])]
            assert refs == [int(qk[-1 - i]["ref"]) for i in last["q"] if i < 0], (what, name, k, "queue refs")
    return compared
