"""The definition of gcl_tcp_rx (include/gclassify.h) in Python, and the cases
the CPU and GPU tests share.  The model transcribes tcp_rx_conn's fast path
(runtime/net/tcp_in.c:197-296) line by line over a dict of PCB fields; it knows
nothing of csrc/gcl_tcprx.h.  Which list entries are TCP segments, and how long
they are, is tests/paycases.py's model of gcl_l4_payload.

A case is tests/l4cases.py's dict (frames, frames_len, offs or stride, pkt_len)
plus sock (u32[n]), conn (CONN records indexed by cookie), and optionally
order, st (l4_status), align and blocks.
"""
import functools

import numpy as np

from tests import l4cases as lc
from tests import paycases as pc

FAST, SLOW, DROP, NOCONN, NA = range(5)
C_BYTES, C_ACKS, C_WAKES, NR = 5, 6, 7, 8
SF_WAKE, SF_ACK_NOW, SF_ACKED, SF_WND = 1, 2, 4, 8
ELIGIBLE, RXQ, ACK_DELAYED, STOPPED, WOKEN, TIMER_ARMED, REP_ACKS_RESET = 1, 2, 4, 8, 16, 32, 64
TCP_FIN, TCP_SYN, TCP_RST, TCP_PUSH, TCP_ACK, TCP_URG = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
TCP_SLOWPATH_FLAGS = TCP_FIN | TCP_RST | TCP_URG
NONE, M32 = 0xFFFFFFFF, 0xFFFFFFFF
MAX_BLOCKS, MAX_CONN, PASS_CONN = 1024, 1 << 20, 2048
CONN = np.dtype([("snd_una", "<u4"), ("snd_nxt", "<u4"), ("snd_wnd", "<u4"), ("snd_wl1", "<u4"),
                 ("snd_wl2", "<u4"), ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("rcv_mss", "<u2"),
                 ("snd_wscale", "u1"), ("flags", "u1"), ("acks_delayed_cnt", "u1"), ("pad", "u1", (15,))])
CONN_OUT = np.dtype([("snd_una", "<u4"), ("snd_wnd", "<u4"), ("snd_wl1", "<u4"), ("snd_wl2", "<u4"),
                     ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("nfast", "<u4"), ("nslow", "<u4"),
                     ("nacks", "<u4"), ("first_slow", "<u4"), ("acks_delayed_cnt", "u1"), ("flags", "u1"),
                     ("pad", "u1", (6,))])
SENTINEL, GUARD = 0xA7, 16
ENTRY = (("verdict", np.uint8), ("sflags", np.uint8), ("rcv_nxt_after", np.uint32), ("copy_len", np.uint16),
         ("dst_off", np.uint64))


# inc/base/stddef.h:144-178
def wraps_lt(a, b):
    return ((a - b) & M32) >= 0x80000000


def wraps_lte(a, b):
    return a == b or wraps_lt(a, b)


def wraps_gt(a, b):
    return wraps_lt(b, a)


def model(case, with_rxq=False):
    """Every output of one call as a dict (the per-entry arrays, out_conn,
    conn_off, counts); with @with_rxq also 'rxq': per connection the bytes of
    the mbufs the fast path appended to c->rxq, in order."""
    order, sock, st, conn = case.get("order"), case["sock"], case.get("st"), case["conn"]
    align = max(case.get("align", 0), 1)
    pay = pc.model(case, order, sock, st)
    n, nconn = len(case["pkt_len"]), len(conn)
    idx = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    m = len(idx)
    out = {f: np.zeros(m, dtype=dt) for f, dt in ENTRY}
    counts = [0] * NR
    pcb = [{k: int(conn[c][k]) for k in CONN.names if k != "pad"} for c in range(nconn)]
    for c in pcb:
        c.update(state_ok=bool(c["flags"] & ELIGIBLE), rxq=bool(c["flags"] & RXQ),
                 ack_delayed=bool(c["flags"] & ACK_DELAYED), stopped=False, woken=False, armed=False,
                 rep_reset=False, nfast=0, nslow=0, nacks=0, first_slow=NONE, bytes=[])
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
        # :221-239
        slow_path = (flags & TCP_SLOWPATH_FLAGS) != 0 or ln == 0 or wraps_gt(ack, snd_nxt)
        slow_path |= not c["state_ok"]
        slow_path |= wraps_lte((c["snd_una"] + c["snd_wnd"]) & M32, c["snd_nxt"])
        slow_path |= seq != c["rcv_nxt"]
        slow_path |= c["rcv_wnd"] < ln
        slow_path |= wraps_gt(ack, snd_nxt)
        if c["stopped"] or slow_path:
            if not c["stopped"]:
                c["first_slow"] = j
            c["stopped"] = True
            c["nslow"] += 1
            out["verdict"][j] = SLOW
            counts[SLOW] += 1
            continue
        sf = 0
        # :247-264
        if wraps_lte(c["snd_una"], ack):
            if c["snd_una"] != ack:
                c["rep_reset"] = True
                c["snd_una"] = ack
                sf |= SF_ACKED
            if wraps_lt(c["snd_wl1"], seq) or (c["snd_wl1"] == seq and wraps_lte(c["snd_wl2"], ack)):
                c["snd_wnd"], c["snd_wl1"], c["snd_wl2"] = win, seq, ack
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
        src = int(pay["src_off"][j])
        c["bytes"].append((j, case["frames"][src:src + ln].tobytes()))
        c["nfast"] += 1
        c["nacks"] += bool(sf & SF_ACK_NOW)
        out["verdict"][j], out["sflags"][j] = FAST, sf
        out["rcv_nxt_after"][j], out["copy_len"][j] = c["rcv_nxt"], ln
        counts[FAST] += 1
        counts[C_BYTES] += ln
        counts[C_ACKS] += bool(sf & SF_ACK_NOW)
        counts[C_WAKES] += bool(sf & SF_WAKE)
    oc, off, at = np.zeros(nconn, dtype=CONN_OUT), np.zeros(nconn + 1, dtype=np.uint64), 0
    for k, c in enumerate(pcb):
        fl = (RXQ if c["rxq"] else 0) | (ACK_DELAYED if c["ack_delayed"] else 0) | \
             (STOPPED if c["stopped"] else 0) | (WOKEN if c["woken"] else 0) | \
             (TIMER_ARMED if c["armed"] else 0) | (REP_ACKS_RESET if c["rep_reset"] else 0)
        oc[k] = (c["snd_una"], c["snd_wnd"], c["snd_wl1"], c["snd_wl2"], c["rcv_nxt"], c["rcv_wnd"], c["nfast"],
                 c["nslow"], c["nacks"], c["first_slow"], c["acks_delayed_cnt"], fl, 0)
        off[k] = at
        pos = 0
        for j, b in c["bytes"]:
            out["dst_off"][j] = at + pos
            pos += len(b)
        assert pos == (c["rcv_nxt"] - int(conn[k]["rcv_nxt"])) & M32
        at += -(-pos // align) * align
    off[nconn] = at
    assert sum(counts[:5]) == m
    res = dict(out, out_conn=oc, conn_off=off, counts=np.array(counts, dtype=np.uint64))
    if with_rxq:
        res["rxq"] = [b"".join(b for _, b in c["bytes"]) for c in pcb]
    return res


# ---------------------------------------------------------------- builders
def conn1(**kw):
    """One established connection with room on every side."""
    d = dict(snd_una=1000, snd_nxt=5000, snd_wnd=60000, snd_wl1=99, snd_wl2=1000, rcv_nxt=100, rcv_wnd=1 << 20,
             rcv_mss=1460, snd_wscale=0, flags=ELIGIBLE, acks_delayed_cnt=0)
    d.update(kw)
    return d


def conns(ds):
    a = np.zeros(len(ds), dtype=CONN)
    for k, d in enumerate(ds):
        for f, v in d.items():
            a[k][f] = v & M32
    return a


def seg(rng, ck, seq, pay, ack=1000, flags=TCP_ACK, win=0xF000, doff=5):
    """(cookie, frame) of one TCP segment"""
    f = pc.tcp_frame(rng, doff, pay)
    f[38:42] = list((seq & M32).to_bytes(4, "big"))
    f[42:46] = list((ack & M32).to_bytes(4, "big"))
    f[47] = flags
    f[48:50] = (win >> 8, win & 0xFF)
    return ck, f


def chain(rng, ck, c, lens, **kw):
    """in-order segments of the payload lengths @lens for connection dict @c"""
    at, res = c["rcv_nxt"], []
    for ln in lens:
        res.append(seg(rng, ck, at, ln, ack=kw.get("ack", c["snd_una"]), flags=kw.get("flags", TCP_ACK),
                       win=kw.get("win", 0xF000)))
        at += ln
    return res


def build(cs, segs, **kw):
    """A case of the connections @cs (dicts) and the (cookie, frame) list @segs."""
    rng = np.random.default_rng(len(segs))
    if segs:
        case = lc.layout([f for _, f in segs], aligns=[int(a) for a in rng.integers(0, 16, size=len(segs))])
    else:
        case = {"frames": np.zeros(64, dtype=np.uint8), "frames_len": 64, "offs": np.zeros(0, dtype=np.uint64),
                "stride": 0, "pkt_len": np.zeros(0, dtype=np.uint16)}
    case["sock"] = np.array([ck for ck, _ in segs], dtype=np.uint32)
    case["conn"] = conns(cs)
    case.update(kw)
    return case


def with_fault(rng, c, pos, what):
    """five in-order segments of 100 B, the one at @pos changed"""
    s = chain(rng, 0, c, [100] * 5)
    at = c["rcv_nxt"] + 100 * pos
    new = {"fin": lambda: seg(rng, 0, at, 100, flags=TCP_ACK | TCP_FIN),
           "rst": lambda: seg(rng, 0, at, 100, flags=TCP_RST),
           "urg": lambda: seg(rng, 0, at, 100, flags=TCP_ACK | TCP_URG),
           "len0": lambda: seg(rng, 0, at, 0),
           "ack_gt": lambda: seg(rng, 0, at, 100, ack=c["snd_nxt"] + 1),
           "seq_ne": lambda: seg(rng, 0, at + 1, 100),
           "too_long": lambda: seg(rng, 0, at, c["rcv_mss"] + 1)}[what]()
    s[pos] = new
    return s


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: the named cases of the issue"""
    rng = np.random.default_rng(91)
    c, res = conn1(), {}
    res["clean_chain"] = build([c], chain(rng, 0, c, [1, 100, 1460, 7, 536]))
    for pos in (0, 2):
        for what in ("fin", "rst", "urg", "len0", "ack_gt", "seq_ne", "too_long"):
            res[f"{what}_at{pos}"] = build([c], with_fault(rng, c, pos, what))
        # rcv_wnd < len: the window holds @pos segments and 99 bytes
        cw = conn1(rcv_wnd=100 * pos + 99)
        res[f"wnd_small_at{pos}"] = build([cw], chain(rng, 0, cw, [100] * 5))
    res["not_eligible"] = build([conn1(flags=0)], chain(rng, 0, c, [100] * 3))
    res["not_eligible_rxq"] = build([conn1(flags=RXQ | ACK_DELAYED)], chain(rng, 0, c, [100] * 3))
    cf = conn1(snd_una=1000, snd_wnd=4000)            # snd_una + snd_wnd == snd_nxt: full
    res["snd_full_at0"] = build([cf], chain(rng, 0, cf, [100] * 3))
    # full mid-chain: the second segment advertises a zero window
    s = chain(rng, 0, c, [100] * 5)
    s[1] = seg(rng, 0, c["rcv_nxt"] + 100, 100, ack=1000, win=0)
    res["snd_full_at2"] = build([c], s)
    # DROP before and after a stop
    s = [seg(rng, 0, 100, 1461), seg(rng, 0, 100, 100), seg(rng, 0, 777, 100), seg(rng, 0, 200, 1461),
         seg(rng, 0, 200, 100)]
    res["drop_before_and_after_stop"] = build([c], s)
    cw = conn1(rcv_wnd=300)
    res["rcv_wnd_exact"] = build([cw], chain(rng, 0, cw, [100, 200, 1]))
    cw = conn1(rcv_nxt=0xFFFFFF00, snd_una=0xFFFFFF00, snd_nxt=0x00000100, snd_wnd=0x300, snd_wl1=0xFFFFFEFF,
               snd_wl2=0xFFFFFF00)
    res["wrap_seq_and_snd"] = build([cw], chain(rng, 0, cw, [200, 100, 300], ack=0xFFFFFF80) +
                                    [seg(rng, 0, 0x00000158, 50, ack=0x00000100, win=7)])
    cw = conn1(snd_una=0xFFFFFF00, snd_nxt=0xFFFFFF80, snd_wnd=0x80)   # una + wnd wraps to exactly snd_nxt
    res["wrap_snd_full"] = build([cw], chain(rng, 0, cw, [100], ack=0xFFFFFF00))
    res["ack_eq_una"] = build([c], chain(rng, 0, c, [100, 100], ack=1000))
    res["ack_older"] = build([c], chain(rng, 0, c, [100, 100], ack=900))
    res["ack_eq_snd_nxt"] = build([c], chain(rng, 0, c, [100, 100], ack=5000))
    cw = conn1(snd_wl1=100)
    res["wl1_tie_wl2_lte"] = build([cw], chain(rng, 0, cw, [100, 100], ack=1000))
    res["wl1_tie_wl2_gt"] = build([conn1(snd_wl1=100, snd_wl2=1001)], chain(rng, 0, cw, [100, 100], ack=1000))
    for ws in (0, 14):
        cw = conn1(snd_wscale=ws)
        res[f"wscale{ws}"] = build([cw], chain(rng, 0, cw, [100, 100], win=0xFFFF))
    for cnt in (0, 1):
        for ad in (0, ACK_DELAYED):
            cw = conn1(acks_delayed_cnt=cnt, flags=ELIGIBLE | ad)
            res[f"delack_cnt{cnt}_ad{ad}"] = build([cw], chain(rng, 0, cw, [10, 20]))
    for psh in (0, TCP_PUSH):
        for rq in (0, RXQ):
            cw = conn1(flags=ELIGIBLE | rq)
            res[f"wake_psh{psh}_rxq{rq}"] = build([cw], chain(rng, 0, cw, [10], flags=TCP_ACK | psh) +
                                                  [seg(rng, 0, 110, 10)])
    res["syn_data_is_fast"] = build([c], chain(rng, 0, c, [100, 100], flags=TCP_ACK | TCP_SYN))
    c2 = conn1(rcv_nxt=50000, snd_una=7, snd_nxt=9, snd_wnd=100)
    a, b = chain(rng, 0, c, [100, 200, 300]), chain(rng, 1, c2, [5, 6, 7])
    res["two_interleaved"] = build([c, c2], [a[0], b[0], b[1], a[1], a[2], b[2]], align=16)
    res["cookie_ge_nconn"] = build([c], [seg(rng, 1, 100, 100), seg(rng, 0, 100, 100), seg(rng, pc.COOKIE_MAX, 200, 1),
                                         seg(rng, pc.S_MISS, 200, 1)])
    s = chain(rng, 0, c, [100, 100, 100])
    res["duplicate_order"] = build([c], s, order=np.array([0, 0, 1, 1, 2, 7, 0xFFFFFFFF, 2], dtype=np.uint32))
    res["m_zero"] = build([c, c2], [])
    res["nconn_one"] = build([c], chain(rng, 0, c, [1460] * 4))
    return res


def random_case(seed, m=4096, nconn=300, fault=0.05, align=0, udp=True, pays=None, flow=None):
    """A random stream of @m entries over @nconn connections; about one
    segment in twenty is a fault of some kind.  @flow(k) overrides the
    connection of entry k."""
    rng = np.random.default_rng(seed)
    cs = []
    for _ in range(nconn):
        una = int(rng.integers(0, 1 << 32))
        rn = int(rng.choice([int(rng.integers(0, 1 << 32)), 0xFFFFFFFF - int(rng.integers(0, 3000))]))
        cs.append(conn1(snd_una=una, snd_nxt=una + int(rng.integers(1, 50000)), snd_wnd=int(rng.integers(50000, 90000)),
                        snd_wl1=rn - int(rng.integers(0, 3)), snd_wl2=una - int(rng.integers(0, 3)), rcv_nxt=rn,
                        rcv_wnd=int(rng.choice([1 << 20, int(rng.integers(500, 20000))])),
                        rcv_mss=int(rng.choice([1460, 536])), snd_wscale=int(rng.integers(0, 15)),
                        flags=(ELIGIBLE if rng.random() < 0.97 else 0) | (RXQ if rng.random() < 0.3 else 0) |
                        (ACK_DELAYED if rng.random() < 0.3 else 0), acks_delayed_cnt=int(rng.integers(0, 2))))
    nxt = [c["rcv_nxt"] for c in cs]
    una = [c["snd_una"] for c in cs]
    segs, st = [], []
    for k in range(m):
        ck = int(rng.integers(0, nconn)) if flow is None else flow(k)
        c = cs[ck]
        ln = int(rng.integers(1, c["rcv_mss"] + 1)) if pays is None else pays
        left = (c["snd_nxt"] - una[ck]) & M32
        ack = una[ck] + int(rng.integers(0, min(left, 2000) + 1)) * int(rng.random() < 0.5)
        flags = TCP_ACK | (TCP_PUSH if rng.random() < 0.2 else 0) | (TCP_SYN if rng.random() < 0.01 else 0)
        s, status = None, lc.GOOD
        if rng.random() < fault:
            what = int(rng.integers(0, 12 if udp else 8))
            if what == 0:
                flags |= int(rng.choice([TCP_FIN, TCP_RST, TCP_URG]))
            elif what == 1:
                ln = 0
            elif what == 2:
                ack = c["snd_nxt"] + 1 + int(rng.integers(0, 100))
            elif what == 3:
                s = seg(rng, ck, nxt[ck] + int(rng.choice([-1, 1, 1460])), ln, ack=ack, flags=flags)
            elif what == 4:
                ln = c["rcv_mss"] + 1
            elif what == 5:
                ack = una[ck] - int(rng.integers(1, 1000))
            elif what == 8:
                s = (ck, pc.udp_frame(rng, ln))
            elif what == 9:
                s = seg(rng, nconn + int(rng.integers(0, 5)), nxt[ck], ln)
            elif what == 10:
                s = seg(rng, int(rng.choice([pc.S_MISS, pc.S_NA, pc.S_MULTI])), nxt[ck], ln)
            elif what == 11:
                status = lc.BAD
        if s is None:
            s = seg(rng, ck, nxt[ck], ln, ack=ack, flags=flags, win=int(rng.integers(0, 1 << 16)),
                    doff=int(rng.choice([5, 8])))
            if ln and ln <= c["rcv_mss"] and status == lc.GOOD:
                nxt[ck] = (nxt[ck] + ln) & M32      # the generator's guess: good enough to keep chains going
                if wraps_lt(una[ck], ack) and wraps_lte(ack, c["snd_nxt"]):
                    una[ck] = ack & M32
        segs.append(s)
        st.append(status)
    case = build(cs, segs, align=align)
    case["st"] = np.array(st, dtype=np.uint8)
    return case


def blank(m, nconn):
    """Every output buffer of a call filled with SENTINEL, GUARD entries longer than the call may write."""
    def arr(k, dt):
        return np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (k + GUARD)), dtype=dt).copy()
    b = {f: arr(m, dt) for f, dt in ENTRY}
    b["out_conn"], b["conn_off"] = arr(nconn, CONN_OUT), arr(nconn + 1, np.uint64)
    return b


def compare(got, want, m, nconn, what):
    """@got (blank() after a call) against @want: the written part equal byte for byte, the guard untouched"""
    for f, k in [(f, m) for f, _ in ENTRY] + [("out_conn", nconn), ("conn_off", nconn + 1)]:
        g = got[f]
        assert len(g) == k + GUARD and (g[k:].view(np.uint8) == SENTINEL).all(), f"{what}: {f} written past its end"
        bad = np.nonzero(g[:k].view(np.uint8) != want[f][:k].view(np.uint8))[0]
        if len(bad):
            e = bad[0] // g.dtype.itemsize
            raise AssertionError(f"{what}: {f}[{e}] = {g[e]} != {want[f][e]} ({len(bad)} bytes differ)")


def run_host(g, case, counts=True):
    """gcl_tcp_rx_host over sentinel-filled outputs: (outputs, counts)"""
    order = case.get("order")
    m, nconn = len(case["pkt_len"]) if order is None else len(order), len(case["conn"])
    out = blank(m, nconn)
    cnt = np.full(NR, 5, dtype=np.uint64) if counts else None
    g.tcp_rx_host(case["frames"], case["pkt_len"], case["sock"], case["conn"], stride=case["stride"],
                  offs=case["offs"], frames_len=case["frames_len"], order=order, m=m, l4_status=case.get("st"),
                  nconn=nconn, align=case.get("align", 0), blocks=case.get("blocks", 0), out=out, counts=cnt)
    return out, None if cnt is None else cnt - np.uint64(5)
