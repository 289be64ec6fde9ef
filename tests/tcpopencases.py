"""What the CPU and GPU tests of gcl_tcp_rx_open (include/gclassify.h) share:
a frame builder, an independent Python model of the rule (written from the
rule's text and the reference's tcp_parse_options, not from csrc/gcl_tcpopen.h),
hand-derived cases with the verdicts written out, random lists, and
sentinel-filled outputs with guards."""
import struct

import numpy as np

M32 = 0xFFFFFFFF
(NA, OOR, SHORT, CLOSED_DROP, CLOSED_RST, CLOSED_RST_ACK, LATER, FULL, DROP, RST, BADOPT, ACCEPT) = range(12)
NR_VERDICTS, C_SEGS, C_SEGSKIP, C_NOSPACE, C_NR = 12, 12, 13, 14, 16
K_RST, K_RST_ACK, K_SYNACK = 2, 3, 4
MISS, SOCK_NA, MULTI = 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFD
FIN, SYN, TRST, PSH, TACK = 0x01, 0x02, 0x04, 0x08, 0x10
OPT_MSS, OPT_WSCALE = 1, 2
SHUTDOWN = 1
NONE = M32
SENTINEL, GUARD = 0xA5, 8
STRIDE, TX_STRIDE, TX_BASE = 128, 64, 192
LISTEN_BASE = 1000

LISTEN = np.dtype([("backlog", "<u4"), ("winmax", "<u4"), ("rcv_mss", "<u2"), ("rcv_wscale", "u1"),
                   ("flags", "u1"), ("pad", "<u4")])
OPEN = np.dtype([("src", "<u4"), ("listener", "<u4"), ("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"),
                 ("rport", "<u2"), ("irs", "<u4"), ("rcv_nxt", "<u4"), ("iss", "<u4"), ("snd_una", "<u4"),
                 ("snd_nxt", "<u4"), ("rcv_wnd", "<u4"), ("winmax", "<u4"), ("snd_mss", "<u2"),
                 ("snd_wscale", "u1"), ("rcv_wscale", "u1"), ("opt_en", "u1"), ("state", "u1"),
                 ("pad", "u1", (10,))])
DESC = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"), ("proto", "u1"),
                 ("tcp_flags", "u1"), ("tcp_off", "u1"), ("ecn", "u1"), ("seq", "<u4"), ("ack", "<u4"),
                 ("win", "<u2"), ("paylen", "<u2"), ("pad", "<u4")])
ENTRY = (("verdict", np.uint8), ("later_of", np.uint32), ("rst_seq", np.uint32))
SEG = (("desc", DESC), ("frame_off", np.uint64), ("seg_conn", np.uint32), ("seg_kind", np.uint8),
       ("seg_src", np.uint32))

LIP, RIP = 0x0A000001, 0x0A000002


def frame(flags, seq=1000, ack=0, opts=b"", payload=b"", off=None, tot=None, lip=LIP, lport=80, rip=RIP,
          rport=40000, proto=6, ethertype=0x0800, vihl=0x45, frag=0):
    """an Ethernet + IPv4 + TCP frame; @off and @tot override what the lengths would give"""
    off = 5 + len(opts) // 4 if off is None else off
    tcp = struct.pack(">HHIIBBHHH", rport, lport, seq & M32, ack & M32, off << 4, flags, 0xFFFF, 0, 0) + opts + payload
    tot = 20 + len(tcp) if tot is None else tot
    ip = struct.pack(">BBHHHBBHII", vihl, 0, tot, 0, frag, 64, proto, 0, rip, lip)
    return b"\x02" * 6 + b"\x04" * 6 + struct.pack(">H", ethertype) + ip + tcp


def listener(backlog=8, winmax=1 << 20, rcv_mss=1460, rcv_wscale=5, flags=0):
    return (backlog, winmax, rcv_mss, rcv_wscale, flags, 0)


def case(pkts, listen=(), order=None, seg_cap=None, open_cap=None, tx_len=None, l4_status=None, hash_slots=0,
         pkt_len=None, stride=STRIDE, lead=0, iss=None):
    """arrays of a call: @pkts is a list of (frame bytes, cookie); frames lie @stride apart behind @lead bytes"""
    n = len(pkts)
    frames = np.zeros(lead + n * stride + 16, dtype=np.uint8)
    plen = np.zeros(max(n, 1), dtype=np.uint16)
    for i, (f, _) in enumerate(pkts):
        assert len(f) <= stride
        frames[lead + i * stride:lead + i * stride + len(f)] = np.frombuffer(f, dtype=np.uint8)
        plen[i] = len(f)
    if pkt_len is not None:
        plen[:n] = pkt_len
    m = n if order is None else len(order)
    segs = m if seg_cap is None else seg_cap
    c = dict(frames=frames, offs=np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(lead), n=n,
             pkt_len=plen, sock=np.array([s for _, s in pkts] + [0] * (n == 0), dtype=np.uint32),
             listen=np.array(list(listen), dtype=LISTEN) if len(listen) else np.zeros(0, dtype=LISTEN),
             order=None if order is None else np.array(order, dtype=np.uint32), m=m,
             iss=np.array(iss if iss is not None else [(0x10000 * (j + 1) + 7) & M32 for j in range(m)] + [0] * (m == 0),
                          dtype=np.uint32),
             seg_cap=segs, open_cap=m if open_cap is None else open_cap,
             tx_len=TX_BASE + segs * TX_STRIDE if tx_len is None else tx_len, hash_slots=hash_slots,
             l4_status=None if l4_status is None else np.array(l4_status, dtype=np.uint8))
    return c


# ---- the model ----

def parse_options(o):
    """tcp_parse_options as written, a read past the end reading 0; returns (opt_en, mss, wscale) or None for the
    input the reference does not return from"""
    rd = lambda p: o[p] if p < len(o) else 0
    ln, p, en, mss, ws = len(o), 0, 0, 0, 0
    while ln > 0:
        opcode = rd(p)
        p += 1
        if opcode == 0:
            break
        if opcode == 1:
            ln -= 1
            continue
        opsize = rd(p)
        p += 1
        if opsize == 0:
            return None
        if opcode == 2 and opsize == 4:
            mss, en = rd(p) << 8 | rd(p + 1), en | OPT_MSS
        elif opcode == 3 and opsize == 3:
            ws, en = min(rd(p), 14), en | OPT_WSCALE
        p += opsize - 2
        ln -= opsize
    return en, mss, ws


def model(c):
    """the rule of gclassify.h over the arrays of @c, entry by entry in list order"""
    fr, flen = c["frames"], len(c["frames"])
    m, lb, nl = c["m"], LISTEN_BASE, len(c["listen"])
    run = [int(x["backlog"]) for x in c["listen"]]
    accepted = {}
    verdict, later_of, rst_seq, opens, segs, optb = [], [], [], [], [], {}
    for j in range(m):
        i = j if c["order"] is None else int(c["order"][j])
        v, lat, rs = None, NONE, 0
        if i >= c["n"]:
            v = OOR
        else:
            o = min(int(c["offs"][i]), flen)
            L = min(int(c["pkt_len"][i]), flen - o)
            B = lambda k: int(fr[o + k]) if o + k < flen else 0
            sk = int(c["sock"][i])
            lis = sk <= 0xFFFFFFEF and lb <= sk < lb + nl
            tot = B(16) << 8 | B(17)
            if not (sk == MISS or lis):
                v = NA
            elif L < 34 or (B(12), B(13), B(14)) != (8, 0, 0x45) or ((B(20) << 8 | B(21)) & 0x3FFF) or B(23) != 6 \
                    or tot < 20 or 14 + tot > L:
                v = NA
            elif c["l4_status"] is not None and (int(c["l4_status"][i]) & 0xF) == 2:
                v = NA
            elif tot - 20 < 20 or L < 54:
                v = SHORT
            else:
                be = lambda k, w: int.from_bytes(bytes(B(k + x) for x in range(w)), "big")
                seq, ack, off, fl = be(38, 4), be(42, 4), B(46) >> 4, B(47)
                tup = (be(30, 4), be(36, 2), be(26, 4), be(34, 2))
                if sk == MISS:
                    if fl & TRST:
                        v = CLOSED_DROP
                    elif fl & TACK:
                        v, rs = CLOSED_RST, ack
                    else:
                        v, rs = CLOSED_RST_ACK, (seq + tot - 20 - 4 * off) & M32
                else:
                    li = sk - lb
                    q = c["listen"][li]
                    if (tup, li) in accepted:
                        v, lat = LATER, accepted[(tup, li)]
                    elif (int(q["flags"]) & SHUTDOWN) or run[li] == 0:
                        v = FULL
                    elif fl & TRST:
                        v = DROP
                    elif fl & TACK:
                        v, rs = RST, ack
                    elif not fl & SYN or tot - 20 != 4 * off or 34 + 4 * off > L:
                        v = DROP
                    else:
                        po = parse_options([B(54 + x) for x in range(4 * off - 20)])
                        if po is None:
                            v = BADOPT
                        else:
                            v = ACCEPT
                            en, mss, ws = po
                            winmax, rws = int(q["winmax"]), int(q["rcv_wscale"])
                            snd_mss = min(max(mss, 88), int(q["rcv_mss"])) if en & OPT_MSS else 1460
                            if not en & OPT_WSCALE:
                                winmax, rws = min(winmax, 65535), 0
                            iss = int(c["iss"][j])
                            rec = dict(src=j, listener=li, lip=tup[0], rip=tup[2], lport=tup[1], rport=tup[3],
                                       irs=seq, rcv_nxt=(seq + 1) & M32, iss=iss, snd_una=iss,
                                       snd_nxt=(iss + 1) & M32, rcv_wnd=winmax, winmax=winmax, snd_mss=snd_mss,
                                       snd_wscale=ws, rcv_wscale=rws, opt_en=en, state=1)
                            run[li] -= 1
                            accepted[(tup, li)] = j
                            ob = ([1, 3, 3, rws] if en & OPT_WSCALE else []) + \
                                 ([2, 4, int(q["rcv_mss"]) >> 8, int(q["rcv_mss"]) & 0xFF] if en & OPT_MSS else [])
                            segs.append(dict(src=j, kind=K_SYNACK, conn=len(opens), lip=tup[0], rip=tup[2],
                                             lport=tup[1], rport=tup[3], flags=0x12, off=5 + len(ob) // 4, seq=iss,
                                             ack=(seq + 1) & M32, win=(winmax >> (rws & 31)) & 0xFFFF, opts=ob))
                            opens.append(rec)
                if v in (RST, CLOSED_RST, CLOSED_RST_ACK):
                    ra = v == CLOSED_RST_ACK
                    segs.append(dict(src=j, kind=K_RST_ACK if ra else K_RST, conn=NONE, lip=tup[0], rip=tup[2],
                                     lport=tup[1], rport=tup[3], flags=0x14 if ra else 0x04, off=5,
                                     seq=0 if ra else rs, ack=rs if ra else 0, win=0, opts=[]))
        verdict.append(v)
        later_of.append(lat)
        rst_seq.append(rs if v in (RST, CLOSED_RST, CLOSED_RST_ACK) else 0)
    fb, st, txl = TX_BASE, TX_STRIDE, c["tx_len"]
    lim = min(c["seg_cap"], (txl - fb) // st if fb <= txl else 0)
    counts = [verdict.count(x) for x in range(NR_VERDICTS)] + [0] * 4
    counts[C_SEGS], counts[C_SEGSKIP] = min(len(segs), lim), len(segs) - min(len(segs), lim)
    counts[C_NOSPACE] = max(0, len(opens) - c["open_cap"])
    return dict(verdict=verdict, later_of=later_of, rst_seq=rst_seq, opens=opens, segs=segs, backlog_out=run,
                lim=lim, counts=counts)


# ---- outputs ----

def blank(c):
    m, sc, oc, nl = c["m"], c["seg_cap"], c["open_cap"], len(c["listen"])
    fill = lambda dt, k: np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (k + GUARD)), dtype=dt).copy()
    out = {f: fill(dt, m) for f, dt in ENTRY}
    out.update({f: fill(dt, sc) for f, dt in SEG})
    out.update(open=fill(OPEN, oc), backlog_out=fill(np.uint32, nl), totals=fill(np.uint64, 2),
               seg_totals=fill(np.uint64, 2))
    # the tx region with a guard on either side; tx() is the region itself
    out["tx_all"] = np.full(c["tx_len"] + 2 * 64, SENTINEL, dtype=np.uint8)
    return out


def tx(out):
    return out["tx_all"][64:len(out["tx_all"]) - 64]


def run_host(g, c, counts=True, **kw):
    out = blank(c)
    cnt = np.full(C_NR, 5, dtype=np.uint64) if counts else None
    t = tx(out)
    res = {k: v for k, v in out.items() if k != "tx_all"}
    res.update(kw.pop("out", {}))
    args = dict(offs=c["offs"], n=c["n"], order=c["order"], m=c["m"], l4_status=c["l4_status"],
                listen_base=LISTEN_BASE, frame_stride=TX_STRIDE, frame_base=TX_BASE, tx_frames_len=c["tx_len"],
                hash_slots=c["hash_slots"], out=res, counts=cnt)
    args.update(kw)
    g.tcp_rx_open_host(c["frames"], c["pkt_len"], c["sock"], c["listen"], c["iss"], c["seg_cap"], c["open_cap"], t,
                       **args)
    return out, None if cnt is None else (cnt - np.uint64(5)).tolist()


def check_model(c, out, counts, what):
    """every output of a call against the model; everything the call must not write still holds the sentinel"""
    w = model(c)
    m, nl = c["m"], len(c["listen"])
    for f in ("verdict", "later_of", "rst_seq"):
        assert out[f][:m].tolist() == w[f], (what, f, out[f][:m].tolist(), w[f])
        assert (out[f][m:].view(np.uint8) == SENTINEL).all(), (what, f, "guard")
    assert out["backlog_out"][:nl].tolist() == w["backlog_out"], (what, "backlog_out")
    assert (out["backlog_out"][nl:].view(np.uint8) == SENTINEL).all(), (what, "backlog guard")
    nopen, wrote = len(w["opens"]), min(len(w["opens"]), c["open_cap"])
    assert out["totals"][:2].tolist() == [nopen, wrote], (what, "totals")
    for k in range(wrote):
        r = out["open"][k]
        for f, val in w["opens"][k].items():
            assert int(r[f]) == val, (what, "open", k, f, int(r[f]), val)
        assert not r["pad"].any(), (what, "open pad")
    assert (out["open"][wrote:].view(np.uint8) == SENTINEL).all(), (what, "open guard")
    nseg, swrote = len(w["segs"]), min(len(w["segs"]), w["lim"])
    assert out["seg_totals"][:2].tolist() == [nseg, swrote], (what, "seg totals", out["seg_totals"][:2], nseg, swrote)
    t = tx(out)
    want_tx = np.full(len(t), SENTINEL, dtype=np.uint8)
    for k in range(swrote):
        s, d = w["segs"][k], out["desc"][k]
        got = (int(out["seg_src"][k]), int(out["seg_kind"][k]), int(out["seg_conn"][k]), int(d["lip"]), int(d["rip"]),
               int(d["lport"]), int(d["rport"]), int(d["tcp_flags"]), int(d["tcp_off"]), int(d["seq"]),
               int(d["ack"]), int(d["win"]))
        assert got == (s["src"], s["kind"], s["conn"], s["lip"], s["rip"], s["lport"], s["rport"], s["flags"],
                       s["off"], s["seq"], s["ack"], s["win"]), (what, "segment", k, got, s)
        assert (int(d["proto"]), int(d["ecn"]), int(d["paylen"]), int(d["pad"])) == (6, 0, 0, 0), (what, k)
        fo = TX_BASE + k * TX_STRIDE
        assert int(out["frame_off"][k]) == fo, (what, "frame_off", k)
        want_tx[fo + 54:fo + 54 + len(s["opts"])] = s["opts"]
    for f, _ in SEG:
        assert (out[f][swrote:].view(np.uint8) == SENTINEL).all(), (what, f, "guard")
    assert t.tobytes() == want_tx.tobytes(), (what, "tx region")
    assert (out["tx_all"][:64] == SENTINEL).all() and (out["tx_all"][-64:] == SENTINEL).all(), (what, "tx guard")
    for f in ("totals", "seg_totals"):
        assert (out[f][2:].view(np.uint8) == SENTINEL).all(), (what, f, "guard")
    if counts is not None:
        assert counts == w["counts"], (what, "counts", counts, w["counts"])
        assert sum(counts[:NR_VERDICTS]) == m, (what, "verdict counters")
    return w


def same(a, b, what):
    """two runs of one case: every byte of every output"""
    for f in a:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


# ---- hand-derived cases: name -> (case, the verdicts, written out by hand) ----

L0, L1 = LISTEN_BASE, LISTEN_BASE + 1
MSS = bytes([2, 4, 0x05, 0xB4])                 # 1460
MSS536 = bytes([2, 4, 0x02, 0x18])
WS7 = bytes([3, 3, 7])
NOP = b"\x01"

# option shapes: name -> (option bytes, (opt_en, snd_mss, snd_wscale) of the ACCEPT against rcv_mss 1460, or None
# for BADOPT); derived by walking tcp_parse_options by hand
OPTION_SHAPES = {
    "none": (b"", (0, 1460, 0)),
    "mss": (MSS536, (OPT_MSS, 536, 0)),
    "mss_small": (bytes([2, 4, 0, 20]), (OPT_MSS, 88, 0)),          # max(20, 88)
    "mss_big": (bytes([2, 4, 0xFF, 0xFF]), (OPT_MSS, 1460, 0)),     # min(65535, rcv_mss)
    "wscale": (NOP + WS7, (OPT_WSCALE, 1460, 7)),
    "mss_wscale": (MSS536 + NOP + WS7, (3, 536, 7)),
    "wscale_mss": (NOP + WS7 + MSS536, (3, 536, 7)),
    "nop_pad": (NOP * 4 + MSS536, (OPT_MSS, 536, 0)),
    "eol_first": (b"\x00" + WS7, (0, 1460, 0)),                     # EOL stops the walk before WSCALE
    "mss_len3": (bytes([2, 3, 9, 1]), (0, 1460, 0)),                # wrong length: skipped by 3, then a NOP
    "wscale_len4": (bytes([3, 4, 7, 0]), (0, 1460, 0)),
    "wscale_15": (NOP + bytes([3, 3, 15]), (OPT_WSCALE, 1460, 14)),
    "mss_twice": (MSS536 + MSS, (OPT_MSS, 1460, 0)),                # the last one wins
    "wscale_twice": (NOP + WS7 + NOP + bytes([3, 3, 2]), (OPT_WSCALE, 1460, 2)),
    # kind 8 with length 1: ptr steps back onto the 1, which reads as a NOP; then 02 04 .. does not fit: kind 2 at
    # byte 2, length 4 at byte 3, value bytes past the end read 0 -> MSS 0 -> 88
    "unknown_len1": (bytes([8, 1, 2, 4]), (OPT_MSS, 88, 0)),
    "unknown_len1_then_mss": (bytes([8, 1, 1, 1]) + MSS536, (OPT_MSS, 536, 0)),
    "unknown_past_end": (bytes([8, 200, 0, 0]) + MSS536, (0, 1460, 0)),   # len goes negative: MSS never seen
    "unknown_len2": (bytes([8, 2, 1, 1]) + MSS536, (OPT_MSS, 536, 0)),
    "mss_cut": (NOP * 2 + bytes([2, 4]), (OPT_MSS, 88, 0)),         # value bytes past the end read 0
    "sack_ts_mss": (bytes([4, 2, 8, 10] + [0] * 8) + MSS536, (OPT_MSS, 536, 0)),
    "forty": (NOP * 33 + MSS536 + WS7, (3, 536, 7)),
    "len0": (bytes([8, 0, 0, 0]), None),
    "len0_after_mss": (MSS536 + bytes([9, 0, 1, 1]), None),
    "opcode_last": (NOP * 3 + bytes([8]), None),                    # its length byte lies past the end: reads 0
    "mss_len0": (bytes([2, 0, 5, 0xB4]), None),
}


def syn(opts=b"", **kw):
    return frame(SYN, opts=opts, **kw)


def hand_cases():
    lq = [listener(), listener(backlog=1, winmax=40000, rcv_wscale=0)]
    H = {}
    H["miss"] = (case([(frame(TRST), MISS), (frame(TACK, ack=777), MISS), (frame(TRST | TACK, ack=5), MISS),
                       (frame(SYN, seq=100), MISS), (frame(0, seq=100), MISS)], lq),
                 [CLOSED_DROP, CLOSED_RST, CLOSED_DROP, CLOSED_RST_ACK, CLOSED_RST_ACK])
    # RST_ACK length arithmetic: options are subtracted, SYN and FIN not counted, off * 4 > tot - 20 wraps
    H["miss_len"] = (case([(frame(SYN, seq=100, opts=MSS, payload=b"abc"), MISS),
                           (frame(SYN | FIN, seq=M32, payload=b"xy"), MISS),
                           (frame(FIN, seq=10, off=15), MISS),
                           (frame(0, seq=10, off=0, payload=b"q" * 7), MISS),
                           (frame(SYN, seq=1, lip=7, rip=9), MISS), (frame(SYN, seq=1, lip=7, rip=9), MISS)], lq),
                     [CLOSED_RST_ACK] * 6)
    H["na"] = (case([(syn(), SOCK_NA), (syn(), 5), (syn(), MULTI), (syn(), L0 + 2), (syn(), L0 - 1),
                     (syn(proto=17), L0), (syn(ethertype=0x86DD), MISS), (syn(vihl=0x46), L0), (syn(frag=0x2000), L0),
                     (syn(frag=0x0001), MISS), (syn(frag=0x4000), L0), (syn(tot=200), L0), (syn(tot=19), MISS),
                     (syn(), L0), (syn(rport=40001), L0)], lq, l4_status=[1] * 13 + [2, 0]),
               [NA] * 10 + [ACCEPT, NA, NA, NA, ACCEPT])
    H["short"] = (case([(syn(tot=39), MISS), (syn(tot=39), L0), (syn(tot=20), L0), (syn(tot=40), MISS),
                        (syn(tot=40), L0)], lq, pkt_len=[54, 54, 34, 54, 53]),
                  [SHORT, SHORT, SHORT, CLOSED_RST_ACK, NA])
    H["listener"] = (case([(frame(TRST), L0), (frame(TACK, ack=4242), L0), (frame(SYN | TACK, ack=1), L0),
                           (frame(0), L0), (frame(FIN), L0), (syn(payload=b"data"), L0), (syn(off=4), L0),
                           (syn(off=6), L0), (syn(opts=MSS, off=5), L0), (syn(opts=MSS + NOP * 4, tot=44), L0),
                           (syn(rport=1), L0)], lq),
                     [DROP, RST, RST, DROP, DROP, DROP, DROP, DROP, DROP, DROP, ACCEPT])
    # a full listener is silent: the ACK gets no RST; shutdown the same
    H["full"] = (case([(syn(rport=1), L1), (syn(rport=2), L1), (syn(rport=3), L1), (frame(TACK, rport=4), L1),
                       (frame(TRST, rport=5), L1), (syn(rport=2), L1), (syn(rport=1), L1),
                       (frame(TACK, rport=1, ack=9), L1), (syn(rport=6), L0)],
                      [listener(), listener(backlog=1)]),
                 [ACCEPT, FULL, FULL, FULL, FULL, FULL, LATER, LATER, ACCEPT])
    H["shutdown"] = (case([(syn(), L0), (frame(TACK), L0), (syn(opts=bytes([8, 0, 0, 0])), L0), (syn(), L1)],
                          [listener(flags=SHUTDOWN), listener()]), [FULL, FULL, FULL, ACCEPT])
    H["backlog0"] = (case([(syn(), L0), (frame(TACK), L0)], [listener(backlog=0)]), [FULL, FULL])
    # a rejected packet gives its slot back: backlog 1 still takes the SYN behind them
    H["gives_back"] = (case([(frame(TRST), L1), (frame(TACK), L1), (syn(opts=bytes([8, 0, 0, 0])), L1),
                             (syn(payload=b"x"), L1), (syn(), L1), (syn(rport=9), L1)], lq),
                       [DROP, RST, BADOPT, DROP, ACCEPT, FULL])
    # LATER: any packet of an accepted tuple, before or after the listener fills; not one that comes before it
    H["later"] = (case([(frame(TACK, ack=3), L0), (syn(), L0), (frame(TACK, ack=3), L0), (frame(TRST), L0),
                        (syn(seq=5), L0), (syn(lport=81), L0), (frame(FIN | TACK, lport=81), L0),
                        (syn(), MISS), (syn(), MISS)], lq),
                  [RST, ACCEPT, LATER, LATER, LATER, ACCEPT, LATER, CLOSED_RST_ACK, CLOSED_RST_ACK])
    # the BADOPT SYN opens nothing, so the SYN behind it is the tuple's ACCEPT
    H["badopt_then_syn"] = (case([(syn(opts=bytes([8, 0, 0, 0])), L0), (syn(), L0), (syn(opts=bytes([8, 0, 0, 0])), L0)],
                                 lq), [BADOPT, ACCEPT, LATER])
    H["order"] = (case([(syn(rport=1), L1), (syn(rport=2), L1), (frame(TACK, ack=8), MISS)], lq,
                       order=[2, 1, 7, 0, 1, 2]), [CLOSED_RST, ACCEPT, OOR, FULL, LATER, CLOSED_RST])
    for name, (ob, res) in OPTION_SHAPES.items():
        H["opt_" + name] = (case([(syn(opts=ob), L0), (syn(opts=ob, rport=2), L1)], lq),
                            [BADOPT, BADOPT] if res is None else [ACCEPT, ACCEPT])
    # the caps: records, segments and the tx region too small
    many = [(syn(rport=1 + x), L0) for x in range(4)] + [(frame(TACK, ack=1), MISS), (syn(rport=50), L0)]
    allv = [ACCEPT] * 4 + [CLOSED_RST, ACCEPT]
    H["open_cap"] = (case(many, lq, open_cap=2), allv)
    H["open_cap0"] = (case(many, lq, open_cap=0), allv)
    H["seg_cap"] = (case(many, lq, seg_cap=3), allv)
    H["seg_cap0"] = (case(many, lq, seg_cap=0), allv)
    H["tx_len"] = (case(many, lq, tx_len=TX_BASE + 2 * TX_STRIDE + TX_STRIDE - 1), allv)
    H["tx_len_short"] = (case(many, lq, tx_len=TX_BASE - 1), allv)
    H["tx_len0"] = (case(many, lq, tx_len=0), allv)
    # the table at its minimum (2 * m slots), so that probes collide: 32 tuples, each twice
    col = [(syn(rport=1 + x % 32, rip=RIP + x % 32 % 3), L0) for x in range(64)]
    H["hash_min"] = (case(col, [listener(backlog=40)], hash_slots=128),
                     [ACCEPT] * 32 + [LATER] * 32)
    H["empty_listen"] = (case([(syn(), LISTEN_BASE), (syn(), MISS)], []), [NA, CLOSED_RST_ACK])
    return H


def random_case(seed, m, nlisten=5, n=None, with_order=True, lead=0, hash_slots=0, backlog=None, caps=False):
    """a list with every route: few tuples, so that duplicates, the backlog and LATER all happen"""
    rng = np.random.default_rng(seed)
    n = m if n is None else n
    shapes = list(OPTION_SHAPES.values())
    ntup = max(2, m // 3)
    pkts = []
    for i in range(n):
        r = rng.integers(0, 100)
        li = int(rng.integers(0, nlisten))
        t = int(rng.integers(0, ntup))
        kw = dict(rport=1024 + t % 50000, rip=RIP + t // 50000, lport=80 + li % 7, seq=int(rng.integers(0, 1 << 32)),
                  ack=int(rng.integers(0, 1 << 32)))
        if r < 55:
            f = syn(opts=shapes[int(rng.integers(0, len(shapes)))][0], **kw)
        elif r < 65:
            f = frame(int(rng.integers(0, 64)), **kw)
        elif r < 75:
            f = frame(TACK, **kw)
        elif r < 80:
            f = syn(payload=b"z" * int(rng.integers(1, 9)), **kw)
        elif r < 85:
            f = syn(off=int(rng.integers(0, 16)), **kw)
        elif r < 90:
            f = syn(tot=int(rng.integers(18, 70)), **kw)
        else:
            f = bytes(rng.integers(0, 256, size=int(rng.integers(0, 100)), dtype=np.uint8))
        s = int(rng.integers(0, 100))
        sock = LISTEN_BASE + li if s < 70 else MISS if s < 90 else int(rng.choice([SOCK_NA, MULTI, 3, LISTEN_BASE + nlisten]))
        pkts.append((f, sock))
    lq = [listener(backlog=int(rng.integers(0, 3 + m // (4 * nlisten))) if backlog is None else backlog, winmax=int(rng.choice([1000, 65535, 1 << 20])),
                   rcv_mss=int(rng.choice([1460, 536, 8960])), rcv_wscale=int(rng.integers(0, 15)),
                   flags=int(rng.integers(0, 8) == 0)) for _ in range(nlisten)]
    order = rng.integers(0, n + 2, size=m).tolist() if with_order else None
    if not with_order:
        assert n == m
    kw = {}
    if caps:
        kw = dict(seg_cap=int(rng.integers(0, m + 1)), open_cap=int(rng.integers(0, m // 2 + 1)))
    c = case(pkts, lq, order=order, lead=lead, hash_slots=hash_slots,
             l4_status=rng.choice([0, 1, 1, 1, 2], size=n).tolist() if seed % 2 else None, **kw)
    c["pkt_len"][:n] = np.minimum(c["pkt_len"][:n], rng.integers(0, 400, size=n)) if seed % 3 == 0 else c["pkt_len"][:n]
    return c


# ---- the chain: gcl_tcp_rx_open -> gcl_tx_hdr -> gcl_l4_csum FILL ----

MAC_L, MAC_R = bytes([2, 0, 0, 0, 0, 1]), bytes([2, 0, 0, 0, 0, 2])


def chain_case():
    """a SYN with both options, a SYN with none, an ACK for a closed port and an ACK for a listener"""
    lq = [listener(), listener()]
    return case([(syn(opts=MSS536 + NOP + WS7, seq=7000), L0), (syn(rport=5, seq=M32), L1),
                 (frame(TACK, ack=99, rport=6), MISS), (frame(TACK, ack=98, rport=7), L0)], lq)


def net_of(g):
    return g.txh_net(LIP, 0xFFFFFF00, LIP & 0xFFFFFF00 | 254, MAC_L)


def host_chain(g, c):
    """the host twins in chain order over the tx region of sentinel-filled outputs; returns (outputs of the open
    call, outputs of gcl_tx_hdr_host, the FILL status)"""
    out, _ = run_host(g, c)
    k = int(out["seg_totals"][1])
    tbl = g.NeighTable()
    tbl.set([(RIP, MAC_R)])
    t = tx(out)
    hdr = g.tx_hdr_host(out["desc"][:max(k, 1)], out["frame_off"][:max(k, 1)], t, net_of(g), table=tbl, m=k)
    st = g.l4_csum_host(t, hdr["pkt_len"], mode=g.L4_FILL, offs=out["frame_off"], n=k,
                        tx_olflags=hdr["tx_olflags"])
    tbl.close()
    return out, hdr, st
