"""What the CPU and GPU tests of gcl_udp_rx (include/gclassify.h) share: a
frame builder, an independent Python model written from udp_conn_recv and
udp_par_recv (runtime/net/udp.c:79-107 and :811-840) as a per-packet queue
simulation (every socket a Python list that datagrams are pushed onto; neither
the closed form of csrc/gcl_udprx.h nor the C), hand-derived cases with their
outputs written out, random lists, and sentinel-filled outputs with guards."""
import struct

import numpy as np

QUEUED, SPAWN, FULL, CLOSED, NOSOCK, NA = range(6)
NR_VERDICTS, C_BYTES, C_POLLINS, C_NR = 6, 6, 7, 8
POLLIN = 1
SHUTDOWN, ERR, SPAWNER = 1, 2, 4
MISS, SOCK_NA, MULTI, COOKIE_MAX = 0xFFFFFFFE, 0xFFFFFFFF, 0xFFFFFFFD, 0xFFFFFFEF
NONE = 0xFFFFFFFF
SENTINEL, GUARD = 0xA5, 8
STRIDE = 128
SOCK_BASE = 500
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

USOCK = np.dtype([("inq_len", "<i4"), ("inq_cap", "<i4"), ("flags", "u1"), ("pad", "u1", (7,))])
USOCK_OUT = np.dtype([("inq_len", "<i4"), ("ntaken", "<u4"), ("ndropped", "<u4"), ("flags", "u1"),
                      ("pad", "u1", (3,))])
REC = np.dtype([("dst_off", "<u8"), ("rip", "<u4"), ("rport", "<u2"), ("len", "<u2")])
ENTRY = (("verdict", np.uint8), ("sflags", np.uint8), ("copy_len", np.uint16), ("dst_off", np.uint64),
         ("rec_idx", np.uint32))

LIP, RIP = 0x0A000001, 0x0A000002


def frame(payload=b"", tot=None, lip=LIP, lport=53, rip=RIP, rport=40000, proto=17, ethertype=0x0800, vihl=0x45,
          frag=0):
    """an Ethernet + IPv4 + UDP frame; @tot overrides what the lengths would give"""
    if isinstance(payload, int):
        payload = bytes((7 * x + payload) & 0xFF for x in range(payload))
    udp = struct.pack(">HHHH", rport, lport, 8 + len(payload), 0) + payload
    tot = 20 + len(udp) if tot is None else tot
    ip = struct.pack(">BBHHHBBHII", vihl, 0, tot, 0, frag, 64, proto, 0, rip, lip)
    return b"\x02" * 6 + b"\x04" * 6 + struct.pack(">H", ethertype) + ip + udp


def tcp_frame():
    tcp = struct.pack(">HHIIBBHHH", 40000, 80, 1, 2, 5 << 4, 0x10, 0xFFFF, 0, 0) + b"tcp!"
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(tcp), 0, 0, 64, 6, 0, RIP, LIP)
    return b"\x02" * 6 + b"\x04" * 6 + struct.pack(">H", 0x0800) + ip + tcp


def usock(inq_len=0, inq_cap=128, flags=0):
    return (inq_len, inq_cap, flags, [0] * 7)


def case(pkts, socks=(), order=None, l4_status=None, pkt_len=None, stride=STRIDE, lead=0, align=0,
         sock_base=SOCK_BASE):
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
    return dict(frames=frames, offs=np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(lead), n=n,
                pkt_len=plen, sock=np.array([s for _, s in pkts] + [0] * (n == 0), dtype=np.uint32),
                usock=np.array(list(socks), dtype=USOCK) if len(socks) else np.zeros(0, dtype=USOCK),
                order=None if order is None else np.array(order, dtype=np.uint32),
                m=n if order is None else len(order), align=align, sock_base=sock_base,
                l4_status=None if l4_status is None else np.array(l4_status, dtype=np.uint8))


# ---- the model: the reference's two functions, one packet at a time ----

def pad(x, align):
    return x if align <= 1 else (x + align - 1) // align * align


def model(c):
    fr, flen = c["frames"], len(c["frames"])
    m, base, ns, align = c["m"], c["sock_base"], len(c["usock"]), c["align"]
    # the runtime's sockets: an ingress queue each, and the words udp_conn_recv looks at
    socks = [dict(inq=[], inq_len=int(u["inq_len"]), inq_cap=int(u["inq_cap"]),
                  inq_err=bool(int(u["flags"]) & ERR), shutdown=bool(int(u["flags"]) & SHUTDOWN),
                  spawner=bool(int(u["flags"]) & SPAWNER), dropped=0, pollin=False) for u in c["usock"]]
    verdict, sflags = [], []
    for j in range(m):
        i = j if c["order"] is None else int(c["order"][j])
        v, sf = NA, 0
        if i < c["n"]:
            o = min(int(c["offs"][i]), flen)
            L = min(int(c["pkt_len"][i]), flen - o)
            B = lambda k: int(fr[o + k]) if o + k < flen else 0
            tot = B(16) << 8 | B(17)
            sk = int(c["sock"][i])
            # what net_rx_trans hands to a UDP socket's recv: an unfragmented IPv4/UDP packet whose checksum
            # held and whose lookup found a socket; mbuf_pull_hdr_or_null needs the 8 bytes of a UDP header
            is_udp = L >= 34 and (B(12), B(13), B(14)) == (8, 0, 0x45) and not ((B(20) << 8 | B(21)) & 0x3FFF) \
                and B(23) == 17 and tot >= 28 and 14 + tot <= L
            bad = c["l4_status"] is not None and (int(c["l4_status"][i]) & 0xF) == 2
            if is_udp and not bad and sk <= COOKIE_MAX:
                if not base <= sk < base + ns:
                    v = NOSOCK
                else:
                    s = socks[sk - base]
                    dg = dict(j=j, len=tot - 28, rip=int.from_bytes(bytes(B(26 + x) for x in range(4)), "big"),
                              rport=B(34) << 8 | B(35))
                    if s["spawner"]:                      # udp_par_recv
                        s["inq"].append(dg)
                        v = SPAWN
                    elif s["inq_len"] >= s["inq_cap"] or s["inq_err"] or s["shutdown"]:
                        s["dropped"] += 1
                        v = CLOSED if s["inq_err"] or s["shutdown"] else FULL
                    else:
                        s["inq"].append(dg)
                        if s["inq_len"] == 0:
                            sf, s["pollin"] = POLLIN, True
                        s["inq_len"] += 1
                        v = QUEUED
        verdict.append(v)
        sflags.append(sf)
    # the layout: every socket's queue as one run, the sockets in turn
    copy_len, dst_off, rec_idx = [0] * m, [0] * m, [NONE] * m
    recs, rec_off, sock_off, at = [], [], [], 0
    for s in socks:
        rec_off.append(len(recs))
        sock_off.append(at)
        for dg in s["inq"]:
            copy_len[dg["j"]], dst_off[dg["j"]], rec_idx[dg["j"]] = dg["len"], at, len(recs)
            recs.append((at, dg["rip"], dg["rport"], dg["len"]))
            at += pad(dg["len"], align)
    rec_off.append(len(recs))
    sock_off.append(at)
    counts = [verdict.count(x) for x in range(NR_VERDICTS)] + [sum(copy_len), sum(sflags)]
    out_sock = [(s["inq_len"], len(s["inq"]), s["dropped"], POLLIN if s["pollin"] else 0) for s in socks]
    return dict(verdict=verdict, sflags=sflags, copy_len=copy_len, dst_off=dst_off, rec_idx=rec_idx, recs=recs,
                out_sock=out_sock, rec_off=rec_off, sock_off=sock_off, counts=counts)


# ---- outputs ----

def blank(c):
    m, ns = c["m"], len(c["usock"])
    fill = lambda dt, k: np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (k + GUARD)), dtype=dt).copy()
    out = {f: fill(dt, m) for f, dt in ENTRY}
    out.update(rec=fill(REC, m), out_sock=fill(USOCK_OUT, ns), rec_off=fill(np.uint32, ns + 1),
               sock_off=fill(np.uint64, ns + 1))
    return out


def run_host(g, c, counts=True, **kw):
    out = blank(c)
    given = isinstance(counts, np.ndarray)   # a caller's own array is accumulated into and not returned
    cnt = counts if given else np.full(C_NR, 5, dtype=np.uint64) if counts else None
    args = dict(offs=c["offs"], n=c["n"], order=c["order"], m=c["m"], l4_status=c["l4_status"],
                nsock=len(c["usock"]), sock_base=c["sock_base"], align=c["align"], out=out, counts=cnt)
    args.update(kw)
    g.udp_rx_host(c["frames"], c["pkt_len"], c["sock"], c["usock"], **args)
    return out, None if cnt is None or given else (cnt - np.uint64(5)).tolist()


def check_model(c, out, counts, what):
    """every output of a call against the model; everything the call must not write still holds the sentinel"""
    w = model(c)
    m, ns = c["m"], len(c["usock"])
    for f, _ in ENTRY:
        assert out[f][:m].tolist() == w[f], (what, f, out[f][:m].tolist(), w[f])
        assert (out[f][m:].view(np.uint8) == SENTINEL).all(), (what, f, "guard")
    nrec = len(w["recs"])
    got = [(int(r["dst_off"]), int(r["rip"]), int(r["rport"]), int(r["len"])) for r in out["rec"][:nrec]]
    assert got == w["recs"], (what, "rec", got, w["recs"])
    assert (out["rec"][nrec:].view(np.uint8) == SENTINEL).all(), (what, "records past rec_off[nsock]")
    got = [(int(r["inq_len"]), int(r["ntaken"]), int(r["ndropped"]), int(r["flags"])) for r in out["out_sock"][:ns]]
    assert got == w["out_sock"], (what, "out_sock", got, w["out_sock"])
    assert not out["out_sock"][:ns]["pad"].any(), (what, "out_sock pad")
    assert (out["out_sock"][ns:].view(np.uint8) == SENTINEL).all(), (what, "out_sock guard")
    for f in ("rec_off", "sock_off"):
        assert out[f][:ns + 1].tolist() == w[f], (what, f, out[f][:ns + 1].tolist(), w[f])
        assert (out[f][ns + 1:].view(np.uint8) == SENTINEL).all(), (what, f, "guard")
    if counts is not None:
        assert counts == w["counts"], (what, "counts", counts, w["counts"])
        assert sum(counts[:NR_VERDICTS]) == m, (what, "verdict counters")
    return w


def same(a, b, what):
    """two runs of one case: every byte of every output"""
    for f in a:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


# ---- hand-derived cases: name -> (case, the outputs written out by hand) ----

S0, S1, S2, S3 = SOCK_BASE, SOCK_BASE + 1, SOCK_BASE + 2, SOCK_BASE + 3
Q, SP, FU, CL, NS = QUEUED, SPAWN, FULL, CLOSED, NOSOCK


def hand_cases():
    H = {}
    dg = lambda s, n=4, **kw: (frame(n, **kw), s)
    # a socket that enters full; inq_cap below inq_len; both negative
    H["enters_full"] = (case([dg(S0), dg(S0), dg(S1), dg(S2), dg(S2)],
                             [usock(4, 4), usock(5, 3), usock(-2, -5)]),
                        dict(verdict=[FU] * 5, sflags=[0] * 5, copy_len=[0] * 5, dst_off=[0] * 5, rec_idx=[NONE] * 5,
                             out_sock=[(4, 0, 2, 0), (5, 0, 1, 0), (-2, 0, 2, 0)], rec_off=[0, 0, 0, 0],
                             sock_off=[0, 0, 0, 0]))
    # negative words with room: -3 -> -2 -> -1 == cap; and -1 -> 0 -> 1 -> 2 == cap, POLLIN on the one that finds 0
    H["negative_room"] = (case([dg(S0), dg(S1), dg(S0), dg(S1), dg(S0), dg(S1), dg(S1)],
                               [usock(-3, -1), usock(-1, 2)]),
                          dict(verdict=[Q, Q, Q, Q, FU, Q, FU], sflags=[0, 0, 0, POLLIN, 0, 0, 0],
                               copy_len=[4, 4, 4, 4, 0, 4, 0], dst_off=[0, 8, 4, 12, 0, 16, 0],
                               rec_idx=[0, 2, 1, 3, NONE, 4, NONE], out_sock=[(-1, 2, 1, 0), (2, 3, 1, POLLIN)],
                               rec_off=[0, 2, 5], sock_off=[0, 8, 20]))
    # the words at the ends of int: nothing overflows
    H["int_extremes"] = (case([dg(S0), dg(S1), dg(S0), dg(S1), dg(S2), dg(S2)],
                              [usock(I32_MIN, I32_MAX), usock(I32_MAX, I32_MIN), usock(I32_MAX - 1, I32_MAX)]),
                         dict(verdict=[Q, FU, Q, FU, Q, FU], out_sock=[(I32_MIN + 2, 2, 0, 0), (I32_MAX, 0, 2, 0),
                                                                       (I32_MAX, 1, 1, 0)]))
    # room for exactly 3 of 4; inq_len != 0 so no POLLIN
    H["room_k_of_k1"] = (case([dg(S0, 1), dg(S0, 2), dg(S0, 3), dg(S0, 4)], [usock(1, 4)]),
                         dict(verdict=[Q, Q, Q, FU], sflags=[0] * 4, copy_len=[1, 2, 3, 0], dst_off=[0, 1, 3, 0],
                              rec_idx=[0, 1, 2, NONE], out_sock=[(4, 3, 1, 0)], rec_off=[0, 3], sock_off=[0, 6]))
    # inq_len == 0: POLLIN on the first only
    H["pollin_first"] = (case([dg(S0), dg(S0), dg(S0)], [usock(0, 8)]),
                         dict(verdict=[Q, Q, Q], sflags=[POLLIN, 0, 0], out_sock=[(3, 3, 0, POLLIN)]))
    # ERR, SHUTDOWN, both; a spawner takes everything, ERR and a cap of 0 notwithstanding
    H["flags"] = (case([dg(S0), dg(S1), dg(S2), dg(S3), dg(S3), dg(S0)],
                       [usock(0, 8, ERR), usock(0, 8, SHUTDOWN), usock(0, 8, ERR | SHUTDOWN),
                        usock(0, 0, SPAWNER | ERR)]),
                  dict(verdict=[CL, CL, CL, SP, SP, CL], sflags=[0] * 6, copy_len=[0, 0, 0, 4, 4, 0],
                       dst_off=[0, 0, 0, 0, 4, 0], rec_idx=[NONE, NONE, NONE, 0, 1, NONE],
                       out_sock=[(0, 0, 2, 0), (0, 0, 1, 0), (0, 0, 1, 0), (0, 2, 0, 0)], rec_off=[0, 0, 0, 0, 2],
                       sock_off=[0, 0, 0, 0, 8]))
    H["spawner_plain"] = (case([dg(S0, 9), dg(S0, 0)], [usock(7, 7, SPAWNER)]),
                          dict(verdict=[SP, SP], copy_len=[9, 0], dst_off=[0, 9], out_sock=[(7, 2, 0, 0)]))
    # a zero-length datagram is a datagram: it takes the slot the third one then lacks
    H["zero_len"] = (case([dg(S0, 0), dg(S0, 5), dg(S0, 3)], [usock(0, 2)]),
                     dict(verdict=[Q, Q, FU], sflags=[POLLIN, 0, 0], copy_len=[0, 5, 0], dst_off=[0, 0, 0],
                          rec_idx=[0, 1, NONE], out_sock=[(2, 2, 1, POLLIN)], rec_off=[0, 2], sock_off=[0, 5]))
    # tot 27: no room for a UDP header (mbuf_pull_hdr_or_null); tot 28: a datagram of length 0
    H["tot_27_28"] = (case([(frame(b"", tot=27), S0), (frame(b"", tot=28), S0), (frame(b"xyz", tot=28), S0)],
                           [usock(3, 9)]),
                      dict(verdict=[NA, Q, Q], copy_len=[0, 0, 0], out_sock=[(5, 2, 0, 0)]))
    # what is no datagram: TCP, a bad checksum, the lookup's three words, IPv6, options, fragments, a cut frame
    H["not_datagrams"] = (case([(tcp_frame(), S0), dg(S0), dg(MISS), dg(MULTI), dg(SOCK_NA), dg(COOKIE_MAX + 1),
                                dg(S0, ethertype=0x86DD), dg(S0, vihl=0x46), dg(S0, frag=0x2000), dg(S0, frag=1),
                                dg(S0, frag=0x4000), dg(S0, tot=200), dg(S0, proto=1), dg(S0)],
                               [usock(0, 8)], l4_status=[1, 2] + [1] * 11 + [0x11]),
                          dict(verdict=[NA] * 10 + [Q, NA, NA, Q], sflags=[0] * 10 + [POLLIN, 0, 0, 0],
                               out_sock=[(2, 2, 0, POLLIN)]))
    # cookies just outside [sock_base, sock_base + nsock)
    H["nosock"] = (case([dg(S0 - 1), dg(S0), dg(S1), dg(S2), dg(0), dg(COOKIE_MAX)], [usock(), usock()]),
                   dict(verdict=[NS, Q, Q, NS, NS, NS], rec_idx=[NONE, 0, 1, NONE, NONE, NONE],
                        out_sock=[(1, 1, 0, POLLIN), (1, 1, 0, POLLIN)], rec_off=[0, 1, 2], sock_off=[0, 4, 8]))
    H["base_zero"] = (case([dg(0), dg(1), dg(2)], [usock(), usock()], sock_base=0),
                      dict(verdict=[Q, Q, NS]))
    # order with duplicates and out-of-range values: packet 1 arrives three times
    H["order"] = (case([dg(S0, 2), dg(S1, 3), dg(S0, 6)], [usock(0, 2), usock(0, 2)], order=[1, 2, 1, 9, 0, 1, 2, 3]),
                  dict(verdict=[Q, Q, Q, NA, Q, FU, FU, NA], sflags=[POLLIN, POLLIN, 0, 0, 0, 0, 0, 0],
                       copy_len=[3, 6, 3, 0, 2, 0, 0, 0], dst_off=[8, 0, 11, 0, 6, 0, 0, 0],
                       rec_idx=[2, 0, 3, NONE, 1, NONE, NONE, NONE],
                       out_sock=[(2, 2, 1, POLLIN), (2, 2, 1, POLLIN)], rec_off=[0, 2, 4], sock_off=[0, 8, 14]))
    # align 64: every taken datagram starts on a 64-B boundary, a zero-length one takes no room
    H["align64"] = (case([dg(S1, 65), dg(S0, 1), dg(S1, 0), dg(S0, 64), dg(S1, 7)], [usock(), usock()], align=64),
                    dict(verdict=[Q] * 5, copy_len=[65, 1, 0, 64, 7], dst_off=[128, 0, 256, 64, 256],
                         rec_idx=[2, 0, 3, 1, 4], rec_off=[0, 2, 5], sock_off=[0, 128, 320]))
    H["nsock0"] = (case([dg(S0), dg(MISS), (tcp_frame(), S0)], []),
                   dict(verdict=[NS, NA, NA], rec_off=[0], sock_off=[0]))
    H["m0"] = (case([], [usock(3, 9), usock(0, 0, ERR)]),
               dict(verdict=[], out_sock=[(3, 0, 0, 0), (0, 0, 0, 0)], rec_off=[0, 0, 0], sock_off=[0, 0, 0]))
    H["m0_nsock0"] = (case([], []), dict(verdict=[], rec_off=[0], sock_off=[0]))
    return H


def check_hand(c, want, out, what):
    m, ns = c["m"], len(c["usock"])
    for f, v in want.items():
        if f == "out_sock":
            got = [(int(r["inq_len"]), int(r["ntaken"]), int(r["ndropped"]), int(r["flags"]))
                   for r in out["out_sock"][:ns]]
        else:
            got = out[f][:ns + 1 if f in ("rec_off", "sock_off") else m].tolist()
        assert got == v, (what, f, got, v)


def random_case(seed, m, nsock=5, n=None, with_order=True, lead=0, align=None, sock_base=SOCK_BASE, caps=None):
    """a list with every verdict: few sockets with little room, so that queues fill inside the list"""
    rng = np.random.default_rng(seed)
    n = m if n is None else n
    pkts = []
    for i in range(n):
        r = int(rng.integers(0, 100))
        kw = dict(rport=1024 + int(rng.integers(0, 60000)), rip=RIP + int(rng.integers(0, 1000)))
        if r < 80:
            f = frame(int(rng.integers(0, 70)) if r < 70 else 0, **kw)
        elif r < 84:
            f = tcp_frame()
        elif r < 90:
            f = frame(int(rng.integers(0, 20)), tot=int(rng.integers(20, 60)), **kw)
        else:
            f = bytes(rng.integers(0, 256, size=int(rng.integers(0, 100)), dtype=np.uint8))
        s = int(rng.integers(0, 100))
        sock = sock_base + int(rng.integers(0, max(nsock, 1))) if s < 85 else \
            int(rng.choice([MISS, SOCK_NA, MULTI, sock_base + nsock, max(sock_base, 1) - 1, 3]))
        pkts.append((f, sock))
    socks = []
    per = m // max(nsock, 1)
    for s in range(nsock):
        kind = (s + seed) % 5 if s < 5 else int(rng.integers(0, 5))
        ln = int(rng.choice([0, 0, 1, 7, -2]))
        if caps is not None:
            socks.append(usock(ln, ln + caps))
        elif kind == 0:       # room for about a third of what arrives
            socks.append(usock(ln, ln + per // 3 + int(rng.integers(0, 3))))
        elif kind == 1:       # room for everything, from empty
            socks.append(usock(0, m + 1))
        elif kind == 2:
            socks.append(usock(ln, int(rng.integers(-3, 4)), SPAWNER | int(rng.integers(0, 4))))
        elif kind == 3:
            socks.append(usock(ln, ln + m, int(rng.integers(1, 4))))
        else:                 # enters full, or with inq_cap below inq_len
            socks.append(usock(ln, ln - int(rng.integers(0, 3))))
    order = rng.integers(0, n + 2, size=m).tolist() if with_order else None
    if not with_order:
        assert n == m
    c = case(pkts, socks, order=order, lead=lead, sock_base=sock_base,
             align=int(rng.choice([0, 1, 4, 64, 256])) if align is None else align,
             l4_status=rng.choice([0, 1, 1, 1, 2], size=n).tolist() if seed % 2 else None)
    if seed % 3 == 0:
        c["pkt_len"][:n] = np.minimum(c["pkt_len"][:n], rng.integers(0, 400, size=n))
    return c


# ---- the chain: gcl_l4_payload -> gcl_udp_rx -> gcl_copy_batch ----

def chain_case(seed=77, m=300, nsock=4):
    """datagrams with distinct payload bytes, so that a region's content names the datagrams in it"""
    rng = np.random.default_rng(seed)
    pkts = []
    for i in range(m):
        ln = int(rng.integers(0, 60))
        pay = bytes((i * 31 + x * 7 + 1) & 0xFF for x in range(ln))
        pkts.append((frame(pay, rport=2000 + i), SOCK_BASE + int(rng.integers(0, nsock + 1))))
    socks = [usock(0, 40), usock(2, 30), usock(0, 0, SPAWNER), usock(0, 100, ERR)][:nsock]
    return case(pkts, socks, align=16)


def host_chain(g, c):
    """the host twins in chain order; returns (udp_rx_host's outputs, the destination region)"""
    pay = g.l4_payload_host(c["frames"], c["pkt_len"], offs=c["offs"], n=c["n"], order=c["order"], m=c["m"],
                            sock=c["sock"], l4_status=c["l4_status"], align=c["align"])
    out, _ = run_host(g, c)
    total = int(out["sock_off"][len(c["usock"])])
    dst = np.full(total + 64, SENTINEL, dtype=np.uint8)
    g.copy_batch_host(c["frames"], pay["src_off"], out["copy_len"][:max(c["m"], 1)], dst,
                      dst_off=out["dst_off"][:max(c["m"], 1)], n=c["m"], olflags=False, rss=False)
    return out, dst, pay
