"""Cases and a model of gcl_tx_hdr (include/gclassify.h), written from the
rule's text and the reference's transmit path (runtime/net/udp.c:24-40,
tcp_out.c:54-81, core.c:504-538, 581-626, 686-737), not from the C;
tests/test_txpath_ref.py holds it to bytes the reference's own code produced.

A case is a dict: desc (TXH_DESC_DTYPE[m]), frame_off (u64[m]), frames_len,
net (a dict of txh_net()'s arguments), cap, shm_base, neigh (a list of (ip,
mac)), hash_bits (None, or the neighbour table's test knob).  The frame region
of a case is frames_len bytes between two guard bands of GUARD bytes, all
pre-filled with SENTINEL; model() returns the whole buffer as it must look
afterwards and every output array.
"""
import numpy as np

from caladan_amd import gclassify as G

SENTINEL = 0xA5
GUARD = 256
OUT_SENTINEL = {"cmd": 0xA5A5A5A5A5A5A5A5, "payload": 0x5A5A5A5A5A5A5A5A, "pkt_len": 0xA5A5,
                "tx_olflags": 0xA5, "hash": 0xA5A5A5A5, "status": 0xA5}
OUT_DTYPE = {"cmd": np.uint64, "payload": np.uint64, "pkt_len": np.uint16, "tx_olflags": np.uint8,
             "hash": np.uint32, "status": np.uint8}
OUT_GUARD = 8  # sentinel elements behind the m entries of every output array

LOOPBACK = 0x7F000001
ADDR, NETMASK, GATEWAY = 0x0A000005, 0xFFFFFF00, 0x0A000001
MAC = bytes([0x02, 0xCA, 0x1A, 0xDA, 0x00, 0x05])
RSS_KEY = G.CALADAN_RSS_KEY


def ip(a, b, c, d):
    return a << 24 | b << 16 | c << 8 | d


def mac_of(addr):
    """a remote neighbour's mac, made from its address"""
    return bytes([0x02, 0x11, addr >> 24 & 0xFF, addr >> 16 & 0xFF, addr >> 8 & 0xFF, addr & 0xFF])


def net(min_pkt_size=0, flags=0, netmask=NETMASK):
    return dict(addr=ADDR, netmask=netmask, gateway=GATEWAY, mac=MAC, min_pkt_size=min_pkt_size, flags=flags)


def descs(rows):
    """rows: dicts of gcl_txh_desc fields (missing ones 0)"""
    d = np.zeros(len(rows), dtype=G.TXH_DESC_DTYPE)
    for i, r in enumerate(rows):
        for f, v in r.items():
            d[f][i] = v
    return d


def case(name, rows, offs, frames_len, neigh, net_=None, cap=0, shm_base=0x100000000, hash_bits=None):
    return dict(name=name, desc=descs(rows) if not isinstance(rows, np.ndarray) else rows,
                frame_off=np.array(offs, dtype=np.uint64), frames_len=frames_len, neigh=neigh,
                net=net_ or net(), cap=cap, shm_base=shm_base, hash_bits=hash_bits)


def toeplitz(key, saddr, daddr, sport, dport):
    """do_toeplitz (runtime/net/core.c:120-139): for every set bit of the
    12-byte tuple, MSB first, the 32 key bits that start at that bit."""
    kbits = int.from_bytes(key, "big")
    nk = 8 * len(key)
    data = int.from_bytes(saddr.to_bytes(4, "big") + daddr.to_bytes(4, "big") + sport.to_bytes(2, "big") +
                          dport.to_bytes(2, "big"), "big")
    h = 0
    for i in range(96):
        if data >> (95 - i) & 1:
            h ^= kbits >> (nk - 32 - i) & 0xFFFFFFFF
    return h


def csum16(b):
    """the end-around-carry sum of @b's big-endian 16-bit words"""
    if len(b) & 1:
        b = b + b"\0"
    s = sum(int.from_bytes(b[i:i + 2], "big") for i in range(0, len(b), 2))
    while s >> 16:
        s = (s >> 16) + (s & 0xFFFF)
    return s


def model(c):
    m = len(c["desc"])
    n = c["net"]
    flen = c["frames_len"]
    buf = np.full(GUARD + flen + GUARD, SENTINEL, dtype=np.uint8)
    table = {a: bytes(mc) for a, mc in c["neigh"]}
    out = {f: np.zeros(m, dtype=dt) for f, dt in OUT_DTYPE.items()}
    counts = np.zeros(G.TXHC_NR, dtype=np.uint64)
    minp = n["min_pkt_size"]
    for j in range(m):
        d = c["desc"][j]
        o = int(c["frame_off"][j])
        proto, off, paylen = int(d["proto"]), int(d["tcp_off"]), int(d["paylen"])
        lip, rip, lport, rport = int(d["lip"]), int(d["rip"]), int(d["lport"]), int(d["rport"])
        tcp = proto == 6
        hl = 4 * off if tcp else 8
        tot = 20 + hl + paylen
        ln = 14 + tot
        elen = max(ln, minp)
        if proto not in (6, 17) or (tcp and not 5 <= off <= 15) or ln > 65535 or \
                (c["cap"] and elen > c["cap"]) or o > flen or elen > flen - o:
            out["status"][j] = G.TXH_REFUSED
            counts[G.TXHC_REFUSED] += 1
            continue
        f = buf[GUARD + o:GUARD + o + elen]
        saddr = lip if lip else (LOOPBACK if rip == LOOPBACK else n["addr"])
        if tcp:
            ph = saddr.to_bytes(4, "big") + rip.to_bytes(4, "big") + bytes([0, 6]) + (hl + paylen).to_bytes(2, "big")
            l4 = lport.to_bytes(2, "big") + rport.to_bytes(2, "big") + int(d["seq"]).to_bytes(4, "big") + \
                int(d["ack"]).to_bytes(4, "big") + bytes([off << 4 & 0xFF, int(d["tcp_flags"])]) + \
                int(d["win"]).to_bytes(2, "big") + csum16(ph).to_bytes(2, "big") + b"\0\0"
        else:
            l4 = lport.to_bytes(2, "big") + rport.to_bytes(2, "big") + (paylen + 8).to_bytes(2, "big") + b"\0\0"
        ecn = int(d["ecn"])
        iph = bytes([0x45, ecn & 3 if ecn & 0x80 else 0]) + tot.to_bytes(2, "big") + b"\0\0" + \
            (0x4000).to_bytes(2, "big") + bytes([64, proto]) + b"\0\0" + saddr.to_bytes(4, "big") + \
            rip.to_bytes(4, "big")
        if n["flags"] & G.TXH_IP_CSUM:
            iph = iph[:10] + (~csum16(iph) & 0xFFFF).to_bytes(2, "big") + iph[12:]
        f[14:34] = np.frombuffer(iph, dtype=np.uint8)
        f[34:34 + len(l4)] = np.frombuffer(l4, dtype=np.uint8)
        out["pkt_len"][j] = ln
        if rip == n["addr"] or rip == LOOPBACK:
            out["status"][j] = G.TXH_SELF
            counts[G.TXHC_SELF] += 1
            continue
        fl = G.OLFLAG_IP_CHKSUM | G.OLFLAG_IPV4 | (G.OLFLAG_TCP_CHKSUM if tcp else 0)
        nh = rip if (rip & n["netmask"]) == (n["addr"] & n["netmask"]) else n["gateway"]
        if nh not in table:
            out["status"][j] = G.TXH_NONEIGH
            out["tx_olflags"][j] = fl
            counts[G.TXHC_NONEIGH] += 1
            continue
        dmac = table[nh]
        f[0:14] = np.frombuffer(dmac + n["mac"] + b"\x08\x00", dtype=np.uint8)
        local = dmac == n["mac"]
        h = dst = 0
        if local:
            fl |= G.TXFLAG_LOCAL | G.TXFLAG_LOCAL_HINT
            h = toeplitz(RSS_KEY, n["addr"], nh, lport, rport)
            dst = nh
            counts[G.TXHC_LOCAL] += 1
        if ln < minp:
            f[ln:minp] = 0
        out["status"][j] = G.TXH_OK
        out["pkt_len"][j] = elen
        out["tx_olflags"][j] = fl
        out["hash"][j] = h
        out["cmd"][j] = dst | elen << 32 | fl << 48
        out["payload"][j] = (c["shm_base"] + o) | (h & 0xFFFF) << 48
        counts[G.TXHC_OK] += 1
        counts[G.TXHC_BYTES] += elen
    return dict(frames=buf, counts=counts, **out)


# --- the cases -------------------------------------------------------------

ON_LINK = [ip(10, 0, 0, 20 + i) for i in range(8)]
LOCAL_IP = ip(10, 0, 0, 77)   # another runtime on this machine: its arp entry carries our mac
OFF_LINK = ip(192, 168, 7, 9)
BASE_NEIGH = [(a, mac_of(a)) for a in ON_LINK] + [(LOCAL_IP, MAC), (GATEWAY, mac_of(GATEWAY))]


def _seg(i, proto, rip, paylen=5, off=5, lip=0, ecn=0):
    return dict(lip=lip, rip=rip, lport=1000 + i % 60000, rport=2000 + (7 * i) % 60000, proto=proto,
                tcp_flags=0x18 if i & 1 else 0x10, tcp_off=off, ecn=ecn, seq=0x01020304 + 977 * i,
                ack=0xF1E2D3C4 - 31 * i & 0xFFFFFFFF, win=0x1234 + i & 0xFFFF, paylen=paylen, pad=0xDEAD0000 + i)


def grid():
    rows, offs, i = [], [], 0
    pitch = 1600
    for proto, toffs in ((17, (5,)), (6, (5, 6, 15))):
        for off in toffs:
            for paylen in (0, 1, 5, 18, 1446):
                for al in range(16):
                    for has_ecn in (0, 1):
                        for lip in (0, ip(10, 0, 0, 6)):
                            rows.append(_seg(i, proto, ON_LINK[i % 7] if i % 9 else LOCAL_IP, paylen, off, lip,
                                             (0x80 | (1 + i % 3)) if has_ecn else i % 4))
                            offs.append(i * pitch + al)
                            i += 1
    return case("grid", rows, offs, i * pitch, BASE_NEIGH)


def route():
    rows, offs = [], []
    dests = [ON_LINK[0], OFF_LINK, ADDR, LOOPBACK, LOCAL_IP, ON_LINK[3], ip(10, 0, 0, 200)]  # the last: no entry
    for i, (proto, rip, lip) in enumerate((p, r, l) for p in (17, 6) for r in dests for l in (0, ip(10, 0, 0, 6))):
        rows.append(_seg(i, proto, rip, paylen=9 + i, lip=lip))
        offs.append(i * 96 + i % 5)
    out = [case("route", rows, offs, len(rows) * 96, BASE_NEIGH),
           # the gateway itself unresolved: every off-link segment is NONEIGH
           case("route_nogw", rows, offs, len(rows) * 96, BASE_NEIGH[:-1]),
           # the gateway is a runtime of this machine (its entry carries our mac)
           case("route_localgw", rows, offs, len(rows) * 96, BASE_NEIGH[:-1] + [(GATEWAY, MAC)]),
           case("route_empty", rows, offs, len(rows) * 96, []),
           case("route_ipcsum", rows, offs, len(rows) * 96, BASE_NEIGH, net(flags=G.TXH_IP_CSUM))]
    return out


def refuse():
    out = []
    ok = _seg(0, 17, ON_LINK[0], paylen=10)          # len 52
    tcp = _seg(1, 6, ON_LINK[1], paylen=10, off=6)   # len 68
    rows = [dict(ok, proto=1), dict(tcp, tcp_off=4), dict(tcp, tcp_off=0), dict(ok, paylen=65536 - 42),
            dict(ok, paylen=65535 - 42), ok, ok, ok, ok, dict(ok, paylen=48), dict(ok, paylen=49), tcp, ok]
    flen = 140000
    # the last frame that fits (len 90) and one a byte too long share the region's end
    offs = [0, 100, 200, 300, 70000, flen, flen + 1, 2 ** 64 - 1, 2 ** 63, flen - 90, flen - 90, 1000, 2000]
    out.append(case("refuse", rows, offs, flen, BASE_NEIGH))
    # cap: exceeded by one, met exactly
    out.append(case("refuse_cap", [ok, dict(ok, paylen=11), tcp], [0, 100, 200], 400, BASE_NEIGH, cap=52))
    # min_pkt_size pushes elen over the cap and over the region's end by one
    out.append(case("refuse_minpkt_cap", [ok, tcp], [0, 100], 400, BASE_NEIGH, net(min_pkt_size=60), cap=59))
    out.append(case("refuse_minpkt_cap_ok", [ok, tcp], [0, 100], 400, BASE_NEIGH, net(min_pkt_size=60), cap=60))
    out.append(case("refuse_minpkt_end", [ok, ok, dict(ok, rip=ADDR), dict(ok, rip=ADDR)],
                    [400 - 59, 400 - 60, 400 - 59, 200], 400, BASE_NEIGH, net(min_pkt_size=60)))
    return out


def pad():
    rows = [_seg(i, 17, ON_LINK[i % 8] if i % 4 else LOCAL_IP, paylen=i) for i in range(20)]        # len 42..61
    rows += [_seg(i, 6, ON_LINK[i % 8], paylen=i) for i in range(8)]                                 # len 54..61
    rows += [_seg(8, 6, ON_LINK[0], paylen=0, off=6), _seg(9, 17, ADDR, paylen=1),
             _seg(10, 17, ip(10, 0, 0, 200), paylen=1)]                                              # 58; SELF; NONEIGH
    offs = [i * 80 + (3 * i) % 16 for i in range(len(rows))]
    return [case("pad", rows, offs, len(rows) * 80, BASE_NEIGH, net(min_pkt_size=60)),
            case("pad255", rows, [i * 272 + i % 16 for i in range(len(rows))], len(rows) * 272, BASE_NEIGH,
                 net(min_pkt_size=255))]


def big_neigh(n=5000, seed=7):
    rng = np.random.default_rng(seed)
    ips = rng.choice(np.arange(ip(10, 0, 0, 0) + 256, ip(10, 0, 0, 0) + 65536, dtype=np.uint32), n, replace=False)
    return [(int(a), MAC if i % 5 == 0 else mac_of(int(a))) for i, a in enumerate(ips)] + \
        [(ip(10, 0, 0, 1), mac_of(ip(10, 0, 0, 1)))]


def big(hash_bits=None, m=20000, seed=11):
    rng = np.random.default_rng(seed)
    neigh = big_neigh()
    known = np.array([a for a, _ in neigh], dtype=np.uint32)
    pitch = 176
    d = np.zeros(m, dtype=G.TXH_DESC_DTYPE)
    kind = rng.integers(0, 10, m)
    d["rip"] = np.where(kind < 6, rng.choice(known, m),
                        np.where(kind == 6, rng.integers(ip(10, 0, 0, 0) + 256, ip(10, 0, 0, 0) + 65536, m),
                                 np.where(kind == 7, rng.integers(0, 2 ** 32, m),
                                          np.where(kind == 8, 0x0A000005, LOOPBACK))))
    d["lip"] = np.where(rng.integers(0, 2, m) == 0, 0, rng.integers(1, 2 ** 32, m))
    d["lport"] = rng.integers(0, 65536, m)
    d["rport"] = rng.integers(0, 65536, m)
    d["proto"] = rng.choice(np.array([6, 17, 6, 17, 6, 17, 6, 17, 6, 17, 6, 17, 6, 17, 6, 17, 6, 17, 1, 0]), m)
    d["tcp_flags"] = rng.integers(0, 256, m)
    d["tcp_off"] = rng.choice(np.array([5, 5, 5, 6, 8, 10, 15, 15, 4, 0, 3]), m)
    d["ecn"] = rng.integers(0, 256, m)
    d["seq"] = rng.integers(0, 2 ** 32, m)
    d["ack"] = rng.integers(0, 2 ** 32, m)
    d["win"] = rng.integers(0, 65536, m)
    d["paylen"] = np.where(rng.integers(0, 50, m) == 0, rng.integers(0, 65536, m), rng.integers(0, 60, m))
    d["pad"] = rng.integers(0, 2 ** 32, m)
    offs = np.arange(m, dtype=np.uint64) * pitch + rng.integers(0, 16, m).astype(np.uint64)
    wild = rng.integers(0, 100, m) == 0
    offs = np.where(wild, rng.integers(0, 2 ** 64, m, dtype=np.uint64), offs)
    # an entry that lands inside another's slot would make the result depend on
    # the order of two lanes: a wild offset is kept only outside the region
    flen = m * pitch
    offs = np.where(wild & (offs < flen), offs + np.uint64(flen), offs)
    # an mtu-sized frame would run over its neighbours: large paylens go to wild offsets or get cut
    bigp = (d["paylen"] > 60) & ~wild
    d["paylen"] = np.where(bigp & (np.arange(m) % 2 == 0), d["paylen"] % 60, d["paylen"])
    offs = np.where((d["paylen"] > 60) & ~wild, np.uint64(flen - 40), offs)  # refused: does not fit
    return case("big" if hash_bits is None else f"big_bits{hash_bits}", d, offs, flen, neigh,
                net(min_pkt_size=60, netmask=0xFFFF0000), cap=1514, hash_bits=hash_bits)


BIG_HASH_BITS = 14  # 5001 entries in 8192 buckets: most buckets are shared, and the set still places


def small_cases():
    return [grid()] + route() + refuse() + pad()


_CACHE = {}


def all_cases():
    """every case, built once (a test must not change one: copy first)"""
    if "all" not in _CACHE:
        _CACHE["all"] = small_cases() + [big(), big(BIG_HASH_BITS)]
    return _CACHE["all"]


def models():
    """name -> (case, model(case)), computed once and shared"""
    if "models" not in _CACHE:
        _CACHE["models"] = {c["name"]: (c, model(c)) for c in all_cases()}
    return _CACHE["models"]


CASE_NAMES = ["grid", "route", "route_nogw", "route_localgw", "route_empty", "route_ipcsum", "refuse",
              "refuse_cap", "refuse_minpkt_cap", "refuse_minpkt_cap_ok", "refuse_minpkt_end", "pad", "pad255",
              "big", f"big_bits{BIG_HASH_BITS}"]
