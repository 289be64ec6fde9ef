"""Test-side definition of the socket demux (gcl_sock_lookup,
gcl_sock_tbl_lookup_host), restated from trans_lookup
(runtime/net/transport.c:341-397) and include/gclassify.h in plain Python and
numpy, and the entry sets, traffic and verdicts its tests share.

The definition keeps two dicts per runtime: its 5-tuple entries keyed by
(proto, lip, lport, rip, rport) and its 3-tuple entries keyed by (proto, lip,
lport), a key given twice holding MULTI.  A packet of runtime u that passes
the frame predicate is looked up in u's 5-tuple dict, then in its 3-tuple
dict by laddr, then by (0, laddr.port); the first answer counts."""
import numpy as np

NA, MISS, MULTI, COOKIE_MAX = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFEF
HIT5, HIT3, HIT3_ANY, N_MULTI, N_MISS, N_NA, NR = 0, 1, 2, 3, 4, 5, 8
M3, M5 = 3, 5
HDR = 64  # bytes of a built frame
ENTRY = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"),
                  ("proto", "u1"), ("match", "u1"), ("pad", "<u2"), ("cookie", "<u4")])
SHARED_IP = 0x0A0000FE  # an address every runtime of random_sets also listens on


def runtime_ip(u):
    return 0x0A000000 + u + 1


# ------------------------------------------------------------------ definition
def make_tables(sets):
    """{uniqid: (dict5, dict3)} of {uniqid: ENTRY array}."""
    tables = {}
    for u, ents in sets.items():
        d5, d3 = {}, {}
        for e in ents:
            if e["match"] == M5:
                k = (int(e["proto"]), int(e["lip"]), int(e["lport"]), int(e["rip"]), int(e["rport"]))
                assert k not in d5, "duplicate 5-tuple: gcl_sock_set refuses the set"
                d5[k] = int(e["cookie"])
            else:
                k = (int(e["proto"]), int(e["lip"]), int(e["lport"]))
                d3[k] = MULTI if k in d3 else int(e["cookie"])  # transport.c:392-396
        tables[int(u)] = (d5, d3)
    return tables


def lookup_one(tables, u, proto, lip, lport, rip, rport):
    """(sock, counter slot) of transport.c:370-396 for runtime @u."""
    d5, d3 = tables.get(u, ({}, {}))
    c = d5.get((proto, lip, lport, rip, rport))       # :371-381
    if c is not None:
        return c, HIT5
    c = d3.get((proto, lip, lport))                   # :384
    if c is not None:
        return c, (N_MULTI if c == MULTI else HIT3)
    c = d3.get((proto, 0, lport))                     # :386-387
    if c is not None:
        return c, (N_MULTI if c == MULTI else HIT3_ANY)
    return MISS, N_MISS                               # :388-389


def verdict_runtime(raw, vbytes, thread_bits, max_runtimes):
    """The runtime each verdict delivers to, -1 where it names none
    (gcl_verdict2_to4 / gcl_verdict1_to4 for the narrow forms)."""
    raw = np.asarray(raw, dtype=np.uint64)
    if vbytes in (8, 4):
        w = (raw >> np.uint64(32)) if vbytes == 8 else raw
        act = (w >> np.uint64(24)) & np.uint64(0x3F)
        ok = act <= 1
        u = w & np.uint64(0xFFFF)
    elif vbytes == 2:
        kind = raw & np.uint64(0xC000)
        ok = (kind == 0) | (kind == 0x4000)
        u = (raw & np.uint64(0x3FFF)) >> np.uint64(thread_bits)
    else:
        ok = (raw & np.uint64(0x80)) == 0
        u = (raw & np.uint64(0x7F)) >> np.uint64(thread_bits)
    ok &= u < max_runtimes
    return np.where(ok, u.astype(np.int64), -1)


def header_bytes(region, frames_len, offs):
    """Frame bytes [12, 38) of the frames at @offs in the first @frames_len
    bytes of @region, zero-padded: u8[n, 26]."""
    region = np.asarray(region, dtype=np.uint8)[:frames_len]
    pad = np.concatenate([region, np.zeros(HDR, dtype=np.uint8)])
    o = np.minimum(np.asarray(offs, dtype=np.uint64), np.uint64(frames_len)).astype(np.int64)
    return pad[o[:, None] + np.arange(12, 38)[None, :]]


def expected(tables, region, frames_len, offs, raw, vbytes, thread_bits, max_runtimes):
    """(sock u32[n], counts u64[NR]) of the definition."""
    n = len(offs)
    sock = np.full(n, NA, dtype=np.uint32)
    counts = np.zeros(NR, dtype=np.uint64)
    if n == 0:
        return sock, counts
    u = verdict_runtime(raw, vbytes, thread_bits, max_runtimes)
    h = header_bytes(region, frames_len, offs).astype(np.int64)
    b = lambda i: h[:, i - 12]  # noqa: E731  frame byte i
    proto = b(23)
    seen = (u >= 0) & (b(12) == 0x08) & (b(13) == 0x00) & (b(14) == 0x45) & ((b(21) & 0x20) == 0) & \
        ((proto == 6) | (proto == 17))
    rip = b(26) << 24 | b(27) << 16 | b(28) << 8 | b(29)
    lip = b(30) << 24 | b(31) << 16 | b(32) << 8 | b(33)
    rport = b(34) << 8 | b(35)
    lport = b(36) << 8 | b(37)
    idx = np.nonzero(seen)[0]
    keys = np.stack([u[idx], proto[idx], lip[idx], lport[idx], rip[idx], rport[idx]], axis=1)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    res = [lookup_one(tables, *(int(x) for x in row)) for row in uniq]
    ans = np.array([r[0] for r in res], dtype=np.uint32).reshape(-1)
    kls = np.array([r[1] for r in res], dtype=np.int64).reshape(-1)
    inv = np.asarray(inv).reshape(-1)
    sock[idx] = ans[inv]
    counts[:N_NA + 1] = np.bincount(kls[inv], minlength=N_NA + 1).astype(np.uint64)
    counts[N_NA] = n - len(idx)
    return sock, counts


# ------------------------------------------------------------------ entry sets
def random_sets(rng, uniqids, per_rt):
    """{uniqid: ENTRY array of about @per_rt entries}: listeners on the
    runtime's own address, on SHARED_IP and on address 0 (the same ports in
    every runtime, with different cookies), reuse_port listeners (the same
    3-tuple two or three times), and connections: most to a listener's laddr,
    so a 5-tuple shadows a 3-tuple.  5-tuple keys are unique."""
    sets = {}
    for u in uniqids:
        ip = runtime_ip(u)
        nl = max(2, per_rt // 4)
        nc = max(1, per_rt - nl)
        e = np.zeros(nl + nc, dtype=ENTRY)
        lis, con = e[:nl], e[nl:]
        lis["match"] = M3
        lis["lip"] = rng.choice([ip, ip, SHARED_IP, 0], size=nl)
        lis["lport"] = 1 + (np.arange(nl) * 7 + rng.integers(0, 3, size=nl)) % 65535
        lis["proto"] = rng.choice([6, 17], size=nl)
        lis["rip"], lis["rport"] = rng.integers(0, 2**32, size=nl), rng.integers(0, 65536, size=nl)  # ignored
        dup = rng.random(nl) < 0.15  # reuse_port: a copy of the listener before it
        dup[0] = False
        for i in np.nonzero(dup)[0]:
            for f in ("lip", "lport", "proto"):
                lis[f][i] = lis[f][i - 1]
        src = rng.integers(0, nl, size=nc)
        con["match"] = M5
        con["lip"] = np.where(lis["lip"][src] == 0, ip, lis["lip"][src])
        con["lport"] = lis["lport"][src]
        con["proto"] = lis["proto"][src]
        fresh = rng.random(nc) < 0.2  # a connection with no listener behind it
        con["lport"] = np.where(fresh, rng.integers(1, 65536, size=nc), con["lport"])
        con["rip"] = 0xC0A80000 + rng.integers(0, 4096, size=nc)
        con["rport"] = rng.integers(1, 65536, size=nc)
        _, first = np.unique(con[["lip", "rip", "lport", "rport", "proto"]], return_index=True)
        e = np.concatenate([lis, con[np.sort(first)]])
        e["cookie"] = rng.integers(0, COOKIE_MAX + 1, size=len(e))
        sets[int(u)] = e
    return sets


# ------------------------------------------------------------------ traffic
KINDS = ("hit", "near_proto", "near_lip", "near_lport", "near_rip", "near_rport", "icmp", "ihl6",
         "mf_as_written", "mf_on_the_wire", "not_ipv4", "version6")


def build_frames(rng, proto, lip, lport, rip, rport):
    """u8[n, 64] Ethernet/IPv4 frames with these tuples: IHL 5, the MF bit of
    the rule clear, every other byte random."""
    n = len(proto)
    f = rng.integers(0, 256, size=(n, HDR), dtype=np.uint8)
    f[:, 12], f[:, 13], f[:, 14] = 0x08, 0x00, 0x45
    f[:, 21] &= 0xDF
    f[:, 23] = proto
    for j in range(4):
        f[:, 26 + j] = (rip >> (24 - 8 * j)) & 0xFF
        f[:, 30 + j] = (lip >> (24 - 8 * j)) & 0xFF
    f[:, 34], f[:, 35] = (rport >> 8) & 0xFF, rport & 0xFF
    f[:, 36], f[:, 37] = (lport >> 8) & 0xFF, lport & 0xFF
    return f


def traffic(rng, sets, n, uniqids=None):
    """(frames u8[n, 64], uniqid i64[n], kind index[n]): packets of the
    runtimes in @uniqids (default: those of @sets), each cut from one of its
    runtime's entries (a connection's 5-tuple; a listener's laddr with a
    random raddr, a random local address for a listener on 0) and then, by
    KINDS, left as it is or changed in exactly one field or header property.
    A runtime without entries gets random tuples."""
    us = np.array(sorted(sets) if uniqids is None else list(uniqids), dtype=np.int64)
    u = us[rng.integers(0, len(us), size=n)]
    proto = rng.choice([6, 17], size=n).astype(np.int64)
    lip = np.array([runtime_ip(int(x)) for x in us])[np.searchsorted(us, u)].astype(np.int64)
    lport = rng.integers(1, 65536, size=n)
    rip = 0xC0A80000 + rng.integers(0, 4096, size=n)
    rport = rng.integers(1, 65536, size=n)
    for x in us:
        ents = sets.get(int(x))
        sel = np.nonzero(u == x)[0]
        if ents is None or not len(ents) or not len(sel):
            continue
        e = ents[rng.integers(0, len(ents), size=len(sel))]
        five = e["match"] == M5
        proto[sel], lport[sel] = e["proto"], e["lport"]
        lip[sel] = np.where(e["lip"] == 0, lip[sel], e["lip"])
        rip[sel] = np.where(five, e["rip"], rip[sel])
        rport[sel] = np.where(five, e["rport"], rport[sel])
    kind = rng.choice(len(KINDS), size=n, p=[0.5] + [0.5 / (len(KINDS) - 1)] * (len(KINDS) - 1))
    k = lambda name: kind == KINDS.index(name)  # noqa: E731
    proto = np.where(k("near_proto"), 23 - proto, proto)  # 6 <-> 17
    lip = np.where(k("near_lip"), lip ^ (1 << rng.integers(0, 32, size=n)), lip)
    lport = np.where(k("near_lport"), lport ^ (1 << rng.integers(0, 16, size=n)), lport)
    rip = np.where(k("near_rip"), rip ^ (1 << rng.integers(0, 32, size=n)), rip)
    rport = np.where(k("near_rport"), rport ^ (1 << rng.integers(0, 16, size=n)), rport)
    proto = np.where(k("icmp"), rng.choice([1, 2, 47, 0, 16, 18], size=n), proto)
    f = build_frames(rng, proto, lip, lport, rip, rport)
    f[k("ihl6"), 14] = 0x46
    f[k("version6"), 14] = 0x65
    f[k("mf_as_written"), 21] |= 0x20   # IP_MF against the little-endian load: byte 21
    f[k("mf_on_the_wire"), 20] |= 0x20  # the wire's MF bit: the rule as written passes it
    f[k("mf_on_the_wire"), 21] &= 0xDF
    et = rng.choice([0x0806, 0x86DD, 0x0801, 0x0008, 0x0900], size=n)
    f[k("not_ipv4"), 12] = (et >> 8)[k("not_ipv4")]
    f[k("not_ipv4"), 13] = (et & 0xFF)[k("not_ipv4")]
    return f, u, kind


# ------------------------------------------------------------------ verdicts
def verdicts_for(rng, u, vbytes, thread_bits, other=0.08):
    """Raw verdicts (u64[n], the low @vbytes bytes count) delivering packet i
    to runtime u[i]: DELIVER or WAKE with random flags, slot and hash; a share
    @other of them another action instead (those packets are NA)."""
    n = len(u)
    u = np.asarray(u, dtype=np.uint64)
    oth = rng.random(n) < other
    act_other = rng.integers(2, 6, size=n).astype(np.uint64)
    wake = rng.random(n) < 0.3
    slot = rng.integers(0, 1 << thread_bits, size=n).astype(np.uint64)
    if vbytes in (8, 4):
        flags = rng.choice([0, 0x40, 0x80, 0xC0], size=n).astype(np.uint64)
        w = np.where(oth, np.uint64(0xFFFF) | np.uint64(0xFF) << np.uint64(16) | act_other << np.uint64(24),
                     u | rng.integers(0, 256, size=n).astype(np.uint64) << np.uint64(16) |
                     (wake.astype(np.uint64) | flags) << np.uint64(24))
        if vbytes == 8:
            w = w << np.uint64(32) | rng.integers(0, 2**32, size=n).astype(np.uint64)
        return w
    q = u << np.uint64(thread_bits) | slot
    if vbytes == 2:
        return np.where(oth, np.uint64(0xC000) | act_other, q | np.where(wake, 0x4000, 0).astype(np.uint64))
    return np.where(oth, np.uint64(0x80) | act_other, q)


def garbage_verdicts(rng, n, vbytes):
    """Random bytes, with the shapes the rule names among them: uniqids at
    and past max_runtimes, the undefined 2-B kind 0x8000, actions past 5."""
    raw = rng.integers(0, 2**63, size=n).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n).astype(np.uint64)
    if vbytes == 2:
        raw[::7] = (raw[::7] & np.uint64(0x3FFF)) | np.uint64(0x8000)
    return raw & np.uint64((1 << (8 * vbytes)) - 1) if vbytes < 8 else raw


def pack_verdicts(raw, vbytes):
    """The verdict array as the library reads it: u8[n * vbytes], little endian."""
    raw = np.ascontiguousarray(raw, dtype="<u8")
    return np.ascontiguousarray(raw.view(np.uint8).reshape(-1, 8)[:, :vbytes]).reshape(-1)


# ------------------------------------------------------------------ the hand-derived fixture
def _ip(s):
    a, b, c, d = (int(x) for x in s.split("."))
    return a << 24 | b << 16 | c << 8 | d


def golden_scenarios():
    """tests/golden/sock_cases.json as a list of dicts: name, max_runtimes,
    sets ({uniqid: ENTRY array}), frames (u8[n, 64]), raw4 (the 4-byte verdict
    of every packet, u64[n]), expect (u32[n]), klass (counter slot, int[n]),
    cites."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sock_cases.json")
    names = {"NA": NA, "MISS": MISS, "MULTI": MULTI}
    slots = {"HIT5": HIT5, "HIT3": HIT3, "HIT3_ANY": HIT3_ANY, "N_MULTI": N_MULTI, "N_MISS": N_MISS,
             "N_NA": N_NA}
    out = []
    for s in json.load(open(path))["scenarios"]:
        sets = {}
        for e in s["entries"]:
            rec = np.zeros(1, dtype=ENTRY)
            rec["lip"], rec["lport"], rec["proto"] = _ip(e["lip"]), e["lport"], e["proto"]
            rec["match"], rec["cookie"] = e["match"], e["cookie"]
            rec["rip"], rec["rport"] = _ip(e.get("rip", "0.0.0.0")), e.get("rport", 0)
            sets.setdefault(e["uniqid"], []).append(rec)
        sets = {u: np.concatenate(v) for u, v in sets.items()}
        pk = s["packets"]
        frames = np.zeros((len(pk), HDR), dtype=np.uint8)
        raw4 = np.zeros(len(pk), dtype=np.uint64)
        for i, p in enumerate(pk):
            f = frames[i]
            f[12], f[13], f[14], f[23] = 0x08, 0x00, 0x45, p["proto"]
            f[26:30] = list(_ip(p["rip"]).to_bytes(4, "big"))
            f[30:34] = list(_ip(p["lip"]).to_bytes(4, "big"))
            f[34:36] = list(p["rport"].to_bytes(2, "big"))
            f[36:38] = list(p["lport"].to_bytes(2, "big"))
            for at, val in p.get("patch", {}).items():
                f[int(at)] = val
            raw4[i] = p["uniqid"] | 0 << 16 if "uniqid" in p else 0xFFFF | 0xFF << 16 | p["action"] << 24
        out.append({
            "name": s["name"], "max_runtimes": s.get("max_runtimes", 16), "sets": sets, "frames": frames,
            "raw4": raw4,
            "expect": np.array([names.get(p["expect"], p["expect"]) for p in pk], dtype=np.uint32),
            "klass": np.array([slots[p["count"]] for p in pk]), "cites": [p["cite"] for p in pk]})
    return out
