"""The definition of gcl_l4_csum (include/gclassify.h) in numpy, and the cases
the CPU and GPU tests share.  The model is written from the header's text: the
pseudo-header is built as twelve bytes, a filled field is zeroed before the
sum, sums are exact Python integers folded at the end.

A case is a dict: frames (u8, the whole region), frames_len, offs (u64[n]) or
None with stride, pkt_len (u16[n]), tx_olflags (u8[n]) or None.
"""
import functools

import numpy as np

VERIFY, FILL = 0, 1
NA, GOOD, BAD, NONE, FILLED_IP, FILLED_L4 = 0, 1, 2, 3, 0x10, 0x20
C_GOOD, C_BAD, C_NONE, C_NA, C_FILLED_IP, C_FILLED_L4, C_BYTES, NR = 0, 1, 2, 3, 4, 5, 6, 8
TCP, UDP = 6, 17
GUARD, FILLBYTE = 64, 0x5A
# the reference's ingress pool: 9408-B elements, 222 per 2 MiB page, data at + 344
ELT, ELT_PER_PAGE, DATA_OFF, PAGE = 9408, (2 << 20) // 9408, 344, 2 << 20
MAX_L4 = 65535 - 14 - 20  # 14 + tot <= pkt_len <= 65535

NA_REASONS = ("short", "ethertype", "ihl6", "mf", "fragoff", "proto1", "tot_small", "tot_past_len",
              "cut", "past_end")


def fold(s):
    s = int(s)
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def words(b):
    """Sum of @b's 16-bit words in memory order; an odd last byte is a low byte."""
    b = np.asarray(b, dtype=np.uint8)
    return int(b[0::2].sum(dtype=np.uint64)) + 256 * int(b[1::2].sum(dtype=np.uint64))


def judge(f, L):
    """(ip_ok, l4_ok, proto, l4len) of the frame bytes @f with @L of them valid."""
    if L < 34 or f[12] != 0x08 or f[13] != 0x00 or f[14] >> 4 != 4 or f[14] & 0xF != 5:
        return False, False, 0, 0
    frag = int(f[20]) << 8 | int(f[21])
    mf, fragoff = frag & 0x2000, frag & 0x1FFF
    proto, tot = int(f[23]), int(f[16]) << 8 | int(f[17])
    ok = not mf and not fragoff and proto in (TCP, UDP) and tot >= 20 + (20 if proto == TCP else 8) \
        and 14 + tot <= L
    return True, ok, proto, tot - 20


def l4_sum(f, proto, l4len):
    """S of the header's text over the bytes as they stand."""
    ph = np.concatenate([f[26:34], np.array([0, proto, l4len >> 8, l4len & 0xFF], dtype=np.uint8)])
    return fold(words(f[34:34 + l4len]) + words(ph))


def model(case, mode):
    """(status u8[n], counts u64[NR], the frames after the call)."""
    frames = case["frames"].copy()
    flen, offs, plen = case["frames_len"], case["offs"], case["pkt_len"]
    n = len(plen)
    status, counts = np.zeros(n, dtype=np.uint8), np.zeros(NR, dtype=np.uint64)
    for i in range(n):
        raw = int(offs[i]) if offs is not None else i * case["stride"]
        o = min(raw, flen)
        L = min(int(plen[i]), flen - o)
        f = frames[o:o + L]
        fl = 0 if mode != FILL else 3 if case["tx_olflags"] is None else int(case["tx_olflags"][i])
        ip_ok, l4_ok, proto, l4len = judge(f, L)
        st = NA
        if ip_ok and fl & 1:
            f[24:26] = 0
            v = ~fold(words(f[14:34])) & 0xFFFF
            f[24], f[25] = v & 0xFF, v >> 8
            st |= FILLED_IP
            counts[C_FILLED_IP] += 1
        if l4_ok:
            fo = 50 if proto == TCP else 40
            if mode == FILL:
                if fl & 2:
                    f[fo:fo + 2] = 0
                    v = ~l4_sum(f, proto, l4len) & 0xFFFF or 0xFFFF
                    f[fo], f[fo + 1] = v & 0xFF, v >> 8
                    st |= FILLED_L4
                    counts[C_FILLED_L4] += 1
                    counts[C_BYTES] += l4len
            elif proto == UDP and f[fo] == 0 and f[fo + 1] == 0:
                st = NONE
            else:
                st = GOOD if l4_sum(f, proto, l4len) == 0xFFFF else BAD
                counts[C_BYTES] += l4len
        status[i] = st
        counts[{GOOD: C_GOOD, BAD: C_BAD, NONE: C_NONE, NA: C_NA}[st & 0xF]] += 1
    return status, counts, frames


# ---------------------------------------------------------------- builders
def frame(rng, proto, l4len, payload=None, pad=0, frag=0x4000):
    """An Ethernet + IPv4 (IHL 5) + L4 frame, 34 + l4len + pad bytes, both
    checksum fields random (fill() makes them right)."""
    f = rng.integers(0, 256, size=34 + l4len + pad, dtype=np.uint8)
    tot = 20 + l4len
    f[12:14] = (0x08, 0x00)
    f[14] = 0x45
    f[16:18] = (tot >> 8, tot & 0xFF)
    f[20:22] = (frag >> 8, frag & 0xFF)
    f[23] = proto
    if payload is not None:
        f[34:34 + l4len] = payload
    return f


def layout(frs, aligns=None, gap=0, head=0, tail=0, pkt_len=None):
    """Frames back to back in one region, frame i starting at an offset that
    is aligns[i] mod 16 (the next one that is free), @gap bytes apart at least."""
    offs, cur = [], head
    for i, f in enumerate(frs):
        if aligns is not None:
            cur += (aligns[i] - cur) % 16
        offs.append(cur)
        cur += len(f) + gap
    region = np.full(offs[-1] + len(frs[-1]) + tail, 0xA5, dtype=np.uint8)
    for o, f in zip(offs, frs):
        region[o:o + len(f)] = f
    plen = np.array([len(f) for f in frs], dtype=np.uint16) if pkt_len is None else \
        np.asarray(pkt_len, dtype=np.uint16)
    return {"frames": region, "frames_len": len(region), "offs": np.array(offs, dtype=np.uint64),
            "stride": 0, "pkt_len": plen, "tx_olflags": None}


def slots(frs, stride, pkt_len=None):
    """Frame i in slot i of @stride bytes."""
    region = np.full(len(frs) * stride, 0xA5, dtype=np.uint8)
    for i, f in enumerate(frs):
        assert len(f) <= stride
        region[i * stride:i * stride + len(f)] = f
    plen = np.array([len(f) for f in frs], dtype=np.uint16) if pkt_len is None else \
        np.asarray(pkt_len, dtype=np.uint16)
    return {"frames": region, "frames_len": len(region), "offs": None, "stride": stride,
            "pkt_len": plen, "tx_olflags": None}


def filled(case):
    """@case with every fillable field made right by the model (tx_olflags 3)."""
    out = dict(case, tx_olflags=None)
    out["frames"] = model(out, FILL)[2]
    return dict(out, tx_olflags=case["tx_olflags"])


def start(case, i):
    return int(case["offs"][i]) if case["offs"] is not None else i * case["stride"]


def spoil(case, rng, idx, where="any"):
    """One L4 byte of each packet in @idx flipped in one bit: a GOOD packet
    becomes BAD (a one-bit change is never a multiple of 0xFFFF).  The
    checksum field itself is left alone, so that a UDP field stays non-zero."""
    for i in idx:
        o = start(case, i)
        f = case["frames"][o:]
        proto, l4len = int(f[23]), (int(f[16]) << 8 | int(f[17])) - 20
        fo = 50 if proto == TCP else 40
        cand = [j for j in {34, 34 + l4len - 1, 34 + int(rng.integers(0, l4len))} if j not in (fo, fo + 1)]
        j = cand[int(rng.integers(0, len(cand)))] if where == "any" else 34 + l4len - 1
        f[j] ^= 1 << int(rng.integers(0, 8))


def grid_frames(seed=11):
    """Every l4len from the protocol's minimum to 130, both protocols, each at
    all 16 alignments (the list repeats every frame 16 times)."""
    rng = np.random.default_rng(seed)
    frs, aligns = [], []
    for proto, lo in ((TCP, 20), (UDP, 8)):
        for l4len in range(lo, 131):
            for a in range(16):
                frs.append(frame(rng, proto, l4len, pad=int(rng.integers(0, 3))))
                aligns.append(a)
    return frs, aligns


BIG = ((TCP, 1460, 7, None), (UDP, 8960, 5, None), (TCP, MAX_L4, 3, None), (UDP, MAX_L4, 0, 0xFF),
       (TCP, MAX_L4, 1, 0xFF), (UDP, MAX_L4 - 1, 15, 0xFF))


def _mark(case, rng):
    """A filled case's packets, by index mod 4: 0, 1 GOOD; 2 BAD; 3 BAD, or
    NONE where it is UDP.  tx_olflags cycles through 0..3 and beyond."""
    n = len(case["pkt_len"])
    spoil(case, rng, [i for i in range(n) if i % 4 == 2])
    for i in range(3, n, 4):
        f = case["frames"][start(case, i):]
        if f[23] == UDP:
            f[40:42] = 0
        else:
            spoil(case, rng, [i], where="last")
    case["tx_olflags"] = (np.arange(n) * 7 % 256).astype(np.uint8)
    return case


@functools.lru_cache(maxsize=None)
def grid_case(with_big=True):
    """The length x alignment grid back to back (a one-byte overrun reads or
    writes a neighbour), then the large datagrams: 1460, 8960 and 65 501 bytes,
    the maximal one also as all 0xFF at an even and an odd address."""
    rng = np.random.default_rng(12)
    frs, aligns = grid_frames()
    if with_big:
        for proto, l4len, a, fillv in BIG:
            pay = None if fillv is None else np.full(l4len, fillv, dtype=np.uint8)
            frs.append(frame(rng, proto, l4len, payload=pay))
            aligns.append(a)
    return _mark(filled(layout(frs, aligns)), rng)


@functools.lru_cache(maxsize=None)
def stride_grid_case():
    """The same lengths in dense 176-B slots (the 16 alignments come from
    shifting the region's base)."""
    rng = np.random.default_rng(13)
    frs = [frame(rng, proto, l4len, pad=(l4len % 3)) for proto, lo in ((TCP, 20), (UDP, 8))
           for l4len in range(lo, 131)]
    return _mark(filled(slots(frs, 176)), rng)


@functools.lru_cache(maxsize=None)
def dense64_case(n=1500, seed=14):
    """64-B slots back to back, every slot full: l4len up to 30, padded to 64."""
    rng = np.random.default_rng(seed)
    frs = []
    for i in range(n):
        proto = TCP if i % 3 == 0 else UDP
        l4len = int(rng.integers(20 if proto == TCP else 8, 31))
        frs.append(frame(rng, proto, l4len, pad=30 - l4len))
    return _mark(filled(slots(frs, 64)), rng)


@functools.lru_cache(maxsize=None)
def tiled_dense64_case(n):
    """@n packets in 64-B slots: dense64_case's region repeated."""
    case = dense64_case()
    reps = -(-n // len(case["pkt_len"]))
    return {"frames": np.tile(case["frames"], reps)[:n * 64].copy(), "frames_len": n * 64, "offs": None,
            "stride": 64, "pkt_len": np.tile(case["pkt_len"], reps)[:n].copy(),
            "tx_olflags": np.tile(case["tx_olflags"], reps)[:n].copy()}


@functools.lru_cache(maxsize=None)
def mtu_case(n=300, seed=15):
    """1536-B slots: MTU frames (tot 1500) and shorter ones."""
    rng = np.random.default_rng(seed)
    frs = [frame(rng, TCP if i % 2 else UDP, 1480 if i % 5 else int(rng.integers(20, 1481)))
           for i in range(n)]
    return _mark(filled(slots(frs, 1536)), rng)


def ingress_offsets(n):
    i = np.arange(n, dtype=np.uint64)
    return (i // ELT_PER_PAGE) * np.uint64(PAGE) + (i % ELT_PER_PAGE) * np.uint64(ELT) + np.uint64(DATA_OFF)


@functools.lru_cache(maxsize=None)
def ingress_case(n=300, seed=16):
    """The reference's ingress geometry: frames at element + 344 of 9408-B
    elements, 222 per 2 MiB page; lengths up to a jumbo frame."""
    rng = np.random.default_rng(seed)
    offs = ingress_offsets(n)
    region = np.full(-(-n // ELT_PER_PAGE) * PAGE, 0xA5, dtype=np.uint8)
    plen = np.zeros(n, dtype=np.uint16)
    for i in range(n):
        l4len = int(rng.choice([26, 1480, 8966, int(rng.integers(20, 9000))]))
        f = frame(rng, TCP if i % 2 else UDP, l4len)
        region[int(offs[i]):int(offs[i]) + len(f)] = f
        plen[i] = len(f)
    case = {"frames": region, "frames_len": len(region), "offs": offs, "stride": 0, "pkt_len": plen,
            "tx_olflags": None}
    return _mark(filled(case), rng)


def na_frames(rng):
    """One frame per NA reason that a frame's own bytes can show, by name."""
    def base(proto=TCP, l4len=40, **kw):
        return frame(rng, proto, l4len, **kw)
    out = {}
    out["short"] = base()[:33]
    f = base(); f[12:14] = (0x86, 0xDD); out["ethertype"] = f
    f = base(); f[14] = 0x46; out["ihl6"] = f
    out["mf"] = base(frag=0x2000)
    out["fragoff"] = base(frag=0x0001)
    f = base(); f[23] = 1; out["proto1"] = f
    f = base(); f[16:18] = (0, 39); out["tot_small"] = f          # TCP needs tot >= 40
    f = base(); f[16:18] = (0, 61); out["tot_past_len"] = f       # 14 + 61 > 74
    return out


@functools.lru_cache(maxsize=None)
def na_case():
    """Every NA reason, one packet each, in NA_REASONS order, between two
    good packets; then the look-alikes that ARE eligible: DF set, the reserved
    flag bit set (not MF, not an offset), UDP with tot exactly 28."""
    rng = np.random.default_rng(17)
    named = na_frames(rng)
    good = frame(rng, UDP, 30)
    frs = [good] + [named[k] for k in NA_REASONS[:8]]
    # "cut": a good frame whose end frames_len cuts off; "past_end": an offset past frames_len
    alike = [frame(rng, TCP, 20, frag=0x4000), frame(rng, TCP, 33, frag=0x8000), frame(rng, UDP, 8)]
    cutf = frame(rng, TCP, 60)
    case = layout(frs + alike + [good.copy(), cutf], gap=5)
    # IHL 6 with a valid-looking tot, and v6-in-v4 version nibble
    case = filled(case)
    case["frames_len"] = int(case["offs"][-1]) + len(cutf) - 1
    case["frames"] = case["frames"][:case["frames_len"]].copy()
    case["offs"] = np.concatenate([case["offs"], np.array([case["frames_len"] + 100], dtype=np.uint64)])
    case["pkt_len"] = np.concatenate([case["pkt_len"], np.array([94], dtype=np.uint16)])
    names = ["good0"] + list(NA_REASONS[:8]) + ["df", "reserved_bit", "udp_min", "good1", "cut", "past_end"]
    return case, names


@functools.lru_cache(maxsize=None)
def edge_case():
    """The region's ends: the first frame at offset 0 and the last ending
    exactly at frames_len (their first and last 16-B chunks are not wholly
    inside the region at a shifted base), a frame cut by frames_len one byte
    short, offsets near, at and past frames_len (UINT64_MAX too), pkt_len 0,
    pkt_len below 34 and pkt_len longer than what frames_len leaves.  The
    entries that overlap real frames are all NA, so FILL has no overlap."""
    rng = np.random.default_rng(18)
    frs = [frame(rng, TCP, 21), frame(rng, UDP, 9), frame(rng, TCP, 300), frame(rng, UDP, 47),
           frame(rng, TCP, 20), frame(rng, UDP, 8), frame(rng, TCP, 77), frame(rng, UDP, 1471)]
    case = filled(layout(frs, gap=1))
    flen = case["frames_len"]
    assert int(case["offs"][-1]) + len(frs[-1]) == flen
    last = int(case["offs"][-1])
    n0 = len(frs)
    case["pkt_len"][-1] += 200   # longer than what frames_len leaves: L is what is there
    case["pkt_len"][3] = 65535
    extra_offs = [last + 1, last + 1480, flen - 20, flen - 1, flen, flen + 1, (1 << 64) - 1,
                  int(case["offs"][2]), int(case["offs"][2]), int(case["offs"][4])]
    extra_len = [len(frs[-1]), 100, 60, 60, 60, 60, 60, 33, 0, 33]
    case["offs"] = np.concatenate([case["offs"], np.array(extra_offs, dtype=np.uint64)])
    case["pkt_len"] = np.concatenate([case["pkt_len"], np.array(extra_len, dtype=np.uint16)])
    # the added entries overlap real frames: none of them may be one FILL writes
    st = model(dict(case, tx_olflags=None), FILL)[0]
    assert (st[:n0] == FILLED_IP | FILLED_L4).all() and (st[n0:] == NA).all()
    return case


def _share(n, *parts):
    """Index sets of the given sizes, disjoint, out of range(n)."""
    out, at = [], 0
    for k in parts:
        out.append(list(range(at, at + k)))
        at += k
    assert at <= n
    return out


@functools.lru_cache(maxsize=None)
def mix_case(n=1200, seed=19):
    """The random mix, constructed so that the shares hold by the model alone:
    of n packets 70 % are L4-eligible; of those 40 % GOOD, 35 % BAD (one L4
    byte flipped), the rest UDP sent without a checksum (NONE) or TCP carrying
    only the pseudo-header sum as the runtime leaves it (BAD until filled);
    the other 30 % cycle through every NA reason.  The order is shuffled, the
    alignments random, lengths from 8 bytes to a jumbo frame."""
    rng = np.random.default_rng(seed)
    n_el = n * 7 // 10
    named = None
    frs, kinds = [], []
    for i in range(n_el):
        proto = TCP if rng.random() < 0.5 else UDP
        l4len = int(rng.choice([int(rng.integers(20, 200)), 1460, int(rng.integers(200, 9000))],
                               p=[0.7, 0.2, 0.1]))
        frs.append(frame(rng, proto, l4len, pad=int(rng.integers(0, 7))))
        kinds.append("good" if i < n_el * 4 // 10 else "bad" if i < n_el * 3 // 4 else "other")
    for i in range(n - n_el):
        reason = NA_REASONS[i % len(NA_REASONS)]
        if reason in ("cut", "past_end"):
            frs.append(frame(rng, TCP, 64))
        else:
            if i % len(NA_REASONS) == 0 or named is None:
                named = na_frames(rng)
            frs.append(named[reason])
        kinds.append(reason)
    perm = rng.permutation(n)
    # the cut frame goes last, so that frames_len can cut it
    cut_first = [j for j in perm if kinds[j] == "cut"][0]
    perm = [j for j in perm if j != cut_first] + [cut_first]
    frs, kinds = [frs[j] for j in perm], [kinds[j] for j in perm]
    case = filled(layout(frs, aligns=[int(a) for a in rng.integers(0, 16, size=n)]))
    case["frames_len"] -= 3
    case["frames"] = case["frames"][:case["frames_len"]].copy()
    for i, kd in enumerate(kinds):
        o = int(case["offs"][i])
        f = case["frames"][o:]
        if kd == "bad":
            spoil(case, rng, [i])
        elif kd == "other":
            if f[23] == UDP:
                f[40:42] = 0
            else:  # the pseudo-header sum alone, as tcp_out.c leaves it for the NIC
                l4len = (int(f[16]) << 8 | int(f[17])) - 20
                ph = np.concatenate([f[26:34], np.array([0, TCP, l4len >> 8, l4len & 0xFF], dtype=np.uint8)])
                v = fold(words(ph))
                f[50], f[51] = v & 0xFF, v >> 8
        elif kd == "cut" and i != n - 1:  # the other "cut" packets: an mbuf shorter than tot says
            case["pkt_len"][i] -= 1
        elif kd == "past_end":
            case["offs"][i] = case["frames_len"] + int(rng.integers(0, 1 << 40))
    case["tx_olflags"] = rng.integers(0, 256, size=n).astype(np.uint8)
    return case, kinds


def zero_result_frame(proto, l4len=64, seed=20):
    """A frame whose S with the field taken as 0 is 0xFFFF, so that ~S is 0 and
    the filled field must be 0xFFFF: two payload bytes are solved for."""
    rng = np.random.default_rng(seed)
    f = frame(rng, proto, l4len)
    fo = 50 if proto == TCP else 40
    f[fo:fo + 2] = 0
    f[60:62] = 0
    s = l4_sum(f, proto, l4len)          # in [1, 0xFFFF]
    w = 0xFFFF - s                        # the word that brings the sum to 0xFFFF
    f[60], f[61] = w & 0xFF, w >> 8
    assert l4_sum(f, proto, l4len) == 0xFFFF
    f[fo:fo + 2] = rng.integers(1, 256, size=2)
    return f
