"""The definition of gcl_l4_payload (include/gclassify.h) in numpy, and the
cases the CPU and GPU tests share.  The model is written from the header's
text: a packet is judged once by its own bytes (the L4 eligibility is
tests/l4cases.py's judge, the definition gcl_l4_csum's tests use), a list
entry then takes the first verdict that applies, and the layout is a cumulative
sum of Python-checked uint64.

A case is tests/l4cases.py's dict (frames, frames_len, offs or stride,
pkt_len); the list and the filters are arguments of model().
"""
import functools

import numpy as np

from tests import l4cases as lc
from tests.l4cases import TCP, UDP

NA, K_UDP, K_TCP, NOSOCK, BADCSUM, OOR = range(6)
C_UDP, C_TCP, C_NA, C_NOSOCK, C_BADCSUM, C_OOR, C_BYTES, NR = 0, 1, 2, 3, 4, 5, 6, 8
COUNTER = {K_UDP: C_UDP, K_TCP: C_TCP, NA: C_NA, NOSOCK: C_NOSOCK, BADCSUM: C_BADCSUM, OOR: C_OOR}
S_NA, S_MISS, S_MULTI, COOKIE_MAX = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFEF
MAX_BLOCKS, TILE = 1024, 256
META = np.dtype([("rip", "<u4"), ("rport", "<u2"), ("proto", "u1"), ("tcp_flags", "u1"),
                 ("seq", "<u4"), ("ack", "<u4")])
SENTINEL, GUARD = 0xA7, 64  # the fill of every output buffer, and the entries kept behind it


def be(f, at, k):
    return int.from_bytes(bytes(f[at:at + k]), "big")


def packets(case):
    """Every packet judged by its own bytes: (kind NA / K_UDP / K_TCP, len,
    src_off, meta) arrays of n + 1 entries; the last stands for 'no packet'."""
    flen, offs, plen = case["frames_len"], case["offs"], case["pkt_len"]
    n = len(plen)
    kind, ln = np.zeros(n + 1, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint16)
    src, meta = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=META)
    for i in range(n):
        raw = int(offs[i]) if offs is not None else i * case["stride"]
        o = min(raw, flen)
        L = min(int(plen[i]), flen - o)
        f = case["frames"][o:o + L]
        _, l4_ok, proto, l4len = lc.judge(f, L)
        if not l4_ok:
            continue
        hl = 4 * (int(f[46]) >> 4) if proto == TCP else 8
        if proto == TCP and (hl < 20 or hl > l4len):  # l4len = tot - 20
            continue
        kind[i] = K_TCP if proto == TCP else K_UDP
        ln[i] = l4len - hl
        src[i] = o + 34 + hl
        assert o <= src[i] <= o + L and int(src[i]) + int(ln[i]) <= o + L
        meta[i] = (be(f, 26, 4), be(f, 34, 2), proto, f[47], be(f, 38, 4), be(f, 42, 4)) if proto == TCP \
            else (be(f, 26, 4), be(f, 34, 2), proto, 0, 0, 0)
    return kind, ln, src, meta


def model(case, order=None, sock=None, l4_status=None, seg_off=None, align=0, pk=None):
    """A dict of every output of one call: src_off, len, dst_off, kind, meta,
    seg_bytes (None without @seg_off), total (u64[1]) and counts (u64[NR])."""
    pk = pk or packets(case)
    n = len(case["pkt_len"])
    idx = np.arange(n, dtype=np.int64) if order is None else np.asarray(order).astype(np.int64)
    m = len(idx)
    oor = idx >= n
    ii = np.where(oor, n, idx)
    kind = pk[0][ii].copy()
    elig = kind != NA
    pad1 = lambda a, fill: np.concatenate([np.asarray(a), [fill]])  # noqa: E731
    bad = elig & ((pad1(l4_status, 0)[ii] & 0xF) == lc.BAD) if l4_status is not None else np.zeros(m, bool)
    nos = elig & ~bad & (pad1(sock, 0)[ii].astype(np.uint64) > COOKIE_MAX) if sock is not None \
        else np.zeros(m, bool)
    kind[oor], kind[bad], kind[nos] = OOR, BADCSUM, NOSOCK
    kept = (kind == K_UDP) | (kind == K_TCP)
    ln = np.where(kept, pk[1][ii], 0).astype(np.uint16)
    src = np.where(kept, pk[2][ii], 0).astype(np.uint64)
    meta = pk[3][ii].copy()
    meta[~kept] = np.zeros(1, dtype=META)[0]
    a = max(align, 1)
    padded = (ln.astype(np.uint64) + np.uint64(a - 1)) // np.uint64(a) * np.uint64(a)
    incl = np.cumsum(padded, dtype=np.uint64)
    total = int(incl[-1]) if m else 0
    assert total == sum(padded.tolist())  # exact Python integers
    dst = (incl - padded).astype(np.uint64)
    seg = None
    if seg_off is not None:
        seg = np.array([int(dst[s]) if s < m else total for s in np.asarray(seg_off).astype(np.int64)],
                       dtype=np.uint64)
    counts = np.zeros(NR, dtype=np.uint64)
    for k, c in COUNTER.items():
        counts[c] = int((kind == k).sum())
    counts[C_BYTES] = int(ln.sum(dtype=np.uint64))
    assert int(counts[:6].sum()) == m
    return {"src_off": src, "len": ln, "dst_off": dst, "kind": kind, "meta": meta, "seg_bytes": seg,
            "total": np.array([total], dtype=np.uint64), "counts": counts}


# ---------------------------------------------------------------- builders
def tcp_frame(rng, doff, pay, pad=0, l4len=None, **kw):
    """A TCP frame with data offset @doff (in dwords) and @pay payload bytes
    behind it; @l4len overrides the L4 length the IP header claims."""
    l4len = 4 * doff + pay if l4len is None else l4len
    f = lc.frame(rng, TCP, l4len, pad=pad, **kw)
    f[46] = doff << 4 | int(rng.integers(0, 16))
    return f


def udp_frame(rng, pay, pad=0, **kw):
    return lc.frame(rng, UDP, 8 + pay, pad=pad, **kw)


@functools.lru_cache(maxsize=None)
def grid_case():
    """TCP data offset 5..15 x payload {0, 1, 15, 16, 17, 1460}, UDP payload
    {0, 1, 17, 1472}, each at all 16 frame alignments, back to back."""
    rng = np.random.default_rng(71)
    frs, aligns = [], []
    for a in range(16):
        for doff in range(5, 16):
            for pay in (0, 1, 15, 16, 17, 1460):
                frs.append(tcp_frame(rng, doff, pay, pad=int(rng.integers(0, 3))))
                aligns.append(a)
        for pay in (0, 1, 17, 1472):
            frs.append(udp_frame(rng, pay, pad=int(rng.integers(0, 3))))
            aligns.append(a)
    return lc.layout(frs, aligns)


NA_NAMES = ("good_udp",) + lc.NA_REASONS[:8] + ("doff4", "hl_past_tot", "pkt_len_short", "good_tcp",
                                                "at_end", "past_end", "max_off", "cut")


@functools.lru_cache(maxsize=None)
def na_case(cut):
    """One packet per NA reason, by NA_NAMES, between good ones.  The last
    frame, TCP with a 24-byte header and 30 payload bytes, is cut by
    frames_len: @cut = 'header' inside its TCP header, 'payload' one byte
    before the payload's end, None not at all (then it is kept)."""
    rng = np.random.default_rng(72)
    named = lc.na_frames(rng)
    short = tcp_frame(rng, 5, 40)
    last = tcp_frame(rng, 6, 30)
    frs = [udp_frame(rng, 30)] + [named[k] for k in lc.NA_REASONS[:8]] + \
          [tcp_frame(rng, 4, 44), tcp_frame(rng, 7, 0, l4len=24), short, tcp_frame(rng, 5, 9)] + [last] * 4
    case = lc.layout(frs, gap=3)
    o_last = int(case["offs"][-1])
    full = o_last + len(last)
    case["frames_len"] = {None: full, "payload": full - 1, "header": o_last + 34 + 10}[cut]
    case["frames"] = case["frames"][:case["frames_len"]].copy()
    case["pkt_len"][11] -= 1   # one short of 14 + tot
    flen = case["frames_len"]
    case["offs"][13:16] = (flen, flen + 77, (1 << 64) - 1)
    return case


SOCKS = (0, COOKIE_MAX, COOKIE_MAX + 1, S_MULTI, S_MISS, S_NA)
STATUSES = (lc.GOOD, lc.BAD, lc.NONE, lc.NA, lc.BAD | 0x30, lc.GOOD | 0x20)


@functools.lru_cache(maxsize=None)
def filter_case():
    """A kept UDP frame, a kept TCP frame, a frame that is not IPv4 and a TCP
    frame with data offset 4, each under every pair of a sock value and an
    l4_status value: every way two or three reasons can apply at once.
    Returns (case, sock u32[n], l4_status u8[n])."""
    rng = np.random.default_rng(73)
    frs, sock, st = [], [], []
    for s in SOCKS:
        for t in STATUSES:
            other = udp_frame(rng, 20)
            other[12:14] = (0x86, 0xDD)
            for f in (udp_frame(rng, 33), tcp_frame(rng, 8, 100), other, tcp_frame(rng, 4, 50)):
                frs.append(f)
                sock.append(s)
                st.append(t)
    case = lc.layout(frs, aligns=[int(a) for a in rng.integers(0, 16, size=len(frs))])
    return case, np.array(sock, dtype=np.uint32), np.array(st, dtype=np.uint8)


def orders(n, seed=74):
    """name -> (order u32[m], seg_off u32[nseg + 1]) over @n packets."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n).astype(np.uint32)
    long = np.concatenate([perm.astype(np.int64), perm[::3].astype(np.int64),
                           rng.integers(n, 1 << 32, size=50, dtype=np.int64),
                           np.array([0xFFFFFFFF, n, n - 1, 0], dtype=np.int64)]).astype(np.uint32)
    rng.shuffle(long)
    m = len(long)
    return {"permutation": (perm, np.array([0, n // 3, n // 2, n], dtype=np.uint32)),
            "shorter": (perm[:n // 2 + 1], np.array([0, 5, 5, n // 2 + 1], dtype=np.uint32)),
            "longer": (long, np.array([0, m - 1, m, m + 1, 7, 0xFFFFFFFF, 3, m // 2, 0x80000000],
                                      dtype=np.uint32))}


# every range of every blocks value makes more than one pass: at the cap a range is 3 tiles
SCAN_K = 683
SCAN_M = 3 * TILE * SCAN_K + 5
SCAN_BLOCKS = (1, 2, 3, 7, MAX_BLOCKS)
assert -(-SCAN_M // TILE) >= 2 * MAX_BLOCKS


@functools.lru_cache(maxsize=None)
def scan_case():
    """SCAN_M entries drawn from the filter case's packets (a few out of
    range), with its sock and l4_status.  Returns (case, sock, st, order)."""
    case, sock, st = filter_case()
    n = len(case["pkt_len"])
    rng = np.random.default_rng(75)
    order = rng.integers(0, n + 3, size=SCAN_M, dtype=np.uint64).astype(np.uint32)
    return case, sock, st, order


BIG_M, BIG_PAY = 70000, 65493


@functools.lru_cache(maxsize=None)
def big_case():
    """BIG_M entries that all name one maximal UDP datagram (tot 65 521,
    payload 65 493 B): with align 256 every entry takes 65 536 B and the total
    passes 2^32."""
    rng = np.random.default_rng(76)
    case = lc.layout([udp_frame(rng, BIG_PAY)])
    assert case["pkt_len"][0] == 65535
    return case, np.zeros(BIG_M, dtype=np.uint32)


def blank_outputs(m, nseg, with_seg=True, with_meta=True):
    """Every output buffer of a call as numpy arrays filled with SENTINEL,
    GUARD entries longer than the call may write."""
    def arr(k, dt):
        return np.frombuffer(bytes([SENTINEL]) * (np.dtype(dt).itemsize * (k + GUARD)), dtype=dt).copy()
    return {"src_off": arr(m, np.uint64), "len": arr(m, np.uint16), "dst_off": arr(m, np.uint64),
            "kind": arr(m, np.uint8), "meta": arr(m, META) if with_meta else None,
            "seg_bytes": arr(nseg + 1, np.uint64) if with_seg else None, "total": arr(1, np.uint64)}


def compare(got, want, m, nseg, what, written=True):
    """@got (blank_outputs after a call, as numpy) against the model's @want:
    exact equality of the written part and an untouched guard.  With @written
    False only total and seg_bytes may have changed (m == 0)."""
    for f, k in (("src_off", m), ("len", m), ("dst_off", m), ("kind", m), ("meta", m),
                 ("seg_bytes", nseg + 1), ("total", 1)):
        g = got[f]
        if g is None:
            continue
        tail = g[k:].view(np.uint8)
        assert (tail == SENTINEL).all() and len(g) == k + GUARD, f"{what}: {f} written past its end"
        if not written and f not in ("seg_bytes", "total"):
            continue
        bad = np.nonzero(g[:k] != want[f][:k])[0]
        assert not len(bad), f"{what}: {f}[{bad[0]}] = {g[bad[0]]} != {want[f][bad[0]]} " \
                             f"({len(bad)} of {k} differ)"
