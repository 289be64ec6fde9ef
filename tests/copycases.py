"""Test-side definition of the loopback frame copy (gcl_copy_batch,
gcl_copy_batch_host), written from include/gclassify.h in numpy and Python
integers, and the case builders its CPU and GPU tests share.

The rule for packet i with L = len[i], d = dst_off[i] (or i * dst_stride):
REFUSED when dst_cap != 0 and L > dst_cap, when there is no dst_off and
L > dst_stride, or when d > dst_len or L > dst_len - d: nothing written,
pkt_len 0.  COPIED otherwise: dst[d + j] = src[src_off[i] + j] when that
index is below src_len, else 0; pkt_len L.  olflags and rss are written for
every packet.

A case is a dict: src (the whole array behind the source, which may go on
past src_len), src_len, src_off, len, dst_len, dst_off (or None), dst_stride,
tx_olflags, hash (or None), dst_cap."""
import numpy as np

COPIED_I, REFUSED_I, BYTES_I, NR = 0, 1, 2, 4
TXFLAG_LOCAL_HINT = 1 << 6
F_RSS_HASH, F_IP_CKSUM_GOOD = 0x01, 0x08
FILL = 0x5A   # what a destination holds before the call
GUARD = 64    # bytes kept on both sides of a destination
U64_MAX = (1 << 64) - 1

GRID_LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 60, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                1023, 1024, 1025, 1500, 1514, 9018)
GRID_SRC_ALIGN = (0, 1, 3, 4, 8, 12, 15)
GRID_DST_ALIGN = (0, 1, 2, 4, 7, 8, 15)
SIZES = (1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097)

# the reference's ingress pool: 9408-B elements, 222 per 2 MiB page, data at + 344
ELT, ELT_PER_PAGE, DATA_OFF, PAGE = 9408, (2 << 20) // 9408, 344, 2 << 20


def loopback_olflags(tx):
    """tx_prepare_tx_mbuf (tx.c:81) + copy_batch (dma.c:182-185)"""
    tx = np.asarray(tx, dtype=np.uint8)
    return (np.where(tx & TXFLAG_LOCAL_HINT, F_RSS_HASH, 0) | F_IP_CKSUM_GOOD).astype(np.uint8)


def expected(case, dst=None):
    """(dst u8[dst_len], pkt_len u16[n], olflags u8[n], rss u32[n], counts
    u64[NR]) of the definition; @dst is the destination before the call (FILL
    everywhere when None) and is left as it is."""
    src, src_len = np.asarray(case["src"], dtype=np.uint8), int(case["src_len"])
    dst_len, dst_off, stride, cap = int(case["dst_len"]), case["dst_off"], int(case["dst_stride"]), \
        int(case["dst_cap"])
    n = len(case["len"])
    out = np.full(dst_len, FILL, dtype=np.uint8) if dst is None else np.array(dst, dtype=np.uint8)
    assert len(out) == dst_len and src_len <= len(src)
    pkt_len = np.zeros(n, dtype=np.uint16)
    counts = np.zeros(NR, dtype=np.uint64)
    for i in range(n):
        L, so = int(case["len"][i]), int(case["src_off"][i])
        d = int(dst_off[i]) if dst_off is not None else i * stride
        if (cap and L > cap) or (dst_off is None and L > stride) or d > dst_len or L > dst_len - d:
            counts[REFUSED_I] += 1
            continue
        have = min(L, max(0, src_len - so))
        out[d:d + have] = src[so:so + have]
        out[d + have:d + L] = 0
        pkt_len[i] = L
        counts[COPIED_I] += 1
        counts[BYTES_I] += L
    tx = case["tx_olflags"] if case["tx_olflags"] is not None else np.zeros(n, dtype=np.uint8)
    rss = np.asarray(case["hash"], dtype=np.uint32) if case["hash"] is not None else \
        np.zeros(n, dtype=np.uint32)
    return out, pkt_len, loopback_olflags(tx), rss, counts


def _case(src, src_off, length, dst_len, dst_off=None, dst_stride=0, src_len=None, dst_cap=0,
          seed=0, flags=True, hashes=True):
    rng = np.random.default_rng(1000 + seed)
    n = len(length)
    return {
        "src": np.ascontiguousarray(src, dtype=np.uint8),
        "src_len": len(src) if src_len is None else src_len,
        "src_off": np.array([int(x) for x in src_off], dtype=np.uint64),
        "len": np.asarray(length, dtype=np.uint16),
        "dst_len": int(dst_len),
        "dst_off": None if dst_off is None else np.array([int(x) for x in dst_off], dtype=np.uint64),
        "dst_stride": dst_stride, "dst_cap": dst_cap,
        "tx_olflags": rng.integers(0, 256, size=n, dtype=np.uint8) if flags else None,
        "hash": rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) if hashes else None,
    }


def _random(rng, size):
    """random bytes with no FILL among them: an untouched byte shows"""
    a = rng.integers(0, 255, size=size, dtype=np.uint8)
    a[a >= FILL] += 1
    return a


def packed(lengths_aligns, seed=0, src_gap=48):
    """Packets (L, source alignment, destination alignment) with the
    destinations packed back to back from offset 0 with no gap: where the
    running offset does not have the wanted alignment a filler packet of 1-15
    bytes (a packet like any other) brings it there.  Sources lie in slots of
    their own, @src_gap or more bytes apart."""
    rng = np.random.default_rng(seed)
    src_off, length, dst_off = [], [], []
    d = s = 0

    def add(L, sa):
        nonlocal d, s
        s = (s + 15) // 16 * 16 + sa
        src_off.append(s)
        length.append(L)
        dst_off.append(d)
        d += L
        s += L + src_gap

    for L, sa, da in lengths_aligns:
        if d % 16 != da:
            add((da - d) % 16, int(rng.integers(0, 16)))
        add(L, sa)
    src = _random(rng, s + 64)
    return _case(src, src_off, length, d, dst_off=dst_off, seed=seed)


def grid_case():
    """Every length x source alignment x destination alignment, and one
    65535-byte packet at alignments (5, 11)."""
    cells = [(L, sa, da) for L in GRID_LENGTHS for sa in GRID_SRC_ALIGN for da in GRID_DST_ALIGN]
    order = np.random.default_rng(7).permutation(len(cells))
    return packed([cells[i] for i in order] + [(65535, 5, 11)], seed=7)


def dense_case(n, seed=0):
    """64-byte slots to 64-byte slots; one packet in eight is shorter."""
    rng = np.random.default_rng(seed + n)
    length = np.where(rng.random(n) < 0.125, rng.integers(0, 64, size=n), 64)
    return _case(_random(rng, n * 64), np.arange(n) * 64, length, n * 64, dst_stride=64, seed=n)


def ingress_offsets(n):
    i = np.arange(n, dtype=np.uint64)
    return (i // ELT_PER_PAGE) * PAGE + (i % ELT_PER_PAGE) * ELT + DATA_OFF


def ingress_case(n, seed=0):
    """The reference's ingress geometry: destinations at element + 344 of
    9408-B elements (dst_off), lengths of a mixed workload (64-B, MTU and a
    few jumbo frames), sources in 1600-B tx slots at any alignment, the jumbo
    frames out of one shared area."""
    rng = np.random.default_rng(seed + 31 * n)
    kind = rng.random(n)
    length = np.where(kind < 0.4, 64, np.where(kind < 0.6, rng.integers(0, 1515, size=n), 1500))
    jumbo = np.arange(n) % 97 == 5
    length[jumbo] = 9000
    src_off = np.arange(n) * 1600 + rng.integers(0, 16, size=n)
    src_off[jumbo] = n * 1600 + rng.integers(0, 16, size=int(jumbo.sum()))
    src = _random(rng, n * 1600 + 9100)
    elems = rng.permutation(n)  # mbufs come off the pool in any order
    dst_len = -(-n // ELT_PER_PAGE) * PAGE
    return _case(src, src_off, length, dst_len, dst_off=ingress_offsets(n)[elems], seed=n,
                 dst_cap=ELT - DATA_OFF)


def source_edge_case(src_len=3000, behind=4096, seed=0):
    """The source region's ends: offsets in [0, 16), frames that end exactly
    at src_len, frames that cross it (a zero tail), offsets at and past it,
    empty frames.  The array behind the source goes on past src_len with
    non-zero bytes that must read as 0."""
    rng = np.random.default_rng(seed + src_len)
    src = _random(rng, behind)
    pk = [(o, L) for o in range(16) for L in (1, 20, 100)]
    pk += [(src_len - L, L) for L in (1, 15, 16, 17, 33, 64, 100, 257) if L <= src_len]
    pk += [(src_len - k, L) for k in range(1, 41) for L in (k + 1, k + 16, 150) if k <= src_len]
    pk += [(o, L) for o in (src_len, src_len + 1, src_len + 16, 1 << 63, U64_MAX, U64_MAX - 15)
           for L in (0, 1, 16, 50)]
    pk += [(0, min(src_len, 400)), (0, src_len + 10 if src_len < 100 else 0)]
    order = rng.permutation(len(pk))
    src_off = [pk[i][0] for i in order]
    length = [pk[i][1] for i in order]
    dst_off = np.concatenate([[0], np.cumsum(length)[:-1]])
    return _case(src, src_off, length, int(np.sum(length)), dst_off=dst_off, src_len=src_len,
                 seed=src_len)


def dest_edge_case(seed=0):
    """The destination region's end, by offsets: d + L == dst_len (copied),
    d + L == dst_len + 1 (refused), d == dst_len with L == 0 (copied),
    d = UINT64_MAX and 2^63, and L > dst_cap, between packets that fit."""
    rng = np.random.default_rng(seed)
    dst_len, cap = 5003, 700
    src = _random(rng, 8192)
    pk = []  # (dst_off, L)
    d = 0
    for L in (64, 1, 0, 333, 700, 17, 128):  # fit: [0, 1243)
        pk.append((d, L))
        d += L
    pk += [(dst_len - 100, 100), (dst_len - 200, 101 + 100), (dst_len, 0), (dst_len, 1),
           (dst_len + 1, 0), (U64_MAX, 0), (U64_MAX, 10), (1 << 63, 64), (U64_MAX - 5, 6),
           (2000, 701), (2000, 65535), (3000, 700), (dst_len - 1, 2), (dst_len - 101, 1)]
    order = rng.permutation(len(pk))
    dst_off = [pk[i][0] for i in order]
    length = [pk[i][1] for i in order]
    src_off = rng.integers(0, 4000, size=len(pk))
    return _case(src, src_off, length, dst_len, dst_off=dst_off, dst_cap=cap, seed=seed)


def stride_edge_case(stride=64, n=200, seed=0):
    """Fixed slots: L > dst_stride is refused, and so is a slot that the
    destination region ends in (the last slots lie past dst_len)."""
    rng = np.random.default_rng(seed + stride)
    length = rng.integers(0, 2 * stride, size=n)
    length[::7] = stride
    dst_len = (n - 3) * stride + 20
    src = _random(rng, n * 2 * stride + 64)
    return _case(src, np.arange(n) * 2 * stride + rng.integers(0, 16, size=n), length, dst_len,
                 dst_stride=stride, seed=stride)


def edge_cases():
    return {
        "source edges": source_edge_case(),
        "source edges, src_len 1000 of 1024": source_edge_case(1000, 1024),
        "src_len 7": source_edge_case(7, 64),
        "src_len 15": source_edge_case(15, 64),
        "destination edges": dest_edge_case(),
        "stride 64": stride_edge_case(64),
        "stride 1536": stride_edge_case(1536, 40),
    }


def mixed_case(n=257, seed=5):
    """@n packets of mixed lengths at any alignment, packed back to back."""
    rng = np.random.default_rng(seed)
    L = rng.choice([0, 1, 60, 64, 65, 128, 300, 1500, 1514, 4000], size=n)
    return packed(list(zip(L.tolist(), rng.integers(0, 16, size=n).tolist(),
                           rng.integers(0, 16, size=n).tolist())), seed=seed)
