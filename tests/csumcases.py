"""Test-side definition of the IPv4 header checksum offload (gcl_rx_csum,
gcl_rx_csum_flags), written from include/gclassify.h in numpy, and the
header set its tests share.

The rule for packet i with entry flags fl: a frame whose bytes 12-13 are not
0x0800, or whose fl says IP_CKSUM_GOOD, keeps fl (SKIPPED); any other
(CHECKED) gets GOOD when the ten 16-bit words of frame bytes [14, 34) sum, in
one's complement, to 0xFFFF and BAD when they do not.  Bytes at or past
frames_len read 0, and an offset at or past it is a frame of zeros."""
import numpy as np

MASK, UNKNOWN, BAD, GOOD, NONE = 0x0C, 0x00, 0x04, 0x08, 0x0C
CHECKED_I, GOOD_I, BAD_I, SKIPPED_I, NR = 0, 1, 2, 3, 4
HDR = 64  # bytes of a case frame


def fold(s):
    s = np.asarray(s, dtype=np.uint64)
    s = (s & 0xFFFF) + (s >> 16)
    return (s & 0xFFFF) + (s >> 16)


def header_sums(region, frames_len, offs):
    """(is IPv4, folded sum of bytes [14, 34)) of the frames at @offs in the
    first @frames_len bytes of @region, zero-padded."""
    region = np.asarray(region, dtype=np.uint8)[:frames_len]
    pad = np.concatenate([region, np.zeros(HDR, dtype=np.uint8)])
    o = np.minimum(np.asarray(offs, dtype=np.uint64), np.uint64(frames_len)).astype(np.int64)
    h = pad[o[:, None] + np.arange(12, 34)[None, :]].astype(np.uint64)
    is_ip = (h[:, 0] == 0x08) & (h[:, 1] == 0x00)
    words = h[:, 2::2] | h[:, 3::2] << 8  # ten little-endian u16
    return is_ip, fold(words.sum(axis=1))


def expected(region, frames_len, offs, flags):
    """(olflags_out u8[n], counts u64[4]) of the definition; @flags is the
    entry flag of every packet (an array, or the default as a scalar)."""
    n = len(offs)
    fl = np.broadcast_to(np.asarray(flags, dtype=np.uint8), (n,))
    if n == 0:
        return np.zeros(0, np.uint8), np.zeros(NR, np.uint64)
    is_ip, s = header_sums(region, frames_len, offs)
    checked = is_ip & ((fl & MASK) != GOOD)
    good = checked & (s == 0xFFFF)
    out = np.where(checked, (fl & ~np.uint8(MASK)) | np.where(good, GOOD, BAD).astype(np.uint8), fl)
    counts = np.array([checked.sum(), good.sum(), (checked & ~good).sum(), (~checked).sum()],
                      dtype=np.uint64)
    return out.astype(np.uint8), counts


def set_checksum(f, span=20):
    """Make the checksum field (frame bytes 24-25) of frame @f valid for the
    @span header bytes from byte 14 (20: what the rule looks at)."""
    f[24:26] = 0
    w = f[14:14 + span].astype(np.uint64)
    s = int(fold((w[0::2] << 8 | w[1::2]).sum()))
    c = ~s & 0xFFFF
    f[24], f[25] = c >> 8, c & 0xFF
    return f


def ipv4_frame(rng, ihl=5):
    f = rng.integers(0, 256, size=HDR, dtype=np.uint8)
    f[12], f[13] = 0x08, 0x00
    f[14] = 0x40 | ihl
    return f


def header_set(seed=3400):
    """(frames u8[m, 64], kinds): the header set a-f of the tests.  kinds[i]
    is 'good', 'bad' or 'skip': what the rule says of frame i when it is
    checked ('skip': not IPv4 whatever the flags)."""
    rng = np.random.default_rng(seed)
    frames, kinds = [], []

    def add(f, kind):
        frames.append(np.array(f, dtype=np.uint8))
        kinds.append(kind)

    for _ in range(33):                                  # a. valid random headers (odd total)
        add(set_checksum(ipv4_frame(rng)), "good")
    one = set_checksum(ipv4_frame(rng))
    for bit in range(160):                               # b. every single-bit flip of one
        f = one.copy()
        f[14 + bit // 8] ^= 1 << (bit % 8)
        add(f, "bad")
    for bit in range(16):                                # c. ... of bytes 12-13: not IPv4
        f = one.copy()
        f[12 + bit // 8] ^= 1 << (bit % 8)
        add(f, "skip")
    for _ in range(16):                                  # d. changes outside [12, 34)
        f = one.copy()
        f[0:12] = rng.integers(0, 256, size=12)
        f[34:64] = rng.integers(0, 256, size=30)
        add(f, "good")
    f = np.zeros(HDR, dtype=np.uint8)                    # e. carries
    f[12] = 0x08
    g = f.copy()
    g[14:34] = 0xFF
    add(g, "good")                                       # all 0xFF: folds to 0xFFFF
    add(f, "bad")                                        # all zero: 0x0000, not 0xFFFF
    for k in range(8):
        f = np.zeros(HDR, dtype=np.uint8)
        f[12] = 0x08
        words = np.where(rng.random(10) < 0.7, 0xFFFF, 0x0001)
        if k == 0:
            words[:] = 0xFFFF
        f[14:34:2], f[15:34:2] = words >> 8, words & 0xFF
        add(set_checksum(f), "good")
        h = f.copy()
        h[33] ^= 0x01
        add(h, "bad")
    # f. options, the whole header valid (bytes past the 64-B frame read 0)
    for ihl in range(6, 16):
        f = ipv4_frame(rng, ihl)
        while True:
            set_checksum(f, span=min(4 * ihl, HDR - 14))
            _, s = header_sums(f, HDR, [0])
            if s[0] != 0xFFFF:
                break
            f[34] ^= 0x55                                # 20-byte sum valid by chance: change an option
        add(f, "bad")
    return np.stack(frames), kinds


def entry_flags(rng, n):
    """Every value of the low nibble in turn, a random high nibble."""
    return ((np.arange(n) % 16) | rng.integers(0, 16, size=n) << 4).astype(np.uint8)
