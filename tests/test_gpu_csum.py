"""GPU: gcl_rx_csum (include/gclassify.h), the IPv4 header checksum offload
of a batch.  Every case compares olflags_out and counts for exact equality
with the numpy definition (tests/csumcases.py); torch only holds buffers.
The last case runs classify -> rx_csum -> plan -> plan_pack and delivers the
records."""
import ctypes

import numpy as np
import pytest

from tests.csumcases import GOOD, HDR, MASK, NR, entry_flags, expected, header_set, set_checksum

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = 22
CANARY = 64
SIZES = (1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097)
N = 4097


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def clf(g):
    c = g.Classifier(0, 16, g.HASH_NIC, 0, 0x01)
    yield c
    c.close()


HEADERS, KINDS = header_set()


def dev(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


def slots(n, stride, seed=1):
    """@n fixed slots of @stride >= 64 bytes: the header set cycled, the rest
    of every slot random (not a header: a read in the wrong place shows)."""
    rng = np.random.default_rng(seed)
    region = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    region[:, :HDR] = HEADERS[np.arange(n) % len(HEADERS)]
    return region.reshape(-1)


def overlapped(n, stride=16, seed=2):
    """A region read at a @stride of 16: frame i is bytes [16 i, 16 i + 64),
    so neighbours share bytes.  Two frames in three are IPv4 (bytes 12-13 of
    frame i are bytes 28-29 of frame i - 1), with a valid checksum (bytes
    24-25 lie in no other frame's header) unless a bit of byte 20 is flipped."""
    rng = np.random.default_rng(seed)
    region = rng.integers(0, 256, size=(n - 1) * stride + HDR, dtype=np.uint8)
    ip = rng.random(n) < 0.67
    for i in np.nonzero(ip)[0]:
        region[i * stride + 12], region[i * stride + 13] = 0x08, 0x00
    for i in np.nonzero(ip)[0]:
        set_checksum(region[i * stride:i * stride + HDR])
    for i in np.nonzero(ip & (rng.random(n) < 0.3))[0]:
        region[i * stride + 20] ^= 0x10
    return region


def run(clf, region, n, stride=0, offs=None, flags=None, frames_len=None, counts=True,
        in_place=False, base_shift=0):
    """One gcl_rx_csum; returns (olflags_out u8[n + CANARY], counts u64[4] or
    None).  @region is the whole tensor behind frames (it may be longer than
    @frames_len); @flags an array (olflags) or None (the context's default)."""
    buf = torch.zeros(len(region) + 64, dtype=torch.uint8, device="cuda")
    fr = buf[base_shift:base_shift + len(region)]
    fr.copy_(torch.from_numpy(np.ascontiguousarray(region)))
    d_offs = dev(np.asarray(offs, dtype=np.uint64)) if offs is not None else None
    d_fl = None
    if flags is not None:
        d_fl = torch.full((n + CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
        d_fl[:n] = torch.from_numpy(np.asarray(flags, dtype=np.uint8))
    out = d_fl if in_place else torch.full((n + CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda") if counts else None
    ret = clf.rx_csum(fr, n, stride, olflags_out=out, counts=cnt, offs=d_offs,
                      olflags=d_fl[:n] if d_fl is not None else None,
                      frames_len=len(region) if frames_len is None else frames_len)
    assert ret is out
    torch.cuda.synchronize()
    return out.cpu().numpy(), (cnt.cpu().numpy().view(np.uint64) if counts else None)


def check(clf, region, n, stride=0, offs=None, flags=None, default=0x01, frames_len=None, what="",
          **kw):
    flen = len(region) if frames_len is None else frames_len
    o = np.asarray(offs, dtype=np.uint64) if offs is not None else \
        np.arange(n, dtype=np.uint64) * np.uint64(stride)
    want, wcnt = expected(region, flen, o, flags if flags is not None else default)
    got, cnt = run(clf, region, n, stride, offs, flags, frames_len, **kw)
    bad = np.nonzero(got[:n] != want)[0]
    assert not len(bad), f"{what}: {len(bad)} of {n} flags differ, first at {bad[0]}: " \
                         f"{got[bad[0]]:#x} != {want[bad[0]]:#x}"
    assert (got[n:] == 0x5A).all(), f"{what}: written past olflags_out[n]"
    if cnt is not None:
        assert cnt.tolist() == wcnt.tolist(), what
        assert cnt[0] == cnt[1] + cnt[2] and cnt[0] + cnt[3] == n, what
    return want, wcnt


@pytest.mark.parametrize("n", SIZES)
def test_dense_slots_at_the_group_wave_and_block_edges(clf, n):
    rng = np.random.default_rng(100 + n)
    _, cnt = check(clf, slots(n, 64), n, 64, flags=entry_flags(rng, n), what=f"n={n}")
    if n >= 255:
        assert cnt.min() > 0


def test_every_block_loops_with_a_ragged_last_pass(g, clf):
    """The launch caps its grid and loops: the smallest n at which every block
    makes a second pass, the last one over a single packet."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * g.CSUM_BLOCKS_PER_CU
    n = (2 * grid - 1) * g.CSUM_BLOCK_PKTS + 1
    assert n <= 1 << 20
    rng = np.random.default_rng(5)
    _, cnt = check(clf, slots(n, 64), n, 64, flags=entry_flags(rng, n), what=f"loop n={n}")
    assert cnt.min() > n // 32


@pytest.mark.parametrize("stride", [16, 64, 80, 1536])
def test_strides(clf, stride):
    rng = np.random.default_rng(stride)
    region = overlapped(N) if stride == 16 else slots(N, stride)
    for flags in (entry_flags(rng, N), None):
        _, cnt = check(clf, region, N, stride, flags=flags, what=f"stride={stride}")
        assert cnt[1] > N // 8 and cnt[2] > N // 8


def test_offsets_of_every_alignment_mixed(clf):
    """Offsets that are 0, 8, 4, 2 and 1 mod 16 in one batch, in random order
    and with repeats; also with the frames pointer itself off alignment."""
    rng = np.random.default_rng(8)
    nslots = 1500
    region = rng.integers(0, 256, size=nslots * 128, dtype=np.uint8)
    shift = np.array([0, 8, 4, 2, 1, 12, 3, 15])[np.arange(nslots) % 8] + 16 * (np.arange(nslots) % 3)
    for s in range(nslots):
        region[s * 128 + shift[s]:s * 128 + shift[s] + HDR] = HEADERS[s % len(HEADERS)]
    pick = rng.integers(0, nslots, size=N)
    offs = (pick * 128 + shift[pick]).astype(np.uint64)
    assert len(np.unique(pick)) < N and {int(o) % 16 for o in offs} >= {0, 8, 4, 2, 1}
    for base_shift in (0, 8, 4, 1):
        _, cnt = check(clf, region, N, offs=offs, flags=entry_flags(rng, N), base_shift=base_shift,
                       what=f"mixed alignments, frames + {base_shift}")
        assert cnt[1] > N // 8 and cnt[2] > N // 8


def test_reference_pool_geometry(clf):
    """9408-B mbuf elements with the frame data at element + 344 (8 mod 16)."""
    rng = np.random.default_rng(9)
    elems = 257
    region = rng.integers(0, 256, size=elems * 9408, dtype=np.uint8)
    for e in range(elems):
        region[e * 9408 + 344:e * 9408 + 344 + HDR] = HEADERS[e % len(HEADERS)]
    pick = np.concatenate([rng.permutation(elems), rng.integers(0, elems, size=N - elems)])
    offs = (pick * 9408 + 344).astype(np.uint64)
    _, cnt = check(clf, region, N, offs=offs, flags=entry_flags(rng, N), what="mbuf pool")
    assert cnt[1] > N // 8 and cnt[2] > N // 8


@pytest.mark.parametrize("flen,base_shift", [(1000, 0), (1024, 0), (1003, 4), (1000, 1)])
def test_region_edges(clf, flen, base_shift):
    """A frame at frames_len - k for every k in [0, 40] (the cut falls on
    every byte of [12, 34)), one at 0, and offsets at and past frames_len.
    The tensor behind frames goes on past frames_len with the rest of a valid
    header: a kernel that reads past frames_len marks GOOD where the
    definition says BAD."""
    rng = np.random.default_rng(flen)
    valid = HEADERS[0]
    assert KINDS[0] == "good"
    seen_cut_bad = 0
    for k in range(41):
        region = rng.integers(0, 256, size=flen + 256, dtype=np.uint8)
        region[:HDR] = valid
        region[flen - k:flen - k + HDR] = valid  # its tail lies past frames_len
        offs = np.array([flen - k, 0, flen, flen + 1, 1 << 40, 1 << 63, flen - k, 512, flen - 64,
                         flen - 65, 16, 48], dtype=np.uint64)
        flags = entry_flags(rng, len(offs)) & 0xF3  # UNKNOWN: all checked
        want, _ = check(clf, region, len(offs), offs=offs, flags=flags, frames_len=flen,
                        base_shift=base_shift, what=f"frames_len={flen} k={k}")
        assert want[1] & MASK == GOOD               # the frame at offset 0
        assert (want[0] & MASK == GOOD) == (k >= 34)
        assert (want[2:6] == flags[2:6]).all()      # frames of zeros: not IPv4
        seen_cut_bad += 14 <= k < 34
    assert seen_cut_bad == 20


def test_default_flags_in_place_and_counts(g, clf):
    region = slots(N, 64)
    rng = np.random.default_rng(12)
    # olflags == NULL with each checksum state as the context's default
    for state in (0x00, 0x04, 0x08, 0x0C):
        c = g.Classifier(0, 16, g.HASH_NIC, 0, 0xA1 | state)
        want, cnt = check(c, region, N, 64, default=0xA1 | state, what=f"default {state:#x}")
        assert (cnt[0] == 0) == (state == 0x08)
        c.close()
    flags = entry_flags(rng, N)
    want, wcnt = check(clf, region, N, 64, flags=flags, in_place=True, what="in place")
    assert (want != flags).any()
    check(clf, region, N, 64, flags=flags, counts=False, what="counts NULL")
    # an output that is not 4-B aligned
    out = torch.full((N + CANARY + 3,), 0x5A, dtype=torch.uint8, device="cuda")
    fr, fl = dev(region), dev(flags)
    for shift in (1, 2, 3):
        out.fill_(0x5A)
        clf.rx_csum(fr, N, 64, olflags_out=out[shift:], olflags=fl)
        got = out.cpu().numpy()
        assert (got[shift:shift + N] == want).all() and (got[:shift] == 0x5A).all() and \
            (got[shift + N:] == 0x5A).all(), f"out + {shift}"
    # two calls into the same counts: twice the numbers
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda")
    out = clf.rx_csum(fr, N, 64, olflags=fl, counts=cnt)
    clf.rx_csum(fr, N, 64, olflags_out=out, olflags=fl, counts=cnt)
    assert out.dtype == torch.uint8 and out.numel() == N
    assert (out.cpu().numpy() == want).all()
    assert cnt.cpu().numpy().view(np.uint64).tolist() == (2 * wcnt).tolist()
    # n == 0 touches nothing
    cnt.fill_(7)
    out = torch.full((CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
    clf.rx_csum(fr, 0, 64, olflags_out=out, olflags=fl, counts=cnt)
    torch.cuda.synchronize()
    assert (out == 0x5A).all() and (cnt == 7).all()


def test_error_returns(g, clf):
    lib = g.lib
    n = 1000
    fr = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    out = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    cnt = torch.full((NR,), 7, dtype=torch.int64, device="cuda")
    offs = torch.zeros(n, dtype=torch.int64, device="cuda")

    def call(ctx=clf._ctx, frames=fr.data_ptr(), frames_len=n * 64, stride=64, offs=None, nn=n,
             o=out.data_ptr(), batch=True):
        b = g.GclBatch(frames=frames, frames_len=frames_len, stride=stride, offs=offs, n=nn)
        return lib.gcl_rx_csum(ctx, ctypes.byref(b) if batch else None, o, cnt.data_ptr(), None)

    assert call(ctx=None) == -EINVAL and call(batch=False) == -EINVAL and call(o=None) == -EINVAL
    assert call(frames=None) == -EINVAL
    assert call(frames_len=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1) == -EINVAL
    for stride in (0, 8, 15, 24, 72, (1 << 20) + 16):
        assert call(stride=stride) == -EINVAL, stride
    torch.cuda.synchronize()
    assert (out == 0x5A).all() and (cnt == 7).all()  # nothing was launched
    # a stride is not looked at when offsets are given; n == 0 needs no array
    assert call(stride=3, offs=offs.data_ptr()) == 0
    assert call(nn=0, frames=None) == 0
    assert call(stride=1 << 20, nn=1) == 0
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == [7, 7, 7, 7 + n + 1]).all()
    with pytest.raises(ValueError):
        clf.rx_csum(fr, n + 1, 64, olflags_out=out)
    with pytest.raises(ValueError):
        clf.rx_csum(fr, n, 64, olflags=out[:n - 1])
    with pytest.raises(ValueError):
        clf.rx_csum(fr, n, 64, counts=cnt[:3])


@pytest.mark.parametrize("vb,R,tb", [(2, 16, 8), (1, 16, 3)])
def test_classify_csum_plan_pack_deliver_end_to_end(g, vb, R, tb):
    """classify -> rx_csum -> plan -> plan_pack on one fuzz batch that arrives
    without a NIC verdict on the checksum: bit 48 of cmd[j] (csum_type
    UNNECESSARY) is set exactly for the packets whose output flags are GOOD,
    and gcl_host_deliver_packed puts those cmd words in the rings."""
    from tests.packcases import deliver_packed
    from tests.plancases import PLAN_BY_RUNTIME, World
    from tests.test_gpu_plan import _classified, _traffic
    clf, rts, v = _classified(vb, R, tb)
    _, (frames, flen, offs, olf, _, _, _) = _traffic(R, 1 if vb <= 2 and tb == 0 else 4)
    n = len(v) // vb
    # the fuzz batch's IPv4 headers carry valid checksums: break a third (the TTL)
    frames = frames.copy()
    rng = np.random.default_rng(90 + vb)
    for i in np.nonzero(rng.random(n) < 0.33)[0]:
        o = int(offs[i])
        if o + 34 <= flen:
            frames[o + 22] ^= 0x04
    entry = (olf & ~np.uint8(MASK)).astype(np.uint8)  # IP_CKSUM_UNKNOWN
    want, wcnt = expected(frames, flen, offs, entry)
    assert wcnt[1] > n // 16 and wcnt[2] > n // 16 and wcnt[3] > 0

    d_offs = dev(offs.astype(np.uint64))
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda")
    flags = clf.rx_csum(dev(frames), n, 0, offs=d_offs, olflags=dev(entry), frames_len=flen, counts=cnt)
    dv = dev(v)
    order, off = clf.plan(dv, n, key=PLAN_BY_RUNTIME)
    plen = rng.integers(0, 65536, size=n).astype(np.uint16)
    shm = 0x7F12_3456_7000
    recs = clf.plan_pack(dv, n, order, pkt_len=dev(plen), olflags=flags, offs=d_offs, shm_base=shm)
    torch.cuda.synchronize()
    got = flags.cpu().numpy()
    assert (got == want).all() and cnt.cpu().numpy().view(np.uint64).tolist() == wcnt.tolist()
    cmd, payload, v4 = (recs[0].cpu().numpy().view(np.uint64)[:n], recs[1].cpu().numpy().view(np.uint64)[:n],
                        recs[2].cpu().numpy().view(np.uint32)[:n])
    order, off = order.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint32)
    unnecessary = ((cmd >> np.uint64(48)) & np.uint64(1)).astype(bool)
    assert (unnecessary == ((got[order] & MASK) == GOOD)).all()
    assert unnecessary.sum() == wcnt[1]

    # the rings: an in-order pass over the output flags, and the packed records
    meta = (rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32), plen, got,
            offs.astype(np.uint64) + np.uint64(shm))
    a, b = World(g, rts, R, 1024, "wake_self"), World(g, rts, R, 1024, "wake_self")
    da = a.deliver(v, vb, tb, meta, n=n)
    for bkt in range(R + 1):
        s = slice(off[bkt], off[bkt + 1])
        deliver_packed(b, (cmd[s], payload[s], v4[s]), order[s], n, bcast_hash=meta[0])
    assert b.delivered == da and da > 1000
    msgs = b.ring_msgs()
    assert a.ring_msgs() == msgs
    sent = [c for ring in msgs.values() for c, _ in ring]
    packed = set(int(c) for c in cmd)
    assert sent and all(c in packed for c in sent)
    assert any(c >> 48 & 1 for c in sent) and any(not (c >> 48 & 1) for c in sent)
