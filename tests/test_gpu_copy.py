"""GPU: gcl_copy_batch (include/gclassify.h), the loopback frame copy of
copy_batch.  Every case compares the ENTIRE destination tensor (pre-filled
with 0x5A, 64 guard bytes on both sides), pkt_len, olflags, rss (each with a
64-element canary tail) and the counts for exact equality with the numpy
definition (tests/copycases.py); torch only holds buffers.  The last case runs
copy_batch -> classify -> plan -> plan_pack and delivers the records."""
import ctypes
import functools

import numpy as np
import pytest

from tests.copycases import (FILL, GUARD, NR, SIZES, dense_case, edge_cases, expected, grid_case,
                             ingress_case, mixed_case)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# the binding's new names, imported directly (torch's HIP runtime is loaded
# first, as everywhere in the suite)
from caladan_amd.gclassify import COPY_NR, GclCopyIn, GclCopyOut, copy_batch_host  # noqa: E402

EINVAL = 22
CANARY = 64
assert COPY_NR == NR


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


def dev(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


# a case and its expected results are computed once and shared, unchanged
@functools.lru_cache(maxsize=None)
def built(kind, arg=None):
    case = {"grid": grid_case, "dense": dense_case, "ingress": ingress_case, "mixed": mixed_case,
            "edge": lambda name: edge_cases()[name]}[kind](*(() if arg is None else (arg,)))
    return case, expected(case)


class Dev:
    """A case's inputs on the device; the source @src_shift bytes into its
    tensor."""

    def __init__(self, case, src_shift=0):
        self.n = len(case["len"])
        host = case["src"] if len(case["src"]) else np.zeros(1, dtype=np.uint8)
        self.sbuf = torch.zeros(len(host) + 16, dtype=torch.uint8, device="cuda")
        self.src = self.sbuf[src_shift:src_shift + len(host)]
        self.src.copy_(torch.from_numpy(host))
        self.src_off, self.len = dev(case["src_off"]), dev(case["len"])
        self.dst_off = dev(case["dst_off"]) if case["dst_off"] is not None else None
        self.txf = dev(case["tx_olflags"]) if case["tx_olflags"] is not None else None
        self.hash = dev(case["hash"]) if case["hash"] is not None else None


def run(clf, case, d=None, group=0, len_hint=0, counts=True, base_shift=0, src_shift=0, stream=None,
        flags=True, hashes=True, olflags=None, rss=None, src=None):
    """One gcl_copy_batch; returns (the destination with its guards, pkt_len
    u16, olflags u8, rss u32 with their canary tails, counts u64[NR] or None)."""
    d = d or Dev(case, src_shift)
    n, dlen = d.n, case["dst_len"]
    buf = torch.full((dlen + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda")
    dst = buf[GUARD + base_shift:GUARD + base_shift + dlen]
    pl = torch.full((n + CANARY,), 0x5A5A, dtype=torch.int16, device="cuda")
    ol = torch.full((n + CANARY,), 0x5A, dtype=torch.uint8, device="cuda") if olflags is None else olflags
    rs = torch.full((n + CANARY,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if rss is None else rss
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda") if counts else None
    if stream is not None:
        torch.cuda.synchronize()
    got = clf.copy_batch(d.src if src is None else src, d.src_off, d.len, n, dst, dst_off=d.dst_off,
                         dst_stride=case["dst_stride"], tx_olflags=d.txf if flags else None,
                         hash=d.hash if hashes else None, src_len=case["src_len"], dst_len=dlen,
                         dst_cap=case["dst_cap"], len_hint=len_hint, group=group, counts=cnt,
                         pkt_len=pl, olflags=ol, rss=rs, stream=stream)
    assert got[0] is pl
    torch.cuda.synchronize()
    return (buf.cpu().numpy(), pl.cpu().numpy().view(np.uint16),
            ol.cpu().numpy() if ol is not False else None,
            rs.cpu().numpy().view(np.uint32) if rs is not False else None,
            cnt.cpu().numpy().view(np.uint64) if counts else None)


def check(clf, case, want, what, base_shift=0, **kw):
    wdst, wpl, wol, wrs, wcnt = want
    n, dlen = len(case["len"]), case["dst_len"]
    buf, pl, ol, rs, cnt = run(clf, case, base_shift=base_shift, **kw)
    whole = np.full(len(buf), FILL, dtype=np.uint8)
    whole[GUARD + base_shift:GUARD + base_shift + dlen] = wdst
    bad = np.nonzero(buf != whole)[0]
    assert not len(bad), f"{what}: {len(bad)} bytes of the destination tensor differ, first at " \
                         f"{bad[0] - GUARD - base_shift}: {buf[bad[0]]:#x} != {whole[bad[0]]:#x}"
    assert (pl[:n] == wpl).all(), what
    assert (pl[n:] == 0x5A5A).all(), f"{what}: written past pkt_len[n]"
    if ol is not None:
        assert (ol[:n] == (wol if kw.get("flags", True) else 0x08)).all(), what
        assert (ol[n:] == 0x5A).all(), f"{what}: written past olflags[n]"
    if rs is not None:
        assert (rs[:n] == (wrs if kw.get("hashes", True) else 0)).all(), what
        assert (rs[n:] == 0x5A5A5A5A).all(), f"{what}: written past rss[n]"
    if cnt is not None:
        assert cnt.tolist() == wcnt.tolist() and cnt[0] + cnt[1] == n, what
    return wcnt


@pytest.mark.parametrize("group", [4, 16, 64])
def test_length_alignment_grid(clf, group):
    """Every length x source alignment x destination alignment and a 65535-B
    packet, destinations back to back: a one-byte overrun hits a neighbour."""
    case, want = built("grid")
    cnt = check(clf, case, want, f"grid G={group}", group=group)
    assert cnt[0] > 26 * 49 and cnt[1] == 0


@pytest.mark.parametrize("n", SIZES)
def test_dense_slots_and_ingress_geometry(clf, n):
    for kind in ("dense", "ingress"):
        case, want = built(kind, n)
        for group in (4, 16, 64):
            check(clf, case, want, f"{kind} n={n} G={group}", group=group)


def test_every_block_loops_with_a_ragged_last_pass(g, clf):
    """The launch caps its grid and loops: the smallest n at which every block
    of the 4-lane kernel makes a second pass, the last one over one packet."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_block = g.COPY_THREADS // 4
    n = (2 * cus * g.COPY_BLOCKS_PER_CU - 1) * per_block + 1
    assert n <= 1 << 18
    case = dense_case(n)
    check(clf, case, expected(case), f"loop n={n}", group=4)


@pytest.mark.parametrize("name", sorted(edge_cases()))
def test_source_and_destination_edges(clf, name):
    """tests/copycases.py: source offsets in [0, 16), frames ending at and
    crossing src_len, offsets at and far past it, src_len < 16, a source
    tensor longer than src_len; d + L at dst_len and one past, d = dst_len
    with L = 0, d = UINT64_MAX, L > dst_cap, L > dst_stride; refused and
    copied packets interleaved."""
    case, want = built("edge", name)
    for group in (4, 16, 64):
        for src_shift in (0, 5):
            cnt = check(clf, case, want, f"{name} G={group} src+{src_shift}", group=group,
                        src_shift=src_shift)
    assert cnt[0] > 0
    if "src_len" not in name and "source" not in name:
        assert cnt[1] > 0


def test_optional_arrays_counts_and_default_group(clf):
    case, want = built("mixed")
    d = Dev(case)
    for flags in (True, False):
        for hashes in (True, False):
            check(clf, case, want, f"tx_olflags {flags} hash {hashes}", d=d, flags=flags, hashes=hashes)
    check(clf, case, want, "no olflags, no rss", d=d, olflags=False, rss=False)
    check(clf, case, want, "counts NULL", d=d, counts=False)
    for hint in (0, 64, 1500, 9000):
        check(clf, case, want, f"len_hint {hint}", d=d, len_hint=hint)
    # allocated by the binding, and two calls into the same counts
    dst = torch.full((case["dst_len"],), FILL, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda")
    pl, ol, rs = clf.copy_batch(d.src, d.src_off, d.len, d.n, dst, dst_off=d.dst_off, tx_olflags=d.txf,
                                hash=d.hash, counts=cnt)
    clf.copy_batch(d.src, d.src_off, d.len, d.n, dst, dst_off=d.dst_off, counts=cnt)
    torch.cuda.synchronize()
    assert (pl.dtype, ol.dtype, rs.dtype) == (torch.int16, torch.uint8, torch.int32)
    assert pl.numel() == ol.numel() == rs.numel() == d.n
    assert (dst.cpu().numpy() == want[0]).all()
    assert (pl.cpu().numpy().view(np.uint16) == want[1]).all() and (ol.cpu().numpy() == want[2]).all()
    assert (rs.cpu().numpy().view(np.uint32) == want[3]).all()
    assert cnt.cpu().numpy().view(np.uint64).tolist() == (2 * want[4]).tolist()


def test_stream_shifted_bases_and_n_zero(clf):
    case, want = built("mixed")
    d = Dev(case)
    check(clf, case, want, "non-default stream", d=d, stream=torch.cuda.Stream().cuda_stream)
    for shift in (1, 4, 7, 8, 15):
        for group in (4, 64):
            check(clf, case, want, f"dst + {shift}, src + {16 - shift} G={group}", base_shift=shift,
                  src_shift=16 - shift, group=group)
    # n == 0 touches nothing
    cnt = torch.full((NR,), 7, dtype=torch.int64, device="cuda")
    dst = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    pl = torch.full((CANARY,), 0x5A5A, dtype=torch.int16, device="cuda")
    clf.copy_batch(d.src, d.src_off, d.len, 0, dst, dst_stride=64, counts=cnt, pkt_len=pl)
    torch.cuda.synchronize()
    assert (dst == FILL).all() and (pl == 0x5A5A).all() and (cnt == 7).all()


def test_error_returns(g, clf):
    lib = g.lib
    n = 1000
    src = torch.zeros(n * 64 + 16, dtype=torch.uint8, device="cuda")
    dst = torch.full((n * 64,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.arange(n, dtype=torch.int64, device="cuda") * 64
    ln = torch.full((n + 1,), 64, dtype=torch.int16, device="cuda")
    pl = torch.full((n + 1,), 0x5A5A, dtype=torch.int16, device="cuda")
    aux = torch.zeros(n + 2, dtype=torch.int64, device="cuda")
    cnt = torch.full((NR + 1,), 7, dtype=torch.int64, device="cuda")

    def call(ctx=clf._ctx, size=ctypes.sizeof(GclCopyIn), group=0, s=src.data_ptr(), src_len=n * 64,
             so=off.data_ptr(), le=ln.data_ptr(), h=None, nn=n, d=dst.data_ptr(), dst_len=n * 64,
             doff=None, stride=64, p=pl.data_ptr(), r=None, c=cnt.data_ptr(), cin=True, cout=True):
        i = GclCopyIn(size=size, group=group, src=s, src_len=src_len, src_off=so, len=le, hash=h, n=nn)
        o = GclCopyOut(dst=d, dst_len=dst_len, dst_off=doff, dst_stride=stride, pkt_len=p, rss=r)
        return lib.gcl_copy_batch(ctx, ctypes.byref(i) if cin else None,
                                  ctypes.byref(o) if cout else None, c, None)

    assert call(ctx=None) == -EINVAL and call(cin=False) == -EINVAL and call(cout=False) == -EINVAL
    assert call(size=ctypes.sizeof(GclCopyIn) - 8) == -EINVAL and call(size=0) == -EINVAL
    for kw in ({"s": None}, {"so": None}, {"le": None}, {"d": None}, {"p": None}):
        assert call(**kw) == -EINVAL, kw
    assert call(src_len=(1 << 64) - 1) == -EINVAL and call(dst_len=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1) == -EINVAL
    for stride in (0, 8, 15, 24, 72, (1 << 20) + 16):
        assert call(stride=stride) == -EINVAL, stride
    for group in (1, 2, 8, 32, 63, 65, 128):
        assert call(group=group) == -EINVAL, group
    a = aux.data_ptr()
    for kw in ({"so": a + 4}, {"le": ln.data_ptr() + 1}, {"h": a + 2}, {"doff": a + 1}, {"p": pl.data_ptr() + 1},
               {"r": a + 1}, {"c": cnt.data_ptr() + 4}):
        assert call(**kw) == -EINVAL, kw
    torch.cuda.synchronize()
    assert (dst == FILL).all() and (pl == 0x5A5A).all() and (cnt == 7).all()  # nothing was launched
    # a stride is not looked at when offsets are given; n == 0 needs no array;
    # the source and the destination may have any alignment
    assert call(stride=3, doff=off.data_ptr()) == 0
    assert call(nn=0, s=None, d=None) == 0
    assert call(s=src.data_ptr() + 3, nn=1, stride=1 << 20) == 0
    torch.cuda.synchronize()
    assert cnt.cpu().numpy()[:NR].tolist() == [7 + n + 1, 7, 7 + 64 * (n + 1), 7]
    with pytest.raises(ValueError):
        clf.copy_batch(src, off, ln, n + 2, dst, dst_stride=64)
    with pytest.raises(ValueError):
        clf.copy_batch(src, off, ln, n, dst, dst_stride=64, pkt_len=pl[:n - 1])
    with pytest.raises(ValueError):
        clf.copy_batch(src, off, ln, n, dst, dst_stride=64, dst_len=n * 64 + 1)
    with pytest.raises(ValueError):
        clf.copy_batch(src, off, ln, n, dst, dst_stride=64, counts=cnt[:3])


def test_pinned_host_source_read_in_place(g, clf):
    """The runtime's tx region read in place: src in host memory registered
    with gcl_host_register, 257 packets of mixed lengths."""
    case, want = built("mixed")
    assert len(case["len"]) >= 257
    host = np.ascontiguousarray(case["src"]).copy()
    g.host_register(host)
    try:
        for group in (4, 16, 64):
            check(clf, case, want, f"registered host source G={group}", src=host, group=group)
    finally:
        g.host_unregister(host)


def test_copy_classify_plan_pack_deliver_end_to_end(g):
    """A mixed batch of loopback and NIC packets: copy_batch places the
    loopback frames into their slots of a pool that already holds the NIC
    frames; classify with dst_hint and the returned olflags, rss and pkt_len
    gives the verdicts and counters of the same classify over a pool assembled
    on the host; plan -> plan_pack -> gcl_host_deliver_packed delivers records
    whose cmd says CHECKSUM_TYPE_UNNECESSARY with the copied length for every
    loopback packet."""
    from tests.packcases import deliver_packed
    from tests.plancases import PLAN_BY_RUNTIME, World
    from tests.test_gpu_plan import _traffic, make_clf
    from tests.rxcases import apply_runtimes
    vb, R, tb, slot = 2, 16, 8, 128
    rts, (frames, flen, offs, olf, rss, fdir, hint) = _traffic(R, 4)
    n = len(offs)
    rng = np.random.default_rng(77)
    offs = offs.astype(np.uint64)
    lb = (rng.random(n) < 0.4) & (offs + np.uint64(slot) <= np.uint64(flen))
    idx = np.nonzero(lb)[0]
    m = len(idx)
    assert 1000 < m < n - 1000
    # the tx region: the loopback frames in slots of their own order, at any alignment
    lens = rng.integers(60, slot + 1, size=m).astype(np.uint16)
    tx_off = (rng.permutation(m) * 160 + rng.integers(0, 16, size=m)).astype(np.uint64)
    tx = rng.integers(0, 256, size=m * 160 + 64, dtype=np.uint8)
    for j, i in enumerate(idx):
        tx[int(tx_off[j]):int(tx_off[j]) + slot] = frames[int(offs[i]):int(offs[i]) + slot]
    txf = rng.integers(0, 256, size=m, dtype=np.uint8)
    txh = rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32)
    # the pool before the copy: NIC frames in place, loopback slots not yet written
    pool = frames.copy()
    for i in idx:
        pool[int(offs[i]):int(offs[i]) + slot] = FILL
    hint = np.where(lb, hint, 0).astype(np.uint32)
    plen = rng.integers(60, 1515, size=n).astype(np.uint16)

    # on the host, with numpy and the host form
    hpool = pool.copy()
    hpl, hol, hrs = copy_batch_host(tx, tx_off, lens, hpool, dst_off=offs[idx], tx_olflags=txf, hash=txh,
                                    dst_len=flen, dst_cap=slot)
    want_pool = pool.copy()
    for j, i in enumerate(idx):
        want_pool[int(offs[i]):int(offs[i]) + int(lens[j])] = tx[int(tx_off[j]):int(tx_off[j]) + int(lens[j])]
    assert (hpool == want_pool).all() and (hpl == lens).all()
    h_olf, h_rss, h_plen = olf.copy(), rss.copy(), plen.copy()
    h_olf[idx], h_rss[idx], h_plen[idx] = hol, hrs, hpl

    clf = make_clf(g, vb, R, tb)
    apply_runtimes(clf, rts)

    def classify(d_pool, d_olf, d_rss):
        v = torch.zeros(n * vb, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(R, dtype=torch.int64, device="cuda")
        st = torch.zeros(g.NR_STATS, dtype=torch.int64, device="cuda")
        clf.classify(d_pool, n, 0, verdicts=v, counts=cnt, stats=st, offs=dev(offs), olflags=d_olf,
                     rss=d_rss, fdir_hi=dev(fdir.astype(np.uint32)), frames_len=flen, dst_hint=dev(hint))
        torch.cuda.synchronize()
        return v, cnt.cpu().numpy(), st.cpu().numpy()

    v_want, c_want, s_want = classify(dev(want_pool), dev(h_olf), dev(h_rss))

    d_pool, d_idx = dev(pool), dev(idx.astype(np.int64))
    ccnt = torch.zeros(NR, dtype=torch.int64, device="cuda")
    pl, ol, rs = clf.copy_batch(dev(tx), dev(tx_off), dev(lens), m, d_pool, dst_off=dev(offs[idx]),
                                tx_olflags=dev(txf), hash=dev(txh), dst_len=flen, dst_cap=slot,
                                len_hint=slot, counts=ccnt)
    d_olf, d_rss, d_plen = dev(olf), dev(rss), dev(plen)
    d_olf[d_idx], d_rss[d_idx], d_plen[d_idx] = ol, rs, pl
    v, c, s = classify(d_pool, d_olf, d_rss)
    assert (d_pool.cpu().numpy() == want_pool).all()
    assert ccnt.cpu().numpy().tolist() == [m, 0, int(lens.sum()), 0]
    assert (v.cpu().numpy() == v_want.cpu().numpy()).all() and (c == c_want).all() and (s == s_want).all()
    assert (d_plen.cpu().numpy().view(np.uint16) == h_plen).all()

    order, off = clf.plan(v, n, key=PLAN_BY_RUNTIME)
    shm = 0x7F12_3456_7000
    recs = clf.plan_pack(v, n, order, pkt_len=d_plen, olflags=d_olf, offs=dev(offs), shm_base=shm)
    torch.cuda.synchronize()
    cmd, payload, v4 = (recs[0].cpu().numpy().view(np.uint64)[:n], recs[1].cpu().numpy().view(np.uint64)[:n],
                        recs[2].cpu().numpy().view(np.uint32)[:n])
    order, off = order.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint32)
    looped = lb[order]
    assert looped.sum() == m
    assert ((cmd[looped] >> np.uint64(48)) & np.uint64(1) == 1).all()  # CHECKSUM_TYPE_UNNECESSARY
    assert ((cmd[looped] >> np.uint64(16)) & np.uint64(0xFFFF) == h_plen[order][looped]).all()
    assert (payload[looped] == offs[order][looped] + np.uint64(shm)).all()

    # the rings: an in-order pass over the merged metadata, and the packed records
    vh = v.cpu().numpy()
    meta = (h_rss, h_plen, h_olf, offs + np.uint64(shm))
    a, b = World(g, rts, R, 1024, "wake_self"), World(g, rts, R, 1024, "wake_self")
    da = a.deliver(vh, vb, tb, meta, n=n)
    for bkt in range(R + 1):
        sl = slice(off[bkt], off[bkt + 1])
        deliver_packed(b, (cmd[sl], payload[sl], v4[sl]), order[sl], n, bcast_hash=meta[0])
    assert b.delivered == da and da > 1000
    msgs = b.ring_msgs()
    assert a.ring_msgs() == msgs
    sent = [(int(c_), int(p_)) for ring in msgs.values() for c_, p_ in ring]
    lb_len = {int(o) + shm: int(ln) for o, ln in zip(offs[idx], lens)}
    lb_sent = [(c_, p_) for c_, p_ in sent if p_ in lb_len]
    assert len(lb_sent) > 100
    assert all(c_ >> 48 & 1 and (c_ >> 16) & 0xFFFF == lb_len[p_] for c_, p_ in lb_sent)
    clf.close()
