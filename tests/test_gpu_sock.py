"""GPU: gcl_sock_lookup (include/gclassify.h), the socket demux of a
classified batch.  Every case compares sock and counts for exact equality
with the plain-Python definition (tests/sockcases.py), with a canary after
sock[n]; torch only holds buffers.  The last case classifies the fuzz batch
of tests/test_gpu_plan.py with GCL_CFG_TRANS_HASH and pins the restated frame
predicate, and the entry a cookie names, to what the classify kernel wrote."""
import ctypes
import functools

import numpy as np
import pytest

from tests import sockcases as sc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, ENOENT, EADDRINUSE, ENOSPC = 22, 2, 98, 28
CANARY = 64
CANARY_WORD = 0x5A5A5A5A
SIZES = (1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097)
N = 4097
# (verdict bytes, max_runtimes, thread_bits)
WIDTHS = [(8, 16, 0), (4, 16, 0), (2, 16, 8), (1, 16, 3)]


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    return gclassify


def dev(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


def make_clf(g, vb, R, tb, present=None):
    flag = {8: 0, 4: g.CFG_VERDICT4, 2: g.CFG_VERDICT2, 1: g.CFG_VERDICT1}[vb]
    c = g.Classifier(0, R, g.HASH_NIC, flag, 0x09, thread_bits=tb)
    for u in range(R) if present is None else present:
        c.runtime_set(u, sc.runtime_ip(u), 1, 1, [0])
    return c


@functools.lru_cache(maxsize=None)
def world(per_rt=40, seed=77):
    """The main cases' entry sets over runtimes 0..13 of 16 (14 and 15 have
    none), their definition tables, and a pool of frames cut from them."""
    rng = np.random.default_rng(seed)
    sets = sc.random_sets(rng, range(14), per_rt)
    frames, u, _ = sc.traffic(rng, sets, 8192, range(16))
    return sets, sc.make_tables(sets), frames, u


@pytest.fixture(scope="module")
def clfs(g):
    """One context per verdict width, holding world()'s sets."""
    out = {}
    for vb, R, tb in WIDTHS:
        c = make_clf(g, vb, R, tb)
        for u, e in world()[0].items():
            c.sock_set(u, e)
        out[vb] = (c, R, tb)
    yield out
    for c, _, _ in out.values():
        c.close()


def run(clf, region, n, raw, vb, stride=0, offs=None, frames_len=None, counts=True, base_shift=0):
    """One gcl_sock_lookup; returns (sock u32[n + CANARY], counts u64[NR] or None)."""
    buf = torch.zeros(len(region) + 64, dtype=torch.uint8, device="cuda")
    fr = buf[base_shift:base_shift + len(region)]
    fr.copy_(torch.from_numpy(np.ascontiguousarray(region)))
    d_offs = dev(np.asarray(offs, dtype=np.uint64)) if offs is not None else None
    out = torch.full((n + CANARY,), CANARY_WORD, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(sc.NR, dtype=torch.int64, device="cuda") if counts else None
    ret = clf.sock_lookup(fr, n, stride, verdicts=dev(sc.pack_verdicts(raw, vb)), sock=out, counts=cnt,
                          offs=d_offs, frames_len=len(region) if frames_len is None else frames_len)
    assert ret is out
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), (cnt.cpu().numpy().view(np.uint64) if counts else None)


def check(clf, tables, region, n, raw, vb, tb, R, stride=0, offs=None, frames_len=None, what="", **kw):
    flen = len(region) if frames_len is None else frames_len
    o = np.asarray(offs, dtype=np.uint64) if offs is not None else \
        np.arange(n, dtype=np.uint64) * np.uint64(stride)
    want, wcnt = sc.expected(tables, region, flen, o, raw, vb, tb, R)
    got, cnt = run(clf, region, n, raw, vb, stride, offs, frames_len, **kw)
    bad = np.nonzero(got[:n] != want)[0]
    assert not len(bad), f"{what}: {len(bad)} of {n} differ, first at {bad[0]}: " \
                         f"{got[bad[0]]:#x} != {want[bad[0]]:#x}"
    assert (got[n:] == CANARY_WORD).all(), f"{what}: written past sock[n]"
    if cnt is not None:
        assert cnt.tolist() == wcnt.tolist(), what
        assert int(cnt.sum()) == n, what
    return want, wcnt


def slots(n, stride, seed=1):
    """@n fixed slots of @stride >= 64 bytes: world()'s frames cycled, the rest
    of every slot random; and the runtime of each packet."""
    _, _, frames, u = world()
    rng = np.random.default_rng(seed)
    region = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    pick = np.arange(n) % len(frames)
    region[:, :sc.HDR] = frames[pick]
    return region.reshape(-1), u[pick]


@pytest.mark.parametrize("vb,R,tb", WIDTHS)
@pytest.mark.parametrize("n", SIZES)
def test_dense_slots_at_the_wave_and_block_edges(clfs, n, vb, R, tb):
    clf = clfs[vb][0]
    rng = np.random.default_rng(100 + n)
    region, u = slots(n, 64)
    _, cnt = check(clf, world()[1], region, n, sc.verdicts_for(rng, u, vb, tb), vb, tb, R, 64,
                   what=f"n={n} vb={vb}")
    if n >= 4097:
        assert cnt[:sc.N_NA + 1].min() > 0, cnt  # no class vacuously right


def test_every_block_loops_with_a_ragged_last_pass(g, clfs):
    """The launch caps its grid and loops: the smallest n at which every block
    makes a second pass, the last one over a single packet."""
    clf, R, tb = clfs[1]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    grid = cus * g.SOCK_BLOCKS_PER_CU
    n = (2 * grid - 1) * g.SOCK_BLOCK_PKTS + 1
    assert n <= 1 << 20
    rng = np.random.default_rng(5)
    region, u = slots(n, 64)
    _, cnt = check(clf, world()[1], region, n, sc.verdicts_for(rng, u, 1, tb), 1, tb, R, 64,
                   what=f"loop n={n}")
    assert cnt[:sc.N_NA + 1].min() > n // 400


@pytest.mark.parametrize("stride", [16, 64, 80, 1536])
def test_strides(clfs, stride):
    clf, R, tb = clfs[4]
    rng = np.random.default_rng(stride)
    if stride == 16:  # frame i is bytes [16 i, 16 i + 64): neighbours share bytes
        _, _, frames, fu = world()
        region = rng.integers(0, 256, size=(N - 1) * 16 + sc.HDR, dtype=np.uint8)
        u = rng.integers(0, 16, size=N)
        for i in range(0, N, 4):  # a whole frame every 64 B, three overlapping reads between
            region[16 * i:16 * i + sc.HDR] = frames[i % len(frames)]
            u[i] = fu[i % len(frames)]
    else:
        region, u = slots(N, stride)
    _, cnt = check(clf, world()[1], region, N, sc.verdicts_for(rng, u, 4, tb), 4, tb, R, stride,
                   what=f"stride={stride}")
    assert cnt[sc.HIT5] > 0 and cnt[sc.HIT3] > 0 and cnt[sc.N_MISS] > 0 and cnt[sc.N_NA] > 0


def test_offsets_of_every_alignment_mixed(clfs):
    """Offsets that are 0, 8, 4, 2 and 1 mod 16 in one batch, in random order
    and with repeats; also with the frames pointer itself off alignment."""
    clf, R, tb = clfs[2]
    _, tables, frames, fu = world()
    rng = np.random.default_rng(8)
    nslots = 1500
    region = rng.integers(0, 256, size=nslots * 128, dtype=np.uint8)
    shift = np.array([0, 8, 4, 2, 1, 12, 3, 15])[np.arange(nslots) % 8] + 16 * (np.arange(nslots) % 3)
    for s in range(nslots):
        region[s * 128 + shift[s]:s * 128 + shift[s] + sc.HDR] = frames[s % len(frames)]
    pick = rng.integers(0, nslots, size=N)
    offs = (pick * 128 + shift[pick]).astype(np.uint64)
    assert len(np.unique(pick)) < N and {int(o) % 16 for o in offs} >= {0, 8, 4, 2, 1}
    raw = sc.verdicts_for(rng, fu[pick % len(frames)], 2, tb)
    for base_shift in (0, 8, 4, 1):
        _, cnt = check(clf, tables, region, N, raw, 2, tb, R, offs=offs, base_shift=base_shift,
                       what=f"mixed alignments, frames + {base_shift}")
        assert cnt[:sc.N_NA + 1].min() > 0


def test_reference_pool_geometry(clfs):
    """9408-B mbuf elements with the frame data at element + 344 (8 mod 16)."""
    clf, R, tb = clfs[1]
    _, tables, frames, fu = world()
    rng = np.random.default_rng(9)
    elems = 257
    region = rng.integers(0, 256, size=elems * 9408, dtype=np.uint8)
    for e in range(elems):
        region[e * 9408 + 344:e * 9408 + 344 + sc.HDR] = frames[e]
    pick = np.concatenate([rng.permutation(elems), rng.integers(0, elems, size=N - elems)])
    offs = (pick * 9408 + 344).astype(np.uint64)
    _, cnt = check(clf, tables, region, N, sc.verdicts_for(rng, fu[pick], 1, tb), 1, tb, R, offs=offs,
                   what="mbuf pool")
    assert cnt[sc.HIT5] > 0 and cnt[sc.HIT3] > 0 and cnt[sc.N_NA] > 0


@pytest.mark.parametrize("flen,base_shift", [(1000, 0), (1024, 0), (1003, 4), (1000, 1)])
def test_region_edges(clfs, flen, base_shift):
    """A frame at frames_len - k for every k in [0, 48] (the cut falls on
    every byte of [12, 38)), one at 0, and offsets at and past frames_len.
    The tensor behind frames goes on past frames_len with the rest of a frame
    that hits: a kernel that reads past frames_len answers its cookie where
    the definition says MISS or NA."""
    clf, R, tb = clfs[4]
    sets, tables, _, _ = world()
    rng = np.random.default_rng(flen)
    e = sets[3][sets[3]["match"] == sc.M5][0]
    f = sc.build_frames(rng, *(np.array([int(e[k])]) for k in ("proto", "lip", "lport", "rip", "rport")))[0]
    seen_cut = 0
    for k in range(49):
        region = rng.integers(0, 256, size=flen + 256, dtype=np.uint8)
        region[:sc.HDR] = f
        region[flen - k:flen - k + sc.HDR] = f  # its tail lies past frames_len
        offs = np.array([flen - k, 0, flen, flen + 1, 1 << 40, 1 << 63, flen - k, 512, flen - 64,
                         flen - 65, 16, 48], dtype=np.uint64)
        raw = np.full(len(offs), 3, dtype=np.uint64)
        want, _ = check(clf, tables, region, len(offs), raw, 4, tb, R, offs=offs, frames_len=flen,
                        base_shift=base_shift, what=f"frames_len={flen} k={k}")
        assert want[1] == e["cookie"]
        assert (want[0] == e["cookie"]) == (k >= 38), k
        assert (want[2:6] == sc.NA).all()  # frames of zeros
        seen_cut += 12 < k < 38
    assert seen_cut == 25


@pytest.mark.parametrize("vb,R,tb", WIDTHS)
def test_garbage_verdicts(clfs, vb, R, tb):
    """Random verdict bytes, uniqids at and past max_runtimes, the undefined
    2-B kind 0x8000: the definition's answer, nothing out of bounds."""
    clf = clfs[vb][0]
    rng = np.random.default_rng(40 + vb)
    region, u = slots(N, 64)
    raw = sc.garbage_verdicts(rng, N, vb)
    if vb >= 4:  # DELIVER / WAKE with every uniqid around max_runtimes
        sh = np.uint64(32 if vb == 8 else 0)
        raw[::3] = (np.arange(len(raw[::3]), dtype=np.uint64) % np.uint64(40)) << sh | \
            (raw[::3] & np.uint64(0xC1)) << (sh + np.uint64(24))
    _, cnt = check(clf, world()[1], region, N, raw, vb, tb, R, 64, what=f"garbage vb={vb}")
    assert cnt[sc.N_NA] > 0 and cnt[sc.N_NA] < N


def test_table_states_and_snapshot_semantics(g):
    """An empty table, one entry, 60 000 entries over 16 runtimes; set,
    lookup, set, lookup on one stream without a synchronise in between; then
    gcl_runtime_del and a lookup: MISS for that runtime."""
    vb, R, tb = 1, 16, 3
    clf = make_clf(g, vb, R, tb)
    rng = np.random.default_rng(60)
    big = sc.random_sets(rng, range(16), 3800)
    assert sum(len(e) for e in big.values()) >= 60000
    frames, u, _ = sc.traffic(rng, big, N, range(16))
    region = frames.reshape(-1)
    raw = sc.verdicts_for(rng, u, vb, tb)
    offs = np.arange(N, dtype=np.uint64) * 64
    fr, dv = dev(region), dev(sc.pack_verdicts(raw, vb))

    want0, cnt0 = check(clf, {}, region, N, raw, vb, tb, R, 64, what="empty table")
    assert cnt0[sc.N_MISS] > N // 2 and cnt0[:sc.N_MULTI + 1].sum() == 0
    # one entry: a listener on the port of the batch's first packet that can reach one
    i = int(np.nonzero(want0 == sc.MISS)[0][0])
    owner = int(sc.verdict_runtime(raw, vb, tb, R)[i])
    e1 = np.zeros(1, dtype=sc.ENTRY)
    e1[0] = (0, 0, int(frames[i, 36]) << 8 | int(frames[i, 37]), 0, frames[i, 23], sc.M3, 0, 4242)
    one = {owner: e1}
    clf.sock_set(owner, e1)
    want1, cnt1 = check(clf, sc.make_tables(one), region, N, raw, vb, tb, R, 64, what="one entry")
    assert want1[i] == 4242 and 0 < cnt1[sc.HIT3_ANY] < N // 8
    clf.sock_set(owner, [])

    # one stream, no synchronise between the calls: each lookup sees the sets before it
    outs = []
    for state in (big, {u_: e[:len(e) // 2] for u_, e in big.items()}, big):
        for u_, e in state.items():
            clf.sock_set(u_, e)
        outs.append((state, clf.sock_lookup(fr, N, 64, verdicts=dv)))
    clf.runtime_del(9)
    after_del = clf.sock_lookup(fr, N, 64, verdicts=dv)
    torch.cuda.synchronize()
    for state, out in outs:
        want, wcnt = sc.expected(sc.make_tables(state), region, N * 64, offs, raw, vb, tb, R)
        assert (out.cpu().numpy().view(np.uint32) == want).all()
        assert wcnt[:sc.N_NA + 1].min() > 0
    assert (outs[0][1].cpu().numpy() != outs[1][1].cpu().numpy()).any()
    # runtime 9 is gone: its verdicts still name it (uniqid < max_runtimes), its table is empty
    rest = {u_: e for u_, e in big.items() if u_ != 9}
    want, _ = sc.expected(sc.make_tables(rest), region, N * 64, offs, raw, vb, tb, R)
    got = after_del.cpu().numpy().view(np.uint32)
    assert (got == want).all()
    mine = (sc.verdict_runtime(raw, vb, tb, R) == 9) & (want != sc.NA)
    assert mine.sum() > 50 and (got[mine] == sc.MISS).all()
    # the runtime is not present any more; a set for one that never was is refused too
    for u_ in (9, R, 4095):
        with pytest.raises(OSError) as ei:
            clf.sock_set(u_, big[9])
        assert ei.value.errno == ENOENT
    clf.close()


def test_set_error_returns_keep_the_previous_set(g):
    clf = make_clf(g, 4, 16, 0, present=[2])
    ok = [(0x0A000001, 80, 6, 3, 7), (0x0A000001, 80, 6, 5, 8, 0x01020304, 99)]
    assert clf.sock_set(2, ok) == 0
    rng = np.random.default_rng(0)
    frames = sc.build_frames(rng, np.array([6, 6]), np.array([0x0A000001] * 2), np.array([80, 80]),
                             np.array([0x01020304, 5]), np.array([99, 99])).reshape(-1)
    raw = np.array([2, 2], dtype=np.uint64)
    for entries, err in (([(1, 0, 6, 3, 1)], EINVAL), ([(1, 1, 6, 4, 1)], EINVAL), ([(1, 1, 1, 3, 1)], EINVAL),
                         ([(1, 1, 6, 3, sc.COOKIE_MAX + 1)], EINVAL),
                         ([(9, 9, 17, 5, 1, 2, 3), (9, 9, 17, 5, 5, 2, 3)], EADDRINUSE)):
        with pytest.raises(OSError) as ei:
            clf.sock_set(2, entries)
        assert ei.value.errno == err
        got, _ = run(clf, frames, 2, raw, 4, 64)
        assert got[:2].tolist() == [8, 7]
    with pytest.raises(OSError) as ei:
        clf.sock_set(3, ok)  # not present
    assert ei.value.errno == ENOENT
    e = np.zeros(g.SOCK_MAX_ENTRIES + 1, dtype=sc.ENTRY)
    e["lport"], e["proto"], e["match"] = 1, 6, sc.M3
    with pytest.raises(OSError) as ei:
        clf.sock_set(2, e)
    assert ei.value.errno == ENOSPC
    assert g.lib.gcl_sock_set(None, 2, None, 0) == -EINVAL
    assert g.lib.gcl_sock_set(clf._ctx, 2, None, 1) == -EINVAL
    got, _ = run(clf, frames, 2, raw, 4, 64)
    assert got[:2].tolist() == [8, 7]
    assert clf.sock_set(2, []) == 0
    got, _ = run(clf, frames, 2, raw, 4, 64)
    assert got[:2].tolist() == [sc.MISS, sc.MISS]
    clf.close()


def test_counts_accumulate_null_counts_and_n_zero(clfs):
    clf, R, tb = clfs[2]
    rng = np.random.default_rng(12)
    region, u = slots(N, 64)
    raw = sc.verdicts_for(rng, u, 2, tb)
    want, wcnt = check(clf, world()[1], region, N, raw, 2, tb, R, 64, counts=False, what="counts NULL")
    _, wcnt = sc.expected(world()[1], region, len(region), np.arange(N, dtype=np.uint64) * 64, raw, 2, tb, R)
    fr, dv = dev(region), dev(sc.pack_verdicts(raw, 2))
    cnt = torch.zeros(sc.NR, dtype=torch.int64, device="cuda")
    out = clf.sock_lookup(fr, N, 64, verdicts=dv, counts=cnt)
    clf.sock_lookup(fr, N, 64, verdicts=dv, sock=out, counts=cnt)
    assert out.dtype == torch.int32 and out.numel() == N
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert cnt.cpu().numpy().view(np.uint64).tolist() == (2 * wcnt).tolist()
    cnt.fill_(7)
    out = torch.full((CANARY,), CANARY_WORD, dtype=torch.int32, device="cuda")
    clf.sock_lookup(fr, 0, 64, verdicts=dv, sock=out, counts=cnt)
    torch.cuda.synchronize()
    assert (out == CANARY_WORD).all() and (cnt == 7).all()


def test_error_returns(g, clfs):
    lib = g.lib
    n = 1000
    fr = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    out = torch.full((n + 1,), CANARY_WORD, dtype=torch.int32, device="cuda")
    cnt = torch.full((sc.NR,), 7, dtype=torch.int64, device="cuda")
    offs = torch.zeros(n, dtype=torch.int64, device="cuda")
    v = torch.zeros(n * 8 + 8, dtype=torch.uint8, device="cuda")

    def call(vb=4, ctx=None, frames=fr.data_ptr(), frames_len=n * 64, stride=64, offs=None, nn=n,
             vv=v.data_ptr(), o=out.data_ptr(), batch=True, null_ctx=False):
        ctx = None if null_ctx else (clfs[vb][0]._ctx if ctx is None else ctx)
        b = g.GclBatch(frames=frames, frames_len=frames_len, stride=stride, offs=offs, n=nn)
        return lib.gcl_sock_lookup(ctx, ctypes.byref(b) if batch else None, vv, o, cnt.data_ptr(), None)

    assert call(null_ctx=True) == -EINVAL and call(batch=False) == -EINVAL
    assert call(o=None) == -EINVAL and call(vv=None) == -EINVAL
    assert call(frames=None) == -EINVAL
    assert call(frames_len=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1) == -EINVAL
    for stride in (0, 8, 15, 24, 72, (1 << 20) + 16):
        assert call(stride=stride) == -EINVAL, stride
    for shift in (1, 2, 3):
        assert call(o=out.data_ptr() + shift) == -EINVAL
    for vb, shifts in ((8, (1, 2, 4)), (4, (1, 2)), (2, (1,))):
        for shift in shifts:
            assert call(vb=vb, vv=v.data_ptr() + shift) == -EINVAL, (vb, shift)
    torch.cuda.synchronize()
    assert (out == CANARY_WORD).all() and (cnt == 7).all()  # nothing was launched
    # a stride is not looked at when offsets are given; n == 0 needs no frames; 1-B verdicts at any address
    assert call(stride=3, offs=offs.data_ptr()) == 0
    assert call(nn=0, frames=None) == 0
    assert call(stride=1 << 20, nn=1) == 0
    assert call(vb=1, vv=v.data_ptr() + 1) == 0
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    assert c[sc.N_NA] == 7 + 2 * n + 1 and (c[:sc.N_NA] == 7).all()  # frames of zeros: NA
    assert out[n].item() == CANARY_WORD
    clf = clfs[4][0]
    with pytest.raises(ValueError):
        clf.sock_lookup(fr, n, 64, verdicts=v[:4 * n - 1])
    with pytest.raises(ValueError):
        clf.sock_lookup(fr, n, 64, verdicts=v, sock=out[:n - 1])
    with pytest.raises(ValueError):
        clf.sock_lookup(fr, n, 64, verdicts=v, counts=cnt[:7])
    with pytest.raises(ValueError):
        clf.sock_lookup(fr, n, 64)


def test_classify_then_sock_lookup_end_to_end(g):
    """The fuzz batch of tests/test_gpu_plan.py through an 8-byte
    GCL_CFG_TRANS_HASH context: sock is NA exactly where the classify verdict
    lacks GCL_ACT_F_TRANS or is not DELIVER / WAKE, which pins the restated
    frame predicate to the classify kernel's; and for every HIT5 / HIT3
    packet, gcl_trans_hash of the runtime's seed and the entry's key is the
    gcl_trans classify wrote: the cookie names the entry in the bucket the
    runtime itself would search."""
    from tests.rxcases import apply_runtimes
    from tests.test_gpu_plan import NPKT, _traffic
    R = 16
    rts, (frames, flen, offs, olf, rss, fdir, _) = _traffic(R, 4)
    clf = g.Classifier(0, R, g.HASH_NIC, g.CFG_TRANS_HASH, 0x09)
    apply_runtimes(clf, rts)
    seeds = {r["uniqid"]: 0x1000193 * (r["uniqid"] + 1) & 0xFFFFFFFF for r in rts}
    for u, s in seeds.items():
        clf.set_trans_seed(u, s)
    n = NPKT
    d_fr, d_offs = dev(frames), dev(offs.astype(np.uint64))
    v = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    tr = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    clf.classify(d_fr, n, 0, verdicts=v, offs=d_offs, olflags=dev(olf), rss=dev(rss.view(np.int32)),
                 fdir_hi=dev(fdir.astype(np.int32)), frames_len=flen, trans=tr)
    torch.cuda.synchronize()
    verd = v.cpu().numpy().view(g.VERDICT_DTYPE)
    trans = tr.cpu().numpy().view(g.TRANS_DTYPE)
    raw = v.cpu().numpy().view(np.uint64)
    act = verd["action"]
    seen = ((act & g.ACT_MASK) <= g.ACT_WAKE) & ((act & g.ACT_F_TRANS) != 0)
    assert 200 < seen.sum() < n - 200

    # entries from the batch's own tuples: connections for a third of the seen packets,
    # listeners for another third
    h = sc.header_bytes(frames, flen, offs).astype(np.int64)
    b = lambda i: h[:, i - 12]  # noqa: E731
    proto, lport, rport = b(23), b(36) << 8 | b(37), b(34) << 8 | b(35)
    rip = b(26) << 24 | b(27) << 16 | b(28) << 8 | b(29)
    lip = b(30) << 24 | b(31) << 16 | b(32) << 8 | b(33)
    sets = {}
    for u in seeds:
        idx = np.nonzero(seen & (verd["uniqid"] == u) & (lport != 0))[0]
        keys = {}
        for j, i in enumerate(idx):
            if j % 3 == 0:
                keys[(sc.M5, int(proto[i]), int(lip[i]), int(lport[i]), int(rip[i]), int(rport[i]))] = 0
            elif j % 3 == 1:
                keys[(sc.M3, int(proto[i]), int(lip[i]), int(lport[i]), 0, 0)] = 0
        e = np.zeros(len(keys), dtype=sc.ENTRY)
        for c, k in enumerate(keys):
            e[c] = (k[2], k[4], k[3], k[5], k[1], k[0], 0, c)  # the cookie is the entry's index
        sets[u] = e
        clf.sock_set(u, e)
    cnt = torch.zeros(sc.NR, dtype=torch.int64, device="cuda")
    sock = clf.sock_lookup(d_fr, n, 0, verdicts=v, offs=d_offs, frames_len=flen, counts=cnt)
    torch.cuda.synchronize()
    got = sock.cpu().numpy().view(np.uint32)
    want, wcnt = sc.expected(sc.make_tables(sets), frames, flen, offs, raw, 8, 0, R)
    assert (got == want).all() and cnt.cpu().numpy().view(np.uint64).tolist() == wcnt.tolist()
    assert ((got == sc.NA) == ~seen).all()
    assert wcnt[sc.HIT5] > 50 and wcnt[sc.HIT3] > 50 and wcnt[sc.N_MISS] > 50
    checked = 0
    for i in np.nonzero(seen & (got <= sc.COOKIE_MAX))[0]:
        u = int(verd["uniqid"][i])
        e = sets[u][int(got[i])]
        h5, h3 = g.trans_hash(seeds[u], int(e["proto"]), int(e["lip"]), int(e["lport"]), int(e["rip"]),
                              int(e["rport"]))
        if e["match"] == sc.M5:
            assert h5 == trans["h5"][i], i
        else:
            assert h3 == trans["h3"][i], i
        checked += 1
    assert checked == wcnt[sc.HIT5] + wcnt[sc.HIT3]
    clf.close()
