"""GPU: gcl_l4_csum (include/gclassify.h), the TCP/UDP checksum offload of a
batch.  Every case compares status (with a canary tail), counts and the ENTIRE
frame tensor (64 guard bytes on both sides) for exact equality with the host
twin gcl_l4_csum_host, which tests/test_l4_host.py holds to the numpy
definition (tests/l4cases.py); torch only holds buffers."""
import ctypes
import functools

import numpy as np
import pytest

from tests import l4cases as lc
from tests.l4cases import BAD, FILL, FILLED_IP, FILLED_L4, GOOD, NA, NONE, NR, TCP, VERIFY

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from caladan_amd.gclassify import GclBatch, GclL4In, L4C_NR, l4_csum_host  # noqa: E402

EINVAL = 22
CANARY = 64
assert L4C_NR == NR


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


@functools.lru_cache(maxsize=None)
def twin(name, mode, tx=True):
    """(case, status, counts, frames after) by the host twin, computed once."""
    case = CASES[name]()
    case = case[0] if isinstance(case, tuple) else case
    fr = case["frames"][:case["frames_len"]].copy()
    counts = np.zeros(NR, dtype=np.uint64)
    st = l4_csum_host(fr, case["pkt_len"], mode=mode, stride=case["stride"], offs=case["offs"],
                      n=len(case["pkt_len"]), tx_olflags=case["tx_olflags"] if tx else None, counts=counts)
    return case, st[:len(case["pkt_len"])], counts, fr


CASES = {"grid": lc.grid_case, "stride_grid": lc.stride_grid_case, "dense64": lc.dense64_case,
         "mtu": lc.mtu_case, "ingress": lc.ingress_case, "na": lc.na_case, "edge": lc.edge_case,
         "mix": lc.mix_case}


class Dev:
    """A case's per-packet arrays on the device."""

    def __init__(self, case):
        self.n = len(case["pkt_len"])
        self.offs = dev(case["offs"]) if case["offs"] is not None else None
        self.plen = dev(case["pkt_len"])
        self.txf = dev(case["tx_olflags"]) if case["tx_olflags"] is not None else None


def run(clf, case, mode, d=None, shift=0, tx=True, counts=True, stream=None, **kw):
    """One gcl_l4_csum over the case's region @shift bytes into a guarded
    tensor; (the whole tensor, status with its canary tail, counts or None)."""
    d = d or Dev(case)
    flen = case["frames_len"]
    host = np.full(flen + 2 * lc.GUARD + 16, lc.FILLBYTE, dtype=np.uint8)
    host[lc.GUARD + shift:lc.GUARD + shift + flen] = case["frames"][:flen]
    buf = torch.from_numpy(host).cuda()
    st = torch.full((d.n + CANARY,), 0x77, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda") if counts else None
    if stream is not None:
        torch.cuda.synchronize()
    got = clf.l4_csum(buf[lc.GUARD + shift:lc.GUARD + shift + flen], d.n, d.plen, mode=mode,
                      stride=case["stride"], offs=d.offs, tx_olflags=d.txf if tx else None, status=st,
                      counts=cnt, stream=stream, **kw)
    assert got is st
    torch.cuda.synchronize()
    return buf.cpu().numpy(), st.cpu().numpy(), cnt.cpu().numpy().view(np.uint64) if counts else None


def check(clf, name, mode, what, shift=0, tx=True, **kw):
    case, wst, wcnt, wfr = twin(name, mode, tx)
    n, flen = len(wst), case["frames_len"]
    buf, st, cnt = run(clf, case, mode, shift=shift, tx=tx, **kw)
    bad = np.nonzero(st[:n] != wst)[0]
    assert not len(bad), f"{what}: status of packet {bad[0]}: {st[bad[0]]:#x} != {wst[bad[0]]:#x}"
    assert (st[n:] == 0x77).all(), f"{what}: written past status[n]"
    whole = np.full(len(buf), lc.FILLBYTE, dtype=np.uint8)
    whole[lc.GUARD + shift:lc.GUARD + shift + flen] = wfr
    bad = np.nonzero(buf != whole)[0]
    assert not len(bad), f"{what}: {len(bad)} bytes of the frame tensor differ, first at " \
                         f"{bad[0] - lc.GUARD - shift}: {buf[bad[0]]:#x} != {whole[bad[0]]:#x}"
    if cnt is not None:
        assert cnt.tolist() == wcnt.tolist() and int(cnt[:4].sum()) == n, what
    return wst, wcnt


@pytest.mark.parametrize("group", [4, 16, 64])
def test_length_alignment_grid_and_large_datagrams(clf, group):
    """Every l4len x alignment back to back, then 1460-, 8960- and 65 501-byte
    datagrams; the all-0xFF maximal ones are the accumulator test."""
    for mode in (VERIFY, FILL):
        wst, wcnt = check(clf, "grid", mode, f"grid G={group} mode {mode}", group=group)
    v = twin("grid", VERIFY)[1]
    assert (v == GOOD).sum() > 1800 and (v == BAD).sum() > 900 and (v == NONE).sum() > 400
    assert v[-2] == GOOD and v[-1] == GOOD  # the 0xFF datagrams at an odd address
    assert wcnt[lc.C_FILLED_L4] > 1800 and wcnt[lc.C_BYTES] > 3 * lc.MAX_L4


@pytest.mark.parametrize("name", ["dense64", "mtu", "ingress", "stride_grid"])
def test_slot_geometries(clf, name):
    for group in (4, 16, 64):
        for mode in (VERIFY, FILL):
            check(clf, name, mode, f"{name} G={group} mode {mode}", group=group)


def test_every_block_loops_with_a_ragged_last_pass(g, clf):
    """The launch caps its grid and loops: with one block per CU, the smallest
    n at which every block of the 4-lane kernel makes a second pass, the last
    one over one packet."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per_block = g.L4_THREADS // 4
    n = (2 * cus - 1) * per_block + 1
    assert n <= 1 << 16
    CASES[f"loop{n}"] = lambda: lc.tiled_dense64_case(n)
    clf.tune(blocks_per_cu=1)
    try:
        for mode in (VERIFY, FILL):
            check(clf, f"loop{n}", mode, f"loop n={n} mode {mode}", group=4)
    finally:
        clf.tune()


def test_region_edges_and_na_reasons(clf):
    """Frames ending exactly at frames_len and cut by it, the region's first
    and last 16 bytes, offsets at and past frames_len; one packet per NA
    reason."""
    for name in ("edge", "na"):
        for group in (4, 16, 64):
            for shift in (0, 1, 9):
                for mode in (VERIFY, FILL):
                    check(clf, name, mode, f"{name} G={group} base + {shift} mode {mode}", group=group,
                          shift=shift)


def test_shifted_bases_stream_and_n_zero(clf):
    case = twin("mix", VERIFY)[0]
    d = Dev(case)
    for shift in range(1, 16):
        check(clf, "mix", FILL if shift & 1 else VERIFY, f"base + {shift}", d=d, shift=shift,
              group=(4, 16, 64)[shift % 3])
    check(clf, "mix", FILL, "non-default stream", d=d, stream=torch.cuda.Stream().cuda_stream)
    check(clf, "mix", FILL, "no tx_olflags", d=d, tx=False)
    check(clf, "mix", VERIFY, "no counts", d=d, counts=False)
    for hint in (0, 64, 1500, 9000):
        check(clf, "mix", VERIFY, f"len_hint {hint}", d=d, len_hint=hint)
    # n == 0 touches nothing
    fr = torch.full((4096,), lc.FILLBYTE, dtype=torch.uint8, device="cuda")
    st = torch.full((CANARY,), 0x77, dtype=torch.uint8, device="cuda")
    cnt = torch.full((NR,), 7, dtype=torch.int64, device="cuda")
    clf.l4_csum(fr, 0, d.plen, mode=FILL, stride=64, status=st, counts=cnt)
    torch.cuda.synchronize()
    assert (fr == lc.FILLBYTE).all() and (st == 0x77).all() and (cnt == 7).all()


def test_random_mix_gpu_twin_and_model_agree(clf):
    """The constructed mix: the shares are asserted on the numpy model's
    output, so a kernel that answers NA too often cannot pass by vacuity."""
    case, kinds = lc.mix_case()
    n = len(kinds)
    mv, mf = lc.model(case, VERIFY), lc.model(case, FILL)
    eligible = mv[0] != NA
    assert eligible.sum() >= 0.6 * n
    assert (mv[0] == GOOD).sum() >= 0.2 * eligible.sum() and (mv[0] == BAD).sum() >= 0.2 * eligible.sum()
    assert (mv[0] == NONE).sum() > 0
    assert set(lc.NA_REASONS) <= set(kinds)
    assert all(mv[0][i] == NA for i, kd in enumerate(kinds) if kd in lc.NA_REASONS)
    for mode, m in ((VERIFY, mv), (FILL, mf)):
        _, wst, wcnt, wfr = twin("mix", mode)
        assert (wst == m[0]).all() and wcnt.tolist() == m[1].tolist()
        assert (wfr == m[2][:case["frames_len"]]).all()
        for group in (0, 4, 16, 64):
            check(clf, "mix", mode, f"mix G={group} mode {mode}", group=group)
    # two calls into the same counts; status allocated by the binding
    d = Dev(case)
    fr = dev(case["frames"][:case["frames_len"]])
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda")
    st = clf.l4_csum(fr, n, d.plen, offs=d.offs, counts=cnt)
    clf.l4_csum(fr, n, d.plen, offs=d.offs, counts=cnt)
    torch.cuda.synchronize()
    assert st.dtype == torch.uint8 and st.numel() == n and (st.cpu().numpy() == mv[0]).all()
    assert cnt.cpu().numpy().view(np.uint64).tolist() == (2 * mv[1]).tolist()


def test_copy_fill_verify_classify_end_to_end(g, clf):
    """Loopback TCP frames as the runtime emits them, the TCP field holding
    only the pseudo-header sum: copy_batch into the rx pool, FILL over the
    pool, VERIFY says GOOD for every packet, and classify's verdicts are what
    they were before the fill."""
    rng = np.random.default_rng(51)
    n, slot = 2000, 1536
    frs = []
    for i in range(n):
        f = lc.frame(rng, TCP, int(rng.integers(20, 1461)))
        l4len = len(f) - 34
        ph = np.concatenate([f[26:34], np.array([0, TCP, l4len >> 8, l4len & 0xFF], dtype=np.uint8)])
        v = lc.fold(lc.words(ph))
        f[50], f[51] = v & 0xFF, v >> 8
        frs.append(f)
    tx = lc.layout(frs, aligns=[int(a) for a in rng.integers(0, 16, size=n)])
    pool = torch.full((n * slot,), lc.FILLBYTE, dtype=torch.uint8, device="cuda")
    pl, ol, rs = clf.copy_batch(dev(tx["frames"]), dev(tx["offs"]), dev(tx["pkt_len"]), n, pool,
                                dst_stride=slot, len_hint=1500)

    def classify():
        v = torch.zeros(n * clf.vbytes, dtype=torch.uint8, device="cuda")
        clf.classify(pool, n, slot, verdicts=v, olflags=ol, rss=rs)
        torch.cuda.synchronize()
        return v.cpu().numpy()

    before = classify()
    st0 = clf.l4_csum(pool, n, pl, mode=VERIFY, stride=slot, len_hint=1500)
    cnt = torch.zeros(NR, dtype=torch.int64, device="cuda")
    stf = clf.l4_csum(pool, n, pl, mode=FILL, stride=slot, len_hint=1500, counts=cnt)
    st1 = clf.l4_csum(pool, n, pl, mode=VERIFY, stride=slot, len_hint=1500, counts=cnt)
    torch.cuda.synchronize()
    assert (st0.cpu().numpy()[:n] == BAD).sum() >= n - 1  # a payload that sums to 0 apart
    assert (stf.cpu().numpy()[:n] == FILLED_IP | FILLED_L4).all()
    assert (st1.cpu().numpy()[:n] == GOOD).all()
    c = cnt.cpu().numpy().view(np.uint64)
    total = int(tx["pkt_len"].astype(np.int64).sum()) - 34 * n
    assert c.tolist() == [n, 0, 0, n, n, n, 2 * total, 0]
    assert (classify() == before).all()
    # and the pool is the twin's fill of the copied frames
    want = np.full(n * slot, lc.FILLBYTE, dtype=np.uint8)
    for i, f in enumerate(frs):
        want[i * slot:i * slot + len(f)] = f
    l4_csum_host(want, tx["pkt_len"], mode=FILL, stride=slot)
    assert (pool.cpu().numpy() == want).all()


def test_error_returns(g, clf):
    lib, n = g.lib, 1000
    fr = torch.full((n * 64,), lc.FILLBYTE, dtype=torch.uint8, device="cuda")
    pl = torch.full((n + 1,), 64, dtype=torch.int16, device="cuda")
    st = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    cnt = torch.full((NR,), 7, dtype=torch.int64, device="cuda")
    size = ctypes.sizeof(GclL4In)

    def call(ctx=clf._ctx, frames=fr.data_ptr(), flen=n * 64, stride=64, p=pl.data_ptr(), nn=n, sz=size,
             mode=0, group=0, s=st.data_ptr(), bb=True, ii=True):
        b = GclBatch(frames=frames, frames_len=flen, stride=stride, pkt_len=p, n=nn)
        i = GclL4In(size=sz, mode=mode, group=group)
        return lib.gcl_l4_csum(ctx, ctypes.byref(b) if bb else None, ctypes.byref(i) if ii else None, s,
                               cnt.data_ptr(), None)

    assert call(ctx=None) == -EINVAL and call(bb=False) == -EINVAL and call(ii=False) == -EINVAL
    assert call(s=None) == -EINVAL
    assert call(sz=size - 8) == -EINVAL and call(sz=0) == -EINVAL
    assert call(mode=2) == -EINVAL and call(mode=0xFFFFFFFF) == -EINVAL
    for group in (1, 2, 8, 32, 63, 65, 128):
        assert call(group=group) == -EINVAL, group
    assert call(p=None) == -EINVAL and call(p=pl.data_ptr() + 1) == -EINVAL
    assert call(frames=None) == -EINVAL and call(flen=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1) == -EINVAL
    for stride in (0, 8, 15, 24, 72, (1 << 20) + 16):
        assert call(stride=stride) == -EINVAL, stride
    torch.cuda.synchronize()
    assert (fr == lc.FILLBYTE).all() and (st == 0x77).all() and (cnt == 7).all()  # nothing was launched
    assert call(nn=0, frames=None, p=None) == 0
    assert call(mode=1) == 0
    torch.cuda.synchronize()
    assert (st == NA).all() and cnt.cpu().numpy().tolist() == [7, 7, 7, 7 + n, 7, 7, 7, 7]
    with pytest.raises(ValueError):
        clf.l4_csum(fr, n + 2, pl, stride=64)
    with pytest.raises(ValueError):
        clf.l4_csum(fr, n, None, stride=64)
    with pytest.raises(ValueError):
        clf.l4_csum(fr, n, pl, stride=64, status=st[:n - 1])
    with pytest.raises(ValueError):
        clf.l4_csum(fr, n, pl, stride=64, frames_len=n * 64 + 1)
    with pytest.raises(ValueError):
        clf.l4_csum(fr, n, pl, stride=64, counts=cnt[:3])
