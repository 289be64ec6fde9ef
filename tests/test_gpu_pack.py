"""GPU: gcl_plan_pack (include/gclassify.h), the packed delivery records of a
plan's index lists.  Every case compares cmd, payload and v4 for exact
equality with the numpy definition (tests/packcases.py); the last one feeds
the records to gcl_host_deliver_packed and compares the rings with an
in-order pass."""
import ctypes
import itertools

import numpy as np
import pytest

from tests.packcases import NO_VERDICT, deliver_packed, pack_expected
from tests.plancases import PLAN_BY_RUNTIME, World

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = 22
NMAX = 70001
SIZES = (1, 2, 63, 64, 65, 127, 129, 255, 257, 4097, NMAX)
CONFIGS = [(8, 16, 0), (4, 4096, 0), (2, 16, 8), (2, 4096, 2), (1, 16, 3)]
SHM_BASE = 0x7F12_3456_7000
CANARY = 64

_rng = np.random.default_rng(8600)
PKT_LEN = _rng.integers(0, 65536, size=NMAX).astype(np.uint16)
OLFLAGS = _rng.integers(0, 16, size=NMAX, dtype=np.uint8)
OFFS = _rng.integers(0, 1 << 40, size=NMAX, dtype=np.uint64)


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


def host(cmd, payload, v4, m):
    torch.cuda.synchronize()
    return (cmd.cpu().numpy().view(np.uint64)[:m], payload.cpu().numpy().view(np.uint64)[:m],
            v4.cpu().numpy().view(np.uint32)[:m])


def classified(vb, R, tb):
    """(classifier, runtimes, verdict bytes of a real classify of a fuzz
    batch), shared with tests/test_gpu_plan.py."""
    from tests.test_gpu_plan import _classified
    return _classified(vb, R, tb)


def big_verdicts(vb, R, tb):
    clf, rts, v = classified(vb, R, tb)
    return clf, np.resize(v.reshape(-1, vb), (NMAX, vb)).reshape(-1)


def same(got, want, what):
    for name, a, b in zip(("cmd", "payload", "v4"), got, want):
        bad = np.nonzero(a != b)[0]
        assert not len(bad), f"{what}: {name} differs at {len(bad)} positions, first {bad[0]}: " \
                             f"{a[bad[0]]:#x} != {b[bad[0]]:#x}"


@pytest.mark.parametrize("vb,R,tb", CONFIGS)
def test_pack_against_definition(g, vb, R, tb):
    """classify -> plan -> pack of the whole order, at the wave, block and
    two-per-lane edges (odd m included)."""
    clf, big = big_verdicts(vb, R, tb)
    plen, olf, offs = dev(PKT_LEN), dev(OLFLAGS), dev(OFFS)
    for n in SIZES:
        v = dev(big[:n * vb])
        order, _ = clf.plan(v, n, key=PLAN_BY_RUNTIME)
        got = host(*clf.plan_pack(v, n, order, pkt_len=plen, olflags=olf, offs=offs, shm_base=SHM_BASE), n)
        o = order.cpu().numpy().view(np.uint32)
        assert (np.sort(o) == np.arange(n)).all()
        want = pack_expected(big, vb, tb, n, o, PKT_LEN, OLFLAGS, 0x09, OFFS, 0, SHM_BASE)
        same(got, want, f"vb={vb} R={R} tb={tb} n={n}")
        assert (got[2] != NO_VERDICT).any()


def test_pack_slices(g):
    """One bucket's slice of the order, passed as an offset pointer that is
    only 4-B aligned: the same records as that slice of the whole pack."""
    vb, R, tb = 1, 16, 3
    clf, big = big_verdicts(vb, R, tb)
    n = NMAX
    v, plen, olf, offs = dev(big[:n * vb]), dev(PKT_LEN), dev(OLFLAGS), dev(OFFS)
    order, off = clf.plan(v, n, key=PLAN_BY_RUNTIME)
    kw = dict(pkt_len=plen, olflags=olf, offs=offs, shm_base=SHM_BASE)
    whole = host(*clf.plan_pack(v, n, order, **kw), n)
    off = off.cpu().numpy().view(np.uint32).astype(np.int64)
    size = np.diff(off)
    full, empty, hostb = int(np.argmax(size[:R])), int(np.argmin(size[:R])), R
    assert size[full] > 1000 and size[empty] == 0 and size[hostb] > 1000
    slices = [(off[b], size[b]) for b in (full, empty, hostb)]
    slices.append((off[full] + 1, size[full] - 1))  # one of the two starts at an odd entry
    assert any(s % 2 for s, _ in slices)
    for start, m in slices:
        got = host(*clf.plan_pack(v, n, order.data_ptr() + 4 * int(start), m=int(m), **kw), int(m))
        same(got, [a[start:start + m] for a in whole], f"slice {start}+{m}")


@pytest.mark.parametrize("vb,R,tb", CONFIGS)
def test_pack_optional_inputs(g, vb, R, tb):
    """Every combination of pkt_len / olflags / offs given or not: length 0,
    the context's default_olflags (0x09: csum 1; 0x01, not GOOD: csum 0), and
    i * stride for stride 64 and 1536; shm_base above 2^32."""
    clf, big = big_verdicts(vb, R, tb)
    flag = {8: 0, 4: g.CFG_VERDICT4, 2: g.CFG_VERDICT2, 1: g.CFG_VERDICT1}[vb]
    clf_bad = g.Classifier(0, R, g.HASH_NIC, flag, 0x01, thread_bits=tb)
    n = 4097
    v, plen, olf, offs = dev(big[:n * vb]), dev(PKT_LEN), dev(OLFLAGS), dev(OFFS)
    order, _ = clf.plan(v, n, key=PLAN_BY_RUNTIME)
    o = order.cpu().numpy().view(np.uint32)
    for use_len, use_olf, use_offs in itertools.product((True, False), repeat=3):
        for c, dflt in ((clf, 0x09), (clf_bad, 0x01)):
            for stride in (64, 1536):
                got = host(*c.plan_pack(v, n, order, pkt_len=plen if use_len else None,
                                        olflags=olf if use_olf else None,
                                        offs=offs if use_offs else None, stride=stride,
                                        shm_base=SHM_BASE), n)
                want = pack_expected(big, vb, tb, n, o, PKT_LEN if use_len else None,
                                     OLFLAGS if use_olf else None, dflt,
                                     OFFS if use_offs else None, stride, SHM_BASE)
                same(got, want, f"vb={vb} len={use_len} olf={use_olf} offs={use_offs} "
                                f"default={dflt:#x} stride={stride}")
                if not use_olf:
                    assert ((got[0] >> np.uint64(48)) == (1 if dflt == 0x09 else 0)).all()
                if not use_len:
                    assert not ((got[0] >> np.uint64(16)) & np.uint64(0xFFFF)).any()
                if not use_offs:
                    assert (got[1] == np.uint64(SHM_BASE) + o.astype(np.uint64) * np.uint64(stride)).all()
    clf_bad.close()


def poisoned(a, n, poison):
    """@a[:n] followed by a poisoned tail in the same allocation."""
    buf = np.full(n + 4096 // a.dtype.itemsize, poison, dtype=a.dtype)
    buf[:n] = a[:n]
    return dev(buf)


@pytest.mark.parametrize("vb,R,tb", CONFIGS)
def test_pack_bounds(g, vb, R, tb):
    """Random u32 in order and random bytes as verdicts: entries >= n get the
    empty record, entries < n the definition, nothing is written past m and no
    record reflects what lies behind the n-th element of an input."""
    clf = classified(vb, R, tb)[0]
    rng = np.random.default_rng(990 + vb + R + tb)
    for n in (257, 30011):
        m = n + 37
        vbytes = rng.integers(0, 256, size=n * vb, dtype=np.uint8)
        order = rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32)
        inside = rng.random(m) < 0.5
        order[inside] = rng.integers(0, n, size=int(inside.sum()))
        order[1:9] = (n, n + 1, n - 1, 0, 2**32 - 1, 2**31, n + 2047, n)  # the tail's first elements
        v = poisoned(vbytes, n * vb, 0xEE)
        plen = poisoned(PKT_LEN, n, 0xFFFF)
        olf = poisoned(OLFLAGS ^ 0x08, n, 0x08)
        offs = poisoned(OFFS, n, 0xDEAD_BEEF_0000_0000)
        out = (torch.full((m + CANARY,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda"),
               torch.full((m + CANARY,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda"),
               torch.full((m + CANARY,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"))
        clf.plan_pack(v, n, dev(order), m=m, pkt_len=plen, olflags=olf, offs=offs,
                      shm_base=SHM_BASE, out=out)
        cmd, payload, v4 = host(*out, m + CANARY)
        what = f"vb={vb} R={R} tb={tb} n={n}"
        assert (cmd[m:] == 0x5A5A5A5A5A5A5A5A).all() and (payload[m:] == 0x5A5A5A5A5A5A5A5A).all() \
            and (v4[m:] == 0x5A5A5A5A).all(), what
        outside = order >= n
        assert outside.sum() > n // 4 and (~outside).sum() > n // 4
        assert not cmd[:m][outside].any() and not payload[:m][outside].any(), what
        assert (v4[:m][outside] == NO_VERDICT).all(), what
        want = pack_expected(vbytes, vb, tb, n, order, PKT_LEN, OLFLAGS ^ 0x08, 0x09, OFFS, 0, SHM_BASE)
        same((cmd[:m], payload[:m], v4[:m]), want, what)


def test_pack_error_returns(g):
    lib = g.lib
    clf = classified(4, 4096, 0)[0]
    n = m = 1000
    v = torch.zeros(n * 4, dtype=torch.uint8, device="cuda")
    order = torch.arange(m, dtype=torch.int32, device="cuda")
    cmd = torch.full((m + 2,), 7, dtype=torch.int64, device="cuda")
    payload = torch.full((m + 2,), 7, dtype=torch.int64, device="cuda")
    v4 = torch.full((m + 4,), 7, dtype=torch.int32, device="cuda")

    def call(size=ctypes.sizeof(g.GclPackIn), vv=v.data_ptr(), oo=order.data_ptr(), mm=m,
             c=cmd.data_ptr(), p=payload.data_ptr(), w=v4.data_ptr(), pin=True, pout=True):
        i = g.GclPackIn(size=size, verdicts=vv, n=n, order=oo, m=mm)
        o = g.GclPackOut(cmd=c, payload=p, v4=w)
        return lib.gcl_plan_pack(clf._ctx, ctypes.byref(i) if pin else None,
                                 ctypes.byref(o) if pout else None, None)

    assert ctypes.sizeof(g.GclPackIn) == 80 and ctypes.sizeof(g.GclPackOut) == 24
    for size in (0, 72, 88):                                    # a wrong size
        assert call(size=size) == -EINVAL
    assert call(pin=False) == -EINVAL and call(pout=False) == -EINVAL
    assert call(oo=None) == -EINVAL                             # NULL order with m > 0
    assert call(vv=None) == -EINVAL
    assert call(oo=order.data_ptr() + 2) == -EINVAL
    assert call(c=None) == -EINVAL and call(p=None) == -EINVAL and call(w=None) == -EINVAL
    assert call(c=cmd.data_ptr() + 8) == -EINVAL                # outputs are 16-B aligned
    assert call(p=payload.data_ptr() + 8) == -EINVAL
    assert call(w=v4.data_ptr() + 4) == -EINVAL and call(w=v4.data_ptr() + 8) == -EINVAL
    assert call(mm=(1 << 31) + 1) == -EINVAL
    torch.cuda.synchronize()
    assert (cmd == 7).all() and (payload == 7).all() and (v4 == 7).all()  # nothing was launched
    # m == 0: a no-op that needs no array at all
    assert call(mm=0, vv=None, oo=None, c=None, p=None, w=None) == 0
    assert call(mm=0, pout=False) == 0 and call(mm=0, size=3) == -EINVAL
    assert call() == 0
    got = host(cmd, payload, v4, m)
    # DELIVER to runtime 0, length 0, the default olflags' csum, offset 0
    assert (got[0] == 1 << 48).all() and not got[1].any() and not got[2].any()
    with pytest.raises(ValueError):
        clf.plan_pack(v, n, order, m=m + 1)
    with pytest.raises(ValueError):
        clf.plan_pack(v, n + 1, order)
    with pytest.raises(ValueError):
        clf.plan_pack(v, n, order, pkt_len=torch.zeros(n - 1, dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError):
        clf.plan_pack(v, n, order.data_ptr())


@pytest.mark.parametrize("vb,R,tb", [(2, 16, 8), (1, 16, 3)])
def test_classify_plan_pack_deliver_end_to_end(g, vb, R, tb):
    """classify -> plan -> pack -> gcl_host_deliver_packed per bucket leaves
    the rings and the counters of gcl_host_deliver2 / 1 over the batch."""
    clf, rts, v = classified(vb, R, tb)
    n = len(v) // vb
    rng = np.random.default_rng(78 + vb)
    meta = (rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32),
            PKT_LEN[:n], OLFLAGS[:n], OFFS[:n] + np.uint64(SHM_BASE))
    dv = dev(v)
    order, off = clf.plan(dv, n, key=PLAN_BY_RUNTIME)
    recs = clf.plan_pack(dv, n, order, pkt_len=dev(PKT_LEN[:n]), olflags=dev(OLFLAGS[:n]),
                         offs=dev(OFFS[:n]), shm_base=SHM_BASE)
    cmd, payload, v4 = host(*recs, n)
    order, off = order.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint32)
    a, b = World(g, rts, R, 1024, "wake_self"), World(g, rts, R, 1024, "wake_self")
    da = a.deliver(v, vb, tb, meta, n=n)
    assert off[-1] == n and len(off) == R + 2
    for bkt in range(R + 1):
        s = slice(off[bkt], off[bkt + 1])
        deliver_packed(b, (cmd[s], payload[s], v4[s]), order[s], n, bcast_hash=meta[0])
    assert b.delivered == da and da > 1000
    assert a.stats.tolist() == b.stats.tolist()
    assert a.ring_msgs() == b.ring_msgs()
    assert sorted(a.events) == sorted(b.events) and any(e[0] == "wake" for e in a.events)
