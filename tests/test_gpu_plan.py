"""GPU: gcl_plan (include/gclassify.h), the stable partition of a classified
batch by runtime or by flow-table queue.  Every case compares order and
bucket_off for exact equality with the definition: the stable argsort of the
keys and the cumulative bucket counts (tests/plancases.py)."""
import ctypes
import functools

import numpy as np
import pytest

from tests.plancases import PLAN_BY_QUEUE, PLAN_BY_RUNTIME, World, plan_expected, plan_keys
from tests.rxcases import apply_runtimes, fuzz_batch, random_runtimes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = 22
NPKT = 5000
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097, 70001)
BLOCKS = (1, 2, 7, 333, 0)

# (verdict bytes, max_runtimes, thread_bits): thread_bits at 0 and at the
# width's maximum for that many runtimes; 17 .. 16385 buckets
CONFIGS = [(8, 16, 0), (8, 4096, 0), (4, 16, 0), (4, 4096, 0),
           (2, 16, 8), (2, 16, 0), (2, 4096, 2), (2, 4096, 0),
           (1, 16, 3), (1, 16, 0)]
CASES = [(vb, R, tb, key) for vb, R, tb in CONFIGS
         for key in ((PLAN_BY_RUNTIME, PLAN_BY_QUEUE) if vb <= 2 else (PLAN_BY_RUNTIME,))]


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    return gclassify


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_clf(g, vb, R, tb):
    flag = {8: 0, 4: g.CFG_VERDICT4, 2: g.CFG_VERDICT2, 1: g.CFG_VERDICT1}[vb]
    return g.Classifier(0, R, g.HASH_NIC, flag, 0x09, thread_bits=tb)


@functools.lru_cache(maxsize=None)
def _traffic(R, max_threads):
    rng = np.random.default_rng(4200 + R + max_threads)
    rts = random_runtimes(rng, R, min(R, 300) if R > 16 else 12, max_threads=max_threads)
    return rts, fuzz_batch(rng, NPKT, rts, R)


@functools.lru_cache(maxsize=None)
def _classified(vb, R, tb):
    """(classifier, runtimes, the batch's verdict bytes as the GPU wrote them)"""
    from caladan_amd import gclassify as g
    rts, (frames, flen, offs, olf, rss, fdir, _) = _traffic(R, 1 if vb <= 2 and tb == 0 else 4)
    clf = make_clf(g, vb, R, tb)
    apply_runtimes(clf, rts)
    v = torch.zeros(NPKT * vb, dtype=torch.uint8, device="cuda")
    clf.classify(dev(frames), NPKT, 0, verdicts=v, offs=dev(offs.astype(np.int64)), olflags=dev(olf),
                 rss=dev(rss.view(np.int32)), fdir_hi=dev(fdir.astype(np.int32)), frames_len=flen)
    torch.cuda.synchronize()
    return clf, rts, v.cpu().numpy()


def run_plan(clf, vbytes_host, n, key, blocks, canary=0):
    """Plan the first @n verdicts of @vbytes_host (raw bytes); returns
    (order, bucket_off) as numpy u32, @canary extra elements included."""
    nb = clf.plan_buckets(key)
    v = dev(vbytes_host[:max(n, 1) * clf.vbytes])
    order = torch.full((n + canary,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    off = torch.full((nb + 1 + canary,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    clf.plan(v, n, key=key, order=order, bucket_off=off, blocks=blocks)
    torch.cuda.synchronize()
    return order.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint32)


def check(clf, vbytes_host, n, key, blocks, want=None, canary=0):
    nbytes = n * clf.vbytes
    if want is None:
        keys, nb = plan_keys(vbytes_host[:nbytes], clf.vbytes, key, clf.max_runtimes, clf.thread_bits)
        assert nb == clf.plan_buckets(key)
        want = plan_expected(keys, nb)
    order, off = run_plan(clf, vbytes_host, n, key, blocks, canary)
    what = f"vb={clf.vbytes} R={clf.max_runtimes} tb={clf.thread_bits} key={key} n={n} blocks={blocks}"
    nb = len(want[1]) - 1
    assert (off[:nb + 1] == want[1]).all(), what
    bad = np.nonzero(order[:n] != want[0])[0]
    assert not len(bad), f"{what}: {len(bad)} positions differ, first at {bad[0]}"
    if canary:
        assert (order[n:] == 0xA5A5A5A5).all() and (off[nb + 1:] == 0xA5A5A5A5).all(), what
    return want


@pytest.mark.parametrize("vb,R,tb,key", CASES)
def test_plan_of_classified_batch(g, vb, R, tb, key):
    """Verdicts of a real classify of a fuzz batch (every action, WAKEs,
    unknown destinations), at every size and every forced range count: ragged
    last ranges, ranges shorter than a wave, more ranges than packets."""
    clf, rts, v = _classified(vb, R, tb)
    keys, nb = plan_keys(v, vb, key, R, tb)
    assert len(np.unique(keys)) > 4 and (keys == nb - 1).any()
    big = np.resize(v.reshape(-1, vb), (max(SIZES), vb)).reshape(-1)
    for n in SIZES:
        want = None
        for blocks in BLOCKS:
            want = check(clf, big, n, key, blocks, want)


def synth(vb, tb, uniq):
    """Verdict bytes steering packet i to runtime uniq[i] (slot 0), or to the
    host bucket (DROP_UNREG) where uniq[i] < 0."""
    uniq = np.asarray(uniq, dtype=np.int64)
    hostb = uniq < 0
    if vb >= 4:
        w = np.where(hostb, 0xFFFF | 0xFF << 16 | 3 << 24, uniq).astype(np.uint32)
        if vb == 4:
            return w.view(np.uint8)
        out = np.zeros((len(uniq), 2), dtype=np.uint32)
        out[:, 0], out[:, 1] = 0x12345678, w
        return out.reshape(-1).view(np.uint8)
    if vb == 2:
        return np.where(hostb, 0xC000 | 3, uniq << tb).astype(np.uint16).view(np.uint8)
    return np.where(hostb, 0x80 | 3, uniq << tb).astype(np.uint8)


@pytest.mark.parametrize("vb,R,tb", [(8, 16, 0), (4, 4096, 0), (2, 4096, 2), (2, 16, 8), (1, 16, 3)])
def test_plan_skew(g, vb, R, tb):
    """Every packet in one runtime, every packet in the host bucket, two
    alternating keys, keys only in the first and in the last real bucket."""
    clf = make_clf(g, vb, R, tb)
    n = 20011
    i = np.arange(n)
    rng = np.random.default_rng(5)
    pats = {"one": np.full(n, R // 2), "host": np.full(n, -1),
            "alternating": np.where(i & 1, R - 2, 3), "ends": np.where(rng.random(n) < 0.5, 0, R - 1)}
    for name, uniq in pats.items():
        v = synth(vb, tb, uniq)
        for key in (PLAN_BY_RUNTIME, PLAN_BY_QUEUE) if vb <= 2 else (PLAN_BY_RUNTIME,):
            keys, nb = plan_keys(v, vb, key, R, tb)
            want_keys = np.where(uniq < 0, nb - 1, uniq << (tb if key == PLAN_BY_QUEUE else 0))
            assert (keys == want_keys).all(), name
            want = None
            for blocks in (0, 7):
                want = check(clf, v, n, key, blocks, want)
    clf.close()


@pytest.mark.parametrize("vb,R,tb,key", CASES)
def test_plan_garbage_verdicts(g, vb, R, tb, key):
    """Uniformly random bytes as verdicts: the definition with its clamp, and
    nothing written past order[n] or bucket_off[nbuckets + 1]."""
    clf = _classified(vb, R, tb)[0]
    rng = np.random.default_rng(900 + vb + R + tb + key)
    for n in (257, 30011):
        v = rng.integers(0, 256, size=n * vb, dtype=np.uint8)
        for blocks in (0, 5):
            check(clf, v, n, key, blocks, canary=64)


def test_plan_workspace_reuse(g):
    """A workspace full of 0xFF gives the same result, and two calls back to
    back on one stream with the same workspace both come out right."""
    clf, rts, v = _classified(2, 4096, 2)
    big = np.resize(v.reshape(-1, 2), (70001, 2)).reshape(-1)
    check(clf, big, 70001, PLAN_BY_QUEUE, 0)
    ws = clf._plan_ws
    ws.fill_(0xFF)
    check(clf, big, 70001, PLAN_BY_QUEUE, 0)
    assert clf._plan_ws is ws
    ws.fill_(0xFF)
    va, vb_ = dev(big), dev(big[::-1].copy())
    oa, fa = clf.plan(va, 70001, key=PLAN_BY_QUEUE)
    ob, fb = clf.plan(vb_, 70001, key=PLAN_BY_RUNTIME)  # no synchronisation in between
    torch.cuda.synchronize()
    assert clf._plan_ws is ws
    for (o, f), (vv, key) in (((oa, fa), (big, PLAN_BY_QUEUE)), ((ob, fb), (big[::-1], PLAN_BY_RUNTIME))):
        keys, nb = plan_keys(np.ascontiguousarray(vv), 2, key, 4096, 2)
        wo, wf = plan_expected(keys, nb)
        assert (f.cpu().numpy().view(np.uint32) == wf).all()
        assert (o.cpu().numpy().view(np.uint32) == wo).all()


def test_plan_error_returns(g):
    lib = g.lib
    clf8 = make_clf(g, 8, 16, 0)
    clf1 = _classified(1, 16, 3)[0]
    nb = ctypes.c_uint32()
    assert lib.gcl_plan_buckets(clf8._ctx, PLAN_BY_RUNTIME, ctypes.byref(nb)) == 0 and nb.value == 17
    assert lib.gcl_plan_buckets(clf8._ctx, PLAN_BY_QUEUE, ctypes.byref(nb)) == -EINVAL
    assert lib.gcl_plan_buckets(clf8._ctx, 2, ctypes.byref(nb)) == -EINVAL
    assert lib.gcl_plan_buckets(clf1._ctx, PLAN_BY_QUEUE, ctypes.byref(nb)) == 0 and nb.value == 129

    n = 1000
    v = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    order = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    off = torch.full((18,), 7, dtype=torch.int32, device="cuda")
    out = g.GclPlanOut(order=order.data_ptr(), bucket_off=off.data_ptr())
    cfg = g.GclPlanCfg(size=ctypes.sizeof(g.GclPlanCfg), key=PLAN_BY_RUNTIME)
    need = ctypes.c_size_t()
    assert lib.gcl_plan_workspace(clf8._ctx, ctypes.byref(cfg), n, ctypes.byref(need)) == 0
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")

    def plan(c=cfg, nn=n, o=out, w=ws.data_ptr(), wb=need.value, vv=v.data_ptr()):
        return lib.gcl_plan(clf8._ctx, ctypes.byref(c) if c else None, vv, nn,
                            ctypes.byref(o) if o else None, w, wb, None)

    assert plan() == 0
    assert plan(wb=need.value - 1) == -EINVAL            # a workspace one byte short
    assert plan(nn=(1 << 31) + 1) == -EINVAL
    assert lib.gcl_plan_workspace(clf8._ctx, ctypes.byref(cfg), (1 << 31) + 1,
                                  ctypes.byref(need)) == -EINVAL
    for size in (0, 12, 20):                             # a wrong cfg.size
        assert plan(c=g.GclPlanCfg(size=size, key=PLAN_BY_RUNTIME)) == -EINVAL
    assert plan(c=g.GclPlanCfg(size=16, key=PLAN_BY_QUEUE)) == -EINVAL  # wide verdicts
    assert plan(c=g.GclPlanCfg(size=16, key=7)) == -EINVAL
    assert plan(c=None) == -EINVAL and plan(o=None) == -EINVAL
    assert plan(o=g.GclPlanOut(order=None, bucket_off=off.data_ptr())) == -EINVAL
    assert plan(o=g.GclPlanOut(order=order.data_ptr(), bucket_off=None)) == -EINVAL
    assert plan(w=None) == -EINVAL and plan(vv=None) == -EINVAL
    torch.cuda.synchronize()
    assert (off.cpu().numpy() == [0] + [n] * 17).all()  # all-zero verdicts: DELIVER to runtime 0
    # n == 0 zeroes bucket_off and needs neither verdicts nor a workspace
    off.fill_(7)
    assert plan(nn=0, w=None, wb=0, vv=None) == 0
    torch.cuda.synchronize()
    assert (off.cpu().numpy() == 0).all()
    clf8.close()


def test_classify_plan_deliver_end_to_end(g):
    """classify -> plan BY_RUNTIME -> gcl_host_deliver_idx per bucket leaves
    the rings of gcl_host_deliver1 over the same batch."""
    clf, rts, v = _classified(1, 16, 3)
    rng = np.random.default_rng(77)
    offs = _traffic(16, 4)[1][2]
    meta = (rng.integers(0, 2**32, size=NPKT, dtype=np.uint64).astype(np.uint32),
            rng.integers(60, 1515, size=NPKT).astype(np.uint16),
            rng.integers(0, 16, size=NPKT, dtype=np.uint8), offs.astype(np.uint64))
    order, off = clf.plan(dev(v), NPKT, key=PLAN_BY_RUNTIME)
    torch.cuda.synchronize()
    order, off = order.cpu().numpy().view(np.uint32), off.cpu().numpy().view(np.uint32)
    a, b = World(g, rts, 16, 1024), World(g, rts, 16, 1024)  # rings that hold the whole batch
    da = a.deliver(v, 1, 3, meta, n=NPKT)
    assert off[-1] == NPKT and len(off) == 18
    for bkt in range(17):
        b.deliver(v, 1, 3, meta, idx=order[off[bkt]:off[bkt + 1]])
    assert b.delivered == da and da > 1000
    assert a.stats.tolist() == b.stats.tolist()
    assert a.ring_msgs() == b.ring_msgs()
