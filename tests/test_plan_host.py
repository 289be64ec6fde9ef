"""gcl_host_deliver_idx (include/gcl_host.h), no GPU: the post-pass over a
delivery plan's index lists leaves the rings, counters and callbacks of the
in-order passes gcl_host_deliver{,4,2,1} -- over a whole batch, and list by
list per runtime (the lists built with numpy's stable argsort, as gcl_plan
defines them)."""
import numpy as np
import pytest

from tests.plancases import PLAN_BY_RUNTIME, World, plan_expected, plan_keys

R, NRT, TB, N = 16, 12, 3, 5000  # 16 runtimes x 8 queues: every width, the 1-byte one too


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def _batch(orc, seed, azure, all_active=False):
    """Oracle verdicts of a fuzz_batch of N packets in all four widths, and
    the per-packet metadata of the post-pass."""
    from tests.rxcases import fuzz_batch, random_runtimes, to_verdict1, to_verdict2, to_verdict4
    rng = np.random.default_rng(seed)
    rts = random_runtimes(rng, R, NRT, max_threads=6)
    if all_active:
        for r in rts:
            if r["active"] == 0:
                r["active"], r["active_idx"] = 1, [0]
                r["flow_tbl"] = orc.steer_flows(r["thread_count"], [0])
    frames, flen, offs, olf, rss, fdir, _ = fuzz_batch(rng, N, rts, R, tail_runts=False)
    t = orc.Tables(R, 0, 0x1 if azure else 0, 0x09)  # NIC hash
    for r in rts:
        assert t.runtime_set(r["uniqid"], r["ip"], r["thread_count"], r["active"], r["flow_tbl"]) == 0
    v, _, _ = t.classify(frames, N, 0, offs=offs, olflags=olf, rss=rss, fdir_hi=fdir, frames_len=flen)
    tc = {r["uniqid"]: r["thread_count"] for r in rts}
    verd = {8: v, 4: to_verdict4(v), 2: to_verdict2(v, tc, TB), 1: to_verdict1(v, tc, TB)}
    pkt_len = rng.integers(60, 1515, size=N).astype(np.uint16)
    meta = (rss.astype(np.uint32), pkt_len, olf, offs.astype(np.uint64))
    return rts, verd, meta


@pytest.fixture(scope="module")
def azure_batch(orc):
    return _batch(orc, 31, azure=True)


@pytest.fixture(scope="module")
def plain_batch(orc):
    return _batch(orc, 32, azure=False)


@pytest.fixture(scope="module")
def active_batch(orc):
    return _batch(orc, 33, azure=False, all_active=True)


@pytest.mark.parametrize("vb", [8, 4, 2, 1])
def test_whole_batch_equals_in_order_pass(g, azure_batch, vb):
    """idx = arange(n): the same rings, counters, return value and callbacks
    (in the same order, with the same packet indices) as the in-order pass,
    wakes, broadcasts and ARP responses included."""
    rts, verd, meta = azure_batch
    act = verd[8]["action"] & 0x3F
    assert (act == g.ACT_WAKE).any() and (act == g.ACT_BROADCAST).any()
    a, b = World(g, rts, R, 8), World(g, rts, R, 8)
    da = a.deliver(verd[vb], vb, TB, meta, n=N)
    db = b.deliver(verd[vb], vb, TB, meta, idx=np.arange(N))
    assert da == db and da > 0
    assert a.stats.tolist() == b.stats.tolist() and a.stats[g.STAT_NAMES.index("RX_UNICAST_FAIL")] > 0
    assert a.events == b.events
    assert {"wake", "own", "poll", "free", "ref", "arp"} <= {e[0] for e in a.events}
    assert a.ring_msgs() == b.ring_msgs()


def _per_runtime(g, rts, verd, meta, vb, ring_size, add_core):
    """One in-order pass against the per-runtime lists delivered one after
    another, the host bucket last (no Azure ARP in these batches: the host
    bucket puts nothing into a ring)."""
    keys, nb = plan_keys(verd[vb], vb, PLAN_BY_RUNTIME, R, TB)
    order, off = plan_expected(keys, nb)
    a, b = World(g, rts, R, ring_size, add_core), World(g, rts, R, ring_size, add_core)
    da = a.deliver(verd[vb], vb, TB, meta, n=N)
    for bkt in range(nb):
        b.deliver(verd[vb], vb, TB, meta, idx=order[off[bkt]:off[bkt + 1]])
    assert b.delivered == da and da > 0
    assert a.stats.tolist() == b.stats.tolist()
    ra, rb = a.ring_msgs(), b.ring_msgs()
    assert ra == rb
    assert sum(len(m) for m in ra.values()) == da
    # the callbacks are the same ones, regrouped by runtime
    assert sorted(a.events) == sorted(b.events)
    for u in a.procs:  # ... and in the same order within one runtime
        own = [e for e in a.events if e[0] in ("own", "poll", "wake") and e[1] == u]
        assert own == [e for e in b.events if e[0] in ("own", "poll", "wake") and e[1] == u]
    return a


@pytest.mark.parametrize("vb", [8, 4, 2, 1])
def test_per_runtime_lists_all_active(g, active_batch, vb):
    rts, verd, meta = active_batch
    a = _per_runtime(g, rts, verd, meta, vb, 64, "wake_self")
    assert not any(e[0] == "wake" for e in a.events)


@pytest.mark.parametrize("vb", [8, 4, 2, 1])
def test_per_runtime_lists_idle_runtimes_no_add_core(g, plain_batch, vb):
    """Runtimes with zero active threads and no sched_add_core: their packets
    go to the idle kthread's ring (rx.c:62-72), list by list as in order."""
    rts, verd, meta = plain_batch
    assert any(r["active"] == 0 for r in rts)
    assert ((verd[8]["action"] & 0x3F) == g.ACT_WAKE).any()
    _per_runtime(g, rts, verd, meta, vb, 64, None)


@pytest.mark.parametrize("vb", [8, 4, 2, 1])
def test_per_runtime_lists_add_core_wakes_own_runtime(g, plain_batch, vb):
    """A sched_add_core that activates a kthread of the woken runtime only
    (inside the guarantee): the later packets of that runtime follow the new
    flow_tbl in both passes."""
    rts, verd, meta = plain_batch
    a = _per_runtime(g, rts, verd, meta, vb, 64, "wake_self")
    assert any(e[0] == "wake" for e in a.events)


@pytest.mark.parametrize("vb", [8, 4, 2, 1])
def test_per_runtime_lists_ring_full(g, plain_batch, vb):
    """Rings of 4 slots fill: RX_UNICAST_FAIL (and the frees that go with it)
    is counted list by list as the in-order pass counts it."""
    rts, verd, meta = plain_batch
    a = _per_runtime(g, rts, verd, meta, vb, 4, "wake_self")
    assert a.stats[g.STAT_NAMES.index("RX_UNICAST_FAIL")] > 100


@pytest.mark.parametrize("vb", [8, 4, 2, 1])
def test_empty_list_and_bad_width(g, plain_batch, vb):
    rts, verd, meta = plain_batch
    w = World(g, rts, R, 8)
    assert w.deliver(verd[vb], vb, TB, meta, idx=np.zeros(0, dtype=np.uint32)) == 0
    assert not w.events and not w.stats.any()
    assert all(not m for m in w.ring_msgs().values())
    # a width that is none of 1, 2, 4, 8, and thread_bits past the width's range
    for bad_vb, tb in ((3, TB), (0, TB), (16, TB), (2, 9), (1, 8)):
        assert w.deliver(verd[vb], bad_vb, tb, meta, idx=np.arange(64)) == 0
    assert not w.events and not w.stats.any()
    assert all(not m for m in w.ring_msgs().values())
