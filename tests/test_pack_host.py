"""gcl_host_deliver_packed (include/gcl_host.h), no GPU: the post-pass over a
list's packed records leaves the ring messages, callbacks, counters and return
value of gcl_host_deliver_idx over the same list.  The records are built with
numpy from the definition in include/gclassify.h (tests/packcases.py), the
lists with numpy's stable argsort as gcl_plan defines them."""
import numpy as np
import pytest

from tests.packcases import NO_VERDICT, deliver_packed, pack_expected
from tests.plancases import PLAN_BY_RUNTIME, World, plan_expected, plan_keys
from tests.test_plan_host import N, R, TB, _batch

WIDTHS = [8, 4, 2, 1]


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def azure_batch(orc):
    return _batch(orc, 31, azure=True)


@pytest.fixture(scope="module")
def plain_batch(orc):
    return _batch(orc, 32, azure=False)


def _lists(verd, vb):
    keys, nb = plan_keys(verd[vb], vb, PLAN_BY_RUNTIME, R, TB)
    order, off = plan_expected(keys, nb)
    return [order[off[b]:off[b + 1]] for b in range(nb)]


def _records(verd, vb, meta, idx):
    _, plen, olf, shm = meta
    return pack_expected(verd[vb], vb, TB, N, idx, pkt_len=plen, olflags=olf, offs=shm)


def _compare(g, rts, verd, meta, vb, ring_size, add_core="wake_self", mutate=None, host_packed=True):
    """Every list of the by-runtime plan into two worlds, one per entry point;
    everything observable must be identical, list by list."""
    a, b = World(g, rts, R, ring_size, add_core), World(g, rts, R, ring_size, add_core)
    if mutate:
        mutate(a), mutate(b)
    lists = _lists(verd, vb)
    for k, idx in enumerate(lists):
        da = a.deliver(verd[vb], vb, TB, meta, idx=idx)
        if k == len(lists) - 1 and not host_packed:
            db = b.deliver(verd[vb], vb, TB, meta, idx=idx)
        else:
            db = deliver_packed(b, _records(verd, vb, meta, idx), idx, N, bcast_hash=meta[0])
        assert da == db, (vb, k)
        assert a.events == b.events, (vb, k)
        assert a.stats.tolist() == b.stats.tolist(), (vb, k)
    assert a.delivered == b.delivered and a.delivered > 0
    ra, rb = a.ring_msgs(), b.ring_msgs()
    assert ra == rb
    return a, ra


@pytest.mark.parametrize("vb", WIDTHS)
def test_wake_with_sched_add_core(g, plain_batch, vb):
    rts, verd, meta = plain_batch
    a, msgs = _compare(g, rts, verd, meta, vb, 64)
    kinds = {e[0] for e in a.events}
    assert {"wake", "own", "poll", "free"} <= kinds
    assert sum(len(m) for m in msgs.values()) == a.delivered


@pytest.mark.parametrize("vb", WIDTHS)
def test_idle_runtimes_without_add_core(g, plain_batch, vb):
    rts, verd, meta = plain_batch
    assert any(r["active"] == 0 for r in rts)
    _compare(g, rts, verd, meta, vb, 64, add_core=None)


@pytest.mark.parametrize("vb", WIDTHS)
def test_rings_fill(g, plain_batch, vb):
    rts, verd, meta = plain_batch
    a, _ = _compare(g, rts, verd, meta, vb, 4)
    assert a.stats[g.STAT_NAMES.index("RX_UNICAST_FAIL")] > 100


@pytest.mark.parametrize("vb", WIDTHS)
def test_broadcast_and_arp_in_host_bucket(g, azure_batch, vb):
    """BROADCAST and ARP_RESPOND sit in the host bucket.  4-, 2- and 1-byte
    contexts deliver it packed (the broadcast hash is bcast_hash[idx[j]]); an
    8-byte context's host bucket stays with gcl_host_deliver_idx."""
    rts, verd, meta = azure_batch
    act = verd[8]["action"] & 0x3F
    assert (act == g.ACT_BROADCAST).any() and (act == g.ACT_ARP_RESPOND).any()
    # rings that still have room when the host bucket, the last list, is delivered
    a, _ = _compare(g, rts, verd, meta, vb, 1024, host_packed=vb != 8)
    assert {"ref", "arp", "own", "free"} <= {e[0] for e in a.events}
    assert a.stats[g.STAT_NAMES.index("RX_UNREGISTERED_MAC")] > 0


def _busiest(rts, verd, min_threads=1):
    """The uniqid with most DELIVER verdicts among runtimes of >= min_threads."""
    v = verd[8]
    ok = [r["uniqid"] for r in rts if r["thread_count"] >= min_threads and r["active"] > 0]
    cnt = {u: int(((v["uniqid"] == u) & ((v["action"] & 0x3F) == 0)).sum()) for u in ok}
    u = max(cnt, key=cnt.get)
    assert cnt[u] > 20
    return u


@pytest.mark.parametrize("vb", WIDTHS)
def test_runtime_absent_from_clients_by_id(g, plain_batch, vb):
    rts, verd, meta = plain_batch
    u = _busiest(rts, verd)

    def drop(w):
        w.by_id[u] = None

    a, msgs = _compare(g, rts, verd, meta, vb, 64, mutate=drop)
    assert a.stats[g.STAT_NAMES.index("RX_UNICAST_FAIL")] > 20
    assert not any(m for (uu, _), m in msgs.items() if uu == u)


@pytest.mark.parametrize("vb", WIDTHS)
def test_slot_at_or_above_thread_count(g, plain_batch, vb):
    """The runtime shrank to one kthread after the batch was classified: every
    verdict naming a slot >= 1 is refused like a full ring, never indexed."""
    rts, verd, meta = plain_batch
    u = _busiest(rts, verd, min_threads=3)
    assert (verd[8]["thread"][verd[8]["uniqid"] == u] >= 1).any()

    def shrink(w):
        p = w.procs[u]
        p.thread_count = 1
        p.active_thread_count = 1
        p.flow_tbl[0] = 0

    a, msgs = _compare(g, rts, verd, meta, vb, 64, mutate=shrink)
    assert a.stats[g.STAT_NAMES.index("RX_UNICAST_FAIL")] > 0
    assert not any(m for (uu, th), m in msgs.items() if uu == u and th > 0)


@pytest.mark.parametrize("vb", WIDTHS)
def test_empty_list_and_null_arrays(g, plain_batch, vb):
    rts, verd, meta = plain_batch
    w = World(g, rts, R, 8)
    empty = np.zeros(0, dtype=np.uint32)
    assert deliver_packed(w, _records(verd, vb, meta, empty), empty, N) == 0
    idx = np.arange(64, dtype=np.uint32)
    cmd, payload, v4 = _records(verd, vb, meta, idx)
    head = (w.by_id, w.R, w.clients, len(w.procs))
    ptr = [cmd.ctypes.data, payload.ctypes.data, v4.ctypes.data, idx.ctypes.data]
    for k in range(4):  # a missing required array: nothing is delivered
        args = list(ptr)
        args[k] = None
        assert g.lib.gcl_host_deliver_packed(*head, *args, 64, N, None, None, w.stats.ctypes.data) == 0
    assert not w.events and not w.stats.any()
    assert all(not m for m in w.ring_msgs().values())


@pytest.mark.parametrize("vb", WIDTHS)
def test_entries_outside_the_batch_are_skipped(g, plain_batch, vb):
    """A list with entries >= n mixed in, each with the empty record
    gcl_plan_pack writes or with garbage: the rings, callbacks and counters of
    the list without them."""
    rts, verd, meta = plain_batch
    rng = np.random.default_rng(7 + vb)
    for idx in _lists(verd, vb)[:6] + _lists(verd, vb)[-1:]:
        a, b = World(g, rts, R, 16), World(g, rts, R, 16)
        da = deliver_packed(a, _records(verd, vb, meta, idx), idx, N, bcast_hash=meta[0])
        at = np.sort(rng.integers(0, len(idx) + 1, size=len(idx) // 3 + 2))
        bad = rng.choice([N, N + 1, 2**31, 2**32 - 1], size=len(at)).astype(np.uint32)
        mixed = np.insert(idx, at, bad)
        cmd, payload, v4 = _records(verd, vb, meta, mixed)
        out = mixed >= N
        assert out.sum() == len(at) and (v4[out] == NO_VERDICT).all() and not cmd[out].any()
        garbage = out & (rng.random(len(mixed)) < 0.5)
        cmd[garbage] = rng.integers(0, 2**63, size=int(garbage.sum()), dtype=np.uint64)
        payload[garbage] = rng.integers(0, 2**63, size=int(garbage.sum()), dtype=np.uint64)
        v4[garbage] = rng.integers(0, 16, size=int(garbage.sum())).astype(np.uint32)  # DELIVER to 0..15
        # bcast_hash is exactly n long: an entry >= n must not index it
        db = deliver_packed(b, (cmd, payload, v4), mixed, N, bcast_hash=meta[0])
        assert da == db
        assert a.events == b.events and a.stats.tolist() == b.stats.tolist()
        assert a.ring_msgs() == b.ring_msgs()
