"""Test-side helpers of the delivery plan (gcl_plan, gcl_host_deliver_idx):
the numpy definition of a plan, and a host world of runtimes and lrpc rings
that a batch's verdicts can be delivered into, in order or list by list."""
import ctypes

import numpy as np

PLAN_BY_RUNTIME, PLAN_BY_QUEUE = 0, 1


def plan_nbuckets(key, max_runtimes, thread_bits):
    return (max_runtimes << thread_bits if key == PLAN_BY_QUEUE else max_runtimes) + 1


def plan_keys(v, vbytes, key, max_runtimes, thread_bits):
    """The bucket of every verdict of @v (a numpy array in the width's own
    dtype, or raw bytes), as include/gclassify.h defines it: the runtime (or
    queue) of a DELIVER / WAKE verdict, the host bucket (the last) for
    everything else and for any key >= nbuckets - 1."""
    nb = plan_nbuckets(key, max_runtimes, thread_bits)
    host = nb - 1
    raw = np.ascontiguousarray(v).view(np.uint8).reshape(-1, vbytes)
    if vbytes in (8, 4):
        assert key == PLAN_BY_RUNTIME
        w = raw[:, vbytes - 4:]  # {uniqid u16, thread u8, action u8}
        k = w[:, 0].astype(np.int64) | w[:, 1].astype(np.int64) << 8
        unicast = (w[:, 3] & 0x3F) <= 1
    elif vbytes == 2:
        x = raw[:, 0].astype(np.int64) | raw[:, 1].astype(np.int64) << 8
        k = x & 0x3FFF
        unicast = (x & 0xC000 == 0x0000) | (x & 0xC000 == 0x4000)
    else:
        x = raw[:, 0].astype(np.int64)
        k = x & 0x7F
        unicast = (x & 0x80) == 0
    if vbytes <= 2 and key == PLAN_BY_RUNTIME:
        k = k >> thread_bits
    return np.where(unicast & (k < host), k, host), nb


def plan_expected(keys, nb):
    """(order, bucket_off) of the definition: the stable argsort of the keys
    and the cumulative bucket counts."""
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    off = np.zeros(nb + 1, dtype=np.uint32)
    off[1:] = np.cumsum(np.bincount(keys, minlength=nb))
    return order, off


class World:
    """Runtimes with their kthread rings (tests/test_cabi.py's Ring and
    _host_procs) and recording callbacks; deliver() runs one post-pass call
    into it, snapshot() reads everything back."""

    def __init__(self, g, rts, R, ring_size, add_core="wake_self"):
        from tests.test_cabi import _host_procs
        self.g, self.R = g, R
        self.procs, self.rings, self._keep = _host_procs(g, rts, ring_size)
        self.by_id = (ctypes.c_void_p * R)()
        for u, p in self.procs.items():
            self.by_id[u] = ctypes.addressof(p)
        self.clients = (ctypes.c_void_p * len(self.procs))(
            *[ctypes.addressof(p) for p in self.procs.values()])
        self.events = []
        self.stats = np.zeros(8, dtype=np.uint64)
        self.delivered = 0
        ev = self.events

        @g.SCHED_ADD_CORE_FN
        def core(arg, pp):  # activates a kthread of the woken runtime only
            p = pp.contents
            if p.active_thread_count == 0:
                p.active_thread_count = 1
                for i in range(p.thread_count):
                    p.flow_tbl[i] = p.thread_count - 1
                ev.append(("wake", p.uniqid))

        @g.FREE_PKT_FN
        def free_pkt(arg, i):
            ev.append(("free", i))

        @g.REFCNT_FN
        def refcnt(arg, i, d):
            ev.append(("ref", i, d))

        @g.OWNED_FN
        def owned(arg, pp, i):
            ev.append(("own", pp.contents.uniqid, i))

        @g.ENABLE_POLL_FN
        def poll(arg, pp, th):
            ev.append(("poll", pp.contents.uniqid, th))

        @g.ARP_RESPOND_FN
        def arp(arg, i):
            ev.append(("arp", i))
            return i % 2 == 0

        self._cbs = (core, free_pkt, refcnt, owned, poll, arp)
        self.ops = g.GclHostOps()
        if add_core:
            self.ops.sched_add_core = core
        self.ops.free_pkt, self.ops.refcnt_update = free_pkt, refcnt
        self.ops.owned, self.ops.enable_poll, self.ops.arp_respond = owned, poll, arp

    def deliver(self, v, vbytes, thread_bits, meta, idx=None, n=None):
        """gcl_host_deliver{,4,2,1} over the first @n verdicts (idx None), or
        gcl_host_deliver_idx over the list @idx.  @meta = (bcast_hash,
        pkt_len, olflags, shmptr)."""
        lib, bh, plen, olf, shm = self.g.lib, *meta
        tail = (ctypes.byref(self.ops), self.stats.ctypes.data)
        head = (self.by_id, self.R, self.clients, len(self.procs), v.ctypes.data)
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32)
            keep = idx if len(idx) else np.zeros(1, dtype=np.uint32)
            d = lib.gcl_host_deliver_idx(*head, vbytes, thread_bits, bh.ctypes.data,
                                         plen.ctypes.data, olf.ctypes.data, 0x09, shm.ctypes.data,
                                         keep.ctypes.data, len(idx), *tail)
        elif vbytes == 8:
            d = lib.gcl_host_deliver(*head, plen.ctypes.data, olf.ctypes.data, 0x09,
                                     shm.ctypes.data, n, *tail)
        elif vbytes == 4:
            d = lib.gcl_host_deliver4(*head, bh.ctypes.data, plen.ctypes.data, olf.ctypes.data, 0x09,
                                      shm.ctypes.data, n, *tail)
        else:
            fn = lib.gcl_host_deliver2 if vbytes == 2 else lib.gcl_host_deliver1
            d = fn(*head, thread_bits, bh.ctypes.data, plen.ctypes.data, olf.ctypes.data, 0x09,
                   shm.ctypes.data, n, *tail)
        self.delivered += d
        return d

    def ring_msgs(self):
        return {k: r.drain() for k, r in self.rings.items()}
