"""Test-side helpers of the packed delivery records (gcl_plan_pack,
gcl_host_deliver_packed): the numpy definition of a list's records, written
from include/gclassify.h, and the call that delivers them into a
plancases.World."""
import ctypes

import numpy as np

NO_VERDICT = 0xFFFF | 0xFF << 16 | 0x3F << 24  # {GCL_NO_RUNTIME, GCL_NO_THREAD, GCL_ACT_MASK}


def widen(v, vbytes, thread_bits):
    """Every verdict of @v (raw bytes, or an array of the width's dtype) as
    the u32 image of its struct gcl_verdict4: uniqid | thread << 16 |
    action << 24."""
    raw = np.ascontiguousarray(v).view(np.uint8).reshape(-1, vbytes)
    if vbytes in (8, 4):  # the last four bytes, flags kept
        return np.ascontiguousarray(raw[:, vbytes - 4:]).view("<u4").reshape(-1).copy()
    tmask = (1 << thread_bits) - 1
    if vbytes == 2:
        x = raw[:, 0].astype(np.uint32) | raw[:, 1].astype(np.uint32) << 8
        kind, q = x & 0xC000, x & 0x3FFF
        unicast = (kind == 0x0000) | (kind == 0x4000)
        act = np.where(unicast, np.where(kind == 0x4000, 1, 0), x & 0x3F)
    else:
        x = raw[:, 0].astype(np.uint32)
        q = x & 0x7F
        unicast = (x & 0x80) == 0
        act = np.where(unicast, 0, x & 0x3F)
    dest = np.where(unicast, ((q >> thread_bits) & 0xFFFF) | ((q & tmask) & 0xFF) << 16,
                    0xFFFF | 0xFF << 16)
    return (dest.astype(np.uint32) | act.astype(np.uint32) << 24).astype(np.uint32)


def pack_expected(v, vbytes, thread_bits, n, order, pkt_len=None, olflags=None, default_olflags=0x09,
                  offs=None, stride=0, shm_base=0):
    """(cmd u64[m], payload u64[m], v4 u32[m]) of the definition for the list
    @order over a batch of @n packets; entries >= n get the empty record."""
    order = np.asarray(order, dtype=np.uint32).astype(np.int64)
    ok = order < n
    i = np.where(ok, order, 0)
    if n == 0:
        m = len(order)
        return np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.full(m, NO_VERDICT, np.uint32)
    ln = pkt_len[:n][i].astype(np.uint64) if pkt_len is not None else np.zeros(len(i), np.uint64)
    fl = olflags[:n][i] if olflags is not None else np.full(len(i), default_olflags, np.uint8)
    csum = ((fl & 0x0C) == 0x08).astype(np.uint64)
    cmd = ln << np.uint64(16) | csum << np.uint64(48)
    off = offs[:n][i].astype(np.uint64) if offs is not None else \
        i.astype(np.uint64) * np.uint64(stride)
    with np.errstate(over="ignore"):
        payload = np.uint64(shm_base) + off
    w = widen(np.ascontiguousarray(v).view(np.uint8)[:n * vbytes], vbytes, thread_bits)[i]
    zero = np.uint64(0)
    return (np.where(ok, cmd, zero), np.where(ok, payload, zero),
            np.where(ok, w, np.uint32(NO_VERDICT)).astype(np.uint32))


def deliver_packed(world, recs, idx, n, bcast_hash=None):
    """gcl_host_deliver_packed of the records @recs = (cmd, payload, v4) of
    the list @idx into the plancases.World @world."""
    cmd, payload, v4 = (np.ascontiguousarray(a) for a in recs)
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    assert len(cmd) == len(payload) == len(v4) == len(idx)
    assert cmd.dtype.itemsize == 8 and payload.dtype.itemsize == 8 and v4.dtype.itemsize == 4
    pad = [a if len(a) else np.zeros(1, dtype=a.dtype) for a in (cmd, payload, v4, idx)]
    d = world.g.lib.gcl_host_deliver_packed(
        world.by_id, world.R, world.clients, len(world.procs), pad[0].ctypes.data,
        pad[1].ctypes.data, pad[2].ctypes.data, pad[3].ctypes.data, len(idx), n,
        bcast_hash.ctypes.data if bcast_hash is not None else None,
        ctypes.byref(world.ops), world.stats.ctypes.data)
    world.delivered += d
    return d
