#!/usr/bin/env python3
"""Time the packed delivery records of a plan (gcl_plan_pack on the GPU,
gcl_host_deliver_packed on the host) against what they replace.

Device (needs a GPU): gcl_plan_pack over the whole order of the by-runtime
plan of bench.py's udp64 configuration (32 Mi packets, 16 runtimes x 8
kthreads, 17 buckets), with 1-byte and with 8-byte verdicts and every optional
array given, against the same records built with torch: index_select of each
input by the order (converted to int64 in advance, untimed, which favours
torch) plus the arithmetic.  Both sides are timed with HIP events over >= 10 ms
of back-to-back launches after a warm-up, in alternating rounds; the median
round is reported.  The roofline fraction is on the algorithmic bytes
m x (4 + vbytes + 2 + 1 + 8 read, 20 written) at 8 TB/s.

Host (CPU only, --host-only runs it alone on any machine): ns per packet of
gcl_host_deliver_packed against gcl_host_deliver_idx over the same 17-bucket
plan of --host-n packets (default 4 Mi, 1-byte verdicts) built with numpy:
uniform runtimes and slots, 3 % of the packets in the host bucket, rings large
enough never to fill, no callbacks, one list after another on one core.  The
records are built in advance (on the GPU in production).  Alternating rounds;
median and minimum are reported, and the two passes must leave identical rings.

A tool, not a gate: prints one JSON line and writes profiles/pack_bench.json.
"""
import argparse
import ctypes
import json
import os
import platform
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HOST_ONLY = "--host-only" in sys.argv
if not HOST_ONLY:  # torch brings its HIP runtime: load it before the library, as bench.py does
    import torch  # noqa: E402

    import bench  # noqa: E402
from caladan_amd import gclassify as g  # noqa: E402

MIN_MS = 10.0
ROUNDS = 5
SHM_BASE = 0x7F12_3456_7000
R, T, TB = 16, 8, 3


# ---------------------------------------------------------------- device
def timed_us(torch, fn, min_ms=MIN_MS, warmup=3):
    """Mean microseconds per call of @fn over >= @min_ms of launches."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    reps = 4
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        total = a.elapsed_time(b)
        if total >= min_ms:
            return total * 1000.0 / reps
        reps = max(reps * 2, int(reps * 1.2 * min_ms / max(total, 1e-3)) + 1)


def torch_records(torch, verdicts, vbytes, tb, idx, pkt_len, olflags, offs):
    """The definition of gcl_plan_pack with torch ops, every entry < n."""
    ln = pkt_len.index_select(0, idx).to(torch.int64) & 0xFFFF
    csum = ((olflags.index_select(0, idx) & 0x0C) == 0x08).to(torch.int64)
    cmd = ln << 16 | csum << 48
    payload = offs.index_select(0, idx) + SHM_BASE
    if vbytes == 8:
        v4 = verdicts.view(torch.int32).view(-1, 2)[:, 1].index_select(0, idx)
    else:
        x = verdicts.index_select(0, idx).to(torch.int32)
        q = x & 0x7F
        unicast = (x & 0x80) == 0
        v4 = torch.where(unicast, q >> tb | (q & ((1 << tb) - 1)) << 16,
                         0xFFFF | 0xFF << 16 | (x & 0x3F) << 24)
    return cmd, payload, v4


def run_device(torch, bench, device, n, vbytes):
    wl, _, stride, R_, T_, _ = bench.WORKLOADS["udp64"]
    clf = bench.classifier(device, R_, T_, vbytes)
    bench.setup_tables(clf, R_, T_)
    frames = torch.zeros(n * stride, dtype=torch.uint8, device=device)
    g.generate(wl, n, stride, R_, frames, seed=bench.SEED)
    verdicts = torch.zeros(n * vbytes, dtype=torch.uint8, device=device)
    clf.classify(frames, n, stride, verdicts=verdicts)
    torch.cuda.synchronize()
    del frames
    order, off = clf.plan(verdicts, n, key=g.PLAN_BY_RUNTIME)
    gen = torch.Generator(device=device).manual_seed(bench.SEED)
    pkt_len = torch.randint(-32768, 32768, (n,), dtype=torch.int16, device=device, generator=gen)
    olflags = torch.randint(0, 16, (n,), dtype=torch.uint8, device=device, generator=gen)
    offs = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=device, generator=gen)
    out = (torch.empty(n, dtype=torch.int64, device=device), torch.empty(n, dtype=torch.int64, device=device),
           torch.empty(n, dtype=torch.int32, device=device))
    idx = order.to(torch.int64)
    torch.cuda.synchronize()

    def pack():
        clf.plan_pack(verdicts, n, order, pkt_len=pkt_len, olflags=olflags, offs=offs,
                      shm_base=SHM_BASE, out=out)

    def with_torch():
        return torch_records(torch, verdicts, vbytes, clf.thread_bits, idx, pkt_len, olflags, offs)

    pack_us, torch_us = [], []
    for _ in range(ROUNDS):
        pack_us.append(timed_us(torch, pack))
        torch_us.append(timed_us(torch, with_torch))
    pack()
    same = all(bool((a == b).all().item()) for a, b in zip(out, with_torch()))
    p, t = statistics.median(pack_us), statistics.median(torch_us)
    alg = n * (4 + vbytes + 2 + 1 + 8 + 20)
    row = {
        "workload": f"udp64, {R_} runtimes x {T_} kthreads, {vbytes}-B verdicts, by-runtime plan, whole order",
        "m": n, "nbuckets": int(off.numel()) - 1,
        "pack_us_median": round(p, 2), "pack_us_rounds": [round(x, 2) for x in pack_us],
        "torch_us_median": round(t, 2), "torch_us_rounds": [round(x, 2) for x in torch_us],
        "torch_over_pack": round(t / p, 3), "pack_gpkt_s": round(n / p / 1e3, 2),
        "algorithmic_bytes": alg,
        "roofline_frac_8TBs": round(alg / (p * 1e-6) / (bench.HBM_PEAK_GBS * 1e9), 4),
        "matches_torch": same,
    }
    clf.close()
    return row


# ---------------------------------------------------------------- host
def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


class Rings:
    """16 runtimes x 8 kthreads, every kthread active, one lrpc ring each."""

    def __init__(self, size):
        self.size = size
        self.tbl = np.zeros((R, T, size, 2), dtype=np.uint64)
        self.wb = (ctypes.c_uint32 * (R * T))()
        self.chans = (g.GclLrpcChanOut * (R * T))()
        self.procs = (g.GclHostProc * R)()
        for r in range(R):
            p = self.procs[r]
            p.uniqid, p.thread_count, p.active_thread_count, p.idle_top = r, T, T, -1
            for t in range(T):
                k = r * T + t
                msgs = ctypes.cast(self.tbl[r, t].ctypes.data, ctypes.POINTER(g.GclLrpcMsg))
                wb = ctypes.cast(ctypes.addressof(self.wb) + 4 * k, ctypes.POINTER(ctypes.c_uint32))
                assert g.lib.gcl_lrpc_init_out(ctypes.byref(self.chans[k]), msgs, size, wb) == 0
                p.flow_tbl[t] = t
                p.rxq[t] = ctypes.pointer(self.chans[k])
        self.by_id = (ctypes.c_void_p * R)(*[ctypes.addressof(self.procs[r]) for r in range(R)])

    def reset(self):
        for c in self.chans:
            c.send_head = c.send_tail = 0

    def state(self):
        heads = [c.send_head for c in self.chans]
        assert max(heads) <= self.size, "a ring filled: raise --ring"
        return heads, int(self.tbl.sum(dtype=np.uint64))


def run_host(n, ring):
    rng = np.random.default_rng(0xCA1ADA4)
    v = (rng.integers(0, R * T, size=n)).astype(np.uint8)            # q = uniqid << 3 | slot
    drop = rng.random(n) < 0.03
    v[drop] = 0x80 | 3                                               # GCL_V1_OTHER | DROP_UNREG
    keys = np.where(drop, R, v >> TB)
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    off = np.zeros(R + 2, dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(keys, minlength=R + 1))
    pkt_len = rng.integers(60, 1515, size=n).astype(np.uint16)
    olflags = rng.integers(0, 16, size=n, dtype=np.uint8)
    shmptr = SHM_BASE + np.arange(n, dtype=np.uint64) * np.uint64(64)
    # the list's records, as gcl_plan_pack defines them
    cmd = pkt_len[order].astype(np.uint64) << np.uint64(16) | \
        ((olflags[order] & 0x0C) == 0x08).astype(np.uint64) << np.uint64(48)
    payload = shmptr[order]
    x = v[order].astype(np.uint32)
    v4 = np.where(x & 0x80, 0xFFFF | 0xFF << 16 | (x & 0x3F) << 24,
                  (x & 0x7F) >> TB | (x & ((1 << TB) - 1)) << 16).astype(np.uint32)

    rings = Rings(ring)
    stats = np.zeros(8, dtype=np.uint64)
    lib = g.lib
    head = (rings.by_id, R, rings.by_id, R)

    def by_idx():
        d = 0
        for b in range(R + 1):
            s, m = int(off[b]), int(off[b + 1] - off[b])
            d += lib.gcl_host_deliver_idx(*head, v.ctypes.data, 1, TB, None, pkt_len.ctypes.data,
                                          olflags.ctypes.data, 0x09, shmptr.ctypes.data,
                                          order.ctypes.data + 4 * s, m, None, stats.ctypes.data)
        return d

    def packed():
        d = 0
        for b in range(R + 1):
            s, m = int(off[b]), int(off[b + 1] - off[b])
            d += lib.gcl_host_deliver_packed(*head, cmd.ctypes.data + 8 * s, payload.ctypes.data + 8 * s,
                                             v4.ctypes.data + 4 * s, order.ctypes.data + 4 * s, m, n,
                                             None, None, stats.ctypes.data)
        return d

    res, state = {"idx": [], "packed": []}, {}
    for rnd in range(ROUNDS + 1):  # round 0 warms up
        for name, fn in (("idx", by_idx), ("packed", packed)):
            rings.reset()
            t0 = time.perf_counter_ns()
            d = fn()
            dt = time.perf_counter_ns() - t0
            assert d == n - int(drop.sum())
            if rnd:
                res[name].append(dt / n)
            else:
                state[name] = rings.state()
    same = state["idx"] == state["packed"]
    i, p = res["idx"], res["packed"]
    return {
        "workload": f"{R} runtimes x {T} kthreads, 1-B verdicts, {R + 1} lists one after another on one core, "
                    "3 % host bucket, no callbacks",
        "cpu": cpu_name(), "n": n, "ring_slots": ring,
        "deliver_idx_ns_per_pkt_median": round(statistics.median(i), 3),
        "deliver_idx_ns_per_pkt_min": round(min(i), 3),
        "deliver_packed_ns_per_pkt_median": round(statistics.median(p), 3),
        "deliver_packed_ns_per_pkt_min": round(min(p), 3),
        "idx_over_packed": round(statistics.median(i) / statistics.median(p), 3),
        "rounds": ROUNDS, "same_rings": same,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=32 << 20, help="device: packets (default 32 Mi)")
    ap.add_argument("--host-n", type=int, default=4 << 20, help="host: packets (default 4 Mi)")
    ap.add_argument("--ring", type=int, default=1 << 16, help="host: slots per ring (a power of two)")
    ap.add_argument("--host-only", action="store_true", help="skip the device part (no GPU needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_bench.json"))
    args = ap.parse_args()
    res = {"tool": "tools/pack_bench.py", "library": g.version()}
    if not HOST_ONLY:
        if not torch.cuda.is_available():
            sys.exit("pack_bench.py: the device part needs a GPU (--host-only for the host part)")
        device = torch.device("cuda:0")
        res.update(box=torch.cuda.get_device_name(0), torch=torch.__version__,
                   device=[run_device(torch, bench, device, args.n, 1),
                           run_device(torch, bench, device, args.n, 8)])
    res["host"] = run_host(args.host_n, args.ring)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
