#!/usr/bin/env python3
"""gcl_tcp_txq on 1 Mi connections: the retransmit queues of a whole runtime in
one call, against its neighbours.

Queue shapes: one entry per connection with its head acknowledged (one_each:
pops only, nothing is ever sent); one unacknowledged entry per connection
(loss: every due connection retransmits it, the loss event across many
connections); a Zipf spread of the same number of entries; one connection
holding all entries.  Due shares: none, 1 % and all of the connections ask for
tcp_retransmit with every entry of their queues older than the timeout, so a
due queue sends up to TCP_RETRANSMIT_BATCH segments.  Baselines: gcl_tcp_tick
over the same connections (its sibling in memory shape: one record per
connection, three launches); a torch formulation of the pops alone (a segmented
reduction over the same arrays); gcl_tcp_txq_host on one core.

Times are medians of --iters calls between two events on one stream, after
--warmup calls; the host twin is timed with perf_counter.  No figure is a gate.
Writes one JSON document (--out, default stdout).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from caladan_amd import gclassify as g  # noqa: E402

NOW = 1 << 40
DUE = NOW - 300000 - 7


def make(nconn, shape, due, seed=1):
    rng = np.random.default_rng(seed)
    if shape in ("one_each", "loss"):
        lens = np.ones(nconn, dtype=np.int64)
    elif shape == "zipf":
        w = 1.0 / np.arange(1, nconn + 1) ** 1.1
        lens = rng.multinomial(nconn, w / w.sum()).astype(np.int64)
        rng.shuffle(lens)
    else:
        lens = np.zeros(nconn, dtype=np.int64)
        lens[nconn // 2] = nconn
    qoff = np.zeros(nconn + 1, dtype=np.uint32)
    qoff[1:] = np.cumsum(lens)
    nent = int(qoff[-1])
    owner = np.repeat(np.arange(nconn), lens)
    pos = np.arange(nent) - qoff[:-1][owner]
    una = rng.integers(0, 1 << 32, nconn, dtype=np.uint64).astype(np.uint32)
    isdue = rng.random(nconn) < due
    ent = np.zeros(nent, dtype=g.TXQ_ENT_DTYPE)
    # the first entry of every queue is acknowledged (not in "loss"), the rest back to back behind snd_una
    ent["seg_seq"] = (una[owner].astype(np.int64) + 1000 * (pos - (shape != "loss"))).astype(np.uint32)
    ent["seg_end"] = ent["seg_seq"] + np.uint32(1000)
    # a due queue's timestamps grow up to DUE at its last entry; the other queues are young throughout
    ent["ts"] = np.where(isdue[owner], DUE - (lens[owner] - 1) + pos, NOW - 1000).astype(np.uint64)
    cold = np.zeros(nent, dtype=g.TXQ_COLD_DTYPE)
    cold["frame_off"] = np.arange(nent, dtype=np.uint64) * 2048
    cold["tcp_flags"], cold["tcp_off"] = 0x10, 5
    conn = np.zeros(nconn, dtype=g.TCP_CONN_DTYPE)
    conn["snd_una"], conn["rcv_nxt"], conn["rcv_wnd"] = una, 7, 1 << 16
    addr = np.zeros(nconn, dtype=g.TCP_ADDR_DTYPE)
    addr["lip"], addr["rip"] = 0x0A000005, 0x0B000000 + np.arange(nconn)
    addr["lport"], addr["rport"] = 80, np.arange(nconn) & 0xFFFF
    want = np.where(isdue, g.TXQ_W_RTO, 0).astype(np.uint8)
    return dict(qoff=qoff, ent=ent, cold=cold, conn=conn, addr=addr, want=want, nent=nent, owner=owner)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return torch.from_numpy(a.view(np.uint8).reshape(len(a), -1)).cuda()
    return torch.from_numpy(a.view({np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).cuda()


def gpu_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nconn", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    clf = g.Classifier(0, 16, g.HASH_JENKINS)
    nconn = a.nconn
    rows = []
    for shape in ("one_each", "loss", "zipf", "one_long"):
        for due in (0.0, 0.01, 1.0):
            c = make(nconn, shape, due)
            nent, cap = c["nent"], 17 * nconn
            d = {k: dev(c[k]) for k in ("qoff", "ent", "cold", "conn", "addr", "want")}
            out = clf.tcp_txq(NOW, d["qoff"], d["ent"], d["cold"], nent, d["conn"], d["addr"], nconn, cap,
                              want=d["want"], frame_stride=2048)
            torch.cuda.synchronize()
            totals = out["totals"].cpu().tolist()
            t_txq = gpu_ms(lambda: clf.tcp_txq(NOW, d["qoff"], d["ent"], d["cold"], nent, d["conn"], d["addr"],
                                               nconn, cap, want=d["want"], frame_stride=2048, out=out),
                           a.warmup, a.iters)
            # the sibling: a sweep over the same connections, the same share of them due (each due one ACKs)
            tmr = np.zeros(nconn, dtype=g.TCP_TMR_DTYPE)
            tmr["state"] = g.TCP_STATE_ESTABLISHED
            tmr["flags"] = g.TMR_LIVE | g.TMR_ACK_DELAYED
            tmr["ack_ts"] = np.where(c["want"] != 0, NOW - 20000, NOW)
            dt = dev(tmr)
            tout = clf.tcp_tick(NOW, dt, d["conn"], d["addr"], nconn, 2 * nconn)
            t_tick = gpu_ms(lambda: clf.tcp_tick(NOW, dt, d["conn"], d["addr"], nconn, 2 * nconn, out=tout),
                            a.warmup, a.iters)
            # the pops alone in torch: the first unacknowledged entry of every segment
            owner = torch.from_numpy(c["owner"]).cuda()
            lo = d["qoff"][:-1].long() & 0xFFFFFFFF
            hi = d["qoff"][1:].long() & 0xFFFFFFFF
            end = torch.from_numpy(c["ent"]["seg_end"].astype(np.int64)).cuda()
            una = torch.from_numpy(c["conn"]["snd_una"].astype(np.int64)).cuda()
            idx = torch.arange(nent, device="cuda")

            def pops():
                diff = (una[owner] - end) & 0xFFFFFFFF                      # wraps_gt(end, una): (int32)(una - end) < 0
                unacked = diff >= 0x80000000
                first = torch.where(unacked, idx, torch.full_like(idx, 1 << 40))
                head = hi.clone().scatter_reduce(0, owner, first, "amin")
                return head - lo
            nacked = pops()
            torch.cuda.synchronize()
            assert torch.equal(nacked.int(), out["out_conn"].view(torch.int32).reshape(nconn, 8)[:, 2])
            t_torch = gpu_ms(pops, a.warmup, a.iters)
            ts = []
            for _ in range(a.host_iters):
                t0 = time.perf_counter()
                h = g.tcp_txq_host(NOW, c["qoff"], c["ent"], c["cold"], c["conn"], c["addr"], cap, want=c["want"],
                                   frame_stride=2048)
                ts.append((time.perf_counter() - t0) * 1e3)
            assert h["totals"].tolist() == [t & ((1 << 64) - 1) for t in totals]
            rows.append(dict(shape=shape, due=due, nconn=nconn, nent=nent, segments=totals[1],
                             txq_ms=round(t_txq, 4), tick_ms=round(t_tick, 4), torch_pops_ms=round(t_torch, 4),
                             host_ms=round(statistics.median(ts), 3),
                             txq_ns_per_entry=round(t_txq * 1e6 / max(nent, 1), 3),
                             host_ns_per_entry=round(statistics.median(ts) * 1e6 / max(nent, 1), 3)))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    doc = dict(tool="tools/txq_bench.py", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup,
               long_threshold=g.TXQ_LONG, rows=rows)
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    clf.close()


if __name__ == "__main__":
    main()
