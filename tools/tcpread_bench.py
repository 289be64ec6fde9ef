#!/usr/bin/env python3
"""gcl_tcp_read over 1 Mi receive-queue entries of 1 448 B: the socket reads of a
whole runtime in one call, against its neighbours.

Queue shapes: 64 Ki connections with 16 entries each (uniform); a Zipf(1.1)
spread of the same entries over the same connections; one connection holding
all of them, which is there to show that no launch walks a queue.  Reads: the
whole queue; half of it, so that every read ends inside an entry; the whole
queue into 4 KiB vectors.  Beside each: gcl_tcp_txq over the same CSR (its
sibling in memory shape); torch.cumsum over the entry lengths plus
gcl_copy_batch over the items the call emitted (what the scans and the copy
that follows cost on their own); gcl_tcp_read_host on one core.

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

MSS = 1448
VEC = 4096


def queue_lens(nconn, nent, shape, rng):
    if shape == "uniform":
        return np.full(nconn, nent // nconn, dtype=np.int64)
    if shape == "zipf":
        w = 1.0 / np.arange(1, nconn + 1) ** 1.1
        lens = rng.multinomial(nent, w / w.sum()).astype(np.int64)
        rng.shuffle(lens)
        return lens
    lens = np.zeros(nconn, dtype=np.int64)
    lens[nconn // 2] = nent
    return lens


def make(nconn, nent, shape, read, seed=1):
    rng = np.random.default_rng(seed)
    if shape == "one":
        nconn = 1024
    lens = queue_lens(nconn, nent, shape, rng)
    qoff = np.zeros(nconn + 1, dtype=np.uint32)
    qoff[1:] = np.cumsum(lens)
    ent = np.zeros(nent, dtype=g.RDQ_ENT_DTYPE)
    ent["off"], ent["len"] = np.arange(nent, dtype=np.uint64) * MSS, MSS
    size = lens * MSS
    want = size // 2 + 1 if read == "half" else size
    rd = np.zeros(nconn, dtype=g.TCP_RD_DTYPE)
    rd["flags"], rd["len"] = g.RD_WANT, want
    rd["dst_off"] = np.concatenate(([0], np.cumsum(size)[:-1]))
    rd["winmax"] = 65535 * 4           # a read of 64 KiB or more sends the window update
    conn = np.zeros(nconn, dtype=g.TCP_CONN_DTYPE)
    conn["rcv_nxt"], conn["rcv_wnd"], conn["snd_nxt"] = 7, 1 << 16, 9
    rd["tx_last_ack"], rd["tx_last_win"] = 7, 1 << 16
    addr = np.zeros(nconn, dtype=g.TCP_ADDR_DTYPE)
    addr["lip"], addr["rip"] = 0x0A000005, 0x0B000000 + np.arange(nconn)
    addr["lport"], addr["rport"], addr["rcv_wscale"] = 80, np.arange(nconn) & 0xFFFF, 7
    c = dict(nconn=nconn, nent=nent, qoff=qoff, ent=ent, rd=rd, conn=conn, addr=addr, voff=None, iov=None, nvec=0)
    if read == "iov":
        nv = (size + VEC - 1) // VEC
        voff = np.zeros(nconn + 1, dtype=np.uint32)
        voff[1:] = np.cumsum(nv)
        nvec = int(voff[-1])
        owner = np.repeat(np.arange(nconn), nv)
        iov = np.zeros(nvec, dtype=g.RD_IOV_DTYPE)
        iov["off"] = rd["dst_off"][owner] + (np.arange(nvec) - voff[:-1][owner]).astype(np.uint64) * VEC
        iov["len"] = VEC
        c.update(voff=voff, iov=iov, nvec=nvec)
    return c


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
    ap.add_argument("--nent", type=int, default=1 << 20)
    ap.add_argument("--nconn", type=int, default=1 << 16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--shapes", default="uniform,zipf,one")
    ap.add_argument("--out")
    a = ap.parse_args()
    clf = g.Classifier(0, 16, g.HASH_JENKINS)
    region = a.nent * MSS
    src = torch.zeros(region, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(region + VEC, dtype=torch.uint8, device="cuda")
    rows = []
    for shape in a.shapes.split(","):
        for read in ("whole", "half", "iov"):
            c = make(a.nconn, a.nent, shape, read)
            nconn, nent, nvec = c["nconn"], c["nent"], c["nvec"]
            cap = nent + max(nvec, nconn)
            d = {k: dev(c[k]) for k in ("qoff", "ent", "rd", "conn", "addr")}
            dv, di = (dev(c["voff"]), dev(c["iov"])) if nvec else (None, None)

            def call(out=None):
                return clf.tcp_read(d["qoff"], d["ent"], nent, d["rd"], d["conn"], d["addr"], nconn, cap, nconn,
                                    voff=dv, iov=di, nvec=nvec, frame_stride=64, out=out)
            out = call()
            torch.cuda.synchronize()
            totals, segs = out["totals"].cpu().tolist(), out["seg_totals"].cpu().tolist()
            t_read = gpu_ms(lambda: call(out), a.warmup, a.iters)
            # the sibling over the same CSR: pops only
            tent = np.zeros(nent, dtype=g.TXQ_ENT_DTYPE)
            tent["seg_end"] = 1
            te, tc = dev(tent), dev(np.zeros(nent, dtype=g.TXQ_COLD_DTYPE))
            tout = clf.tcp_txq(1 << 40, d["qoff"], te, tc, nent, d["conn"], d["addr"], nconn, 16)
            t_txq = gpu_ms(lambda: clf.tcp_txq(1 << 40, d["qoff"], te, tc, nent, d["conn"], d["addr"], nconn, 16,
                                               out=tout), a.warmup, a.iters)
            # what the scan and the copy behind the call cost on their own
            lens = torch.from_numpy(c["ent"]["len"].astype(np.int64)).cuda()
            k = totals[1]

            def scan_copy():
                torch.cumsum(lens, 0)
                clf.copy_batch(src, out["src_off"], out["len"], k, dst, dst_off=out["dst_off"], olflags=False,
                               rss=False)
            t_scan = gpu_ms(scan_copy, a.warmup, max(a.iters // 2, 1))
            ts = []
            for _ in range(a.host_iters):
                t0 = time.perf_counter()
                h = g.tcp_read_host(c["qoff"], c["ent"], c["rd"], c["conn"], c["addr"], cap, nconn, voff=c["voff"],
                                    iov=c["iov"], nvec=nvec)
                ts.append((time.perf_counter() - t0) * 1e3)
            assert h["totals"].tolist() == [t & ((1 << 64) - 1) for t in totals]
            rows.append(dict(shape=shape, read=read, nconn=nconn, nent=nent, nvec=nvec, items=totals[1],
                             bytes=totals[2], acks=segs[1], read_ms=round(t_read, 4), txq_ms=round(t_txq, 4),
                             cumsum_copy_ms=round(t_scan, 4), host_ms=round(statistics.median(ts), 3),
                             read_ns_per_entry=round(t_read * 1e6 / nent, 3)))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    doc = dict(tool="tools/tcpread_bench.py", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup,
               rows=rows)
    text = json.dumps(doc, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    clf.close()


if __name__ == "__main__":
    main()
