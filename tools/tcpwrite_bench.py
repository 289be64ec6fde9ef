#!/usr/bin/env python3
"""gcl_tcp_write over 1 Mi segments of 1 448 B: the socket writes of a whole
runtime in one call, against its neighbours.

Shapes: 64 Ki connections writing 16 segments each (uniform); a Zipf(1.1)
spread of the same segments over the same connections; one connection writing
all of them, which is there to show that nothing that grows with the bytes
runs serially.  Writes: plain (tcp_write3), and the same bytes through 16
vectors of uneven length (tcp_writev2), whose last vector is pushed.  Beside
each: gcl_tx_seg over the same plain writes (handed the winlen this call works
out); gcl_tcp_read over a CSR of the same size (one 1 448 B entry per segment,
read whole); gcl_tcp_write_host on one core.

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
NVEC = 16
STRIDE = 1536
# sixteen uneven shares of a write, in 1/136ths: every vector ends inside a segment
SHARES = np.array([1, 16, 2, 15, 3, 14, 4, 13, 5, 12, 6, 11, 7, 10, 8, 9], dtype=np.int64)


def seg_counts(nconn, nseg, shape, rng):
    if shape == "uniform":
        return np.full(nconn, nseg // nconn, dtype=np.int64)
    if shape == "zipf":
        w = 1.0 / np.arange(1, nconn + 1) ** 1.1
        n = rng.multinomial(nseg, w / w.sum()).astype(np.int64)
        rng.shuffle(n)
        return n
    n = np.zeros(nconn, dtype=np.int64)
    n[nconn // 2] = nseg
    return n


def make(nconn, nseg, shape, mode, seed=1):
    rng = np.random.default_rng(seed)
    if shape == "one":
        nconn = 1024
    segs = seg_counts(nconn, nseg, shape, rng)
    size = segs * MSS
    wr = np.zeros(nconn, dtype=g.TCP_WR_DTYPE)
    wr["flags"], wr["snd_mss"], wr["len"], wr["tx_last_ack"] = g.WR_WANT, MSS, size, 7
    wr["src_off"] = np.concatenate(([0], np.cumsum(size)[:-1]))
    conn = np.zeros(nconn, dtype=g.TCP_CONN_DTYPE)
    conn["snd_una"], conn["snd_nxt"], conn["snd_wnd"] = 1000, 1000, (1 << 31) - 1
    conn["rcv_nxt"], conn["rcv_wnd"] = 7, 1 << 16
    addr = np.zeros(nconn, dtype=g.TCP_ADDR_DTYPE)
    addr["lip"], addr["rip"] = 0x0A000005, 0x0B000000 + np.arange(nconn)
    addr["lport"], addr["rport"], addr["rcv_wscale"] = 80, np.arange(nconn) & 0xFFFF, 7
    c = dict(nconn=nconn, segs=segs, size=size, wr=wr, conn=conn, addr=addr, voff=None, iov=None, nvec=0)
    if mode == "vec16":
        wr["flags"] |= g.WR_VEC
        lens = size[:, None] * SHARES[None, :] // SHARES.sum()
        lens[:, -1] += size - lens.sum(axis=1)
        iov = np.zeros(nconn * NVEC, dtype=g.RD_IOV_DTYPE)
        iov["len"] = lens.reshape(-1)
        starts = np.cumsum(lens, axis=1) - lens + wr["src_off"][:, None].astype(np.int64)
        iov["off"] = starts.reshape(-1)
        c.update(voff=(np.arange(nconn + 1) * NVEC).astype(np.uint32), iov=iov, nvec=nconn * NVEC)
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
    ap.add_argument("--nseg", type=int, default=1 << 20)
    ap.add_argument("--nconn", type=int, default=1 << 16)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--shapes", default="uniform,zipf,one")
    ap.add_argument("--modes", default="plain,vec16")
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    clf = g.Classifier(0, 16, g.HASH_JENKINS)
    rows = []
    for shape in a.shapes.split(","):
        for mode in a.modes.split(","):
            c = make(a.nconn, a.nseg, shape, mode)
            nconn, nvec = c["nconn"], c["nvec"]
            cap = a.nseg + (NVEC + 2) * nconn
            d = {k: dev(c[k]) for k in ("wr", "conn", "addr")}
            dv, di = (dev(c["voff"]), dev(c["iov"])) if nvec else (None, None)

            def call(out=None):
                return clf.tcp_write(5, d["wr"], d["conn"], d["addr"], nconn, cap, cap, voff=dv, iov=di, nvec=nvec,
                                     frame_stride=STRIDE, out=out)
            out = call()
            torch.cuda.synchronize()
            totals = out["totals"].cpu().tolist()
            row = dict(shape=shape, mode=mode, nconn=nconn, nvec=nvec, segs=totals[1], items=totals[3],
                       slots=totals[4], bytes=totals[5], write_ms=round(gpu_ms(lambda: call(out), a.warmup, a.iters), 4))
            row["write_ns_per_seg"] = round(row["write_ms"] * 1e6 / max(totals[1], 1), 3)
            if not a.no_yardsticks:
                if mode == "plain":       # the segmenter over the same writes
                    send = np.zeros(nconn, dtype=g.SEG_SEND_DTYPE)
                    for f in ("lip", "rip", "lport", "rport"):
                        send[f] = c["addr"][f]
                    send["proto"], send["mss"], send["snd_nxt"], send["ack"], send["win"] = 6, MSS, 1000, 7, 512
                    send["len"], send["winlen"], send["src_off"] = c["size"], (1 << 31) - 1, c["wr"]["src_off"]
                    ds = dev(send)
                    sout = clf.tx_seg(ds, nconn, cap, stride=STRIDE)
                    row["tx_seg_ms"] = round(gpu_ms(lambda: clf.tx_seg(ds, nconn, cap, stride=STRIDE, out=sout),
                                                    a.warmup, a.iters), 4)
                    torch.cuda.synchronize()
                    assert int(sout["total_segs"].cpu()[0]) == totals[1]
                # the reads over a CSR of the same size
                qoff = np.zeros(nconn + 1, dtype=np.uint32)
                qoff[1:] = np.cumsum(c["segs"])
                nent = int(qoff[-1])
                ent = np.zeros(nent, dtype=g.RDQ_ENT_DTYPE)
                ent["off"], ent["len"] = np.arange(nent, dtype=np.uint64) * MSS, MSS
                rd = np.zeros(nconn, dtype=g.TCP_RD_DTYPE)
                rd["flags"], rd["len"], rd["winmax"] = g.RD_WANT, c["size"], 65535 * 4
                dq, de, dr = dev(qoff), dev(ent), dev(rd)
                rout = clf.tcp_read(dq, de, nent, dr, d["conn"], d["addr"], nconn, nent + nconn, nconn)
                row["tcp_read_ms"] = round(gpu_ms(lambda: clf.tcp_read(dq, de, nent, dr, d["conn"], d["addr"], nconn,
                                                                       nent + nconn, nconn, out=rout),
                                                  a.warmup, a.iters), 4)
                ts = []
                for _ in range(a.host_iters):
                    t0 = time.perf_counter()
                    h = g.tcp_write_host(5, c["wr"], c["conn"], c["addr"], cap, cap, voff=c["voff"], iov=c["iov"],
                                         frame_stride=STRIDE, nvec=nvec)
                    ts.append((time.perf_counter() - t0) * 1e3)
                assert h["totals"].tolist() == totals
                row["host_ms"] = round(statistics.median(ts), 3)
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    doc = dict(tool="tools/tcpwrite_bench.py", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup,
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
