#!/usr/bin/env python3
"""Time gcl_tx_hdr on the GPU beside gcl_copy_batch of 64-byte frames at the
same n, and gcl_tx_hdr_host on one core.

  python tools/txhdr_bench.py [--n 1048576] [--iters 20] [--out profiles/txhdr_bench.json]

Rows: UDP and TCP segments, frames at a 64-byte and a 1536-byte pitch, against
neighbour tables of 16, 4 Ki and 64 Ki entries (every destination resolves,
one in eight is local); then the copy row; then the host twin (n / 8 entries,
scaled).  Every GPU figure is the median of --iters timed launches after
warm-up, by HIP events on the launch stream; the outputs of the first launch
are held to the host twin on a sample.  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_us(fn, iters, warmup=3):
    import torch
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
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def make(G, n, proto, pitch, neigh_ips, seed=1):
    rng = np.random.default_rng(seed)
    d = np.zeros(n, dtype=G.TXH_DESC_DTYPE)
    d["rip"] = rng.choice(neigh_ips, n)
    d["lport"] = rng.integers(1, 65536, n)
    d["rport"] = rng.integers(1, 65536, n)
    d["proto"] = proto
    d["tcp_flags"] = 0x10
    d["tcp_off"] = 5
    d["seq"] = rng.integers(0, 2 ** 32, n)
    d["ack"] = rng.integers(0, 2 ** 32, n)
    d["win"] = 0x2000
    d["paylen"] = 64 - 54 if pitch == 64 else 1460
    offs = np.arange(n, dtype=np.uint64) * np.uint64(pitch)
    return d, offs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    n = a.n
    addr, mask, gw = 0x0A000005, 0xFFFF0000, 0x0A000001
    mac = bytes([2, 0xCA, 0x1A, 0xDA, 0, 5])
    net = G.txh_net(addr, mask, gw, mac)
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    rows = []
    dev = lambda x: torch.from_numpy(x.view(np.uint8) if x.dtype == G.TXH_DESC_DTYPE else x.view(np.int64)).cuda()
    for entries in (16, 4096, 65536):
        ips = (0x0A000100 + np.arange(entries)).astype(np.uint32)
        neigh = np.zeros(entries, dtype=G.NEIGH_ENTRY_DTYPE)
        neigh["ip"] = ips
        neigh["mac"][:] = np.frombuffer(mac, dtype=np.uint8)
        neigh["mac"][np.arange(entries) % 8 != 0, 5] = 9   # seven in eight are remote
        clf.neigh_set(neigh)
        tbl = G.NeighTable()
        tbl.set(neigh)
        for proto, pname in ((17, "udp"), (6, "tcp")):
            for pitch in (64, 1536):
                d, offs = make(G, n, proto, pitch, ips)
                frames = torch.zeros(n * pitch, dtype=torch.uint8, device="cuda")
                dd, do = dev(d), dev(offs)
                out = clf.tx_hdr(dd, do, n, frames, net)
                torch.cuda.synchronize()
                k = min(n, 4096)
                hf = np.zeros(k * pitch, dtype=np.uint8)
                h = G.tx_hdr_host(d[:k], offs[:k], hf, net, table=tbl)
                ok = bool(np.array_equal(frames[:k * pitch].cpu().numpy(), hf) and
                          np.array_equal(out["cmd"][:k].cpu().numpy().view(np.uint64), h["cmd"][:k]))
                med, best = median_us(lambda: clf.tx_hdr(dd, do, n, frames, net, out=out), a.iters)
                rows.append(dict(row=f"tx_hdr {pname} pitch {pitch}", neigh=entries, n=n, us=round(med, 1),
                                 best_us=round(best, 1), mpps=round(n / med, 1), matches_host=ok))
                del frames
    # the yardstick: gcl_copy_batch of 64-byte frames at the same n
    src = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    so = torch.arange(n, dtype=torch.int64, device="cuda") * 64
    ln = torch.full((n,), 64, dtype=torch.int16, device="cuda")
    bufs = clf.copy_batch(src, so, ln, n, dst, dst_stride=64, len_hint=64)
    med, best = median_us(lambda: clf.copy_batch(src, so, ln, n, dst, dst_stride=64, len_hint=64,
                                                 pkt_len=bufs[0], olflags=bufs[1], rss=bufs[2]), a.iters)
    rows.append(dict(row="copy_batch 64-byte frames", n=n, us=round(med, 1), best_us=round(best, 1),
                     mpps=round(n / med, 1)))
    # the host twin on one core
    k = max(n // 8, 1)
    d, offs = make(G, k, 17, 64, ips)
    hf = np.zeros(k * 64, dtype=np.uint8)
    out = G.tx_hdr_host(d, offs, hf, net, table=tbl)
    t0 = time.perf_counter()
    G.tx_hdr_host(d, offs, hf, net, table=tbl, out=out)
    dt = time.perf_counter() - t0
    rows.append(dict(row="tx_hdr_host udp pitch 64, one core", neigh=65536, n=k, us=round(dt * 1e6, 1),
                     mpps=round(k / (dt * 1e6), 2)))
    res = dict(tool="txhdr_bench", device=torch.cuda.get_device_name(0), n=n, iters=a.iters, rows=rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
