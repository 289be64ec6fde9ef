#!/usr/bin/env python3
"""Time gcl_tcp_tick and gcl_tcp_rx_acks on the GPU beside the same compaction
in torch (torch.cumsum over the per-item segment counts plus a masked gather of
the emitting indices), gcl_tx_hdr over the segments they emit, and the host
twins on one core.

  python tools/tcptmr_bench.py [--nconn 1048576] [--rounds 15] [--out profiles/tcptmr_bench.json]

The sweep: nconn established connections whose timer is due for none, 1 % and
all of them; a due connection has a delayed ACK that ran out (one segment).
The ACK path: the outputs of one gcl_tcp_rx call over nconn in-order segments
of 65 536 connections (tools/tcprx_bench.py's 'conns' shape: every second
segment of a connection asks for an ACK).
Every GPU figure is the median over --rounds rounds; a round times every row
once, in turn, so that drift hits all alike; HIP events on the launch stream,
three warm-up rounds.  The first call's outputs are held to the host twin.
Prints one JSON object.
"""
import argparse
import datetime
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

NOW = 10_000_000_000


def sweep_shape(G, nconn, due, seed=7):
    rng = np.random.default_rng(seed)
    tmr = np.zeros(nconn, dtype=G.TCP_TMR_DTYPE)
    hit = rng.random(nconn) < due if 0 < due < 1 else np.full(nconn, due >= 1)
    tmr["next_timeout"] = np.where(hit, NOW - 3, NOW + 5000)
    tmr["ack_ts"] = NOW - 10003
    tmr["state"], tmr["flags"] = G.TCP_STATE_ESTABLISHED, G.TMR_LIVE | G.TMR_ACK_DELAYED
    conn = np.zeros(nconn, dtype=G.TCP_CONN_DTYPE)
    for f in ("snd_una", "snd_nxt", "rcv_nxt", "rcv_wnd"):
        conn[f] = rng.integers(0, 1 << 32, nconn)
    addr = np.zeros(nconn, dtype=G.TCP_ADDR_DTYPE)
    addr["lip"], addr["rip"] = 0x0A000005, 0x0A000014 + rng.integers(0, 3, nconn)
    addr["lport"], addr["rport"], addr["rcv_wscale"] = rng.integers(1, 1 << 16, nconn), 80, 7
    return tmr, conn, addr, int(hit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nconn", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G
    from tcprx_bench import NCONN, SLOT, shape

    n = a.nconn
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    clf.neigh_set([(0x0A000014 + k, bytes([2, 0, 0, 0, 1, k])) for k in range(3)])
    net = G.txh_net(0x0A000005, 0xFFFFFF00, 0x0A000001, bytes([2, 0, 0, 0, 0, 5]))
    jobs, rows, host_rows = [], [], []

    def rec(x):
        return torch.from_numpy(x.view(np.uint8).reshape(len(x), -1)).cuda()

    def add(row, fn):
        rows.append(row)
        jobs.append((row, fn))

    def yardsticks(name, counts, k, out):
        """the same compaction in torch, and gcl_tx_hdr over the k segments"""
        idx = torch.arange(len(counts), dtype=torch.int32, device="cuda")

        def scan_gather():
            pos = torch.cumsum(counts, 0)
            return pos, idx[counts != 0]
        add(dict(row=f"torch.cumsum + masked gather over the counts of {name}", items=len(counts), segs=k), scan_gather)
        if k:
            frames = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
            hout = clf.tx_hdr(out["desc"], out["frame_off"], k, frames, net)
            add(dict(row=f"tx_hdr over the segments of {name}", segs=k),
                lambda: clf.tx_hdr(out["desc"], out["frame_off"], k, frames, net, out=hout))

    for name, due in (("none due", 0.0), ("1 % due", 0.01), ("all due", 1.0)):
        tmr, conn, addr, k = sweep_shape(G, n, due)
        d = dict(tmr=rec(tmr), conn=rec(conn), addr=rec(addr))
        out = clf.tcp_tick(NOW, d["tmr"], d["conn"], d["addr"], n, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = G.tcp_tick_host(NOW, tmr, conn, addr, n)
        dt = time.perf_counter() - t0
        ok = out["totals"].cpu().numpy().tolist() == [k, k] == h["totals"].tolist() and \
            np.array_equal(out["desc"].cpu().numpy()[:k].reshape(-1), h["desc"][:k].view(np.uint8)) and \
            np.array_equal(out["out_tmr"].cpu().numpy().reshape(-1), h["out_tmr"].view(np.uint8))
        add(dict(row=f"tcp_tick {name}", items=n, segs=k, matches_host=bool(ok)),
            lambda d=d, out=out: clf.tcp_tick(NOW, d["tmr"], d["conn"], d["addr"], n, n, out=out))
        counts = torch.from_numpy((tmr["next_timeout"] <= NOW).astype(np.int32)).cuda()
        yardsticks(f"tcp_tick {name}", counts, k, out)
        host_rows.append(dict(row=f"tcp_tick_host {name}, one core", items=n, segs=k, us=round(dt * 1e6, 1),
                              ns_per_item=round(dt * 1e9 / n, 3)))

    ck = np.arange(n) % NCONN
    fr, plen, sock, conn = shape(G, n, ck, NCONN)
    addr = sweep_shape(G, NCONN, 0.0)[2]
    d = dict(fr=torch.from_numpy(fr).cuda(), plen=torch.from_numpy(plen.view(np.int16)).cuda(),
             sock=torch.from_numpy(sock.view(np.int32)).cuda(), conn=rec(conn), addr=rec(addr))
    rx = clf.tcp_rx(d["fr"], n, d["plen"], d["sock"], d["conn"], NCONN, stride=SLOT)
    out = clf.tcp_rx_acks(rx["verdict"], rx["sflags"], rx["rcv_nxt_after"], n, d["sock"], n, d["conn"], d["addr"],
                          NCONN, n)
    torch.cuda.synchronize()
    hv = {f: rx[f].cpu().numpy()[:n] for f in ("verdict", "sflags")}
    hv["rcv_nxt_after"] = rx["rcv_nxt_after"].cpu().numpy()[:n].view(np.uint32)
    t0 = time.perf_counter()
    h = G.tcp_rx_acks_host(hv["verdict"], hv["sflags"], hv["rcv_nxt_after"], sock, conn, addr, n)
    dt = time.perf_counter() - t0
    k = int(h["totals"][1])
    ok = out["totals"].cpu().numpy().tolist() == h["totals"].tolist() and \
        np.array_equal(out["desc"].cpu().numpy()[:k].reshape(-1), h["desc"][:k].view(np.uint8))
    add(dict(row="tcp_rx_acks of a tcp_rx call", items=n, segs=k, matches_host=bool(ok)),
        lambda: clf.tcp_rx_acks(rx["verdict"], rx["sflags"], rx["rcv_nxt_after"], n, d["sock"], n, d["conn"],
                                d["addr"], NCONN, n, out=out))
    counts = ((rx["sflags"][:n] & G.TCPRX_SF_ACK_NOW) != 0).to(torch.int32)
    yardsticks("tcp_rx_acks", counts, k, out)
    host_rows.append(dict(row="tcp_rx_acks_host, one core", items=n, segs=k, us=round(dt * 1e6, 1),
                          ns_per_item=round(dt * 1e9 / n, 3)))

    ts = {id(r): [] for r, _ in jobs}
    for rnd in range(3 + a.rounds):
        for row, fn in jobs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= 3:
                ts[id(row)].append(e0.elapsed_time(e1) * 1e3)
    for row, _ in jobs:
        t = ts[id(row)]
        row.update(us=round(float(np.median(t)), 1), best_us=round(float(np.min(t)), 1))
        if "items" in row:
            row["ns_per_item"] = round(float(np.median(t)) * 1e3 / row["items"], 3)
    res = dict(tool="tcptmr_bench", date=datetime.date.today().isoformat(), device=torch.cuda.get_device_name(0),
               nconn=n, rounds=a.rounds, rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
