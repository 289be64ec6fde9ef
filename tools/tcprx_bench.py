#!/usr/bin/env python3
"""Time gcl_tcp_rx on the GPU beside gcl_l4_payload over the same list (the
same header reads: the floor of its first launch), a stable torch.sort of the
cookies (the grouping) and gcl_tcp_rx_host on one core.

  python tools/tcprx_bench.py [--m 1048576] [--rounds 15] [--out profiles/tcprx_bench.json]

m in-order TCP segments of 1448 payload bytes in 1536-byte slots, three ways:
  conns   65 536 connections x m / 65 536 segments, arrivals interleaved
  zipf    the same connections drawn by a Zipf law (exponent 1.1)
  one     one connection: serial by nature; its per-segment cost is reported
          beside the others', not hidden
Every GPU figure is the median over --rounds rounds; a round times every row
once, in turn, so that drift hits all alike; HIP events on the launch stream,
three warm-up rounds.  The first call's outputs are held to the host twin on
the 'one' shape's prefix and by the FAST count everywhere.  Prints one JSON
object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAY, SLOT, NCONN = 1448, 1536, 1 << 16


def shape(G, m, cookie, nconn, seed=5):
    """frames (u8[m, SLOT]), pkt_len, sock and conn of m in-order segments whose connections are @cookie"""
    rng = np.random.default_rng(seed)
    conn = np.zeros(nconn, dtype=G.TCP_CONN_DTYPE)
    conn["snd_una"] = rng.integers(0, 1 << 32, nconn)
    conn["snd_nxt"] = conn["snd_una"] + np.uint32(1000)
    conn["snd_wnd"], conn["rcv_wnd"], conn["rcv_mss"], conn["flags"] = 1 << 20, 0xFFFFFFFF, 1460, G.TCPC_ELIGIBLE
    conn["rcv_nxt"] = rng.integers(0, 1 << 32, nconn)
    conn["snd_wl1"] = conn["rcv_nxt"] - np.uint32(1)
    by = np.argsort(cookie, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(cookie, minlength=nconn))])[:-1]
    rank = np.empty(m, dtype=np.int64)
    rank[by] = np.arange(m) - start[cookie[by]]
    seq = (conn["rcv_nxt"][cookie].astype(np.int64) + rank * PAY) & 0xFFFFFFFF
    fr = np.zeros((m, SLOT), dtype=np.uint8)
    tot = 40 + PAY
    fr[:, 12:24] = (0x08, 0x00, 0x45, 0, tot >> 8, tot & 0xFF, 0, 0, 0x40, 0, 64, 6)
    for k in range(4):
        fr[:, 38 + k] = (seq >> (24 - 8 * k)) & 0xFF
        fr[:, 42 + k] = (conn["snd_una"][cookie].astype(np.int64) >> (24 - 8 * k)) & 0xFF
    fr[:, 46], fr[:, 47], fr[:, 48:50] = 0x50, 0x10, 0xFF
    return fr, np.full(m, 54 + PAY, dtype=np.uint16), cookie.astype(np.uint32), conn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="conns,zipf,one", help="which shapes to run (a kernel trace wants one)")
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    m = a.m
    rng = np.random.default_rng(6)
    p = np.arange(1, NCONN + 1) ** -1.1
    cookies = {"conns": (np.arange(m) % NCONN, NCONN),
               "zipf": (rng.choice(NCONN, m, p=p / p.sum()), NCONN),
               "one": (np.zeros(m, dtype=np.int64), 1)}
    cookies = {k: v for k, v in cookies.items() if k in a.shapes.split(",")}
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    jobs, rows, host_rows = [], [], []
    for name, (ck, nconn) in cookies.items():
        fr, plen, sock, conn = shape(G, m, ck, nconn)
        d = dict(fr=torch.from_numpy(fr).cuda(), plen=torch.from_numpy(plen.view(np.int16)).cuda(),
                 sock=torch.from_numpy(sock.view(np.int32)).cuda(),
                 conn=torch.from_numpy(conn.view(np.uint8).reshape(nconn, 48)).cuda())
        out = clf.tcp_rx(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT)
        pout = clf.l4_payload(d["fr"], m, d["plen"], stride=SLOT, sock=d["sock"])
        torch.cuda.synchronize()
        k = min(m, 1 << 17)
        t0 = time.perf_counter()
        h = G.tcp_rx_host(fr[:k].reshape(-1), plen[:k], sock[:k], conn, stride=SLOT)
        dt = time.perf_counter() - t0
        ok = bool((out["verdict"].cpu().numpy()[:m] == G.TCPRX_FAST).all())
        if name == "one":
            ok = ok and np.array_equal(out["dst_off"][:k].cpu().numpy().view(np.uint64), h["dst_off"][:k])
        rows.append(dict(row=f"tcp_rx {name}", m=m, nconn=nconn, all_fast_and_matches_host=ok))
        jobs.append((rows[-1], lambda d=d, nconn=nconn, out=out:
                     clf.tcp_rx(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT, out=out)))
        rows.append(dict(row=f"l4_payload over the list of {name}", m=m))
        jobs.append((rows[-1], lambda d=d, pout=pout:
                     clf.l4_payload(d["fr"], m, d["plen"], stride=SLOT, sock=d["sock"], out=pout)))
        rows.append(dict(row=f"torch.sort(stable) of the cookies of {name}", m=m))
        jobs.append((rows[-1], lambda d=d: torch.sort(d["sock"], stable=True)))
        host_rows.append(dict(row=f"tcp_rx_host {name}, one core", m=k, us=round(dt * 1e6, 1),
                              ns_per_seg=round(dt * 1e9 / k, 3)))
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
        row.update(us=round(float(np.median(t)), 1), best_us=round(float(np.min(t)), 1),
                   ns_per_seg=round(float(np.median(t)) * 1e3 / m, 3))
    res = dict(tool="tcprx_bench", device=torch.cuda.get_device_name(0), m=m, rounds=a.rounds,
               rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
