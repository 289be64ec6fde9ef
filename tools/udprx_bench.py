#!/usr/bin/env python3
"""Time gcl_udp_rx on the GPU beside gcl_l4_payload over the same list (the
same header reads: the floor of its first launch), a stable torch.sort of the
cookies (the grouping), gcl_tcp_rx over the same three shapes as TCP segments,
and gcl_udp_rx_host on one core.

  python tools/udprx_bench.py [--m 1048576] [--rounds 15] [--out profiles/udprx_bench.json]

m UDP datagrams in 64-byte frames, three ways:
  socks   65 536 sockets x m / 65 536 datagrams, arrivals interleaved
  zipf    the same sockets drawn by a Zipf law (exponent 1.1)
  one     one socket takes every datagram
each with room for every datagram ("room") and with inq_cap 512 from an empty
queue ("cap512").  Every GPU figure is the median over --rounds rounds; a round
times every row once, in turn, so that drift hits all alike; HIP events on the
launch stream, three warm-up rounds, all in one process.  The first call's
verdict counts are held to the closed count of what fits, and its outputs to
the host twin on a prefix of the list.  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOT, NSOCK, PAY_UDP, PAY_TCP, CAP = 64, 1 << 16, 22, 8, 512


def udp_frames(m, cookie):
    fr = np.zeros((m, SLOT), dtype=np.uint8)
    tot = 28 + PAY_UDP
    fr[:, 12:24] = (0x08, 0x00, 0x45, 0, tot >> 8, tot & 0xFF, 0, 0, 0x40, 0, 64, 17)
    fr[:, 26:30] = (10, 0, 0, 2)
    fr[:, 34] = 0x80 | ((cookie >> 8) & 0x7F)
    fr[:, 35] = cookie & 0xFF
    return fr, np.full(m, 14 + tot, dtype=np.uint16)


def tcp_frames(G, m, cookie, nconn, seed=5):
    """m in-order TCP segments of PAY_TCP bytes in the same 64-byte slots, and their connections"""
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
    seq = (conn["rcv_nxt"][cookie].astype(np.int64) + rank * PAY_TCP) & 0xFFFFFFFF
    fr = np.zeros((m, SLOT), dtype=np.uint8)
    tot = 40 + PAY_TCP
    fr[:, 12:24] = (0x08, 0x00, 0x45, 0, tot >> 8, tot & 0xFF, 0, 0, 0x40, 0, 64, 6)
    for k in range(4):
        fr[:, 38 + k] = (seq >> (24 - 8 * k)) & 0xFF
        fr[:, 42 + k] = (conn["snd_una"][cookie].astype(np.int64) >> (24 - 8 * k)) & 0xFF
    fr[:, 46], fr[:, 47], fr[:, 48:50] = 0x50, 0x10, 0xFF
    return fr, np.full(m, 14 + tot, dtype=np.uint16), conn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="socks,zipf,one", help="which shapes to run (a kernel trace wants one)")
    ap.add_argument("--no-yardsticks", action="store_true", help="gcl_udp_rx rows only (a kernel trace)")
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    m = a.m
    rng = np.random.default_rng(6)
    p = np.arange(1, NSOCK + 1) ** -1.1
    cookies = {"socks": (np.arange(m) % NSOCK, NSOCK),
               "zipf": (rng.choice(NSOCK, m, p=p / p.sum()), NSOCK),
               "one": (np.zeros(m, dtype=np.int64), 1)}
    cookies = {k: v for k, v in cookies.items() if k in a.shapes.split(",")}
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    t = lambda x: torch.from_numpy(x).cuda()
    jobs, rows, host_rows = [], [], []
    for name, (ck, ns) in cookies.items():
        fr, plen = udp_frames(m, ck)
        sock = ck.astype(np.uint32)
        per = np.bincount(ck, minlength=ns)
        d = dict(fr=t(fr), plen=t(plen.view(np.int16)), sock=t(sock.view(np.int32)))
        for var, cap in (("room", m + 1), ("cap512", CAP)):
            us = np.zeros(ns, dtype=G.UDP_SOCK_DTYPE)
            us["inq_cap"] = cap
            dus = t(us.view(np.uint8).reshape(ns, 16))
            out = clf.udp_rx(d["fr"], m, d["plen"], d["sock"], dus, ns, stride=SLOT)
            torch.cuda.synchronize()
            v = out["verdict"].cpu().numpy()[:m]
            fits = int(np.minimum(per, cap).sum())
            k = min(m, 1 << 17)
            t0 = time.perf_counter()
            h = G.udp_rx_host(fr[:k].reshape(-1), plen[:k], sock[:k], us, stride=SLOT)
            dt = time.perf_counter() - t0
            ok = int((v == G.UDPRX_QUEUED).sum()) == fits and int((v == G.UDPRX_FULL).sum()) == m - fits
            ok = ok and np.array_equal(v[:k] == G.UDPRX_QUEUED, h["verdict"][:k] == G.UDPRX_QUEUED) if var == "room" \
                else ok
            rows.append(dict(row=f"udp_rx {name} {var}", m=m, nsock=ns, queued=fits, counts_and_host_prefix_ok=bool(ok)))
            jobs.append((rows[-1], lambda d=d, ns=ns, out=out, dus=dus:
                         clf.udp_rx(d["fr"], m, d["plen"], d["sock"], dus, ns, stride=SLOT, out=out)))
            host_rows.append(dict(row=f"udp_rx_host {name} {var}, one core", m=k, us=round(dt * 1e6, 1),
                                  ns_per_dgram=round(dt * 1e9 / k, 3)))
        if a.no_yardsticks:
            continue
        pout = clf.l4_payload(d["fr"], m, d["plen"], stride=SLOT, sock=d["sock"])
        rows.append(dict(row=f"l4_payload over the list of {name}", m=m))
        jobs.append((rows[-1], lambda d=d, pout=pout:
                     clf.l4_payload(d["fr"], m, d["plen"], stride=SLOT, sock=d["sock"], out=pout)))
        rows.append(dict(row=f"torch.sort(stable) of the cookies of {name}", m=m))
        jobs.append((rows[-1], lambda d=d: torch.sort(d["sock"], stable=True)))
        tfr, tplen, conn = tcp_frames(G, m, ck, ns)
        td = dict(fr=t(tfr), plen=t(tplen.view(np.int16)), conn=t(conn.view(np.uint8).reshape(ns, 48)))
        tout = clf.tcp_rx(td["fr"], m, td["plen"], d["sock"], td["conn"], ns, stride=SLOT)
        torch.cuda.synchronize()
        rows.append(dict(row=f"tcp_rx over {name} as TCP segments", m=m, nconn=ns,
                         all_fast=bool((tout["verdict"].cpu().numpy()[:m] == G.TCPRX_FAST).all())))
        jobs.append((rows[-1], lambda d=d, td=td, ns=ns, tout=tout:
                     clf.tcp_rx(td["fr"], m, td["plen"], d["sock"], td["conn"], ns, stride=SLOT, out=tout)))
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
        x = ts[id(row)]
        row.update(us=round(float(np.median(x)), 1), best_us=round(float(np.min(x)), 1),
                   ns_per_entry=round(float(np.median(x)) * 1e3 / m, 3))
    res = dict(tool="udprx_bench", device=torch.cuda.get_device_name(0), m=m, rounds=a.rounds,
               rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
