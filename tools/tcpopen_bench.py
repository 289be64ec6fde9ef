#!/usr/bin/env python3
"""Time gcl_tcp_rx_open on the GPU, gcl_sock_lookup + gcl_tcp_rx_ctl over the
same frames beside it, and gcl_tcp_rx_open_host on one core.

  python tools/tcpopen_bench.py [--m 1048576] [--rounds 15] [--out profiles/tcpopen_bench.json]

The same m SYN frames (MSS and WSCALE options, 128-byte slots, m distinct
tuples spread over 16 listeners) for every row; the rows differ in the cookies,
the order and the backlogs:
  miss      every cookie GCL_SOCK_MISS: every entry a CLOSED_RST_ACK
  distinct  every entry a SYN of its own tuple on a listener with room: every
            entry an ACCEPT
  repeat10  the same with one entry in ten naming an earlier packet again:
            those are LATER
  full64    every listener full after its first 64
and, for comparison, gcl_sock_lookup over the frames and gcl_tcp_rx_ctl over m
entries that each ask for a RST|ACK.  A sample is --reps calls between two HIP
events on the launch stream; a round takes one sample of every row in turn;
three warm-up rounds; medians.  The first call's outputs are held to the host
twin on a prefix.  No time is a pass criterion.  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SLOT, NLISTEN, BASE = 128, 16, 1000
LIP, RIP0 = 0x0A000001, 0x0B000000


def frames_of(m):
    """m SYN frames: daddr LIP, dport 80 + i % 16, saddr and sport from i, options MSS 1460 and WSCALE 7"""
    f = np.zeros((m, SLOT), dtype=np.uint8)
    i = np.arange(m, dtype=np.uint64)
    f[:, 12], f[:, 14], f[:, 17], f[:, 22], f[:, 23] = 0x08, 0x45, 48, 64, 6
    rip = (RIP0 + (i >> np.uint64(14))).astype(np.uint32)
    for k in range(4):
        f[:, 26 + k] = (rip >> (24 - 8 * k)) & 0xFF
        f[:, 30 + k] = (LIP >> (24 - 8 * k)) & 0xFF
        f[:, 38 + k] = ((i * np.uint64(2654435761)) >> np.uint64(24 - 8 * k)) & np.uint64(0xFF)
    sport = (1024 + (i & np.uint64(0x3FFF))).astype(np.uint32)
    f[:, 34], f[:, 35] = sport >> 8, sport & 0xFF
    f[:, 37] = 80 + (i % np.uint64(NLISTEN))
    f[:, 46], f[:, 47], f[:, 48] = 7 << 4, 0x02, 0xFF
    f[:, 54:62] = [2, 4, 0x05, 0xB4, 1, 3, 3, 7]
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    m = a.m
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    t8 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    fr = frames_of(m)
    plen = np.full(m, 62, dtype=np.uint16)
    iss = (np.arange(m, dtype=np.uint64) * np.uint64(40503) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rng = np.random.default_rng(1)
    ident = np.arange(m, dtype=np.uint32)
    rep = ident.copy()
    again = rng.random(m) < 0.1
    rep[again] = (rng.random(int(again.sum())) * ident[again]).astype(np.uint32)
    shapes = {"miss": (np.full(m, G.SOCK_MISS, dtype=np.uint32), ident, 1 << 20),
              "distinct": ((BASE + ident % NLISTEN).astype(np.uint32), ident, 1 << 20),
              "repeat10": ((BASE + ident % NLISTEN).astype(np.uint32), rep, 1 << 20),
              "full64": ((BASE + ident % NLISTEN).astype(np.uint32), ident, 64)}
    d_fr, d_plen, d_iss = t8(fr), t8(plen.view(np.int16)), t8(iss.view(np.int32))
    tx = torch.zeros(m * 64, dtype=torch.uint8, device="cuda")
    jobs, rows, host_rows = [], [], []
    k = min(m, 1 << 17)
    for name, (sock, order, backlog) in shapes.items():
        listen = np.zeros(NLISTEN, dtype=G.TCP_LISTEN_DTYPE)
        listen["backlog"], listen["winmax"], listen["rcv_mss"], listen["rcv_wscale"] = backlog, 1 << 20, 1460, 5
        d = dict(sock=t8(sock.view(np.int32)), order=t8(order.view(np.int32)),
                 listen=t8(listen.view(np.uint8).reshape(NLISTEN, 16)))
        cnt = torch.zeros(G.OPENC_NR, dtype=torch.int64, device="cuda")
        call = lambda d=d, out=None, cnt=None: clf.tcp_rx_open(
            d_fr, m, d_plen, d["sock"], m, d["listen"], NLISTEN, d_iss, m, m, tx, stride=SLOT, order=d["order"],
            listen_base=BASE, out=out, counts=cnt)
        out = call(cnt=cnt)
        torch.cuda.synchronize()
        htx = np.zeros(k * 64, dtype=np.uint8)
        t0 = time.perf_counter()
        h = G.tcp_rx_open_host(fr.reshape(-1), plen, sock, listen, iss[:k], k, k, htx, stride=SLOT, order=order[:k], m=k,
                               listen_base=BASE)
        dt = time.perf_counter() - t0
        c = cnt.cpu().numpy()
        ok = all(np.array_equal(out[f][:k].cpu().numpy().reshape(-1).view(h[f].dtype)[:k], h[f][:k])
                 for f in ("verdict", "later_of", "rst_seq"))
        rows.append(dict(row=f"tcp_rx_open {name}", m=m, prefix_matches_host=bool(ok), accepts=int(c[G.OPEN_ACCEPT]),
                         later=int(c[G.OPEN_LATER]), full=int(c[G.OPEN_FULL]),
                         closed_rst_ack=int(c[G.OPEN_CLOSED_RST_ACK]), segs=int(c[G.OPENC_SEGS])))
        jobs.append((rows[-1], lambda call=call, out=out: call(out=out)))
        host_rows.append(dict(row=f"tcp_rx_open_host {name}, one core", m=k, us=round(dt * 1e6, 1),
                              ns_per_entry=round(dt * 1e9 / k, 3)))
    # the comparison: the demux of the same frames, and a control-segment call where every entry asks for a RST|ACK
    clf.runtime_set(1, LIP, 8, 8, list(range(8)))
    clf.sock_set(1, [])
    verd = torch.zeros(m * clf.vbytes, dtype=torch.uint8, device="cuda")
    clf.classify(d_fr, m, stride=SLOT, verdicts=verd)
    sk = torch.zeros(m, dtype=torch.int32, device="cuda")
    clf.sock_lookup(d_fr, m, stride=SLOT, verdicts=verd, sock=sk)
    rows.append(dict(row="sock_lookup", m=m))
    jobs.append((rows[-1], lambda: clf.sock_lookup(d_fr, m, stride=SLOT, verdicts=verd, sock=sk)))
    z8 = torch.zeros(m, dtype=torch.uint8, device="cuda")
    z32 = torch.zeros(m, dtype=torch.int32, device="cuda")
    ev = torch.full((m,), G.TCPS_RST_ACK, dtype=torch.uint8, device="cuda")
    conn = torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
    addr = torch.zeros((1, 16), dtype=torch.uint8, device="cuda")
    ctl = lambda out=None: clf.tcp_rx_ctl(z8, z8, z32, ev, z32, m, z32, m, conn, addr, 1, m, out=out)
    co = ctl()
    rows.append(dict(row="tcp_rx_ctl, every entry a RST|ACK", m=m))
    jobs.append((rows[-1], lambda: ctl(out=co)))
    ts = {id(r): [] for r, _ in jobs}
    for rnd in range(3 + a.rounds):
        for row, fn in jobs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            e1.synchronize()
            if rnd >= 3:
                ts[id(row)].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    for row, _ in jobs:
        t = ts[id(row)]
        row.update(us=round(float(np.median(t)), 1), best_us=round(float(np.min(t)), 1),
                   worst_us=round(float(np.max(t)), 1), ns_per_entry=round(float(np.median(t)) * 1e3 / m, 3))
    by = {r["row"]: r for r in rows}
    both = by["sock_lookup"]["us"] + by["tcp_rx_ctl, every entry a RST|ACK"]["us"]
    hb = {r["row"]: r for r in host_rows}
    for name in shapes:
        r = by[f"tcp_rx_open {name}"]
        r.update(ratio_to_lookup_plus_ctl=round(r["us"] / both, 3),
                 host_one_core_over_gpu=round(hb[f"tcp_rx_open_host {name}, one core"]["ns_per_entry"] /
                                              r["ns_per_entry"], 1))
    res = dict(tool="tcpopen_bench", device=torch.cuda.get_device_name(0), m=m, rounds=a.rounds, reps=a.reps,
               rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
