#!/usr/bin/env python3
"""Time gcl_tcp_rx_full on the GPU beside gcl_tcp_rx over the same list and
gcl_tcp_rx_full_host on one core.

  python tools/tcprxf_bench.py [--m 1048576] [--rounds 15] [--out profiles/tcprxf_bench.json]

m segments in 1536-byte slots, four ways:
  fast    65 536 connections, in-order text of 1448 bytes, arrivals
          interleaved: every segment takes the fast path.  gcl_tcp_rx is timed
          on the same list, twice per round: the spread between its two rows is
          the margin the new walk is held against
  acks    the same connections, every segment a pure ACK that moves snd_una
  zipf    connections drawn by a Zipf law (exponent 1.1); a third of the
          segments pure ACKs, 1 % duplicates, the rest in-order text
  one     one connection holding every segment (half text, half pure ACKs):
          the serial floor, in ns per segment
Every GPU figure is the median over --rounds rounds; a round times every row
once, in turn, so that drift hits all alike; HIP events on the launch stream,
three warm-up rounds.  The first call's outputs are held to the host twin on
a prefix and by the handled count everywhere.  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAY, SLOT, NCONN = 1448, 1536, 1 << 16


def shape(G, m, cookie, nconn, kind, seed=5):
    """frames (u8[m, SLOT]), pkt_len, sock and conn of m segments whose connections are @cookie; @kind[k] is
    0 text, 1 a pure ACK that moves snd_una by one, 2 a duplicate ACK (a window of 0)"""
    rng = np.random.default_rng(seed)
    conn = np.zeros(nconn, dtype=G.TCP_CONN_DTYPE)
    conn["snd_una"] = rng.integers(0, 1 << 32, nconn)
    # 2^29 bytes in flight under a window of 0xFFFF << 14: the send window never fills
    conn["snd_nxt"] = conn["snd_una"] + np.uint32(1 << 29)
    conn["snd_wnd"], conn["snd_wscale"] = 0xFFFF << 14, 14
    conn["rcv_wnd"], conn["rcv_mss"], conn["flags"] = 0x7FFFFFFF, 1460, G.TCPC_ELIGIBLE
    conn["rcv_nxt"] = rng.integers(0, 1 << 32, nconn)
    conn["snd_wl1"] = conn["rcv_nxt"] - np.uint32(1)
    conn["snd_wl2"] = conn["snd_una"]
    by = np.argsort(cookie, kind="stable")
    start = np.concatenate([[0], np.cumsum(np.bincount(cookie, minlength=nconn))])[:-1]

    def before(x):
        """per entry, the sum of @x over the earlier entries of its connection"""
        xs = x[by].astype(np.int64)
        cs = np.cumsum(xs) - xs
        res = np.empty(m, dtype=np.int64)
        res[by] = cs - cs[start[cookie[by]]]
        return res

    ln = np.where(kind == 0, PAY, 0)
    seq = (conn["rcv_nxt"][cookie].astype(np.int64) + before(ln)) & 0xFFFFFFFF
    ack = (conn["snd_una"][cookie].astype(np.int64) + before(kind == 1) + (kind == 1)) & 0xFFFFFFFF
    fr = np.zeros((m, SLOT), dtype=np.uint8)
    tot = 40 + ln
    fr[:, 12:24] = (0x08, 0x00, 0x45, 0, 0, 0, 0, 0, 0x40, 0, 64, 6)
    fr[:, 16], fr[:, 17] = tot >> 8, tot & 0xFF
    for k in range(4):
        fr[:, 38 + k] = (seq >> (24 - 8 * k)) & 0xFF
        fr[:, 42 + k] = (ack >> (24 - 8 * k)) & 0xFF
    fr[:, 46], fr[:, 47] = 0x50, 0x10
    fr[:, 48] = fr[:, 49] = np.where(kind == 2, 0, 0xFF)
    return fr, (54 + ln).astype(np.uint16), cookie.astype(np.uint32), conn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="fast,acks,zipf,one")
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    m = a.m
    rng = np.random.default_rng(6)
    p = np.arange(1, NCONN + 1) ** -1.1
    u = rng.random(m)
    shapes = {"fast": (np.arange(m) % NCONN, NCONN, np.zeros(m, dtype=np.int64)),
              "acks": (np.arange(m) % NCONN, NCONN, np.ones(m, dtype=np.int64)),
              "zipf": (rng.choice(NCONN, m, p=p / p.sum()), NCONN, np.where(u < 0.01, 2, np.where(u < 0.34, 1, 0))),
              "one": (np.zeros(m, dtype=np.int64), 1, (np.arange(m) & 1).astype(np.int64))}
    shapes = {k: v for k, v in shapes.items() if k in a.shapes.split(",")}
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    jobs, rows, host_rows = [], [], []
    for name, (ck, nconn, kind) in shapes.items():
        fr, plen, sock, conn = shape(G, m, ck, nconn, kind)
        d = dict(fr=torch.from_numpy(fr).cuda(), plen=torch.from_numpy(plen.view(np.int16)).cuda(),
                 sock=torch.from_numpy(sock.view(np.int32)).cuda(),
                 conn=torch.from_numpy(conn.view(np.uint8).reshape(nconn, 48)).cuda())
        cnt = torch.zeros(G.TCPRXFC_NR, dtype=torch.int64, device="cuda")
        out = clf.tcp_rx_full(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT, counts=cnt)
        torch.cuda.synchronize()
        k = min(m, 1 << 17)
        t0 = time.perf_counter()
        h = G.tcp_rx_full_host(fr[:k].reshape(-1), plen[:k], sock[:k], conn, stride=SLOT)
        dt = time.perf_counter() - t0
        c = cnt.cpu().numpy()
        ok = bool((out["verdict"].cpu().numpy()[:m] == G.TCPRX_FAST).all())
        for f in ("sflags", "copy_len", "rcv_nxt_after"):
            ok = ok and np.array_equal(out[f][:k].cpu().numpy().view(h[f].dtype), h[f][:k])
        rows.append(dict(row=f"tcp_rx_full {name}", m=m, nconn=nconn, all_handled_and_matches_host=ok,
                         rule2=int(c[G.TCPRXFC_RULE2]), dupacks=int(c[G.TCPRXFC_DUPACKS]),
                         fastrtx=int(c[G.TCPRXFC_FASTRTX])))
        jobs.append((rows[-1], lambda d=d, nconn=nconn, out=out:
                     clf.tcp_rx_full(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT, out=out)))
        if name == "fast":
            old = clf.tcp_rx(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT)
            for tag in ("first row", "second row"):
                rows.append(dict(row=f"tcp_rx {name}, {tag}", m=m, nconn=nconn))
                jobs.append((rows[-1], lambda d=d, nconn=nconn, old=old:
                             clf.tcp_rx(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT, out=old)))
        host_rows.append(dict(row=f"tcp_rx_full_host {name}, one core", m=k, us=round(dt * 1e6, 1),
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
                   worst_us=round(float(np.max(t)), 1), ns_per_seg=round(float(np.median(t)) * 1e3 / m, 3))
    res = dict(tool="tcprxf_bench", device=torch.cuda.get_device_name(0), m=m, rounds=a.rounds,
               rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
