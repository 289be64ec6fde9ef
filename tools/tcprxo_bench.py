#!/usr/bin/env python3
"""Time gcl_tcp_rx_ooo on the GPU beside gcl_tcp_rx_full over the same list and
gcl_tcp_rx_ooo_host on one core.

  python tools/tcprxo_bench.py [--m 1048576] [--rounds 15] [--out profiles/tcprxo_bench.json]

m segments of 1448 bytes in 1536-byte slots over 65 536 connections whose
arrivals are interleaved, five ways:
  inorder   every segment in order, every queue empty (q_off NULL): the new walk
            adds the queue-empty test to gcl_tcp_rx_full's.  gcl_tcp_rx_full is
            timed on the same list twice per round: the spread between its two
            rows is the margin, and ratio_to_full is held against it
  swap1     1 % of the segments trade places with the next one of their
  swap10    connection, and 10 %: a queue of one entry, filled and drained
  fullq     in order, but every connection enters with 64 queue entries far
            ahead that never drain: every segment takes the slow rule and the
            drain test, and 4 Mi entries go in and come back out
  one       one connection holding every segment, 1 % swapped: the serial
            floor, in ns per segment
A sample is --reps calls between two HIP events on the launch stream (32 by
default: more than 10 ms a sample; profiles/tcprxo_bench.json was taken with
--rounds 10 --reps 24, which the file records); a round takes one sample of every row in
turn, so that drift hits all alike; three warm-up rounds; medians.  The first
call's outputs are held to the host twin on a prefix.  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tcprxf_bench import NCONN, SLOT, shape  # noqa: E402


def swapped(fr, nconn, frac, seed):
    """@frac of the segments trade places with the next one of their connection (arrivals are round-robin)"""
    m = len(fr)
    rng = np.random.default_rng(seed)
    j = np.nonzero((rng.random(m) < frac) & ((np.arange(m) // nconn) % 2 == 0) & (np.arange(m) + nconn < m))[0]
    fr = fr.copy()
    fr[j], fr[j + nconn] = fr[j + nconn].copy(), fr[j].copy()
    return fr, len(j)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="inorder,swap1,swap10,fullq,one")
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    m = a.m
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    jobs, rows, host_rows = [], [], []
    for name in a.shapes.split(","):
        nconn = 1 if name == "one" else NCONN
        ck = np.zeros(m, dtype=np.int64) if name == "one" else np.arange(m) % NCONN
        fr, plen, sock, conn = shape(G, m, ck, nconn, np.zeros(m, dtype=np.int64))
        nswap, q_off, q = 0, None, None
        if name in ("swap1", "swap10", "one"):
            fr, nswap = swapped(fr, nconn, 0.10 if name == "swap10" else 0.01, 7)
        if name == "fullq":
            conn["flags"] = G.TCPC_ESTABLISHED
            q = np.zeros(nconn * G.TCPOOO_CAP, dtype=G.TCP_OOO_ENT_DTYPE)
            k = np.arange(G.TCPOOO_CAP, dtype=np.uint32)[None, :]
            q["seq"] = (conn["rcv_nxt"][:, None] + np.uint32(1 << 28) + np.uint32(2000) * k).reshape(-1)
            q["end"] = q["seq"] + np.uint32(1448)
            q["ref"], q["flags"] = np.arange(len(q)), 0x10
            q_off = (np.arange(nconn + 1) * G.TCPOOO_CAP).astype(np.uint32)
        nq = 0 if q is None else len(q)
        cap = nq + m
        d = dict(fr=torch.from_numpy(fr).cuda(), plen=torch.from_numpy(plen.view(np.int16)).cuda(),
                 sock=torch.from_numpy(sock.view(np.int32)).cuda(),
                 conn=torch.from_numpy(conn.view(np.uint8).reshape(nconn, 48)).cuda(),
                 q_off=None if q is None else torch.from_numpy(q_off.view(np.int32)).cuda(),
                 q=None if q is None else torch.from_numpy(q.view(np.uint8).reshape(nq, 16)).cuda())
        cnt = torch.zeros(G.TCPRXOC_NR, dtype=torch.int64, device="cuda")
        kw = dict(stride=SLOT, q_off=d["q_off"], q=d["q"], nq=nq, q_out_cap=cap)
        out = clf.tcp_rx_ooo(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, counts=cnt, **kw)
        torch.cuda.synchronize()
        k = min(m, 1 << 17)
        t0 = time.perf_counter()
        h = G.tcp_rx_ooo_host(fr[:k].reshape(-1), plen[:k], sock[:k], conn, stride=SLOT, q_off=q_off, q=q, nq=nq,
                              q_out_cap=cap)
        dt = time.perf_counter() - t0
        c = cnt.cpu().numpy()
        ok = bool((out["verdict"].cpu().numpy()[:m] == G.TCPRX_FAST).all())
        # the prefix sees the same arrivals, so its entries agree except where a swap partner lies past it
        lim = k - nconn if nswap else k
        for f in ("sflags", "copy_len", "rcv_nxt_after"):
            ok = ok and np.array_equal(out[f][:lim].cpu().numpy().view(h[f].dtype), h[f][:lim])
        rows.append(dict(row=f"tcp_rx_ooo {name}", m=m, nconn=nconn, nq=nq, swaps=nswap,
                         all_handled_and_matches_host=ok, rule2=int(c[G.TCPRXFC_RULE2]), ooo=int(c[G.TCPRXOC_OOO]),
                         queued=int(c[G.TCPRXOC_QUEUED]), drained=int(c[G.TCPRXOC_DRAINED]),
                         held=int(c[G.TCPRXOC_HELD]), qout_entries=int(out["totals"].cpu().numpy().view(np.uint64)[0])))
        jobs.append((rows[-1], lambda d=d, nconn=nconn, out=out, kw=kw:
                     clf.tcp_rx_ooo(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, out=out, **kw)))
        if name == "inorder":
            old = clf.tcp_rx_full(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT)
            for tag in ("first row", "second row"):
                rows.append(dict(row=f"tcp_rx_full {name}, {tag}", m=m, nconn=nconn))
                jobs.append((rows[-1], lambda d=d, nconn=nconn, old=old:
                             clf.tcp_rx_full(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, stride=SLOT, out=old)))
        host_rows.append(dict(row=f"tcp_rx_ooo_host {name}, one core", m=k, us=round(dt * 1e6, 1),
                              ns_per_seg=round(dt * 1e9 / k, 3)))
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
                   worst_us=round(float(np.max(t)), 1), ns_per_seg=round(float(np.median(t)) * 1e3 / m, 3))
    by = {r["row"]: r for r in rows}
    if "tcp_rx_ooo inorder" in by:
        f1, f2 = by["tcp_rx_full inorder, first row"]["us"], by["tcp_rx_full inorder, second row"]["us"]
        by["tcp_rx_ooo inorder"].update(ratio_to_full=round(by["tcp_rx_ooo inorder"]["us"] / ((f1 + f2) / 2), 4),
                                        margin_us=round(abs(f1 - f2), 1),
                                        over_full_us=round(by["tcp_rx_ooo inorder"]["us"] - (f1 + f2) / 2, 1))
    res = dict(tool="tcprxo_bench", device=torch.cuda.get_device_name(0), m=m, rounds=a.rounds, reps=a.reps,
               rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
