#!/usr/bin/env python3
"""Time gcl_tcp_rx_states on the GPU beside gcl_tcp_rx_ooo over the same list,
gcl_tcp_rx_ctl beside gcl_tcp_rx_acks, and the two host twins on one core.

  python tools/tcprxs_bench.py [--m 1048576] [--rounds 15] [--out profiles/tcprxs_bench.json]

m segments in 1536-byte slots over 65 536 connections whose arrivals are
interleaved, four ways:
  inorder    1448-byte segments in order, every connection ESTABLISHED (state
             given), every queue empty.  gcl_tcp_rx_ooo is timed on the same
             list twice per round: the spread between its two rows is the
             margin, and ratio_to_ooo is held against it
  lifetimes  every connection enters in SYN_RECEIVED and gets the ACK that
             opens it, 14 data segments and a FIN: sixteen segments, the first
             and the last under the slow rule
  closed     the inorder list with every connection CLOSED: every segment is
             answered by a RST|ACK and nothing else moves
  one        one ESTABLISHED connection holding every segment: the serial
             floor, in ns per segment
and gcl_tcp_rx_ctl beside gcl_tcp_rx_acks over the outputs of the inorder call
(ACKs only), and over the outputs of the closed call (every entry a RST|ACK).
A sample is --reps calls between two HIP events on the launch stream; a round
takes one sample of every row in turn, so that drift hits all alike; three
warm-up rounds; medians.  The first call's outputs are held to the host twin
on a prefix.  Prints one JSON object.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="inorder,lifetimes,closed,one")
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    m = a.m
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    jobs, rows, host_rows = [], [], []
    t8 = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    for name in a.shapes.split(","):
        nconn = 1 if name == "one" else NCONN
        ck = np.zeros(m, dtype=np.int64) if name == "one" else np.arange(m) % NCONN
        kind = np.zeros(m, dtype=np.int64)
        state = np.full(nconn, G.TCP_STATE_ESTABLISHED, dtype=np.uint8)
        if name == "lifetimes":
            r = np.arange(m) // NCONN
            kind[(r % 16 == 0) | (r % 16 == 15)] = 1
            state[:] = G.TCP_STATE_SYN_RECEIVED
        if name == "closed":
            state[:] = G.TCP_STATE_CLOSED
        fr, plen, sock, conn = shape(G, m, ck, nconn, kind)
        if name == "lifetimes":
            fr[(np.arange(m) // NCONN) % 16 == 15, 47] |= 0x01
        d = dict(fr=t8(fr), plen=t8(plen.view(np.int16)), sock=t8(sock.view(np.int32)),
                 conn=t8(conn.view(np.uint8).reshape(nconn, 48)), state=t8(state))
        cnt = torch.zeros(G.TCPRXSC_NR, dtype=torch.int64, device="cuda")
        kw = dict(stride=SLOT, q_out_cap=m)
        out = clf.tcp_rx_states(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, state=d["state"], counts=cnt, **kw)
        torch.cuda.synchronize()
        k = min(m, 1 << 17)
        t0 = time.perf_counter()
        h = G.tcp_rx_states_host(fr[:k].reshape(-1), plen[:k], sock[:k], conn, stride=SLOT, q_out_cap=m, state=state)
        dt = time.perf_counter() - t0
        c = cnt.cpu().numpy()
        ok = bool((out["verdict"].cpu().numpy()[:m] == G.TCPRX_FAST).all())
        for f in ("sflags", "copy_len", "rcv_nxt_after", "ev", "rst_seq", "state_after"):
            ok = ok and np.array_equal(out[f][:k].cpu().numpy().reshape(-1).view(h[f].dtype)[:k], h[f][:k])
        rows.append(dict(row=f"tcp_rx_states {name}", m=m, nconn=nconn, all_handled_and_matches_host=ok,
                         rule2=int(c[G.TCPRXFC_RULE2]), acks=int(c[G.TCPRXC_ACKS]), rsts=int(c[G.TCPRXSC_RSTS]),
                         fins=int(c[G.TCPRXSC_FINS]), state_changes=int(c[G.TCPRXSC_STATE_CHANGES])))
        jobs.append((rows[-1], lambda d=d, nconn=nconn, out=out, kw=kw:
                     clf.tcp_rx_states(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, state=d["state"], out=out,
                                       **kw)))
        host_rows.append(dict(row=f"tcp_rx_states_host {name}, one core", m=k, us=round(dt * 1e6, 1),
                              ns_per_seg=round(dt * 1e9 / k, 3)))
        if name == "inorder":
            old = clf.tcp_rx_ooo(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, **kw)
            for tag in ("first row", "second row"):
                rows.append(dict(row=f"tcp_rx_ooo {name}, {tag}", m=m, nconn=nconn))
                jobs.append((rows[-1], lambda d=d, nconn=nconn, old=old, kw=kw:
                             clf.tcp_rx_ooo(d["fr"], m, d["plen"], d["sock"], d["conn"], nconn, out=old, **kw)))
        if name in ("inorder", "closed"):
            addr = torch.zeros((nconn, 16), dtype=torch.uint8, device="cuda")
            ca = (out["verdict"], out["sflags"], out["rcv_nxt_after"])
            cb = (m, d["sock"], m, d["conn"], addr, nconn, m)
            co = clf.tcp_rx_ctl(*ca, out["ev"], out["rst_seq"], *cb)
            ao = clf.tcp_rx_acks(*ca, *cb)
            torch.cuda.synchronize()
            wrote = int(co["totals"].cpu().numpy().view(np.uint64)[1])
            same = all(torch.equal(co[f][:wrote], ao[f][:wrote]) for f in ("desc", "seg_src")) if name == "inorder" \
                else None
            rows.append(dict(row=f"tcp_rx_ctl {name}", m=m, segments=wrote, equals_tcp_rx_acks=same))
            jobs.append((rows[-1], lambda ca=ca, cb=cb, out=out, co=co:
                         clf.tcp_rx_ctl(*ca, out["ev"], out["rst_seq"], *cb, out=co)))
            rows.append(dict(row=f"tcp_rx_acks {name}", m=m,
                             segments=int(ao["totals"].cpu().numpy().view(np.uint64)[1])))
            jobs.append((rows[-1], lambda ca=ca, cb=cb, ao=ao: clf.tcp_rx_acks(*ca, *cb, out=ao)))
            hv = [out[f][:k].cpu().numpy().reshape(-1).view(dt_)[:k] for f, dt_ in
                  (("verdict", np.uint8), ("sflags", np.uint8), ("rcv_nxt_after", np.uint32), ("ev", np.uint8),
                   ("rst_seq", np.uint32))]
            t0 = time.perf_counter()
            G.tcp_rx_ctl_host(*hv, sock[:k], conn, np.zeros(nconn, dtype=G.TCP_ADDR_DTYPE), k)
            dt = time.perf_counter() - t0
            host_rows.append(dict(row=f"tcp_rx_ctl_host {name}, one core", m=k, us=round(dt * 1e6, 1),
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
    if "tcp_rx_states inorder" in by:
        f1, f2 = by["tcp_rx_ooo inorder, first row"]["us"], by["tcp_rx_ooo inorder, second row"]["us"]
        by["tcp_rx_states inorder"].update(ratio_to_ooo=round(by["tcp_rx_states inorder"]["us"] / ((f1 + f2) / 2), 4),
                                           margin_us=round(abs(f1 - f2), 1),
                                           over_ooo_us=round(by["tcp_rx_states inorder"]["us"] - (f1 + f2) / 2, 1))
        by["tcp_rx_ctl inorder"].update(ratio_to_acks=round(by["tcp_rx_ctl inorder"]["us"] /
                                                            by["tcp_rx_acks inorder"]["us"], 4))
    res = dict(tool="tcprxs_bench", device=torch.cuda.get_device_name(0), m=m, rounds=a.rounds, reps=a.reps,
               rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
