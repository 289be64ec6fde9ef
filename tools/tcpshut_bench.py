#!/usr/bin/env python3
"""Time gcl_tcp_shut over 1 Mi connections beside gcl_tcp_tick over the same
connections, in one process, and gcl_tcp_shut_host on one core.

  python tools/tcpshut_bench.py [--nconn 1048576] [--rounds 9] [--out profiles/tcpshut_bench.json]

gcl_tcp_shut: nobody acting; 1 % closing (a FIN each); everybody closing from
ESTABLISHED (a FIN each); everybody aborting (an RST each).  gcl_tcp_tick: the
timer due for none, 1 % and all (a delayed ACK that ran out: one segment each),
and the all-due row once more at the end, which gives the run-to-run spread.

A figure is the median over --rounds rounds; a round times every row once, in
turn, so that drift hits all alike.  A row's timed window is as many calls
between two HIP events on the launch stream as make it at least 10 ms long
(calibrated once, after three warm-up calls); the figure is the window divided
by the calls.  Bytes per call come from the struct sizes: what the launches
read and write per connection and per segment (BYTES below), each 16-B word
counted once although a 64-B line may be fetched for it.  The first call's
outputs are held to the host twin.  No figure is a gate.  Prints one JSON
object.
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

NOW = 10_000_000_000
# per connection: decide reads the request, the timer record and the first PCB word and writes
# out_conn and its workspace byte, emit reads the byte; per segment: the other PCB words and the
# address in, desc, txq_ent, txq_cold, frame_off, seg_conn, seg_kind, seg_src and first_seg out
BYTES = dict(shut=(16 + 64 + 16 + 48 + 1 + 1, 32 + 16 + 32 + 16 + 16 + 8 + 4 + 1 + 4 + 4),
             # decide reads the timer record and writes out_tmr, emit reads its action word; per
             # segment: the PCB words and the address in, desc, frame_off, seg_conn, seg_kind, seg_src out
             tick=(64 + 32 + 16, 32 + 16 + 32 + 8 + 4 + 1 + 4))


def shapes(G, n, seed=7):
    rng = np.random.default_rng(seed)
    tmr = np.zeros(n, dtype=G.TCP_TMR_DTYPE)
    tmr["next_timeout"], tmr["ack_ts"] = NOW + 5000, NOW - 10003
    tmr["state"], tmr["flags"] = G.TCP_STATE_ESTABLISHED, G.TMR_LIVE | G.TMR_ACK_DELAYED
    conn = np.zeros(n, dtype=G.TCP_CONN_DTYPE)
    for f in ("snd_una", "snd_nxt", "rcv_nxt", "rcv_wnd"):
        conn[f] = rng.integers(0, 1 << 32, n)
    addr = np.zeros(n, dtype=G.TCP_ADDR_DTYPE)
    addr["lip"], addr["rip"] = 0x0A000005, 0x0A000014 + rng.integers(0, 3, n)
    addr["lport"], addr["rport"], addr["rcv_wscale"] = rng.integers(1, 1 << 16, n), 80, 7
    return tmr, conn, addr, rng.random(n) < 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nconn", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window-ms", type=float, default=10.0)
    ap.add_argument("--only", default=None, help="time the rows whose name holds this (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    n = a.nconn
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    tmr, conn, addr, one_pct = shapes(G, n)

    def rec(x):
        return torch.from_numpy(x.view(np.uint8).reshape(len(x), -1)).cuda()
    d = dict(conn=rec(conn), addr=rec(addr), tmr=rec(tmr))
    rows, jobs, host_rows = [], [], []

    def add(row, fn):
        rows.append(row)
        if a.only is None or a.only in row["row"]:
            jobs.append((row, fn))

    for name, op, who in (("none acting", G.SHUT_OP_NONE, None), ("1 % closing", G.SHUT_OP_CLOSE, one_pct),
                          ("all sending a FIN", G.SHUT_OP_CLOSE, np.ones(n, dtype=bool)),
                          ("all aborting", G.SHUT_OP_ABORT, np.ones(n, dtype=bool))):
        shut = np.zeros(n, dtype=G.TCP_SHUT_DTYPE)
        if who is not None:
            shut["op"][who] = op
        k = int(who.sum()) if who is not None else 0
        ds = rec(shut)
        out = clf.tcp_shut(NOW, ds, d["tmr"], d["conn"], d["addr"], n, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = G.tcp_shut_host(NOW, shut, tmr, conn, addr, n)
        dt = time.perf_counter() - t0
        ok = out["totals"].cpu().numpy().tolist() == [k, k] == h["totals"].tolist() and \
            np.array_equal(out["out_conn"].cpu().numpy().reshape(-1), h["out_conn"].view(np.uint8)) and \
            np.array_equal(out["desc"].cpu().numpy()[:k].reshape(-1), h["desc"][:k].view(np.uint8)) and \
            np.array_equal(out["txq_ent"].cpu().numpy()[:k].reshape(-1), h["txq_ent"][:k].view(np.uint8))
        add(dict(row=f"tcp_shut {name}", call="shut", items=n, segs=k, matches_host=bool(ok)),
            lambda ds=ds, out=out: clf.tcp_shut(NOW, ds, d["tmr"], d["conn"], d["addr"], n, n, out=out))
        host_rows.append(dict(row=f"tcp_shut_host {name}, one core", items=n, segs=k, us=round(dt * 1e6, 1),
                              ns_per_item=round(dt * 1e9 / n, 3)))

    for name, who in (("none due", None), ("1 % due", one_pct), ("all due", np.ones(n, dtype=bool)),
                      ("all due, again", np.ones(n, dtype=bool))):
        t = tmr.copy()
        if who is not None:
            t["next_timeout"][who] = NOW - 3
        k = int(who.sum()) if who is not None else 0
        dt_ = rec(t)
        out = clf.tcp_tick(NOW, dt_, d["conn"], d["addr"], n, n)
        torch.cuda.synchronize()
        assert out["totals"].cpu().numpy().tolist() == [k, k]
        add(dict(row=f"tcp_tick {name}", call="tick", items=n, segs=k),
            lambda dt_=dt_, out=out: clf.tcp_tick(NOW, dt_, d["conn"], d["addr"], n, n, out=out))

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    reps = {}
    for row, fn in jobs:
        window(fn, 3)
        reps[id(row)] = max(1, int(np.ceil(a.window_ms / max(window(fn, 4) / 4, 1e-3))))
    ts = {id(r): [] for r, _ in jobs}
    for _ in range(a.rounds):
        for row, fn in jobs:
            ts[id(row)].append(window(fn, reps[id(row)]) * 1e3 / reps[id(row)])
    for row, _ in jobs:
        t = ts[id(row)]
        per_conn, per_seg = BYTES[row["call"]]
        nbytes = per_conn * row["items"] + per_seg * row["segs"]
        row.update(calls_per_window=reps[id(row)], us=round(float(np.median(t)), 1), min_us=round(float(np.min(t)), 1),
                   max_us=round(float(np.max(t)), 1), bytes=nbytes,
                   gb_per_s=round(nbytes / (float(np.median(t)) * 1e-6) / 1e9, 1))
    res = dict(tool="tcpshut_bench", date=datetime.date.today().isoformat(), device=torch.cuda.get_device_name(0),
               nconn=n, rounds=a.rounds, window_ms=a.window_ms, rows=rows + host_rows)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
