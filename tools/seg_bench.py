#!/usr/bin/env python3
"""Time gcl_tx_seg on the GPU beside gcl_tx_hdr over the segments it wrote, the
torch way to expand (cumsum + repeat_interleave over the same counts) and
gcl_tx_seg_host on one core.

  python tools/seg_bench.py [--m 1048576] [--rounds 15] [--out profiles/seg_bench.json]

Shapes, each in both layouts (slots of 2048 bytes, packed):
  one    m writes of one 64-byte segment each
  zipf   m writes whose lengths follow a Zipf law (exponent 1.2) over 1..64
         segments of mss 1460, about 10 segments a write
  skew   one 64 MiB write (mss 1460: 45 965 segments) among m - 1 64-byte ones
Every GPU figure is the median over --rounds rounds; a round times every shape
and yardstick once, in turn, so that drift hits all alike; HIP events on the
launch stream, three warm-up rounds.  The first call's outputs are held to the
host twin on a prefix.  bytes_per_seg is what the four launches move by the
layout of their arrays (not a counter).  Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bytes the launches move: per write (count reads the write and stores status, sent, snd_nxt_out, nseg and the
# layout bytes; writes re-reads four of them and stores status, seg_first, B and the compacted pair), per segment
# (desc, frame_off, src_off, len, dst_off, send_idx) and per OK write once more in the expansion (the write, B, the pair)
PER_WRITE = 48 + (1 + 4 + 4 + 4 + 8) + (1 + 4 + 4 + 8) + (1 + 4 + 8 + 4 + 4)
PER_SEG = 32 + 8 + 8 + 2 + 8 + 4
PER_OK_WRITE = 48 + 8 + 8


def shapes(G, m, seed=3):
    rng = np.random.default_rng(seed)

    def base():
        s = np.zeros(m, dtype=G.SEG_SEND_DTYPE)
        s["lip"], s["rip"] = 0x0A000005, 0x0A000100 + rng.integers(0, 16, m)
        s["lport"], s["rport"] = rng.integers(1, 65536, m), rng.integers(1, 65536, m)
        s["proto"], s["mss"], s["win"] = 6, 1460, 0x2000
        s["snd_nxt"], s["ack"] = rng.integers(0, 2 ** 32, m), rng.integers(0, 2 ** 32, m)
        s["len"], s["winlen"] = 10, 1 << 30          # 54 + 10: a 64-byte frame
        s["src_off"] = np.arange(m, dtype=np.uint64) * np.uint64(64)
        return s

    one = base()
    zipf = base()
    k = np.arange(1, 65)
    p = k ** -1.2
    zipf["len"] = rng.choice(k, m, p=p / p.sum()) * 1460
    skew = base()
    skew["len"][m // 2] = 64 << 20
    return {"one": one, "zipf": zipf, "skew": skew}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from caladan_amd import gclassify as G

    m = a.m
    clf = G.Classifier(0, 16, G.HASH_JENKINS)
    mac = bytes([2, 0xCA, 0x1A, 0xDA, 0, 5])
    net = G.txh_net(0x0A000005, 0xFFFF0000, 0x0A000001, mac)
    clf.neigh_set([(0x0A000100 + i, mac[:5] + bytes([9])) for i in range(16)])
    jobs, rows = [], []
    for name, send in shapes(G, m).items():
        nseg = np.maximum(1, -(-np.minimum(send["len"], send["winlen"]).astype(np.int64) // 1460))
        segs = int(nseg.sum())
        dsend = torch.from_numpy(send.view(np.uint8).reshape(m, 48)).cuda()
        for layout, stride in (("slots", 2048), ("packed", 0)):
            out = clf.tx_seg(dsend, m, segs, stride=stride)
            torch.cuda.synchronize()
            k = min(m, 2048)
            h = G.tx_seg_host(send[:k], segs, stride=stride)
            n = int(h["total_segs"][0])
            ok = bool(int(out["total_segs"].cpu()[0]) == segs and
                      np.array_equal(out["frame_off"][:n].cpu().numpy().view(np.uint64), h["frame_off"][:n]) and
                      np.array_equal(out["desc"][:n].cpu().numpy().reshape(-1), h["desc"][:n].view(np.uint8)))
            row = dict(row=f"tx_seg {name} {layout}", m=m, segs=segs, matches_host=ok,
                       bytes_per_seg=round(PER_SEG + (PER_WRITE + PER_OK_WRITE) * m / segs, 1))
            rows.append(row)
            jobs.append((row, lambda dsend=dsend, segs=segs, stride=stride, out=out:
                         clf.tx_seg(dsend, m, segs, stride=stride, out=out)))
            if layout == "packed":
                # the yardsticks over this shape: gcl_tx_hdr reading the descriptors just written ...
                frames = torch.empty(int(out["total_bytes"].cpu()[0]), dtype=torch.uint8, device="cuda")
                hout = clf.tx_hdr(out["desc"], out["frame_off"], segs, frames, net)
                row = dict(row=f"tx_hdr over the segments of {name}", segs=segs)
                rows.append(row)
                jobs.append((row, lambda out=out, segs=segs, frames=frames, hout=hout:
                             clf.tx_hdr(out["desc"], out["frame_off"], segs, frames, net, out=hout)))
                # ... and torch's expansion of the same counts: the start and the write of every segment
                cnt = torch.from_numpy(nseg).cuda()
                ar = torch.arange(m, device="cuda")
                row = dict(row=f"torch cumsum + repeat_interleave, counts of {name}", segs=segs)
                rows.append(row)
                jobs.append((row, lambda cnt=cnt, ar=ar, segs=segs:
                             (torch.cumsum(cnt, 0), torch.repeat_interleave(ar, cnt, output_size=segs))))
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
                   ns_per_seg=round(float(np.median(t)) * 1e3 / row["segs"], 3))
        if "bytes_per_seg" in row:
            row["gb_per_s"] = round(row["bytes_per_seg"] * row["segs"] / (float(np.median(t)) * 1e3), 1)
    # the host twin on one core, m / 8 writes of each shape's kind
    for name, send in shapes(G, max(m // 8, 1)).items():
        if name == "skew":
            continue
        segs = int(np.maximum(1, -(-send["len"].astype(np.int64) // 1460)).sum())
        out = G.tx_seg_host(send, segs)
        t0 = time.perf_counter()
        G.tx_seg_host(send, segs, out=out)
        dt = time.perf_counter() - t0
        rows.append(dict(row=f"tx_seg_host {name} packed, one core", m=len(send), segs=segs,
                         us=round(dt * 1e6, 1), ns_per_seg=round(dt * 1e9 / segs, 3)))
    by = {r["row"]: r for r in rows}
    ratio = {lay: round(by[f"tx_seg skew {lay}"]["ns_per_seg"] / by[f"tx_seg one {lay}"]["ns_per_seg"], 3)
             for lay in ("slots", "packed")}
    res = dict(tool="seg_bench", device=torch.cuda.get_device_name(0), m=m, rounds=a.rounds, rows=rows,
               skew_over_one_ns_per_seg=ratio)
    clf.close()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
