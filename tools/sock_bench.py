#!/usr/bin/env python3
"""Time the socket demux of a classified batch (gcl_sock_lookup) against the
nearest measured kernel, gcl_rx_csum, over the same batch.

Device (needs a GPU): bench.py's udp64 batch (32 Mi packets in dense 64-B
slots) classified by a 1-byte-verdict context, then gcl_sock_lookup with 1 Ki,
64 Ki and 1 Mi entries in the table.  The entries are cut from the generated
frames' own tuples (half connections, half listeners, dealt to the runtime
the frame's destination address names).  The generator draws source
address and both ports uniformly, so a packet outside the sampled frames hits
only a listener on its (address, port): the share that hits grows with the
table and is reported with each row (the six counters).  gcl_rx_csum over
the same frames reads almost the same bytes (frame bytes [12, 34) against
[12, 38), one byte written per packet against four plus one verdict byte
read) and no table.  Both are timed with HIP events over >= 10 ms of
back-to-back launches after a warm-up, in alternating rounds; the median round
is reported, with the ratio to gcl_rx_csum at each table size.  Every step
runs in a child process of its own under its own time limit.

Host (CPU only, --host-only runs it alone on any machine): ns per packet of
gcl_sock_tbl_lookup_host on one core, over 1 Mi random UDP packets for 16
runtimes and a 64 Ki-entry table cut from the first of them.

A tool, not a gate: prints one JSON line and writes profiles/sock_bench.json.
"""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MIN_MS = 10.0
ROUNDS = 5
TABLE_SIZES = (1 << 10, 1 << 16, 1 << 20)
STEP_LIMIT_S = 420
R, TB = 16, 3  # bench.py's config: 16 runtimes x 8 kthreads, 1-byte verdicts


def entries_from_frames(g, hdr, want):
    """{uniqid: SOCK_ENTRY_DTYPE array}, @want entries in all, cut from the
    64-B frames @hdr (u8[m, 64]): even rows a connection, odd rows a listener;
    the runtime is the one whose address (gcl_runtime_ip) the frame is for."""
    h = hdr.astype(np.int64)
    be = lambda a, n: sum(h[:, a + j] << (8 * (n - 1 - j)) for j in range(n))  # noqa: E731
    lip, rip, lport, rport, proto = be(30, 4), be(26, 4), be(36, 2), be(34, 2), h[:, 23]
    u = lip - g.runtime_ip(0)
    ok = (u >= 0) & (u < R) & (lport != 0) & ((proto == 6) | (proto == 17))
    e = np.zeros(len(h), dtype=g.SOCK_ENTRY_DTYPE)
    five = np.arange(len(h)) % 2 == 0
    e["lip"], e["lport"], e["proto"] = lip, lport, proto
    e["rip"], e["rport"] = np.where(five, rip, 0), np.where(five, rport, 0)
    e["match"] = np.where(five, g.SOCK_MATCH_5TUPLE, g.SOCK_MATCH_3TUPLE)
    e, u = e[ok], u[ok]
    _, first = np.unique(e[["lip", "rip", "lport", "rport", "proto", "match"]], return_index=True)
    first = np.sort(first)[:want]
    e, u = e[first], u[first]
    e["cookie"] = np.arange(len(e))
    return {int(x): e[u == x] for x in np.unique(u)}


def timed_us(torch, fn, min_ms=MIN_MS, warmup=3):
    """Mean microseconds per call of @fn over >= @min_ms of launches."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    reps = 4
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        total = a.elapsed_time(b)
        if total >= min_ms:
            return total * 1000.0 / reps
        reps = max(reps * 2, int(reps * 1.2 * min_ms / max(total, 1e-3)) + 1)


def step_device(nentries):
    """One table size, in this process: classify, set, then alternate rounds
    of gcl_sock_lookup and gcl_rx_csum."""
    import torch

    import bench
    from caladan_amd import gclassify as g
    wl, n, stride, nrt, T, _ = bench.WORKLOADS["udp64"]
    assert nrt == R
    device = torch.device("cuda:0")
    clf = g.Classifier(0, R, g.HASH_JENKINS, g.CFG_VERDICT1, g.F_RSS_HASH | g.F_IP_CKSUM_UNKNOWN,
                       thread_bits=TB)
    for u in range(R):
        clf.runtime_set(u, g.runtime_ip(u), T, T, list(range(T)))
    frames = torch.zeros(n * stride, dtype=torch.uint8, device=device)
    g.generate(wl, n, stride, R, frames, seed=bench.SEED)
    verdicts = torch.zeros(n, dtype=torch.uint8, device=device)
    clf.classify(frames, n, stride, verdicts=verdicts)
    torch.cuda.synchronize()
    m = min(n, 4 * nentries + 4096)
    hdr = frames[:m * stride].cpu().numpy().reshape(m, stride)[:, :64]
    sets = entries_from_frames(g, hdr, nentries)
    t0 = time.perf_counter()
    for u, e in sets.items():
        clf.sock_set(u, e)
    set_ms = (time.perf_counter() - t0) * 1e3
    sock = torch.empty(n, dtype=torch.int32, device=device)
    flags = torch.empty(n, dtype=torch.uint8, device=device)
    counts = torch.zeros(g.SOCK_NR, dtype=torch.int64, device=device)
    arms = {
        "csum": lambda: clf.rx_csum(frames, n, stride, olflags_out=flags),
        "sock": lambda: clf.sock_lookup(frames, n, stride, verdicts=verdicts, sock=sock),
        "sock_counts": lambda: clf.sock_lookup(frames, n, stride, verdicts=verdicts, sock=sock, counts=counts),
    }
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            us[k].append(timed_us(torch, fn))
    counts.zero_()
    arms["sock_counts"]()
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64).tolist()
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"entries": int(sum(len(e) for e in sets.values())), "packets": n, "stride": stride,
           "table_bytes": 16 + 40 * max(8, 1 << int(np.ceil(np.log2(max(sum(len(e) for e in sets.values()), 1))))),
           "sock_set_ms_total": round(set_ms, 2),
           "counts_hit5_hit3_any_multi_miss_na": c[:6], "counts_sum_is_n": sum(c[:6]) == n}
    for k in arms:
        res[k + "_us_median"] = round(med[k], 2)
        res[k + "_us_rounds"] = [round(x, 2) for x in us[k]]
        res[k + "_gpkt_s"] = round(n / med[k] / 1e3, 2)
    res["sock_over_csum"] = round(med["sock"] / med["csum"], 3)
    res["sock_counts_over_csum"] = round(med["sock_counts"] / med["csum"], 3)
    res["box"], res["torch"] = torch.cuda.get_device_name(0), torch.__version__
    clf.close()
    return res


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def step_host(npkts=1 << 20, nentries=1 << 16):
    """ns per packet of gcl_sock_tbl_lookup_host on one core."""
    from caladan_amd import gclassify as g
    rng = np.random.default_rng(0xCA1ADA4)
    frames = rng.integers(0, 256, size=(npkts, 64), dtype=np.uint8)
    frames[:, 12], frames[:, 13], frames[:, 14] = 0x08, 0x00, 0x45
    frames[:, 21] &= 0xDF
    frames[:, 23] = 17
    u = rng.integers(0, R, size=npkts)
    ip = g.runtime_ip(0) + u
    for j in range(4):
        frames[:, 30 + j] = (ip >> (24 - 8 * j)) & 0xFF
    frames[frames[:, 36] == 0, 36] = 1
    sets = entries_from_frames(g, frames[:4 * nentries], nentries)
    tbl = g.SockTable()
    for x, e in sets.items():
        tbl.set(x, e)
    verdicts = (u << TB).astype(np.uint8)
    region = frames.reshape(-1)
    ns = []
    for rnd in range(ROUNDS + 1):  # round 0 warms up
        t0 = time.perf_counter_ns()
        _, cnt = tbl.lookup(region, npkts, verdicts, 1, TB, R, stride=64)
        dt = time.perf_counter_ns() - t0
        if rnd:
            ns.append(dt / npkts)
    return {"workload": f"{npkts} udp packets in 64-B slots, {sum(len(e) for e in sets.values())} entries, "
                        "1-byte verdicts, one core", "cpu": cpu_name(),
            "counts_hit5_hit3_any_multi_miss_na": cnt[:6].tolist(),
            "ns_per_pkt_median": round(statistics.median(ns), 2), "ns_per_pkt_min": round(min(ns), 2),
            "rounds": ROUNDS}


def child(args):
    """Run one step in a fresh process under its own time limit; its JSON."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", *args], capture_output=True,
                       text=True, timeout=STEP_LIMIT_S)
    if r.returncode != 0:
        sys.exit(f"sock_bench.py: step {args} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--host-only", action="store_true", help="skip the device part (no GPU needed)")
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sock_bench.json"))
    args = ap.parse_args()
    if args.step:
        res = step_host() if args.step[0] == "host" else step_device(int(args.step[1]))
        print(json.dumps(res))
        return
    from caladan_amd import gclassify as g
    res = {"tool": "tools/sock_bench.py", "library": g.version()}
    if not args.host_only:
        res["device"] = [child(["device", str(sz)]) for sz in TABLE_SIZES]
    res["host"] = child(["host"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
