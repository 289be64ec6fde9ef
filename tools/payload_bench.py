#!/usr/bin/env python3
"""Time the payload descriptors and packed receive layout of a batch
(gcl_l4_payload) beside two device yardsticks and the host twin.

Two batches: bench.py's udp64 batch (32 Mi generated 64-B UDP frames in dense
64-B slots, 16 runtimes) and 1 Mi 1514-B TCP frames (tot 1500, 1460 payload
bytes behind a 20-byte header) in 1536-B slots.

Arms, per batch, in one process: gcl_l4_payload with the identity order, and
with the order and bucket_off of a gcl_plan over the batch's classify verdicts
(a gather through order[]); gcl_rx_csum over the same frames (one launch that
reads one header per packet, the cost of touching every frame once); and
torch.cumsum over an int64[m] (a device-wide scan of as many elements, 16 B of
traffic per element against the 35 B per entry gcl_l4_payload writes and the
2 B it re-reads).  Each is timed with HIP events over >= 10 ms of
back-to-back launches after a warm-up, in alternating rounds; the median
round is reported.

Every batch is a GPU step of its own: the parent starts it as a fresh process
under `timeout` and stops at the first step that fails, so that nothing more
is started on a GPU that has faulted or hung.

Host (CPU only, --host-only runs it alone on any machine): gcl_l4_payload_host
over 64 Ki hot 64-B UDP frames on one core.

A tool, not a gate: prints one JSON line, writes profiles/payload_bench.json
and, with --table, prints the markdown table DESIGN.md carries.
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
STEP_TIMEOUT_S = 240
R, T = 16, 8
# name: (packets, slot stride, frame length)
SHAPES = {"udp64": (32 << 20, 64, 64), "tcp1500": (1 << 20, 1536, 1514)}


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


def tcp_headers(frames2d, flen, ips):
    """Well-formed Ethernet + IPv4 + TCP headers (data offset 5) over the rows
    of @frames2d, row i addressed to runtime i % len(ips)."""
    tot = flen - 14
    for col, v in ((12, 0x08), (13, 0x00), (14, 0x45), (16, tot >> 8), (17, tot & 0xFF), (20, 0x40),
                   (21, 0x00), (23, 6), (46, 0x50)):
        frames2d[:, col] = v
    n = frames2d.shape[0]
    for k, ip in enumerate(ips):
        for c, byte in enumerate(ip.to_bytes(4, "big")):
            frames2d[k:n:len(ips), 30 + c] = byte


def run_step(name):
    """One batch on the GPU: the child process of a step."""
    import torch

    from caladan_amd import gclassify as g
    n, stride, flen = SHAPES[name]
    device = torch.device("cuda:0")
    clf = g.Classifier(0, R, g.HASH_JENKINS)
    for r in range(R):
        clf.runtime_set(r, g.runtime_ip(r), T, T, g.steer_flows(T, list(range(T))))
    plen = torch.empty(n, dtype=torch.int16, device=device)
    if name == "udp64":
        frames = torch.zeros(n * stride, dtype=torch.uint8, device=device)
        g.generate(g.WL_UDP64, n, stride, R, frames, pkt_len=plen)
    else:
        gen = torch.Generator(device=device)
        gen.manual_seed(0xCA1ADA4)
        frames = torch.randint(0, 256, (n, stride), dtype=torch.uint8, device=device, generator=gen)
        tcp_headers(frames, flen, [g.runtime_ip(r) for r in range(R)])
        frames = frames.reshape(-1)
        plen.fill_(flen)
    verdicts = torch.zeros(n * 8, dtype=torch.uint8, device=device)
    clf.classify(frames, n, stride, verdicts=verdicts)
    order, boff = clf.plan(verdicts, n)
    nseg = clf.plan_buckets()
    out = {"src_off": torch.empty(n, dtype=torch.int64, device=device),
           "len": torch.empty(n, dtype=torch.int16, device=device),
           "dst_off": torch.empty(n, dtype=torch.int64, device=device),
           "kind": torch.empty(n, dtype=torch.uint8, device=device),
           "meta": torch.empty((n, 16), dtype=torch.uint8, device=device),
           "total": torch.empty(1, dtype=torch.int64, device=device)}
    out_plan = dict(out, seg_bytes=torch.empty(nseg + 1, dtype=torch.int64, device=device))
    counts = torch.zeros(g.PAYC_NR, dtype=torch.int64, device=device)
    olf = torch.empty(n, dtype=torch.uint8, device=device)
    ones = torch.ones(n, dtype=torch.int64, device=device)
    scan = torch.empty(n, dtype=torch.int64, device=device)
    torch.cuda.synchronize()

    arms = {
        "payload_identity": lambda: clf.l4_payload(frames, n, plen, stride=stride, out=out, counts=counts),
        "payload_plan_order": lambda: clf.l4_payload(frames, n, plen, stride=stride, order=order, m=n,
                                                     seg_off=boff, nseg=nseg, out=out_plan, counts=counts),
        "rx_csum": lambda: clf.rx_csum(frames, n, stride, olflags_out=olf),
        "torch_cumsum_int64": lambda: torch.cumsum(ones, 0, out=scan),
    }
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            us[k].append(timed_us(torch, fn))
    counts.zero_()
    arms["payload_identity"]()
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64).tolist()
    total = int(out["total"].cpu().numpy().view(np.uint64)[0])
    med = {k: statistics.median(v) for k, v in us.items()}
    res = {"shape": f"{name}: {n} x {flen}-B frames in {stride}-B slots", "entries": n,
           "us_median": {k: round(v, 2) for k, v in med.items()},
           "us_rounds": {k: [round(x, 2) for x in v] for k, v in us.items()},
           "ns_per_entry": {k: round(med[k] * 1e3 / n, 4) for k in med},
           "identity_time_over_rx_csum": round(med["payload_identity"] / med["rx_csum"], 4),
           "identity_time_over_cumsum": round(med["payload_identity"] / med["torch_cumsum_int64"], 4),
           "plan_order_time_over_identity": round(med["payload_plan_order"] / med["payload_identity"], 4),
           "counts": c, "total_bytes": total, "kept": c[g.PAYC_UDP] + c[g.PAYC_TCP],
           "box": torch.cuda.get_device_name(0), "torch": torch.__version__}
    clf.close()
    print(json.dumps(res))


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def run_host():
    """gcl_l4_payload_host over a batch that stays in cache, one call per
    round (the loop over the entries is the library's)."""
    from caladan_amd import gclassify as g
    n, stride = 64 << 10, 64  # 4 MiB of frames: hot in L2/L3
    rng = np.random.default_rng(0xCA1ADA4)
    frames = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    for col, v in ((12, 0x08), (13, 0x00), (14, 0x45), (16, 0), (17, 50), (20, 0x40), (21, 0), (23, 17)):
        frames[:, col] = v
    frames = frames.reshape(-1)
    plen = np.full(n, 64, dtype=np.uint16)
    out = None
    ns = []
    for rnd in range(ROUNDS + 1):  # round 0 warms up
        t0 = time.perf_counter_ns()
        for _ in range(16):
            out = g.l4_payload_host(frames, plen, stride=stride, out=out)
        dt = time.perf_counter_ns() - t0
        if rnd:
            ns.append(dt / (16 * n))
    assert (out["kind"] == g.PAY_UDP).all() and int(out["total"][0]) == n * 22
    med = statistics.median(ns)
    return {"workload": f"{n} hot 64-B UDP frames, identity order, one core", "cpu": cpu_name(),
            "ns_per_entry_median": round(med, 2), "rounds": ROUNDS}


def table(res):
    """The markdown table of DESIGN.md from a result dict."""
    rows = ["| batch | arm | us per call | ns per entry |", "|---|---|---|---|"]
    for d in res.get("device", []):
        for k, v in d["us_median"].items():
            rows.append(f"| {d['shape'].split(':')[0]} | {k} | {v} | {d['ns_per_entry'][k]} |")
    if not res.get("device"):
        rows.append("| (no GPU number was taken) | | | |")
    h = res["host"]
    rows.append(f"| host | gcl_l4_payload_host, {h['workload']} | | {h['ns_per_entry_median']} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--host-only", action="store_true", help="skip the device part (no GPU needed)")
    ap.add_argument("--step", choices=sorted(SHAPES), help="(internal) run one GPU step in this process")
    ap.add_argument("--table", action="store_true", help="also print the markdown table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_bench.json"))
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    from caladan_amd import gclassify as g
    res = {"tool": "tools/payload_bench.py", "library": g.version()}
    if not args.host_only:
        res["device"] = []
        for name in SHAPES:
            r = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable,
                                os.path.abspath(__file__), "--step", name], capture_output=True, text=True)
            if r.returncode != 0:  # start nothing more on the GPU
                res["failed_step"] = {"step": name, "rc": r.returncode, "stderr": r.stderr[-2000:]}
                break
            res["device"].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res["host"] = run_host()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    if args.table:
        print(table(res))
    if "failed_step" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
