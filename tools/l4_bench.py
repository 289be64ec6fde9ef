#!/usr/bin/env python3
"""Time the TCP/UDP checksum offload of a batch (gcl_l4_csum), VERIFY and FILL,
against two device yardsticks that move the same bytes and the host twin.

Three frame shapes, each a batch of more than 256 MiB so that it is read from
HBM: 64-B UDP frames in dense 64-B slots (4 Mi packets), 1514-B TCP frames (tot
1500) in 1536-B slots (256 Ki packets) and 9000-B TCP frames in 9216-B slots
(32 Ki packets).  The frames are random payload under well-formed headers,
filled once, so that VERIFY says GOOD for every packet; the kernel's work does
not depend on the verdict.

Arms, per shape, in one process: gcl_l4_csum VERIFY and FILL (with counts);
gcl_copy_batch of the same frames into a second pool (reads the same bytes and
also writes them); torch.sum over the same buffer viewed as int32 (a streaming
read reduction); and VERIFY with gcl_tune.blocks_per_cu 4, 6 and 8 beside the
default grid cap.  Each is timed with HIP events over >= 10 ms of back-to-back
launches after a warm-up, in alternating rounds; the median round is reported.
GB/s is frame bytes (n x frame length) per second; the copy moves twice that.

Every shape is a GPU step of its own: the parent starts it as a fresh process
under `timeout` and stops at the first step that fails, so that nothing more
is started on a GPU that has faulted or hung.

Host (CPU only, --host-only runs it alone on any machine): gcl_l4_csum_host
VERIFY over 4096 hot MTU frames on one core.

A tool, not a gate: prints one JSON line and writes profiles/l4_bench.json.
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
# name: (packets, slot stride, frame length, protocol)
SHAPES = {"udp64": (4 << 20, 64, 64, 17), "tcp1500": (256 << 10, 1536, 1514, 6),
          "tcp9000": (32 << 10, 9216, 9000, 6)}


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


def headers(frames2d, flen, proto):
    """Well-formed Ethernet + IPv4 + L4 headers over the rows of @frames2d."""
    tot = flen - 14
    for col, v in ((12, 0x08), (13, 0x00), (14, 0x45), (16, tot >> 8), (17, tot & 0xFF), (20, 0x40),
                   (21, 0x00), (23, proto)):
        frames2d[:, col] = v


def run_step(name):
    """One shape on the GPU: the child process of a step."""
    import torch

    from caladan_amd import gclassify as g
    n, stride, flen, proto = SHAPES[name]
    device = torch.device("cuda:0")
    clf = g.Classifier(0, 16, g.HASH_NIC, 0, 0x01)
    gen = torch.Generator(device=device)
    gen.manual_seed(0xCA1ADA4)
    frames = torch.randint(0, 256, (n, stride), dtype=torch.uint8, device=device, generator=gen)
    headers(frames, flen, proto)
    frames = frames.reshape(-1)
    plen = torch.full((n,), flen, dtype=torch.int16, device=device)
    status = torch.empty(n, dtype=torch.uint8, device=device)
    counts = torch.zeros(g.L4C_NR, dtype=torch.int64, device=device)
    pool = torch.empty_like(frames)
    src_off = torch.arange(n, dtype=torch.int64, device=device) * stride
    cp_len = torch.empty(n, dtype=torch.int16, device=device)
    clf.l4_csum(frames, n, plen, mode=g.L4_FILL, stride=stride, status=status, len_hint=flen)
    torch.cuda.synchronize()

    def verify():
        clf.l4_csum(frames, n, plen, mode=g.L4_VERIFY, stride=stride, status=status, counts=counts,
                    len_hint=flen)

    def capped(per_cu):
        def fn():
            clf.tune(blocks_per_cu=per_cu)
            verify()
            clf.tune()
        return fn

    arms = {
        "verify": verify,
        "fill": lambda: clf.l4_csum(frames, n, plen, mode=g.L4_FILL, stride=stride, status=status,
                                    counts=counts, len_hint=flen),
        "copy_batch": lambda: clf.copy_batch(frames, src_off, plen, n, pool, dst_stride=stride,
                                             len_hint=flen, pkt_len=cp_len, olflags=False, rss=False),
        "torch_sum_int32": lambda: torch.sum(frames.view(torch.int32)),
        "verify_cap4": capped(4), "verify_cap6": capped(6), "verify_cap8": capped(8),
    }
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            us[k].append(timed_us(torch, fn))
    counts.zero_()
    verify()
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64).tolist()
    med = {k: statistics.median(v) for k, v in us.items()}
    nbytes = n * flen
    res = {"shape": f"{name}: {n} x {flen}-B frames in {stride}-B slots", "frame_bytes": nbytes,
           "buffer_bytes": n * stride,
           "us_median": {k: round(v, 2) for k, v in med.items()},
           "us_rounds": {k: [round(x, 2) for x in v] for k, v in us.items()},
           "gb_s": {k: round(nbytes / med[k] / 1e3, 1) for k in ("verify", "fill", "copy_batch")},
           "torch_sum_gb_s_buffer": round(n * stride / med["torch_sum_int32"] / 1e3, 1),
           "verify_time_over_copy": round(med["verify"] / med["copy_batch"], 4),
           "fill_time_over_copy": round(med["fill"] / med["copy_batch"], 4),
           "verify_time_over_torch_sum": round(med["verify"] / med["torch_sum_int32"], 4),
           "fill_time_over_torch_sum": round(med["fill"] / med["torch_sum_int32"], 4),
           "verify_counts": c, "all_good": c[g.L4C_GOOD] == n,
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
    """gcl_l4_csum_host VERIFY over a batch that stays in cache, one call per
    round (the loop over the packets is the library's)."""
    from caladan_amd import gclassify as g
    n, stride, flen, proto = 4096, 1536, 1514, 6  # 6 MiB: hot in L2/L3
    rng = np.random.default_rng(0xCA1ADA4)
    frames = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    headers(frames, flen, proto)
    frames = frames.reshape(-1)
    plen = np.full(n, flen, dtype=np.uint16)
    g.l4_csum_host(frames, plen, mode=g.L4_FILL, stride=stride)
    ns = []
    for rnd in range(ROUNDS + 1):  # round 0 warms up
        t0 = time.perf_counter_ns()
        for _ in range(16):
            st = g.l4_csum_host(frames, plen, mode=g.L4_VERIFY, stride=stride)
        dt = time.perf_counter_ns() - t0
        if rnd:
            ns.append(dt / (16 * n))
    assert (st == g.L4_GOOD).all()
    med = statistics.median(ns)
    return {"workload": f"VERIFY of {n} hot {flen}-B TCP frames, one core", "cpu": cpu_name(),
            "ns_per_pkt_median": round(med, 1), "gb_s": round(flen / med, 2), "rounds": ROUNDS}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--host-only", action="store_true", help="skip the device part (no GPU needed)")
    ap.add_argument("--step", choices=sorted(SHAPES), help="(internal) run one GPU step in this process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l4_bench.json"))
    args = ap.parse_args()
    if args.step:
        run_step(args.step)
        return
    from caladan_amd import gclassify as g
    res = {"tool": "tools/l4_bench.py", "library": g.version()}
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
    if "failed_step" in res:
        sys.exit(1)


if __name__ == "__main__":
    main()
