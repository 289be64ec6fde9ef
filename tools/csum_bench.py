#!/usr/bin/env python3
"""Time the IPv4 header checksum offload of a batch (gcl_rx_csum) against the
memory traffic its frame layout cannot do without.

Device (needs a GPU): gcl_rx_csum over bench.py's udp64 batch (32 Mi packets
in dense 64-B slots), with an ol_flags input (IP_CKSUM_UNKNOWN: every packet
checked) and without one (a context whose default_olflags are UNKNOWN), and
over its tcp1500 batch (8 Mi packets in 1536-B slots), each with and without
the counters.  The yardstick is gcl_access_probe with GCL_PROBE_MIN | 1 over
the same batch in the same process: one 16-B load per header line and one
byte written per packet.  Both are timed with HIP events over >= 10 ms of
back-to-back launches after a warm-up, in alternating rounds; the median
round is reported.  The generator's headers carry valid checksums, so every
checked packet comes out IP_CKSUM_GOOD; the kernel's work does not depend on
the verdict.  The roofline fraction is on the algorithmic bytes, 22 B of
header plus the flag bytes per packet, at 8 TB/s; the bytes that move are
whole 128-B lines (64 B per packet in dense slots, 128 B in wide ones), given
beside it.

Host (CPU only, --host-only runs it alone on any machine): ns per packet of
gcl_rx_csum_flags over --host-n hot frames (default 4 Mi calls over 4096
64-B frames that stay in L1/L2) on one core, called from a C loop.

A tool, not a gate: prints one JSON line and writes profiles/csum_bench.json.
"""
import argparse
import ctypes
import json
import os
import platform
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HOST_ONLY = "--host-only" in sys.argv
if not HOST_ONLY:  # torch brings its HIP runtime: load it before the library, as bench.py does
    import torch  # noqa: E402

    import bench  # noqa: E402
from caladan_amd import gclassify as g  # noqa: E402

MIN_MS = 10.0
ROUNDS = 5
UNKNOWN_FLAGS = g.F_RSS_HASH | g.F_IP_CKSUM_UNKNOWN


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


def run_device(torch, bench, device, name):
    wl, n, stride, R, T, _ = bench.WORKLOADS[name]
    clf = g.Classifier(device.index or 0, R, g.HASH_JENKINS, 0, UNKNOWN_FLAGS)
    frames = torch.zeros(n * stride, dtype=torch.uint8, device=device)
    cdf, nflows = None, 0
    if wl == g.WL_TCP1500_ZIPF:
        nflows = 1 << 20
        cdf = torch.from_numpy(g.zipf_cdf(nflows, 0.99).view(np.int64)).to(device)
    g.generate(wl, n, stride, R, frames, seed=bench.SEED, zipf_cdf_dev=cdf, nflows=nflows)
    olflags = torch.full((n,), UNKNOWN_FLAGS, dtype=torch.uint8, device=device)
    out = torch.empty(n, dtype=torch.uint8, device=device)
    probe_out = torch.empty(n, dtype=torch.uint8, device=device)
    counts = torch.zeros(g.CSUM_NR, dtype=torch.int64, device=device)
    torch.cuda.synchronize()

    arms = {
        "probe_min": lambda: clf.access_probe(frames, n, stride, out=probe_out, vbytes=1, minimal=True),
        "probe_min_olflags": lambda: clf.access_probe(frames, n, stride, out=probe_out, vbytes=1,
                                                      olflags=olflags, minimal=True),
        "csum": lambda: clf.rx_csum(frames, n, stride, olflags_out=out),
        "csum_counts": lambda: clf.rx_csum(frames, n, stride, olflags_out=out, counts=counts),
        "csum_olflags": lambda: clf.rx_csum(frames, n, stride, olflags_out=out, olflags=olflags),
        "csum_olflags_counts": lambda: clf.rx_csum(frames, n, stride, olflags_out=out, olflags=olflags,
                                                   counts=counts),
    }
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            us[k].append(timed_us(torch, fn))
    counts.zero_()
    arms["csum_olflags_counts"]()
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64).tolist()
    flags_seen = torch.unique(out).cpu().tolist()
    med = {k: statistics.median(v) for k, v in us.items()}
    line_bytes = n * (64 if stride == 64 else 128)

    def row(arm, probe, flag_bytes):
        alg = n * (22 + flag_bytes)
        t = med[arm] * 1e-6
        return {
            "us_median": round(med[arm], 2), "us_rounds": [round(x, 2) for x in us[arm]],
            "probe": probe, "over_probe": round(med[arm] / med[probe], 4),
            "gpkt_s": round(n / med[arm] / 1e3, 2),
            "algorithmic_bytes": alg,
            "roofline_frac_8TBs_algorithmic": round(alg / t / (bench.HBM_PEAK_GBS * 1e9), 4),
            "line_bytes": line_bytes + n * flag_bytes,
            "roofline_frac_8TBs_lines": round((line_bytes + n * flag_bytes) / t / (bench.HBM_PEAK_GBS * 1e9), 4),
        }

    res = {
        "workload": f"{name}: {n} packets in {stride}-B slots",
        "probe_min_us_median": round(med["probe_min"], 2),
        "probe_min_us_rounds": [round(x, 2) for x in us["probe_min"]],
        "probe_min_olflags_us_median": round(med["probe_min_olflags"], 2),
        "probe_min_olflags_us_rounds": [round(x, 2) for x in us["probe_min_olflags"]],
        "csum_no_olflags": row("csum", "probe_min", 1),
        "csum_no_olflags_counts": row("csum_counts", "probe_min", 1),
        "csum_olflags": row("csum_olflags", "probe_min_olflags", 2),
        "csum_olflags_counts": row("csum_olflags_counts", "probe_min_olflags", 2),
        "counts_checked_good_bad_skipped": c, "flags_out_values": flags_seen,
        "counts_consistent": c[0] == c[1] + c[2] and c[0] + c[3] == n,
    }
    clf.close()
    return res


# ---------------------------------------------------------------- host
def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


HOST_LOOP_C = r"""
#include <stddef.h>
#include <stdint.h>
uint8_t gcl_rx_csum_flags(const uint8_t *frame, size_t len, uint8_t olflags);
uint64_t csum_loop(const uint8_t *frames, uint64_t nframes, uint64_t calls, uint8_t fl)
{
	uint64_t acc = 0;
	for (uint64_t i = 0; i < calls; i++)
		acc += gcl_rx_csum_flags(frames + 64 * (i % nframes), 64, fl);
	return acc;
}
"""


def run_host(calls):
    """ns per gcl_rx_csum_flags call from a C loop (a ctypes call per packet
    would time the interpreter): a small shim is compiled against the library."""
    nframes = 4096
    rng = np.random.default_rng(0xCA1ADA4)
    frames = rng.integers(0, 256, size=(nframes, 64), dtype=np.uint8)
    frames[:, 12], frames[:, 13] = 0x08, 0x00
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "loop.c"), os.path.join(d, "loop.so")
        with open(src, "w") as f:
            f.write(HOST_LOOP_C)
        libdir = os.path.dirname(g.LIB_PATH)
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, src, "-L" + libdir,
                               "-l:" + os.path.basename(g.LIB_PATH), "-Wl,-rpath," + libdir])
        loop = ctypes.CDLL(so)
        loop.csum_loop.restype = ctypes.c_uint64
        loop.csum_loop.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint8]
        ns = []
        for rnd in range(ROUNDS + 1):  # round 0 warms up
            t0 = time.perf_counter_ns()
            acc = loop.csum_loop(frames.ctypes.data, nframes, calls, UNKNOWN_FLAGS)
            dt = time.perf_counter_ns() - t0
            if rnd:
                ns.append(dt / calls)
    assert acc > 0
    return {"workload": f"{calls} calls over {nframes} hot 64-B IPv4 frames, flags UNKNOWN, one core",
            "cpu": cpu_name(), "ns_per_pkt_median": round(statistics.median(ns), 3),
            "ns_per_pkt_min": round(min(ns), 3), "rounds": ROUNDS}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--host-n", type=int, default=4 << 20, help="host: calls (default 4 Mi)")
    ap.add_argument("--host-only", action="store_true", help="skip the device part (no GPU needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csum_bench.json"))
    args = ap.parse_args()
    res = {"tool": "tools/csum_bench.py", "library": g.version()}
    if not HOST_ONLY:
        if not torch.cuda.is_available():
            sys.exit("csum_bench.py: the device part needs a GPU (--host-only for the host part)")
        device = torch.device("cuda:0")
        res.update(box=torch.cuda.get_device_name(0), torch=torch.__version__,
                   device=[run_device(torch, bench, device, "udp64"),
                           run_device(torch, bench, device, "tcp1500")])
        for r in res["device"]:
            for k in ("csum_no_olflags", "csum_olflags"):
                r[k]["gpu_ns_per_pkt"] = round(r[k]["us_median"] * 1e3 / int(r["workload"].split()[1]), 5)
    res["host"] = run_host(args.host_n)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
