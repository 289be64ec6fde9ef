#!/usr/bin/env python3
"""Time gcl_plan (the GPU stable partition of a classified batch by
destination) on bench.py's own udp64 configuration, against
torch.sort(keys, stable=True) on the same device.

Two workloads, both 32 Mi udp64 packets over 16 runtimes x 8 kthreads:
  1-byte verdicts, GCL_PLAN_BY_RUNTIME (17 buckets)
  2-byte verdicts, GCL_PLAN_BY_QUEUE   (129 buckets)
The baseline sorts the same keys, extracted in advance (untimed) to the
narrowest integer dtype that holds them: this favours the baseline, which
reads 1 B per packet where the plan decodes the verdicts itself.  Each side is
timed with HIP events over >= 10 ms of back-to-back launches after a warm-up.
The roofline fraction is on the algorithmic bytes n x (2 x vbytes + 4) (the
verdicts read twice, one u32 index written) at 8 TB/s.

A tool, not a gate: prints one JSON line and writes profiles/plan_bench.json.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from caladan_amd import gclassify as g  # noqa: E402

MIN_MS = 10.0


def timed_us(fn, min_ms=MIN_MS, warmup=3):
    """Mean microseconds per call of @fn over >= @min_ms of launches."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    reps, total = 4, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        total = a.elapsed_time(b)
        if total >= min_ms:
            return total * 1000.0 / reps, reps
        reps = max(reps * 2, int(reps * 1.2 * min_ms / max(total, 1e-3)) + 1)


def keys_of(verdicts, vbytes, key, R, tb):
    """The plan's keys of a 1- or 2-byte verdict tensor, as the narrowest
    unsigned-capable torch dtype (the baseline's input)."""
    nb = (R << tb if key == g.PLAN_BY_QUEUE else R) + 1
    if vbytes == 1:
        x = verdicts.to(torch.int32)
        q, unicast = x & 0x7F, (x & 0x80) == 0
    else:
        x = verdicts.view(torch.int16).to(torch.int32) & 0xFFFF
        q, unicast = x & 0x3FFF, (x & 0x8000) == 0
    k = q if key == g.PLAN_BY_QUEUE else q >> tb
    k = torch.where(unicast & (k < nb - 1), k, torch.full_like(k, nb - 1))
    return k.to(torch.uint8 if nb <= 256 else torch.int16), nb


def run(device, n, vbytes, key):
    wl, _, stride, R, T, _ = bench.WORKLOADS["udp64"]
    clf = bench.classifier(device, R, T, vbytes)
    bench.setup_tables(clf, R, T)
    frames = torch.zeros(n * stride, dtype=torch.uint8, device=device)
    g.generate(wl, n, stride, R, frames, seed=bench.SEED)
    verdicts = torch.zeros(n * vbytes, dtype=torch.uint8, device=device)
    clf.classify(frames, n, stride, verdicts=verdicts)
    torch.cuda.synchronize()
    del frames
    keys, nb = keys_of(verdicts, vbytes, key, R, clf.thread_bits)
    assert nb == clf.plan_buckets(key)
    order = torch.empty(n, dtype=torch.int32, device=device)
    off = torch.empty(nb + 1, dtype=torch.int32, device=device)

    plan_us, plan_reps = timed_us(lambda: clf.plan(verdicts, n, key=key, order=order, bucket_off=off))
    sort_us, sort_reps = timed_us(lambda: torch.sort(keys, stable=True))
    # the two agree (order is the stable argsort of the keys)
    idx = torch.sort(keys, stable=True)[1]
    same = bool((idx.to(torch.int32) == order).all().item())
    counts = torch.bincount(keys.to(torch.int64), minlength=nb)
    same = same and bool((off[1:].to(torch.int64) == torch.cumsum(counts, 0)).all().item())
    alg_bytes = n * (2 * vbytes + 4)
    row = {
        "workload": f"udp64, {R} runtimes x {T} kthreads, {vbytes}-B verdicts",
        "key": "BY_QUEUE" if key == g.PLAN_BY_QUEUE else "BY_RUNTIME",
        "n": n, "nbuckets": nb, "workspace_bytes": int(clf._plan_ws.numel()),
        "plan_us": round(plan_us, 2), "plan_launches_timed": plan_reps,
        "torch_sort_us": round(sort_us, 2), "torch_sort_launches_timed": sort_reps,
        "torch_sort_key_dtype": str(keys.dtype).replace("torch.", ""),
        "torch_over_plan": round(sort_us / plan_us, 3),
        "plan_gpkt_s": round(n / plan_us / 1e3, 2),
        "algorithmic_bytes": alg_bytes,
        "roofline_frac_8TBs": round(alg_bytes / (plan_us * 1e-6) / (bench.HBM_PEAK_GBS * 1e9), 4),
        "matches_torch_sort": same,
    }
    clf.close()
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=bench.WORKLOADS["udp64"][1], help="packets (default 32 Mi)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plan_bench.py needs a GPU")
    device = torch.device("cuda:0")
    res = {"tool": "tools/plan_bench.py", "box": torch.cuda.get_device_name(0),
           "library": g.version(), "torch": torch.__version__,
           "rows": [run(device, args.n, 1, g.PLAN_BY_RUNTIME), run(device, args.n, 2, g.PLAN_BY_QUEUE)]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
