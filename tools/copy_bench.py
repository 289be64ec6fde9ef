#!/usr/bin/env python3
"""Time the loopback frame copy of a batch (gcl_copy_batch) against the
device's own copy speed.

Needs a GPU.  Three shapes, each with source and destination both 16-B
aligned and with the source moved by 1 and by 4 bytes against the destination:

  udp64    16 Mi 64-B frames out of dense 64-B tx slots into dense 64-B slots
           (dst_stride 64), 1 GiB of payload
  tcp1500  1 Mi 1500-B frames out of 1536-B tx slots into 1536-B slots
           (dst_stride 1536)
  ingress  128 Ki frames into the reference's ingress geometry (dst_off: mbuf
           data at element + 344 of 9408-B elements, the pool's elements in a
           random order), lengths of the mixed workload (70 % 64..1514 B
           uniform, 20 % 64 B, 10 % 9000 B), out of 9216-B tx slots

The yardstick is torch's device-to-device copy_ of one contiguous uint8 buffer
holding the same number of payload bytes, in the same process.  Both are
timed with HIP events over >= 10 ms of back-to-back launches after a warm-up,
in alternating rounds; the median round is reported, with the bytes moved
(payload read + payload written) over the time.  The A/B rows time the lanes
per packet (group 4, 16, 64 against the library's choice) and the grid's cap
(gcl_tune.blocks_per_cu 4, 6, 8) on the aligned form of every shape.  Loads
and stores are plain in every row: a non-temporal form has not been built, so
that question is open.

A tool, not a gate: prints one JSON line and writes profiles/copy_bench.json.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (torch brings its HIP runtime: load it before the library)

from caladan_amd import gclassify as g  # noqa: E402

MIN_MS = 10.0
ROUNDS = 5
SEED = 0xCA1ADA4


def timed_us(fn, min_ms=MIN_MS, warmup=3):
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


def dev(a, device):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).to(device)


def shape(name, scale):
    """(n, lengths u16[n], src_off u64[n], src bytes, dst_off or None,
    dst_stride, dst bytes, len_hint)"""
    rng = np.random.default_rng(SEED)
    if name == "udp64":
        n = (16 << 20) // scale
        return n, np.full(n, 64, np.uint16), np.arange(n, dtype=np.uint64) * 64, n * 64, None, 64, n * 64, 64
    if name == "tcp1500":
        n = (1 << 20) // scale
        return (n, np.full(n, 1500, np.uint16), np.arange(n, dtype=np.uint64) * 1536, n * 1536, None,
                1536, n * 1536, 1500)
    n = g.IOKERNEL_NUM_MBUFS // scale
    u = rng.random(n)
    lens = np.where(u < 0.7, rng.integers(64, 1515, size=n), np.where(u < 0.9, 64, 9000)).astype(np.uint16)
    dst_off = g.mbuf_data_offsets(n)[rng.permutation(n)]
    return (n, lens, np.arange(n, dtype=np.uint64) * 9216, n * 9216, dst_off, 0, g.mbuf_region_bytes(n),
            0)


def run_shape(name, device, scale):
    n, lens, src_off, src_bytes, dst_off, stride, dst_bytes, hint = shape(name, scale)
    payload = int(lens.astype(np.uint64).sum())
    clf = g.Classifier(device.index or 0, 16, g.HASH_NIC, 0, 0x01)
    src = torch.empty(src_bytes + 16, dtype=torch.uint8, device=device).random_(0, 256)
    dst = torch.zeros(dst_bytes, dtype=torch.uint8, device=device)
    d_len = dev(lens, device)
    d_dst_off = dev(dst_off, device) if dst_off is not None else None
    pl = torch.empty(n, dtype=torch.int16, device=device)
    ol = torch.empty(n, dtype=torch.uint8, device=device)
    rs = torch.empty(n, dtype=torch.int32, device=device)
    counts = torch.zeros(g.COPY_NR, dtype=torch.int64, device=device)
    flat_a = torch.empty(payload, dtype=torch.uint8, device=device).random_(0, 256)
    flat_b = torch.empty(payload, dtype=torch.uint8, device=device)
    offs = {k: dev(src_off + np.uint64(k), device) for k in (0, 1, 4)}
    torch.cuda.synchronize()

    def copy(shift=0, group=0, with_counts=False):
        return lambda: clf.copy_batch(src, offs[shift], d_len, n, dst, dst_off=d_dst_off, dst_stride=stride,
                                      len_hint=hint, group=group, pkt_len=pl, olflags=ol, rss=rs,
                                      counts=counts if with_counts else None)

    arms = {"torch_copy": lambda: flat_b.copy_(flat_a)}
    for k in (0, 1, 4):
        arms[f"copy_shift{k}"] = copy(k)
    arms["copy_shift0_counts"] = copy(0, with_counts=True)
    for grp in (4, 16, 64):
        arms[f"copy_shift0_group{grp}"] = copy(0, grp)
    us = {k: [] for k in arms}
    for _ in range(ROUNDS):
        for k, fn in arms.items():
            us[k].append(timed_us(fn))
    # the grid's cap: the same launch under gcl_tune.blocks_per_cu
    for per_cu in (4, 6, 8):
        clf.tune(blocks_per_cu=per_cu)
        us[f"copy_shift0_blocks_per_cu{per_cu}"] = [timed_us(copy(0)) for _ in range(ROUNDS)]
    clf.tune()
    counts.zero_()
    copy(0, with_counts=True)()
    torch.cuda.synchronize()
    c = counts.cpu().numpy().view(np.uint64).tolist()
    med = {k: statistics.median(v) for k, v in us.items()}
    rows = {}
    for k in us:
        rows[k] = {"us_median": round(med[k], 2), "us_rounds": [round(x, 2) for x in us[k]],
                   "over_torch_copy": round(med[k] / med["torch_copy"], 4),
                   "payload_tb_s_read_plus_write": round(2 * payload / med[k] / 1e6, 3)}
    res = {"shape": name, "packets": n, "payload_bytes": payload, "len_hint": hint,
           "dst": f"dst_stride {stride}" if dst_off is None else "dst_off: element + 344 of 9408-B elements",
           "rows": rows, "counts_copied_refused_bytes": c[:3],
           "counts_consistent": c[0] == n and c[1] == 0 and c[2] == payload}
    clf.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", type=int, default=1, help="divide every shape's packet count (rehearsals)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "copy_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("copy_bench.py needs a GPU")
    device = torch.device("cuda:0")
    res = {"tool": "tools/copy_bench.py", "library": g.version(), "box": torch.cuda.get_device_name(0),
           "torch": torch.__version__, "min_ms_per_timing": MIN_MS, "rounds": ROUNDS,
           "non_temporal": "not measured: loads and stores are plain in every row",
           "shapes": [run_shape(s, device, args.scale) for s in ("udp64", "tcp1500", "ingress")]}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
