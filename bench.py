"""Benchmark: device-resident rx classify + Jenkins flow hash (BASELINE.json).

One step = one pass of the classify kernel over this GPU's batch of frames
already resident in HBM (the rx_one_pkt loop of iokernel/rx.c:281-287 for a
whole batch), plus -- with more than one GPU -- an RCCL all_gather of every
rank's per-runtime packet counts and rx counters over xGMI.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scaling weak|strong]
                    [--full] [--dump-outputs DIR]
    torchrun --nproc-per-node N bench.py --gpus N ...

Rank 0 prints one JSON line.  Workload (configs[1] of BASELINE.json): 32 Mi
synthetic 64-B Eth/IPv4/UDP frames per GPU, uniform 5-tuples, 16 runtimes x 8
kthreads, JENKINS flow hash; packets are sharded round-robin across ranks in
64 Ki-packet blocks.  --scaling weak (default) keeps 32 Mi packets per GPU;
--scaling strong splits SURVEY §8(e)'s 256 Mi-packet batch (config 4) over
the ranks.

A plain run sets up, warms up, times the K steps and prints the line.  With
--full, at N=1 the layout's ceiling, the gcl_group rows, the secondary config
(1500-B TCP, Zipf-0.99 flows, 1024 runtimes), the integrated ingress-pool
shape, the host-memory and rx_burst pipeline rows and the CPU baseline (the
oracle's restatement of rx.c on this host's cores) are added.
--dump-outputs DIR writes what the last timed step computed (dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from caladan_amd import gclassify as g  # noqa: E402
from caladan_amd import shard  # noqa: E402

METRIC = "Mpkt/s device-resident rx classify+Jenkins-hash, 64B & 1500B frames"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s peak (spec)
L2_PEAK_GBS = 34500.0  # MI355X_MICROARCH.md "L2 (per XCD)": ~34.5 TB/s over the 8 XCDs
SEED = 0xCA1ADA4
SHARD_BLOCK = 64 * 1024

WORKLOADS = {
    # name: (generator, pkts per GPU, slot stride, runtimes, threads, description)
    "udp64": (g.WL_UDP64, 32 << 20, 64, 16, 8,
              "32Mi Eth/IPv4/UDP 64B frames per GPU in HBM, uniform 5-tuples, 16 runtimes x 8 kthreads"),
    "tcp1500": (g.WL_TCP1500_ZIPF, 8 << 20, 1536, 1024, 4,
                "8Mi Eth/IPv4/TCP 1500B frames (1536B slots), Zipf-0.99 over 1Mi flows, 1024 runtimes x 4 kthreads"),
    # the same 1500-B TCP stream with DPDK buffer split (RTE_ETH_RX_OFFLOAD_BUFFER_SPLIT):
    # the NIC writes each frame's first 64 B into a dense header slab
    "tcp1500_hsplit": (g.WL_TCP1500_ZIPF, 8 << 20, 64, 1024, 4,
                       "8Mi Eth/IPv4/TCP 1500B frames, header-split: 64B header slab, Zipf-0.99, 1024 runtimes x 4 kthreads"),
    "mixed": (g.WL_MIXED, 1 << 20, 9216, 16, 8,
              "1Mi mixed frames (70% IPv4 TCP/UDP 64..9014B, 20% IPv6, 10% ARP), 9216B slots, 16 runtimes"),
}
# algorithmic bytes per packet: one 64-B header granule read + one verdict
# written, 8 B (gcl_verdict), 4 B (gcl_verdict4), 2 B or 1 B (the kthread-queue
# verdicts of GCL_CFG_VERDICT2 / VERDICT1) (DESIGN.md "Roofline"); tables and
# counters amortise to ~0.
HDR_BYTES = 64
# Through round 3 the bench default was the 2-byte queue verdict (GCL_CFG_VERDICT2): the flat
# kthread-queue index q = uniqid << thread_bits | thread that the lrpc
# post-pass (gcl_host_deliver2) indexes its rings with, a wake's flow_tbl
# slot, or a tagged drop/broadcast action -- everything rx_send_pkt_to_runtime
# needs.  It halves the write requests of the 4-byte form: 331 vs 342 us for
# udp64 and 174 vs 180 us for tcp1500 on the same buffers
# (profiles/archive/r02_defer_ab.jsonl).  The 4- and 8-byte forms stay as rows.
# Since round 4 the headline runs the 1-byte form (GCL_CFG_VERDICT1: the
# same queue index in one byte, which 16 runtimes x 8 kthreads fit, WAKE left
# to the post-pass's live active count): 330.7 vs 333.7-336.4 us, 101.3 vs
# 99.6-100.4 Gpkt/s in alternating fresh processes (profiles/r04_verdict1_ab.jsonl).
VERDICT_BYTES = 1
# the secondary (config 3, 1500-B TCP) line's verdict: 1024 x 4 queues need 2 B
SECONDARY_VERDICT_BYTES = 2
# the integrated ingress rows (e2e.ingress_pool) keep the 2-byte form their
# PMC passes were taken with (profiles/pmc_ingress_nic_v2.json)
INGRESS_VERDICT_BYTES = 2
VERDICT_NAMES = {8: "gcl_verdict, 8 B", 4: "gcl_verdict4, 4 B",
                 2: "queue verdict (GCL_CFG_VERDICT2), 2 B",
                 1: "queue verdict (GCL_CFG_VERDICT1), 1 B"}


def verdict_cfg(vbytes, R, T):
    """(cfg flags, thread_bits) of a context writing @vbytes-byte verdicts
    for R runtimes of up to T kthreads."""
    if vbytes == 1:
        tb = g.thread_bits_for(R, T)
        if tb is None or (R << tb) > g.V1_QUEUES:
            raise ValueError(f"1-byte verdicts need R << thread_bits <= 128 ({R} x {T})")
        return g.CFG_VERDICT1, tb
    if vbytes == 2:
        return g.CFG_VERDICT2, g.thread_bits_for(R, T)
    return (g.CFG_VERDICT4 if vbytes == 4 else 0), 0


def fit_vbytes(vbytes, R, T):
    """@vbytes, or the 2-byte queue verdict where the 1-byte one cannot name
    every queue (1024 runtimes x 4 kthreads)."""
    if vbytes == 1:
        tb = g.thread_bits_for(R, T)
        if tb is None or (R << tb) > g.V1_QUEUES:
            return 2
    return vbytes


def classifier(device, R, T, vbytes, extra_flags=0, hash_mode=g.HASH_JENKINS):
    fl, tb = verdict_cfg(vbytes, R, T)
    return g.Classifier(device.index or 0, R, hash_mode, fl | extra_flags, thread_bits=tb)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# One JSON line on stdout and nothing else: libraries that print banners to
# stdout (RCCL's version block) are moved to stderr at the fd level.
_JSON_FD = None


def _claim_stdout():
    global _JSON_FD
    sys.stdout.flush()
    _JSON_FD = os.dup(1)
    os.dup2(2, 1)


def emit_json(obj):
    line = (json.dumps(obj) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(line.decode())
        sys.stdout.flush()
    else:
        os.write(_JSON_FD, line)


# The driver keeps only the tail of stdout (~8.5 KB): round 4's 23-KB line
# was cut and never parsed.  The stdout line is the summary below, held
# under LINE_LIMIT bytes; the full result goes to DETAIL_PATH and stderr.
LINE_LIMIT = 8192
DETAIL_PATH = os.environ.get("GCL_BENCH_DETAIL", os.path.join("gpurun_out", "bench_detail.json"))
CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                 "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def _pick(d, *keys):
    """The keys of dict @d that exist (nested dicts are never walked)."""
    if not isinstance(d, dict):
        return None
    return {k: d[k] for k in keys if k in d}


def _roof(r, *extra):
    return _pick(r, "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_source",
                 "kernel_ms", "bytes_per_pkt", "ceiling_ms", "frac_of_ceiling", "read_sol", *extra)


def _cpu_mode(m):
    return _pick(m, "1core_mpps", "1core_lrpc_mpps", "all_cores_mpps", "all_cores", "spread_1core",
                 "spread_all_cores")


def _pipe_row(rows, burst, workers, verdicts, hash_prefix):
    for r in rows or ():
        if (r.get("burst") == burst and r.get("workers") == workers and
                r.get("verdicts") == verdicts and str(r.get("hash", "")).startswith(hash_prefix)):
            return _pick(r, "mpps_one_core", "burst_latency_p50_us", "burst_latency_p99_us",
                         "submit_ns_per_pkt", "deliver_ns_per_pkt", "delivered_check", "mpps_samples")
    return None


def compact(result, detail_path=DETAIL_PATH):
    """The stdout line: the contract keys plus one summary row per measured
    section (the VERDICT r04 list), every other field in the detail file."""
    out = {k: result[k] for k in CONTRACT_KEYS if k in result}
    if "roofline" in result:
        out["roofline"] = _roof(result["roofline"])
    for k in ("kernel_only",):
        if k in result:
            out[k] = _pick(result[k], "value", "unit", "ms_per_step", "gpu_ms_per_step")
    for k in ("counts_check", "exchange", "e2e_multi", "launch"):
        if k in result:
            out[k] = result[k]
    if "placement" in result:
        p = result["placement"]
        out["placement"] = _pick(p, "policy", "probe_us_chosen", "classes_seen", "replaced")
        if "policy" in out["placement"] and "probe_us_chosen" in out["placement"]:
            del out["placement"]["policy"]  # placed: the probe figures say so
    cpu = result.get("cpu_baseline")
    if cpu:
        out["cpu_baseline"] = {**_pick(cpu, "value", "unit", "cores", "kind", "sample", "pinning",
                                       "cpu_model", "nproc", "seconds", "gpu_over_1core_nic", "error"),
                               "nic_mode": _cpu_mode(cpu.get("nic_mode")),
                               "jenkins_mode": _cpu_mode(cpu.get("jenkins_mode"))}
    grp = result.get("group")
    if grp:
        out["group"] = _pick(grp, "n_gpus", "exchange", "value", "gpu_ms_per_step", "counts_check", "error")
    node = result.get("group_node")
    if node:
        out["group_node"] = _pick(node, "n_gpus", "exchange", "rccl_ranks", "value", "ms_per_step",
                                  "counts_check", "error")
    sec = result.get("secondary")
    if sec:
        s = {"workload": "tcp1500 (config 3)", **_pick(sec, "verdict", "value", "unit", "ms_per_step"),
             "roofline": _roof(sec.get("roofline", {}))}
        c3 = sec.get("cpu_baseline", {})
        if c3:
            s["cpu_1core_mpps"] = {"nic": c3.get("nic_mode", {}).get("1core_mpps"),
                                   "jenkins": c3.get("jenkins_mode", {}).get("1core_mpps")}
        out["secondary"] = s
        hs = sec.get("header_split_layout")
        if hs:
            out["header_split"] = {"value": hs.get("value"), "frac": hs.get("roofline", {}).get("frac"),
                                   "kernel_ms": hs.get("roofline", {}).get("kernel_ms")}
        tp = sec.get("udp64_toeplitz")
        if tp:
            out["toeplitz"] = {"value": tp.get("value"), "frac": tp.get("roofline", {}).get("frac")}
        ov = sec.get("udp64_other_verdicts")
        if ov:
            out["udp64_other_verdicts"] = {o.get("verdict", "?").split(",")[-1].strip(): o.get("value")
                                           for o in ov}
    e2e = result.get("e2e")
    if e2e:
        e = {}
        for name in ("udp64", "mixed"):
            if name in e2e:
                e[name] = _pick(e2e[name], "zerocopy_mpps", "copy_hdr_2streams_mpps", "copy_full_frames_mpps")
        tr = e2e.get("mixed", {}).get("trace_replay")
        if tr:
            e["mixed_trace_replay_mpps"] = tr.get("zerocopy_mpps")
        ing = e2e.get("ingress_pool", {}).get("integrated_nic")
        if ing:
            e["ingress_integrated_nic"] = {
                "device_resident_mpps": ing.get("device_resident_mpps"),
                "frac": ing.get("roofline", {}).get("frac"),
                "frac_of_ceiling": ing.get("roofline", {}).get("frac_of_ceiling"),
                "zerocopy_mpps": ing.get("zerocopy_mpps"), "counts_check": ing.get("counts_check")}
        ws = e2e.get("ingress_pool", {}).get("integrated_nic_working_set")
        if ws:
            e["ingress_working_set_nic"] = {
                "device_resident_mpps": ws.get("device_resident_mpps"),
                "frac_l2": ws.get("roofline", {}).get("frac"),
                "frac_of_ceiling": ws.get("roofline", {}).get("frac_of_ceiling"),
                "counts_check": ws.get("counts_check")}
        rows = e2e.get("rx_burst_pipeline", {}).get("runs")
        rec = "read in place, stamped header records in the slot"
        e["pipeline"] = {"records_1x1_nic": _pipe_row(rows, 64, 1, rec, "nic"),
                         "records_4x8_nic": _pipe_row(rows, 64, 4, rec, "nic"),
                         "records_1x1_jenkins": _pipe_row(rows, 64, 1, rec, "jenkins"),
                         "records_4x8_jenkins": _pipe_row(rows, 64, 4, rec, "jenkins")}
        ing = e2e.get("rx_burst_pipeline_ingress")
        if ing:
            def _ing(rows, **want):
                for row in rows or ():
                    if all(row.get(k) == v for k, v in want.items()):
                        return _pick(row, "mpps_one_core", "burst_latency_p50_us", "burst_latency_p99_us",
                                     "submit_ns_per_pkt", "ns_per_pkt", "nic_wait_frac", "delivered_check",
                                     "mpps_samples", "error")
                return None
            rec = "read in place, stamped header records in the slot"
            e["pipeline_cold_headers"] = {
                "records_1x1_nic": _ing(ing.get("gpu"), workers=1, verdicts=rec),
                "records_4x8_nic": _ing(ing.get("gpu"), workers=4, verdicts=rec),
                "records_8x16_nic": _ing(ing.get("gpu"), workers=8, verdicts=rec),
                "offsets_4x8_nic": _ing(ing.get("gpu"), workers=4, verdicts="read in place"),
                "cpu_1core_classify_nic": _ing(ing.get("cpu"), post="classify only", prefetch="rx.c's stride 2"),
                "cpu_1core_lrpc_nic": _ing(ing.get("cpu"), post="classify + rx_make_cmd + lrpc_send",
                                           prefetch="rx.c's stride 2"),
                "cpu_1core_lrpc_nic_burst_prefetch": _ing(ing.get("cpu"), post="classify + rx_make_cmd + lrpc_send",
                                                          prefetch="the burst's 64 headers, then rx.c's stride 2"),
            }
        lp = e2e.get("rxloop", {})
        for k in ("loop_burst64_w1_d1_hdr_records", "loop_burst64_w4_d8_hdr_records"):
            if k in lp:
                e.setdefault("rxloop", {})[k] = _pick(lp[k], "p50_us", "p99_us", "mpps")
        out["e2e"] = e
    out["detail"] = detail_path
    # never past the limit: drop the least central summaries first
    for k in ("udp64_other_verdicts", "placement", "toeplitz", "header_split", "group_node",
              "e2e_multi", "exchange", "group", "e2e", "secondary"):
        if len(json.dumps(out)) < LINE_LIMIT:
            break
        out.pop(k, None)
    return out


def emit_result(result):
    """Full result to DETAIL_PATH and stderr, the compact line to stdout."""
    full = json.dumps(result)
    try:
        os.makedirs(os.path.dirname(DETAIL_PATH) or ".", exist_ok=True)
        with open(DETAIL_PATH, "w") as f:
            f.write(full + "\n")
    except OSError as e:
        log(f"bench.py: could not write {DETAIL_PATH}: {e}")
    log("bench detail:", full)
    emit_json(compact(result))


def setup_tables(clf, R, T, seed=SEED):
    """Runtime r owns 10.0.0.(r+1); active kthreads seeded in [1, T];
    flow tables from the sched_steer_flows rule (gcl_steer_flows)."""
    rng = np.random.default_rng(seed)
    tables = []
    for r in range(R):
        act = int(rng.integers(1, T + 1))
        idx = [int(x) for x in rng.choice(T, size=act, replace=False)]
        fl = g.steer_flows(T, idx)
        clf.runtime_set(r, g.runtime_ip(r), T, act, fl)
        tables.append((r, g.runtime_ip(r), T, act, fl))
    return tables


def zero_fill(buf):
    """Zero a DeviceBuffer with hipMemset (slots are only partly generated)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    assert hip.hipMemset(buf.data_ptr(), 0, buf.numel()) == 0
    hip.hipDeviceSynchronize()


def hip_copy(dst, src, nbytes):
    """hipMemcpy (kind default: direction from the pointers) between tensors
    and DeviceBuffers, synchronous."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    for b in (dst, src):
        assert nbytes <= b.numel() * b.element_size()
    assert hip.hipMemcpy(dst.data_ptr(), src.data_ptr(), nbytes, 4) == 0  # hipMemcpyDefault
    hip.hipDeviceSynchronize()


# start-up placement check (Workload.check_placement): the kernel over the
# chosen pair must run within this factor of the probe's time (per verdict
# width), else the pool is placed again, at most PLACEMENT_TRIES times.  Fast
# pairs measured kernel/probe 0.97-1.02 with 2-byte verdicts and 1.01-1.06
# with 4-byte ones, slow pairs 1.12 and 1.19 (profiles/archive/r02_pair_check.jsonl,
# r02_bench_spread_settle.jsonl, gpurun_out/r02c, r02g)
PLACEMENT_SLACK = {1: 1.07, 2: 1.07, 4: 1.10, 8: 1.10}
PLACEMENT_TRIES = 3
# the slack above was calibrated on 16-runtime udp64 pairs only; with 1024
# runtimes the kernel's time is not predicted by the probe's read+write
# shape (the header-split pool ran 94-96 us against an 81-83 us probe on
# every placement, BENCH_r02.json, r04), so those pools are checked with
# gcl_access_probe instead: the kernel's memory requests without the
# classification, whose time depends on the placement and not on the
# runtime count.  ACCESS_SLACK[vbytes] bounds it against the pair probe's
# chosen time the way PLACEMENT_SLACK bounds the kernel.
PLACEMENT_CHECK_RUNTIMES = (16,)
ACCESS_SLACK = {1: 1.10, 2: 1.10, 4: 1.10, 8: 1.10}
# strided slots: the kernel within this of gcl_access_probe on the same pair
# (tcp1500 measured 1.03: profiles/r04_bench.json, secondary.roofline)
LAYOUT_SLACK = 1.10
PROBE_READ_CAP = 4 << 30  # gcl_dev_alloc_paired's probe reads at most this much


class Workload:
    def __init__(self, name, rank, world, device, hash_mode=g.HASH_JENKINS, vbytes=None,
                 n=None):
        wl, n_default, stride, R, T, desc = WORKLOADS[name]
        n = n_default if n is None else n
        if vbytes is None:  # the bench default where it fits, else the 2-byte form
            vbytes = fit_vbytes(VERDICT_BYTES, R, T)
        self.name, self.wl, self.n, self.stride, self.R, self.T, self.desc = name, wl, n, stride, R, T, desc
        self.vbytes = vbytes
        self.bytes_per_pkt = HDR_BYTES + vbytes
        self.device = device
        self.placement_checks = []
        if os.environ.get("GCL_BENCH_TORCH_ALLOC") == "1":
            self.frames = torch.zeros(n * stride, dtype=torch.uint8, device=device)
            self.verdicts = torch.empty(n * vbytes, dtype=torch.uint8, device=device)
        else:  # library-owned hipMalloc (gcl_dev_alloc), zeroed
            # the verdict ring first, then the frame pool placed against it
            # (gcl_dev_alloc_paired: DESIGN.md §4 "Buffer placement") where
            # the kernel stores a verdict per packet (4-/8-B verdicts: placed
            # 344 against 389 us plain, profiles/r06_placement_ab.jsonl); a
            # dense slab with 1-/2-B verdicts defers them until after its
            # reads, which takes the placement class away, and a plain pool
            # runs faster (udp64 316-320 placed against 307-308 plain, tcp1500
            # 176-179 against 171-172).  GCL_BENCH_PLACEMENT=0 / 1 forces it
            self.verdicts = g.DeviceBuffer(n * vbytes, device.index or 0)
            env = os.environ.get("GCL_BENCH_PLACEMENT")
            self.paired = env != "0" if env is not None else vbytes > 2
            self.frames = self._new_pool()
        self.counts = torch.zeros(R + g.NR_STATS, dtype=torch.int64, device=device)

        self.cdf_dev = None
        self.nflows = 0
        if wl == g.WL_TCP1500_ZIPF:
            self.nflows = 1 << 20
            self.cdf_dev = torch.from_numpy(g.zipf_cdf(self.nflows, 0.99).view(np.int64)).to(device)
        self.rank, self.world = rank, world
        self._fill(self.frames)
        fl, tb = verdict_cfg(vbytes, R, T)
        self.clf = g.Classifier(device.index or 0, R, hash_mode, fl, thread_bits=tb)
        self.tables = setup_tables(self.clf, R, T)
        torch.cuda.synchronize()
        if getattr(self, "paired", False):
            if stride == HDR_BYTES:
                self.check_placement(access=R not in PLACEMENT_CHECK_RUNTIMES)
            else:
                self.check_layout()

    def _new_pool(self):
        buf = g.DeviceBuffer(self.n * self.stride, self.device.index or 0,
                             partner=self.verdicts if self.paired else None, vbytes=self.vbytes)
        torch.cuda.synchronize()
        zero_fill(buf)
        return buf

    def _fill(self, buf):
        g.generate(self.wl, self.n, self.stride, self.R, buf, seed=SEED, rank=self.rank,
                   world=self.world, shard_block=SHARD_BLOCK, zipf_cdf_dev=self.cdf_dev,
                   nflows=self.nflows)

    def kernel_us(self, reps=5):
        """Mean classify launch time over this pair, into scratch counters."""
        scratch = torch.zeros_like(self.counts)
        st = torch.cuda.current_stream()

        def go():
            self.clf.classify(self.frames, self.n, self.stride, verdicts=self.verdicts,
                              counts=scratch[:self.R], stats=scratch[self.R:], stream=st.cuda_stream)
        go()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            go()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    def access_us(self, reps=5):
        """Mean gcl_access_probe time over this pair (the kernel's loads and
        stores without the classification)."""
        st = torch.cuda.current_stream()

        def go():
            self.clf.access_probe(self.frames, self.n, self.stride, out=self.verdicts,
                                  stream=st.cuda_stream)
        go()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            go()
        e1.record(st)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    def check_placement(self, tries=PLACEMENT_TRIES, access=False):
        """Keep the frame pool only if the classify kernel itself runs in the
        fast class over it: its launch time within PLACEMENT_SLACK[vbytes] of the
        probe's chosen time (scaled to the probe's 4 GiB read cap).  A pool
        that fails is placed again against the same ring (the old one held
        while the search runs, so the next lands elsewhere), regenerated,
        and checked again -- a start-up placement, like the iokernel's
        (iokernel/rx.c:398-415)."""
        for k in range(tries + 1):
            info = self.frames.pair_info
            # the probe read min(pool, 4 GiB) and wrote probe_write_bytes of
            # the ring: scale its time to the kernel's whole read + write
            rd, wr = self.n * self.stride, self.n * self.vbytes
            probed = min(rd, PROBE_READ_CAP) + max(1, min(wr, info["probe_write_bytes"] or wr))
            scale = (rd + wr) / probed
            us = self.access_us() if access else self.kernel_us()
            limit = info["probe_us_chosen"] * scale * (ACCESS_SLACK if access else PLACEMENT_SLACK)[self.vbytes]
            ok = us <= limit
            # the other time too (calibration data for ACCESS_SLACK)
            other = self.kernel_us() if access else self.access_us()
            self.placement_checks.append({("access_probe_us" if access else "kernel_us"): round(us, 2),
                                          ("kernel_us" if access else "access_probe_us"): round(other, 2),
                                          "checked_with": "gcl_access_probe" if access else "classify kernel",
                                          "probe_us_chosen":
                                          info["probe_us_chosen"], "limit_us": round(limit, 2),
                                          "classes_seen": info["classes_seen"], "passed": ok,
                                          **({"kept": True} if ok else
                                             {"kept_failed": True} if k == tries else {})})
            if ok or k == tries:
                return
            old = self.frames
            self.frames = self._new_pool()
            old.free()
            self._fill(self.frames)
            torch.cuda.synchronize()

    def check_layout(self):
        """Strided slots (tcp1500's 1536 B): the pair probe that placed the
        pool reads it densely, so its time does not predict a strided
        launch's.  The check here is the kernel against gcl_access_probe --
        the same strided header loads and verdict stores without the
        classification -- on the same buffers: within LAYOUT_SLACK of it, the
        launch runs at what its access pattern allows over this pair."""
        ku, au = self.kernel_us(), self.access_us()
        ok = ku <= au * LAYOUT_SLACK
        self.placement_checks.append({"kernel_us": round(ku, 2), "access_probe_us": round(au, 2),
                                      "checked_with": "classify kernel against gcl_access_probe "
                                                      "(strided slots)",
                                      "limit_us": round(au * LAYOUT_SLACK, 2), "passed": ok,
                                      **({"kept": True} if ok else {"kept_failed": True})})

    def step(self, stream):
        self.clf.classify(self.frames, self.n, self.stride, verdicts=self.verdicts,
                          counts=self.counts[:self.R], stats=self.counts[self.R:], stream=stream)


# steps per multi-GPU counts exchange: 8 udp64 steps = 3.5 ms, far fresher than
# the iokernel's once-a-second stats dump, and the exchange's cross-stream
# event packets (~13 us each on the compute queue) amortise to <0.5%
EXCHANGE_EVERY = 8


class Exchange:
    """Multi-GPU step: classify into a [counts | stats] vector, then one RCCL
    all_gather of it on a side stream that overlaps the following steps'
    kernels; node-wide totals accumulate on that stream.  The vector covers
    `period` steps (the iokernel reads its counters periodically, not per
    burst).  A ring of NBUF vectors lets a gather finish up to NBUF-1 periods
    late before its vector is reused, and the side stream zeroes a vector
    after gathering it, so the compute stream only ever waits on an event."""

    NBUF = 4

    def __init__(self, w, world, device, period=1):
        L = w.R + g.NR_STATS
        self.world = world
        self.period = max(1, period)
        self.cnt = [torch.zeros(L, dtype=torch.int64, device=device) for _ in range(self.NBUF)]
        self.gat = [torch.zeros(world * L, dtype=torch.int64, device=device)
                    for _ in range(self.NBUF)]
        self.acc = torch.zeros(L, dtype=torch.int64, device=device)
        self.done = [None] * self.NBUF
        self.comm = torch.cuda.Stream(device=device)
        self.k = 0      # periods exchanged
        self.inner = 0  # steps accumulated into the current vector

    def step(self, w):
        b = self.k % self.NBUF
        cur = torch.cuda.current_stream()
        if self.inner == 0 and self.done[b] is not None and not self.done[b].query():
            cur.wait_event(self.done[b])  # a barrier packet only when really needed
        w.clf.classify(w.frames, w.n, w.stride, verdicts=w.verdicts, counts=self.cnt[b][:w.R],
                       stats=self.cnt[b][w.R:], stream=cur.cuda_stream)
        self.inner += 1
        if self.inner == self.period:
            self._exchange(cur)

    def _exchange(self, cur):
        b = self.k % self.NBUF
        ev = torch.cuda.Event()
        ev.record(cur)
        with torch.cuda.stream(self.comm):
            self.comm.wait_event(ev)
            work = shard.allgather_counts(self.cnt[b], self.gat[b], async_op=True)
            if work is not None:
                work.wait()
            self.acc.add_(shard.global_counts(self.gat[b], self.world))
            self.cnt[b].zero_()
            d = torch.cuda.Event()
            d.record(self.comm)
            self.done[b] = d
        self.k += 1
        self.inner = 0

    def drain(self):
        cur = torch.cuda.current_stream()
        if self.inner:
            self._exchange(cur)
        cur.wait_stream(self.comm)


# GPU time of continuous steps (warmup + settle) before the timed region
SETTLE_MS = float(os.environ.get("GCL_BENCH_SETTLE_MS", "30"))
# the shortest timed window of timed_launches: its wall clock also holds the
# queue's fill before the first launch and the wake-up after the last (~60 us
# together), which 10 launches of a 56-us kernel bill at 6 us each (r06ah:
# the ingress working set 62.1 us per launch by the wall, 56.1 by events)
WINDOW_MS = float(os.environ.get("GCL_BENCH_WINDOW_MS", "10"))


def run_timed(w, steps, warmup, world, ex=None, before_last=None):
    """Warm up, then time exactly `steps` steps between a barrier +
    synchronize on both sides.  Returns (wall seconds, max over ranks;
    GPU ms per step, max over ranks): the second is a HIP event pair on the
    launch stream around the timed steps, so it is the classify kernels'
    back-to-back time (launch gaps included) and never exceeds the wall
    time of a step.  `before_last` (--dump-outputs) is called on the launch
    stream just before the last timed step."""
    stream = torch.cuda.current_stream()

    def one():
        if ex is not None:
            ex.step(w)
        else:
            w.step(stream.cuda_stream)

    # settle: the kernel reaches its steady launch time only after ~40
    # back-to-back launches (~15 ms) following any pause -- 359 -> 343 -> 336
    # us per launch over the first 60 udp64 launches, then flat
    # (profiles/archive/r02_drift_v2.jsonl) -- so the timed steps start after at
    # least SETTLE_MS of continuous steps, warmup included.  The step time is
    # estimated from the warmup (one settle step when there is none), and all
    # ranks run the same number of settle steps (the counts check needs it).
    t_w = time.perf_counter()
    for _ in range(warmup):
        one()
    pre = 0
    if warmup == 0 and SETTLE_MS > 0:
        one()
        pre = 1
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t_w) * 1e3 / max(warmup + pre, 1)
    settle = max(0, int(SETTLE_MS / max(step_ms, 1e-3)) + 1 - warmup - pre) if SETTLE_MS > 0 else 0
    if world > 1:
        t = torch.tensor([settle], dtype=torch.int64)
        if torch.distributed.get_backend() == "nccl":
            t = t.cuda()
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        settle = int(t.item())
    for _ in range(settle):
        one()
    settle += pre
    if ex is not None:
        ex.drain()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    run_timed.last_settle = settle
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(stream)
    for k in range(steps):
        if before_last is not None and k == steps - 1:
            before_last()
        one()
    if ex is not None:
        ex.drain()
    e1.record(stream)
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    gpu_ms = e0.elapsed_time(e1) / steps
    if world > 1:  # the slowest rank's wall time and GPU step time
        t = torch.tensor([el, gpu_ms], dtype=torch.float64)
        if torch.distributed.get_backend() == "nccl":
            t = t.cuda()
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        el, gpu_ms = float(t[0].item()), float(t[1].item())
    return el, gpu_ms


def group_bench(w, steps, warmup, device_index, period=EXCHANGE_EVERY, settle=None):
    """The multi-GPU step as the single-process iokernel links it
    (include/gcl_group.h): a gcl_group over this process's GPUs (one here)
    classifying the headline batch on the group's own stream, with the
    per-runtime counts and rx counters all-gathered through RCCL
    (ncclCommInitAll + ncclAllGather) every `period` steps on a side stream.
    Same buffers as the headline; timed like run_timed (settle, then K steps
    between synchronisations), the node-wide counts read back and checked.
    `settle`: untimed steps before the timed ones (the headline's own count:
    a settle sized from the warmup's wall time, which includes the group's
    first table upload, can leave the timed steps in the launch-time ramp)."""
    fl, tb = verdict_cfg(w.vbytes, w.R, w.T)
    grp = g.Group([device_index], w.R, g.HASH_JENKINS, flags=fl, thread_bits=tb,
                  exchange=g.XCHG_RCCL)
    try:
        for (r, ip, T, act, fl_tbl) in w.tables:
            grp.runtime_set(r, ip, T, act, fl_tbl)
        st = torch.cuda.ExternalStream(grp.stream(0), device=w.device)
        shard_d = {"frames": w.frames, "n": w.n, "stride": w.stride}
        k = [0]

        def one():
            grp.classify([shard_d], [w.verdicts])
            k[0] += 1
            if k[0] % period == 0:
                grp.exchange()

        t0 = time.perf_counter()
        for _ in range(max(warmup, 1)):
            one()
        grp.sync()
        step_ms = (time.perf_counter() - t0) * 1e3 / max(warmup, 1)
        if settle is None:
            settle = int(SETTLE_MS / max(step_ms, 1e-3)) + 1
        for _ in range(settle):
            one()
        grp.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(st)
        for _ in range(steps):
            one()
        e1.record(st)
        grp.sync()
        el = time.perf_counter() - t0
        grp.exchange()
        c, s, per = grp.read()
        ok = int(c.sum()) == w.n * k[0] and int(s[g.RX_PULLED]) == w.n * k[0]
        return {"what": ("gcl_group (include/gcl_group.h): one process driving this node's GPUs, "
                         "round-robin shards, RCCL ncclAllGather of u64[R+8] every "
                         f"{period} steps on a side stream; the headline buffers"),
                "n_gpus": grp.n, "exchange": "rccl",
                "value": round(w.n * grp.n * steps / el / 1e6, 1), "unit": "Mpkt/s",
                "ms_per_step": round(el / steps * 1e3, 4),
                "gpu_ms_per_step": round(e0.elapsed_time(e1) / steps, 4),
                "exchanges": int(k[0] // period) + 1, "settle_steps": settle,
                "counts_check": "ok" if ok else f"MISMATCH {int(c.sum())} != {w.n * k[0]}"}
    finally:
        grp.close()


def group_node_bench(ndev, steps, warmup, period=EXCHANGE_EVERY, vbytes=VERDICT_BYTES, shared=False):
    """The single-process multi-GPU step over `ndev` GPUs of this node (run in
    a child process by group_node_line): the udp64 workload sharded
    round-robin in 64 Ki-packet blocks, each GPU's 32 Mi-packet shard
    generated in its own HBM (a frame pool placed against its verdict ring),
    one gcl_group over all of them classifying every GPU's shard per step and
    all-gathering the counts through RCCL (ncclCommInitAll) every `period`
    steps.  Wall time between full synchronisations of every GPU; the
    node-wide counts read back through the exchange and checked.  `shared`
    (rehearsals only): fewer GPUs visible than `ndev`, so contexts share them
    and the exchange is the host sum (RCCL refuses two ranks on one device)."""
    wl, n, stride, R, T, _ = WORKLOADS["udp64"]
    fl, tb = verdict_cfg(vbytes, R, T)
    visible = torch.cuda.device_count()
    devs = [d % visible for d in range(ndev)] if shared else list(range(ndev))
    frames, verdicts = [], []
    for i, d in enumerate(devs):
        with torch.cuda.device(d):
            v = g.DeviceBuffer(n * vbytes, d)
            f = g.DeviceBuffer(n * stride, d, partner=v, vbytes=vbytes)
            torch.cuda.synchronize()
            zero_fill(f)
            g.generate(wl, n, stride, R, f, seed=SEED, rank=i, world=ndev, shard_block=SHARD_BLOCK)
            torch.cuda.synchronize()
            frames.append(f)
            verdicts.append(v)
    xchg = g.XCHG_HOST if shared else g.XCHG_RCCL
    grp = g.Group(devs, R, g.HASH_JENKINS, flags=fl, thread_bits=tb, exchange=xchg)
    try:
        rccl_ranks = grp.rccl_ranks()
        rng = np.random.default_rng(SEED)
        for r in range(R):
            act = int(rng.integers(1, T + 1))
            idx = [int(x) for x in rng.choice(T, size=act, replace=False)]
            grp.runtime_set(r, g.runtime_ip(r), T, act, g.steer_flows(T, idx))
        shards = [{"frames": f, "n": n, "stride": stride} for f in frames]
        k = [0]

        def one():
            grp.classify(shards, verdicts)
            k[0] += 1
            if k[0] % period == 0:
                grp.exchange()

        t0 = time.perf_counter()
        for _ in range(max(warmup, 1)):
            one()
        grp.sync()
        step_ms = (time.perf_counter() - t0) * 1e3 / max(warmup, 1)
        for _ in range(int(SETTLE_MS / max(step_ms, 1e-3)) + 1):
            one()
        grp.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        grp.sync()
        el = time.perf_counter() - t0
        grp.exchange()
        c, s, per = grp.read()
        ok = (int(c.sum()) == n * ndev * k[0] and int(s[g.RX_PULLED]) == n * ndev * k[0] and
              all(int(per[i, R + g.RX_PULLED]) == n * k[0] for i in range(ndev)))
        return {"what": (f"gcl_group over {ndev} GPU(s) from one process: round-robin 64Ki-pkt shards, "
                         f"{n} pkts per GPU per step, "
                         + (f"RCCL ncclAllGather of u64[R+8] every {period} steps" if not shared else
                            f"host sum of u64[R+8] every {period} steps (rehearsal: {ndev} contexts on "
                            f"{visible} GPU(s))")),
                "n_gpus": ndev, "devices": devs, "exchange": "rccl" if not shared else "host (shared GPU)",
                "rccl_ranks": rccl_ranks,
                "value": round(n * ndev * steps / el / 1e6, 1), "unit": "Mpkt/s",
                "ms_per_step": round(el / steps * 1e3, 4), "steps": steps,
                "exchanges": int(k[0] // period) + 1,
                "counts_check": "ok" if ok else "MISMATCH"}
    finally:
        grp.close()


GROUP_CHILD_TIMEOUT_S = 300


def group_node_line(args, ngpus):
    """group_node_bench over exactly @ngpus GPUs (the line's N), in a fresh
    child process with its own time limit (an RCCL or driver stall there
    cannot take the bench line down with it): the multi-GPU step as the
    single-process iokernel links it (include/gcl_group.h), beside the N
    one-process-per-GPU ranks the line's `value` times.  At N=1 the `group`
    row already covers one GPU, so only when forced.  More GPUs than visible
    only with --allow-shared-gpu (a rehearsal: host exchange)."""
    import subprocess
    if ngpus < 2 and not args.group_node_force:
        return None
    visible = torch.cuda.device_count()  # counting devices does not initialise the GPU
    shared = ngpus > visible
    if shared and not args.allow_shared_gpu:
        return {"n_gpus": ngpus, "error": f"{ngpus} GPUs asked, {visible} visible"}
    cmd = [sys.executable, os.path.abspath(__file__), "--group-child", str(ngpus),
           "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--allow-shared-gpu"] if shared else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=GROUP_CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        return {"n_gpus": ngpus, "error": f"timeout ({GROUP_CHILD_TIMEOUT_S} s)"}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"n_gpus": ngpus, "error": (r.stderr.strip()[-300:] or f"rc {r.returncode}")}
    out = json.loads(lines[-1])
    if not shared:
        out["host_ingress_c"] = grouppipe_run(ngpus)
    return out


def cpu_child_line(args, value):
    """The CPU baseline (cpu_baseline) in a fresh CPU-only child process, for
    the N>1 lines: rank 0's process holds a GPU context and its rank's
    buffers, the child only the oracle.  `gpu_over_1core_nic` is this line's
    whole-job value over one core."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-child", "--cpu-budget", str(args.cpu_budget)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=max(120.0, 6 * args.cpu_budget))
    except subprocess.TimeoutExpired:
        return {"error": "cpu child timeout"}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        return {"error": (r.stderr.strip()[-300:] or f"rc {r.returncode}")}
    cpu = json.loads(lines[-1])
    if cpu.get("value"):
        cpu["gpu_over_1core_nic"] = round(value / cpu["value"], 1)
    return cpu


def node_extras(args, world, value):
    """What an N>1 line carries beside its own ranks' measurement (rank 0,
    after the process group is gone): the product's multi-GPU path over the
    same N GPUs (group_node) and the CPU baseline timed on this host."""
    out = {}
    if not args.no_group:
        node = group_node_line(args, world)
        if node is not None:
            out["group_node"] = node
    if not args.no_cpu:
        out["cpu_baseline"] = cpu_child_line(args, value)
    return out


def grouppipe_run(ndev, n=8 << 20, iters=5):
    """tools/grouppipe: the same group driven from C over a host-memory
    ingress batch (n udp64 frames in pinned memory split over the GPUs,
    zero-copy and header DMA-gather); PCIe-inclusive, never `value`."""
    import subprocess
    exe = os.path.join(ROOT, "tools", "grouppipe")
    if not os.access(exe, os.X_OK):
        return {"skipped": "tools/grouppipe not built"}
    try:
        r = subprocess.run([exe, str(ndev), str(n), str(iters)], capture_output=True, text=True, timeout=180)
    except subprocess.TimeoutExpired:
        return {"error": "timeout (180 s)"}
    if r.returncode != 0:
        return {"error": r.stderr.strip()[-300:] or f"rc {r.returncode}"}
    return json.loads(r.stdout.strip().splitlines()[-1])


# a committed PMC pass stands for this run's launch only if its kernel time
# is within this of the launch time measured here (a stale profile of a
# different kernel build or placement is dropped, not passed off as current)
PMC_TIME_SLACK = 0.15


def pmc_traffic(name, vbytes, kernel_ms=None, scale=1.0):
    """(HBM bytes per launch, source label) from the committed PMC passes
    (profiles/pmc_*.json, tools/prof_summary.py: FETCH_SIZE + WRITE_SIZE,
    gfx950-corrected), scaled by @scale packets; (None, label) when there is
    no profile or its kernel time disagrees with @kernel_ms.  The counters are
    NOT taken in this run: rocprofv3 --pmc cannot run under the bench's own
    timing, so the label names the file and the kernel time it was taken at."""
    rel = f"profiles/pmc_{name}{'' if vbytes == 8 else f'_v{vbytes}'}.json"
    try:
        with open(os.path.join(ROOT, rel)) as f:
            prof = json.load(f)
    except (OSError, ValueError):
        return None, None
    traffic = prof.get("hbm_bytes_per_launch")
    avg_ms = (prof.get("avg_kernel_ns") or 0) / 1e6 * scale
    label = f"{rel}: committed PMC pass, not this run's counters; kernel avg {avg_ms:.4f} ms there"
    if traffic is None:
        return None, label
    if kernel_ms and avg_ms and abs(avg_ms / kernel_ms - 1) > PMC_TIME_SLACK:
        return None, label + f" vs {kernel_ms:.4f} ms here: dropped as stale"
    return traffic * scale, label


READ_SOL_PATH = "profiles/r06_read_sol.jsonl"


def read_sol():
    """The HBM read speed of light measured on an MI355X box (tools/read_sol:
    the fastest of 81 pure streaming-read shapes over a 2 GiB slab, the
    udp64 slab's size), from the committed file; None without it."""
    try:
        with open(os.path.join(ROOT, READ_SOL_PATH)) as f:
            last = json.loads(f.read().strip().splitlines()[-1])
        return float(last["best_GBs"])
    except (OSError, ValueError, KeyError, IndexError):
        return None


def roofline_obj(bytes_per_launch, kernel_ms, traffic, extra=None, bound="hbm", peak=HBM_PEAK_GBS):
    """@traffic: None, or (bytes, source label) from pmc_traffic.  An HBM-bound
    row also gets `read_sol`: its algorithmic rate over the measured read
    speed of light (read_sol)."""
    traffic, source = traffic if isinstance(traffic, tuple) else (traffic, None)
    achieved = bytes_per_launch / (kernel_ms * 1e-3) / 1e9
    r = {"bound": bound, "achieved": round(achieved, 1), "peak": peak, "unit": "GB/s",
         "frac": round(achieved / peak, 4), "traffic": traffic,
         "kernel_ms": round(kernel_ms, 4)}
    if source:
        r["traffic_source"] = source
    sol = read_sol() if bound == "hbm" else None
    if sol:
        r["read_sol"] = {"GBs": sol, "frac": round(achieved / sol, 4),
                         "src": f"{READ_SOL_PATH}: committed tools/read_sol run, not this process"}
    if extra:
        r.update(extra)
    if traffic:
        moved = traffic / (kernel_ms * 1e-3) / 1e9
        r["moved"] = {"achieved": round(moved, 1), "frac": round(moved / HBM_PEAK_GBS, 4),
                      "what": "HBM bytes moved per launch (PMC traffic) / kernel time"}
    return r


def roofline(w, kernel_ms):
    """The roofline object of one workload's classify launch.  The committed
    PMC passes were taken at the workload's default batch size, so their
    bytes are scaled per packet to this launch's (strong scaling)."""
    traffic = pmc_traffic(w.name, w.vbytes, kernel_ms, w.n / WORKLOADS[w.name][1])
    return roofline_obj(w.n * w.bytes_per_pkt, kernel_ms, traffic,
                        {"bytes_per_pkt": w.bytes_per_pkt})


def placement(w):
    """How the frame pool was placed against the verdict ring
    (gcl_dev_alloc_paired: DESIGN.md §4 "Buffer placement")."""
    info = getattr(w.frames, "pair_info", None)
    if info is None:
        return {"policy": "plain hipMalloc (gcl_dev_alloc): the kernel defers its 1-/2-B verdicts, "
                          "which takes the placement class away"}
    checks = getattr(w, "placement_checks", [])
    return {"policy": "gcl_dev_alloc_paired (frame pool placed against the verdict ring)",
            **info,
            "class_chosen": ("fast (cross-class pair: both classes seen)" if info["classes_seen"] == 2
                             else "unknown (one class in every candidate)"),
            "kernel_checks": checks, "replaced": sum(1 for c in checks if c.get("passed") is False
                                                     and not c.get("kept_failed"))}


def e2e_bench(device, vbytes=VERDICT_BYTES, reps=3):
    """Rates with the frames in pinned HOST memory (the NIC's mbufs) and the
    verdicts returned to host memory: PCIe-inclusive, never `value`.
    DMA-gather of the 64-B header granules (COPY), PCIe zero-copy reads by the
    kernel (ZEROCOPY), and for jumbo frames the naive full-frame H2D copy."""
    out = {}
    for name, n in (("udp64", 32 << 20), ("mixed", 256 << 10)):
        wl, _, stride, R, T, _ = WORKLOADS[name]
        dfr = torch.zeros(n * stride, dtype=torch.uint8, device=device)
        g.generate(wl, n, stride, R, dfr, seed=SEED)
        hfr = torch.empty(n * stride, dtype=torch.uint8).pin_memory()
        hfr.copy_(dfr)
        hv = torch.empty(n * vbytes, dtype=torch.uint8).pin_memory()
        clf = classifier(device, R, T, vbytes)
        setup_tables(clf, R, T)
        res = {"pkts": n, "slot_stride": stride}
        for tag, mode, nst in (("copy_hdr_2streams", g.E2E_COPY, 2), ("copy_hdr_4streams", g.E2E_COPY, 4),
                               ("zerocopy", g.E2E_ZEROCOPY, 1)):
            clf.classify_host(hfr, n, stride, verdicts=hv, mode=mode, nstreams=nst)
            t0 = time.perf_counter()
            for _ in range(reps):
                clf.classify_host(hfr, n, stride, verdicts=hv, mode=mode, nstreams=nst)
            dt = (time.perf_counter() - t0) / reps
            res[tag + "_mpps"] = round(n / dt / 1e6, 1)
        # naive: copy whole frames H2D, classify in HBM, copy verdicts back
        dv = torch.empty(n * vbytes, dtype=torch.uint8, device=device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            dfr.copy_(hfr, non_blocking=True)
            clf.classify(dfr, n, stride, verdicts=dv, stream=torch.cuda.current_stream().cuda_stream)
            hv.copy_(dv, non_blocking=True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / reps
        res["copy_full_frames_mpps"] = round(n / dt / 1e6, 2)
        res["h2d_full_frames_GBs"] = round(n * stride / dt / 1e9, 1)
        out[name] = res
        del dfr, hfr, hv, dv, clf
        torch.cuda.empty_cache()
    out["rxloop"] = rxloop_bench(device, vbytes)
    out["rx_burst_pipeline"] = rxpipe_bench()
    out["rx_burst_pipeline_ingress"] = ingress_pipeline_bench()
    out["mixed"]["trace_replay"] = trace_replay(device)
    out["ingress_pool"] = ingress_pool_bench(device, INGRESS_VERDICT_BYTES)
    return out


def e2e_multi(device, rank, world, vbytes, reps=3, n=256 << 10, keep=None):
    """Config 5 on N GPUs: every rank classifies its round-robin shard of the
    mixed jumbo trace from pinned host memory, PCIe zero-copy and header
    DMA-gather; barrier + max-over-ranks timing, RX_PULLED summed over ranks
    as the accounting check.  PCIe-inclusive: never `value`.  `keep` (a dict,
    tests) receives this rank's last verdicts and its accumulated stats."""
    wl, _, stride, R, T, _ = WORKLOADS["mixed"]
    dfr = torch.zeros(n * stride, dtype=torch.uint8, device=device)
    g.generate(wl, n, stride, R, dfr, seed=SEED, rank=rank, world=world, shard_block=SHARD_BLOCK)
    hfr = torch.empty(n * stride, dtype=torch.uint8).pin_memory()
    hfr.copy_(dfr)
    del dfr
    torch.cuda.synchronize()
    hv = torch.empty(n * vbytes, dtype=torch.uint8).pin_memory()
    clf = classifier(device, R, T, vbytes)
    setup_tables(clf, R, T)
    nccl = torch.distributed.get_backend() == "nccl"
    res = {"pkts_per_gpu": n, "slot_stride": stride, "n_gpus": world}
    calls = 0
    stats = np.zeros(g.NR_STATS, dtype=np.uint64)
    for tag, mode, nst in (("zerocopy", g.E2E_ZEROCOPY, 1), ("copy_hdr_2streams", g.E2E_COPY, 2)):
        clf.classify_host(hfr, n, stride, verdicts=hv, stats=stats, mode=mode, nstreams=nst)
        calls += 1
        torch.cuda.synchronize()
        torch.distributed.barrier()
        t0 = time.perf_counter()
        for _ in range(reps):
            clf.classify_host(hfr, n, stride, verdicts=hv, stats=stats, mode=mode, nstreams=nst)
        calls += reps
        el = time.perf_counter() - t0
        t = torch.tensor([el], dtype=torch.float64)
        t = t.cuda() if nccl else t
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        res[tag + "_mpps"] = round(world * n * reps / float(t.item()) / 1e6, 1)
    pulled = torch.tensor([int(stats[6])], dtype=torch.int64)  # GCL_RX_PULLED
    pulled = pulled.cuda() if nccl else pulled
    torch.distributed.all_reduce(pulled)
    res["rx_pulled_check"] = "ok" if int(pulled.item()) == world * n * calls else \
        f"MISMATCH {int(pulled.item())} != {world * n * calls}"
    if keep is not None:
        keep.update(verdicts=hv.numpy().copy(), stats=stats.copy(), calls=calls, n=n)
    del hfr, hv, clf
    torch.cuda.empty_cache()
    return res


def rxpipe_bench(reps=3):
    """The whole rx_burst replacement on ONE host core (tools/rxpipe.cpp, C):
    persistent GPU loop + the lrpc post-pass (gcl_host_deliver4) into 128
    kthread rings, bursts of 64..4096 mbufs from a registered host region.
    Compare with cpu_baseline.lrpc_1core_mpps (the reference's classify +
    lrpc_send on one core).  Built by __graft_entry__.build()."""
    import subprocess
    exe = os.path.join(ROOT, "tools", "rxpipe")
    if not os.access(exe, os.X_OK):
        return {"skipped": "tools/rxpipe not built (python -c 'import __graft_entry__ as g; g.build()')"}
    rows = []
    # burst 64 is the reference's own (IOKERNEL_RX_BURST_SIZE, defs.h:75):
    # throughput there is workers / round trip, so it is run at 1, 4, 8, 16
    # and 32 workers; verdicts are read in place in the slot
    # (gcl_rxloop_peek), and once copied out (the round-2 form) for comparison.
    # The flow hash is the JENKINS 5-tuple computed on the GPU, and in the
    # "nic" rows the mbuf's hash.rss submitted with the packets -- what rx.c
    # itself steers by (rx.c:83), and what cpu_baseline.nic_mode times
    nic = "RXPIPE_HASH=nic"
    for cfg in (("64", "1", "1", "20000"), ("64", "4", "8", "20000"), ("64", "4", "8", "20000", "copy"),
                ("64", "8", "16", "40000"), ("64", "16", "32", "40000"), ("64", "32", "64", "60000"),
                ("64", "8", "16", "40000", "inline"), ("64", "16", "32", "40000", "inline"),
                ("64", "1", "1", "20000", "records"), ("64", "4", "8", "20000", "records"),
                ("64", "8", "16", "40000", "records"),
                ("64", "16", "32", "40000", "records"),
                (nic, "64", "1", "1", "20000", "records"), (nic, "64", "4", "8", "20000", "records"),
                (nic, "64", "8", "16", "40000", "records"), (nic, "64", "16", "32", "40000", "records"),
                ("256", "4", "8", "10000"),
                ("1024", "8", "16", "4000"), ("4096", "16", "16", "1000")):
        env = dict(os.environ)
        if cfg[0] == nic:
            env["RXPIPE_HASH"] = "nic"
            cfg = cfg[1:]
        # the host core's rate swings run to run on a shared host: three
        # fresh processes per row, the median one reported with all three rates
        samples, err = [], None
        for _ in range(reps):
            try:
                r = subprocess.run([exe, *cfg], capture_output=True, text=True, timeout=120, env=env)
            except subprocess.TimeoutExpired:
                err = {"burst": int(cfg[0]), "error": "timeout"}
                break
            if r.returncode != 0:
                err = {"burst": int(cfg[0]), "error": r.stderr.strip()[-200:]}
                break
            samples.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if err:
            rows.append(err)
            break
        samples.sort(key=lambda x: x["mpps_one_core"])
        row = dict(samples[len(samples) // 2])
        row["mpps_samples"] = [x["mpps_one_core"] for x in samples]
        rows.append(row)
    return {"host_cores": 1, "reps_per_row": reps, "reported": "median of the row's runs", "runs": rows}


def cpupipe_exe():
    """tools/cpupipe built for this host (-march=native, as the CPU baseline's
    oracle is, orc.build(native=True)) on first use, else the portable build
    __graft_entry__.build() made; None if neither exists."""
    import subprocess
    src = os.path.join(ROOT, "tools", "cpupipe.cpp")
    native = os.path.join(ROOT, "tools", "_build", "cpupipe_native")
    portable = os.path.join(ROOT, "tools", "cpupipe")
    if not (os.access(native, os.X_OK) and os.path.getmtime(native) >= os.path.getmtime(src)):
        try:
            os.makedirs(os.path.dirname(native), exist_ok=True)
            obj = native + "_orc.o"
            subprocess.run(["gcc", "-std=gnu11", "-O3", "-march=native", "-fPIC", "-c",
                            os.path.join(ROOT, "oracle", "orc.c"), "-o", obj], check=True, capture_output=True,
                           timeout=120)
            subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-march=native",
                            "-I" + os.path.join(ROOT, "include"), "-o", native, src, "-x", "none", obj, "-lpthread"],
                           check=True, capture_output=True, timeout=300)
        except (OSError, subprocess.SubprocessError) as e:
            log("cpupipe native build failed, using the portable build:", e)
            native = None
    if native and os.access(native, os.X_OK):
        return native
    return portable if os.access(portable, os.X_OK) else None


def median_runs(cmd, env, reps, timeout=180):
    """@reps fresh runs of a pipeline tool: (median row with every run's rate, error row or None)."""
    import subprocess
    samples = []
    for _ in range(reps):
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
        except subprocess.TimeoutExpired:
            return None, {"cmd": " ".join(cmd[1:]), "error": "timeout"}
        if r.returncode != 0:
            return None, {"cmd": " ".join(cmd[1:]), "error": r.stderr.strip()[-200:]}
        samples.append(json.loads(r.stdout.strip().splitlines()[-1]))
    samples.sort(key=lambda x: x["mpps_one_core"])
    row = dict(samples[len(samples) // 2])
    row["mpps_samples"] = [x["mpps_one_core"] for x in samples]
    return row, None


def ingress_pipeline_bench(reps=3):
    """The rx_burst replacement and the reference's CPU path on IDENTICAL
    inputs with cold headers: bursts of 64 mbufs of the
    reference's pool geometry (data at element + 344 of 9408-B elements,
    defs.h:503-506) from an emulated NIC that writes every frame with
    non-temporal stores just before handing its descriptor over (no CPU cache
    holds the header, as behind a NIC without DDIO) and recycles the mbufs
    through a mempool (tools/nicsim.h).  GPU rows: tools/rxpipe
    RXPIPE_POOL=ingress (header records and stamped offsets); CPU rows:
    tools/cpupipe, the oracle's rx_one_pkt with rx.c's direct loads and
    prefetch stride 2 (+ lrpc_send) on one core; NIC hash.rss in both."""
    exe = os.path.join(ROOT, "tools", "rxpipe")
    cpu_exe = cpupipe_exe()
    env = {**os.environ, "RXPIPE_POOL": "ingress", "RXPIPE_HASH": "nic"}
    out = {"inputs": ("NIC-emulated ingress pool: 16384 mbufs at element + 344 of 9408-B elements, frames "
                      "written by 4 NIC threads with non-temporal stores (cold headers), mempool recycling; "
                      "NIC hash.rss"), "reps_per_row": reps, "gpu": [], "cpu": []}
    if os.access(exe, os.X_OK):
        for cfg in (("64", "1", "1", "20000", "records"), ("64", "4", "8", "20000", "records"),
                    ("64", "8", "16", "40000", "records"), ("64", "4", "8", "20000"), ("64", "8", "16", "40000")):
            row, err = median_runs([exe, *cfg], env, reps)
            out["gpu"].append(row or err)
            if err:
                break
    if cpu_exe:
        # the reference's own loop (rx.c's prefetch stride 2), classify-only
        # and + lrpc_send; then the latter with the whole burst's headers
        # prefetched first, the help the records submit gives the GPU's host side
        for post in (("classify",), ("lrpc",), ("lrpc", "prefetch")):
            row, err = median_runs([cpu_exe, "100000", *post], env, reps)
            out["cpu"].append(row or err)
            if err:
                break
    return out


def rxloop_bench(device, vbytes, iters=2000, rounds=3):
    """Burst latency at the reference's granularity (rx_burst's <= 64 mbufs,
    iokernel/rx.c:270-290): the persistent rx loop (gcl_rxloop_*) reading the
    frames zero-copy from pinned host memory, against one launch per burst
    (gcl_classify_host ZEROCOPY, timed from Python, so ctypes overhead is
    included)."""
    wl, _, stride, R, T, _ = WORKLOADS["udp64"]
    n = 1 << 16
    dfr = torch.zeros(n * stride, dtype=torch.uint8, device=device)
    g.generate(wl, n, stride, R, dfr, seed=SEED)
    hfr = torch.empty(n * stride, dtype=torch.uint8).pin_memory()
    hfr.copy_(dfr)
    torch.cuda.synchronize()
    clf = classifier(device, R, T, vbytes)
    setup_tables(clf, R, T)
    out = {"frames": "udp64 synthetic, pinned host memory, read zero-copy"}

    def pct(lat):
        us = np.sort(lat.astype(np.float64)) / 1e3
        return {"p50_us": round(float(us[len(us) // 2]), 2),
                "p99_us": round(float(us[int(len(us) * 0.99)]), 2),
                "mean_us": round(float(us.mean()), 2)}

    # The host's latency mode drifts in streaks, so the rows
    # run interleaved in three rounds and each reports its median round
    # (by p50), with every round's p50.
    cfgs = ((64, 1, 1, 0), (64, 1, 1, g.LOOP_INLINE_HDRS), (64, 1, 1, g.LOOP_HDR_RECORDS),
            (256, 1, 1, 0), (1024, 1, 1, 0), (64, 4, 8, 0), (64, 4, 8, g.LOOP_HDR_RECORDS),
            (1024, 8, 16, 0))
    runs = {c: [] for c in cfgs}
    for _ in range(rounds):
        for burst, workers, depth, fl in cfgs:
            loop = clf.rxloop(hfr, slots=16, max_burst=burst, workers=workers, lifetime_ms=30000,
                              flags=fl)
            try:
                offs = np.arange(burst, dtype=np.uint64) * np.uint64(stride)
                loop.drive(offs, 50, depth)  # warm
                lat, el = loop.drive(offs, iters, depth)
            finally:
                loop.stop()
            r = pct(lat)
            r["mpps"] = round(burst * iters / (el / 1e9) / 1e6, 2)
            runs[(burst, workers, depth, fl)].append(r)
    for (burst, workers, depth, fl), rs in runs.items():
        rs.sort(key=lambda r: r["p50_us"])
        r = dict(rs[len(rs) // 2])
        r["p50_us_rounds"] = [x["p50_us"] for x in rs]
        out[f"loop_burst{burst}_w{workers}_d{depth}" + {0: "", g.LOOP_INLINE_HDRS: "_inline_hdrs",
                                                          g.LOOP_HDR_RECORDS: "_hdr_records"}[fl]] = r
    hv = torch.empty(64 * vbytes, dtype=torch.uint8).pin_memory()
    lat = []
    for i in range(iters // 4 + 20):
        t0 = time.perf_counter_ns()
        clf.classify_host(hfr, 64, stride, verdicts=hv, mode=g.E2E_ZEROCOPY, nstreams=1)
        if i >= 20:
            lat.append(time.perf_counter_ns() - t0)
    out["launch_per_burst64"] = pct(np.array(lat))
    del dfr, hfr, hv, clf
    torch.cuda.empty_cache()
    return out


def timed_launches(fn, reps):
    """(wall s, GPU ms) per call of `fn` over at least `reps` back-to-back
    calls on the current stream -- more where `reps` calls would take less
    than WINDOW_MS -- after untimed calls covering SETTLE_MS (the settle
    phase of run_timed)."""
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    est_ms = max((time.perf_counter() - t0) * 1e3, 1e-3)
    for _ in range(int(SETTLE_MS / est_ms) + 1):
        fn()
    torch.cuda.synchronize()
    # the settle phase's own rate, without the single call's sync latency
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    est_ms = max((time.perf_counter() - t0) * 1e3 / reps, 1e-3)
    reps = max(reps, int(WINDOW_MS / est_ms))
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, e0.elapsed_time(e1) / reps


def ceiling(clf, frames, n, stride, out, kernel_ms, reps=10, **kw):
    """The layout's own ceiling, measured in this process on the same buffers:
    gcl_access_probe -- the classify launch's loads (frame bytes [0, 40) as
    16-B chunks, the descriptor arrays) and its per-packet stores, no
    classification -- timed like the kernel.  frac_of_ceiling = probe time /
    kernel time: how close the kernel runs to what this frame layout allows
    (e.g. one 128-B line per header of a 1536-B slot).  The fastest of
    three timed rounds: the ceiling is what the shape reaches, and a single
    round's noise (~1 %) put tcp1500's ratio above 1 (r06p)."""
    st = torch.cuda.current_stream().cuda_stream
    pms = min(timed_launches(lambda: clf.access_probe(frames, n, stride, out=out, stream=st, **kw), reps)[1]
              for _ in range(3))
    return {"ceiling_ms": round(pms, 4), "frac_of_ceiling": round(pms / kernel_ms, 4),
            "ceiling_what": ("gcl_access_probe on the same buffers: the launch's header loads, "
                             "descriptor loads and per-packet stores without the classification")}


# Algorithmic bytes of the integrated rx_burst shape, per
# packet: the 64-B header granule + the descriptor's u64 offset into the mbuf
# pool + u8 ol_flags + u32 hash.rss + the verdict.
INGRESS_DESC_BYTES = 8 + 1 + 4
INGRESS_WORKING_SET = 4096


def ingress_pool_bench(device, vbytes, cycles=64, reps=10, zerocopy=True,
                       rows=("nic", "jenkins", "working_set")):
    """Frames where the reference keeps them (§8f-2): the 131072-mbuf ingress
    pool, 9408-B elements, 222 per 2 MiB page, frame data at element + 344
    (8-B aligned; iokernel/defs.h:70, :503-523).  A batch is `cycles` random
    passes over the pool (descriptor i -> offs[i], like rte_eth_rx_burst
    handing back recycled mbufs), each descriptor with the mbuf's ol_flags
    and hash.rss, classified in GCL_HASH_NIC mode -- the integrated rx_burst
    replacement of INTEGRATION.md §4.  Device-resident (pool in HBM, with a
    roofline) and PCIe zero-copy (pool in pinned host memory, as the shm
    region would be).  The JENKINS row with offsets only is kept beside it."""
    wl, _, _, R, T, _ = WORKLOADS["udp64"]
    P = g.IOKERNEL_NUM_MBUFS
    hdr = torch.zeros(P * 64, dtype=torch.uint8, device=device)
    olf_p = torch.zeros(P, dtype=torch.uint8, device=device)
    rss_p = torch.zeros(P, dtype=torch.int32, device=device)
    g.generate(wl, P, 64, R, hdr, olflags=olf_p, rss=rss_p, seed=SEED)
    pool_offs = torch.from_numpy(g.mbuf_data_offsets(P).view(np.int64)).to(device)
    region = torch.zeros(g.mbuf_region_bytes(P), dtype=torch.uint8, device=device)
    region[(pool_offs[:, None] + torch.arange(64, device=device)).view(-1)] = hdr
    del hdr
    gen = torch.Generator(device="cpu").manual_seed(SEED)
    order = torch.cat([torch.randperm(P, generator=gen) for _ in range(cycles)]).to(device)
    offs = pool_offs[order].contiguous()
    olf = olf_p[order].contiguous()
    rss = rss_p[order].contiguous()
    n = offs.numel()
    out = {"mbufs": P, "pkts_per_batch": n, "frame_data_offset": "element + 344 (8-B aligned)",
           "descriptor_order": f"{cycles} random permutations of the pool"}
    cnt = torch.zeros(R + g.NR_STATS, dtype=torch.int64, device=device)
    if os.environ.get("GCL_BENCH_PLACEMENT", "1") != "0":
        # the device-resident pool placed against the verdict ring, as the
        # udp64 frame pool is (gcl_dev_alloc_paired, DESIGN.md §4 "Buffer
        # placement"): the iokernel places its ingress region once at start-up
        dv = g.DeviceBuffer(n * vbytes, device.index or 0)
        placed = g.DeviceBuffer(region.numel(), device.index or 0, partner=dv, vbytes=vbytes)
        torch.cuda.synchronize()
        hip_copy(placed, region, region.numel())
        del region
        region = placed
        out["placement"] = placed.pair_info
    else:
        dv = torch.empty(n * vbytes, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream().cuda_stream
    nic = classifier(device, R, T, vbytes, hash_mode=g.HASH_NIC)
    setup_tables(nic, R, T)
    bpp = HDR_BYTES + INGRESS_DESC_BYTES + vbytes

    def counts_ok():
        tot = int(cnt[:R].sum().item())
        return tot % n == 0 and int(cnt[R + g.RX_PULLED].item()) == tot

    if "nic" in rows:
        cnt.zero_()

        def nic_step():
            nic.classify(region, n, 0, verdicts=dv, counts=cnt[:R], stats=cnt[R:], offs=offs,
                         olflags=olf, rss=rss, stream=st)

        wall, gms = timed_launches(nic_step, reps)
        out["integrated_nic"] = {
            "what": "offs[] + ol_flags[] + hash.rss[] per descriptor, GCL_HASH_NIC (INTEGRATION.md §4)",
            "device_resident_mpps": round(n / wall / 1e6, 1),
            "counts_check": "ok" if counts_ok() else "MISMATCH",
            "roofline": roofline_obj(n * bpp, gms, pmc_traffic("ingress_nic", vbytes, gms),
                                     {"bytes_per_pkt": bpp,
                                      **ceiling(nic, region, n, 0, dv, gms, offs=offs, olflags=olf,
                                                rss=rss)})}
    jen = None
    if "jenkins" in rows:
        cnt.zero_()
        jen = classifier(device, R, T, vbytes)
        setup_tables(jen, R, T)

        def jen_step():
            jen.classify(region, n, 0, verdicts=dv, counts=cnt[:R], stats=cnt[R:], offs=offs,
                         stream=st)

        wall_j, gms_j = timed_launches(jen_step, reps)
        out["jenkins_offs_only"] = {"device_resident_mpps": round(n / wall_j / 1e6, 1),
                                    "kernel_ms": round(gms_j, 4),
                                    "counts_check": "ok" if counts_ok() else "MISMATCH"}
    if "working_set" in rows:
        # the working set the reference really cycles: mbufs come back through
        # the iokernel lcore's LIFO mempool cache (MBUF_CACHE_SIZE 250, rx.c:21)
        # into an RX ring of 256 / 2048 descriptors (dpdk.c:50-53), so a few
        # thousand mbufs are in rotation, not the whole 131072-mbuf pool
        ws = INGRESS_WORKING_SET
        sub = torch.randperm(P, generator=gen)[:ws]
        order_ws = torch.cat([sub[torch.randperm(ws, generator=gen)] for _ in range(n // ws)]).to(device)
        offs_w, olf_w, rss_w = (pool_offs[order_ws].contiguous(), olf_p[order_ws].contiguous(),
                                rss_p[order_ws].contiguous())
        cnt.zero_()

        def ws_step():
            nic.classify(region, n, 0, verdicts=dv, counts=cnt[:R], stats=cnt[R:], offs=offs_w,
                         olflags=olf_w, rss=rss_w, stream=st)

        wall_w, gms_w = timed_launches(ws_step, reps)
        out["integrated_nic_working_set"] = {
            "what": (f"as integrated_nic, descriptors drawn from a working set of {ws} mbufs in random "
                     f"order (RX ring 2048 + mempool cache 250 + in flight)"),
            "device_resident_mpps": round(n / wall_w / 1e6, 1),
            "counts_check": "ok" if counts_ok() else "MISMATCH",
            # the working set's frames (~1 MB of header lines) stay in L2:
            # the bound is the L2's, not HBM's (HBM moves 0.26 of its peak)
            "roofline": roofline_obj(n * bpp, gms_w, pmc_traffic("ingress_ws", vbytes, gms_w),
                                     {"bytes_per_pkt": bpp,
                                      **ceiling(nic, region, n, 0, dv, gms_w, offs=offs_w, olflags=olf_w,
                                                rss=rss_w)},
                                     bound="l2", peak=L2_PEAK_GBS)}
        del offs_w, olf_w, rss_w, order_ws
    if not zerocopy or "nic" not in rows:
        del region, offs, olf, rss, dv, nic, jen
        torch.cuda.empty_cache()
        return out
    # zero-copy: the pool in pinned host memory, descriptors and verdicts too
    hreg = torch.empty(region.numel(), dtype=torch.uint8).pin_memory()
    hip_copy(hreg, region, region.numel())
    del region
    hoffs = offs.cpu().pin_memory()
    holf = olf.cpu().pin_memory()
    hrss = rss.cpu().pin_memory()
    hv = torch.empty(n * vbytes, dtype=torch.uint8).pin_memory()
    kw = dict(verdicts=hv, offs=hoffs, olflags=holf, rss=hrss, mode=g.E2E_ZEROCOPY)
    nic.classify_host(hreg, n, 0, **kw)
    t0 = time.perf_counter()
    for _ in range(3):
        nic.classify_host(hreg, n, 0, **kw)
    out["integrated_nic"]["zerocopy_mpps"] = round(n / ((time.perf_counter() - t0) / 3) / 1e6, 1)
    # COPY over the same descriptors: the header gather kernel pulls each
    # mbuf's first 80 B out of the pinned pool into HBM rows, chunk by chunk
    # on 2 or 4 streams, and the batch kernel classifies the rows
    for nst in (2, 4):
        kwc = dict(kw, mode=g.E2E_COPY, nstreams=nst, chunk=1 << 20)
        nic.classify_host(hreg, n, 0, **kwc)
        t0 = time.perf_counter()
        for _ in range(3):
            nic.classify_host(hreg, n, 0, **kwc)
        out["integrated_nic"][f"copy_gather_{nst}streams_mpps"] = round(
            n / ((time.perf_counter() - t0) / 3) / 1e6, 1)
    del hreg, hoffs, holf, hrss, hv, offs, olf, rss, dv, nic, jen
    torch.cuda.empty_cache()
    return out


def trace_replay(device, n=64 << 10, reps=3):
    """Config 5's ingest path: the mixed jumbo stream written as a pcap trace,
    loaded by gcl_pcap_load into host memory, registered, and classified by
    the kernel over PCIe (ZEROCOPY, frames at arbitrary 16-B offsets)."""
    import tempfile
    wl, _, stride, R, T, _ = WORKLOADS["mixed"]
    dfr = torch.zeros(n * stride, dtype=torch.uint8, device=device)
    dpl = torch.zeros(n, dtype=torch.int16, device=device)
    dfl = torch.zeros(n, dtype=torch.uint8, device=device)
    g.generate(wl, n, stride, R, dfr, olflags=dfl, seed=SEED, pkt_len=dpl)
    frames = dfr.cpu().numpy()
    pl = dpl.cpu().numpy().view(np.uint16)
    olf = np.ascontiguousarray(dfl.cpu().numpy())
    del dfr
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "mixed.pcap")
        g.pcap_write(path, frames, pl, stride=stride)
        fsize = os.path.getsize(path)
        t0 = time.perf_counter()
        tr = g.Trace(path)
        load_s = time.perf_counter() - t0
    clf = g.Classifier(device.index or 0, R, g.HASH_JENKINS)
    setup_tables(clf, R, T)
    hv = np.zeros(n, dtype=g.VERDICT_DTYPE)
    regs = (tr.frames, tr.offs, olf, hv)
    for a in regs:
        g.host_register(a)
    try:
        kw = dict(verdicts=hv, offs=tr.offs, olflags=olf, frames_len=tr.frames_len,
                  mode=g.E2E_ZEROCOPY)
        clf.classify_host(tr.frames, n, 0, **kw)
        t0 = time.perf_counter()
        for _ in range(reps):
            clf.classify_host(tr.frames, n, 0, **kw)
        dt = (time.perf_counter() - t0) / reps
    finally:
        for a in regs:
            g.host_unregister(a)
    return {"pkts": n, "pcap_bytes": fsize, "pcap_load_s": round(load_s, 3),
            "zerocopy_mpps": round(n / dt / 1e6, 1),
            "wire_bytes_rate_GBs": round(float(pl.astype(np.float64).sum()) / dt / 1e9, 1)}


# The GPU box's CPU share for one GPU (the pool's rule for worker pools;
# os.cpu_count() there reports the whole host)
BOX_CPU_SHARE = 16


# bounded CPU samples of each timed stream (SURVEY §8d "CPU timing beside
# it"; BASELINE.md: 64 B, 1500 B with 1024 runtimes and Zipf, mixed jumbo):
# (packets, share of the budget).  The 1500-B and jumbo samples are far larger
# than the host's caches, so every header is a DRAM miss as on the NIC's mbufs.
CPU_STREAMS = {"udp64": (2 << 20, 0.5), "tcp1500": (512 << 10, 0.25), "mixed": (256 << 10, 0.25)}
ZIPF_FLOWS = 1 << 20


def _proc_stat_idle():
    """Idle + iowait jiffies of every CPU (/proc/stat), {} on error."""
    idle = {}
    try:
        with open("/proc/stat") as f:
            for line in f:
                if line.startswith("cpu") and line[3].isdigit():
                    p = line.split()
                    idle[int(p[0][3:])] = int(p[4]) + int(p[5])
    except (OSError, ValueError, IndexError):
        return {}
    return idle


def _siblings(cpu):
    """The SMT siblings of @cpu (sysfs thread_siblings_list), @cpu included."""
    try:
        with open(f"/sys/devices/system/cpu/cpu{cpu}/topology/thread_siblings_list") as f:
            out = set()
            for part in f.read().strip().split(","):
                lo, _, hi = part.partition("-")
                out.update(range(int(lo), int(hi or lo) + 1))
            return frozenset(out)
    except (OSError, ValueError):
        return frozenset((cpu,))


def pick_cores(k, allowed=None, idle_a=None, idle_b=None, siblings=_siblings):
    """@k CPUs on @k distinct physical cores of this process's affinity mask,
    the idlest cores first (idle jiffies of the CPU and its SMT siblings over
    100 ms; highest CPU number on a tie, away from CPU 0's housekeeping) --
    the way tools/rxpipe.cpp pins its host core, and the iokernel its
    dataplane lcore (dpdk.c:276-280)."""
    if allowed is None:
        try:
            allowed = sorted(os.sched_getaffinity(0))
        except AttributeError:  # pragma: no cover
            allowed = list(range(os.cpu_count() or 1))
    if idle_a is None:
        idle_a = _proc_stat_idle()
        time.sleep(0.1)
        idle_b = _proc_stat_idle()
    cores = {}
    for c in allowed:
        cores.setdefault(siblings(c), []).append(c)
    ranked = []
    for sib, cpus in cores.items():
        idle = sum(idle_b.get(s, 0) - idle_a.get(s, 0) for s in sib)
        ranked.append((idle, max(cpus), min(cpus)))
    ranked.sort(reverse=True)
    return [cpu for _, _, cpu in ranked[:k]]


CPU_REPS = 3  # runs per baseline cell, the median reported


def _median_rate(samples):
    s = sorted(samples)
    return s[len(s) // 2]


def cpu_stream(name, n, budget_s, native, threads):
    """rx.c's per-packet work on this host's cores over a sample of stream
    @name, timed on the oracle's restatement (TEST INFRASTRUCTURE, used here
    only as the baseline): rx_one_pkt with rx.c's direct header-struct loads
    (rx.c:127-167), bursts of 64 with prefetch stride 2 (rx.c:281-287),
    -O3 -march=native; 1 core classify-only, 1 core classify + lrpc_send into
    4096-deep rings (rx.c:76-92), and @threads cores on contiguous shards.
      nic_mode     hash.rss from the NIC (rx.c:83) -- what rx.c computes;
      jenkins_mode the 13-B lookup3 flow hash computed on the CPU, the same
                   work as the GPU lines."""
    from oracle import orc
    wl, _, stride, R, T, _ = WORKLOADS[name]
    cdf = orc.zipf_cdf(ZIPF_FLOWS) if wl == g.WL_TCP1500_ZIPF else None
    pkt_len = np.zeros(n, dtype=np.uint16)
    frames, olf, rss = orc.generate(wl, n, stride, R, seed=SEED, native=native, cdf=cdf,
                                    pkt_len=pkt_len)

    def tables(mode):
        t = orc.Tables(R, mode, 0, g.F_RSS_HASH | g.F_IP_CKSUM_GOOD, native=native)
        rng = np.random.default_rng(SEED)
        for r in range(R):
            act = int(rng.integers(1, T + 1))
            idx = [int(x) for x in rng.choice(T, size=act, replace=False)]
            t.runtime_set(r, orc.runtime_ip(r), T, act, orc.steer_flows(T, idx))
        return t

    spent = 0.0
    res = {"sample": f"first {n} pkts of the {name} stream ({stride}-B slots, {R} runtimes x {T})",
           "pkts": n}
    # pinned: one core (the idlest physical core) for the 1-core cells, that
    # core and the next idlest ones for the all-cores cell
    cpus = pick_cores(threads)
    res["cpus"] = cpus
    modes = (("nic_mode", g.HASH_NIC), ("jenkins_mode", g.HASH_JENKINS))
    kw = dict(olflags=olf, rss=rss, pkt_len=pkt_len, direct=True)
    cells = {}
    for mname, mode in modes:
        t = tables(mode)
        probe = t.bench(frames, n, stride, threads=1, passes=1, cpus=cpus[:1], **kw)
        spent += probe
        budget = budget_s * 0.5 / CPU_REPS
        cells[mname] = dict(t=t, p1=max(1, int(budget * 0.35 / max(probe, 1e-6))),
                            pl=max(1, int(budget * 0.3 / max(probe * 1.3, 1e-6))),
                            pm=max(1, int(budget * 0.35 / max(probe / len(cpus), 1e-6))),
                            r1=[], rl=[], rm=[])
    # The 1-core cells of both modes interleaved over CPU_REPS rounds (a
    # drift of the host hits them alike), then the all-cores cells: a 1-core
    # cell timed right after an all-cores one ran 3-22 % slow (classify-only
    # below classify + lrpc_send on the mixed stream, gpurun_out/r05j) even
    # with the untimed first pass every thread makes (orc.c bench_thread).
    time.sleep(0.5)
    # one throwaway 1-core cell first: the first cell after the pause ran up
    # to 6 % fast (tcp1500, profiles/r05_bench_detail.json)
    c0 = cells[modes[0][0]]
    spent += c0["t"].bench(frames, n, stride, threads=1, passes=c0["p1"], cpus=cpus[:1], **kw)
    for _ in range(CPU_REPS):
        for mname, _m in modes:
            c = cells[mname]
            s1 = c["t"].bench(frames, n, stride, threads=1, passes=c["p1"], cpus=cpus[:1], **kw)
            sl = c["t"].bench(frames, n, stride, threads=1, passes=c["pl"], lrpc=True, cpus=cpus[:1], **kw)
            spent += s1 * (c["p1"] + 1) / c["p1"] + sl * (c["pl"] + 1) / c["pl"]
            c["r1"].append(round(n * c["p1"] / s1 / 1e6, 2))
            c["rl"].append(round(n * c["pl"] / sl / 1e6, 2))
    for _ in range(CPU_REPS):
        for mname, _m in modes:
            c = cells[mname]
            sm = c["t"].bench(frames, n, stride, threads=len(cpus), passes=c["pm"], cpus=cpus, **kw)
            spent += sm * (c["pm"] + 1) / c["pm"]
            c["rm"].append(round(n * c["pm"] / sm / 1e6, 2))
    for mname, _m in modes:
        c = cells[mname]
        r1, rl, rm = c["r1"], c["rl"], c["rm"]
        res[mname] = {"1core_mpps": _median_rate(r1), "1core_lrpc_mpps": _median_rate(rl),
                      "all_cores_mpps": _median_rate(rm), "all_cores": len(cpus),
                      "samples": {"1core": r1, "1core_lrpc": rl, "all_cores": rm},
                      # (max - min) / median: the 1-core cells (`value`'s
                      # kind) apart from the all-cores one, which the host's
                      # other tenants share memory bandwidth with
                      "spread_1core": round(max((max(x) - min(x)) / _median_rate(x) for x in (r1, rl)), 4),
                      "spread_all_cores": round((max(rm) - min(rm)) / _median_rate(rm), 4),
                      "passes": [c["p1"], c["pl"], c["pm"]]}
    res["seconds"] = round(spent, 2)
    del frames
    return res


def cpu_baseline(budget_s=30.0):
    """The CPU baseline beside every timed stream: `value` is one core's
    classify-only rate on the udp64 stream in NIC mode (the reference's own
    per-packet work, one dataplane core, dpdk.c:276-280); `streams` holds the
    same measurement on the tcp1500 and mixed samples, which bench.py also
    attaches to the lines they stand beside."""
    from oracle import orc
    try:
        orc.build(native=True)
        native = True
    except Exception as e:  # pragma: no cover - gcc missing on the box
        log("native oracle build failed, using portable build:", e)
        native = False
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        avail = os.cpu_count() or 1
    threads = max(1, min(BOX_CPU_SHARE, avail))
    streams = {name: cpu_stream(name, n, budget_s * share, native, threads)
               for name, (n, share) in CPU_STREAMS.items()}
    u = streams["udp64"]
    cpu_model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {
        "value": u["nic_mode"]["1core_mpps"], "unit": "Mpkt/s", "cores": 1, "kind": "port",
        "sample": (f"first {u['pkts']} pkts of the udp64 stream, classify-only rx_one_pkt restatement "
                   f"with rx.c's direct header loads and the NIC's hash.rss (rx.c:83), bursts of 64, "
                   f"prefetch stride 2, -O3 -march={'native' if native else 'x86-64-v2'}; "
                   f"median of {CPU_REPS} pinned runs"),
        "pinning": (f"1-core cells on CPU {u['cpus'][0]} (idlest physical core of the affinity mask), "
                    f"all-cores cells on {len(u['cpus'])} distinct physical cores"),
        "nic_mode": u["nic_mode"], "jenkins_mode": u["jenkins_mode"],
        "streams": {k: v for k, v in streams.items() if k != "udp64"},
        "all_cores_note": (f"{threads} threads: the GPU box's CPU share for one GPU "
                           f"(min({BOX_CPU_SHARE}, {avail} CPUs in this process's affinity mask)); "
                           f"the host reports nproc={os.cpu_count()}"),
        "cpu_model": cpu_model, "nproc": os.cpu_count(),
        "seconds": round(sum(v["seconds"] for v in streams.values()), 2),
    }


STRONG_TOTAL_PKTS = 256 << 20


def pick_device(local, world, allow_shared):
    """One process per GPU: rank -> LOCAL_RANK's device.  More ranks than
    visible GPUs is refused (two ranks on one GPU would halve each one's
    bandwidth and read as bad scaling) unless --allow-shared-gpu, which only
    the single-GPU rehearsals (gloo) use."""
    ndev = torch.cuda.device_count()
    if ndev == 0:
        raise SystemExit("bench.py: no GPU visible")
    if local >= ndev:
        if not allow_shared:
            raise SystemExit(f"bench.py: LOCAL_RANK {local} but only {ndev} GPU(s) visible; "
                             f"refusing to put two ranks on one GPU (--allow-shared-gpu to rehearse)")
        return local % ndev
    return local


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def rank_envs(n, port, base=None):
    """The environment torchrun would give each of @n local ranks."""
    base = dict(os.environ if base is None else base)
    return [{**base, "RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_RANK": str(r),
             "LOCAL_WORLD_SIZE": str(n), "GROUP_RANK": "0", "MASTER_ADDR": "127.0.0.1",
             "MASTER_PORT": str(port)} for r in range(n)]


SPAWN_TIMEOUT_S = float(os.environ.get("GCL_BENCH_SPAWN_TIMEOUT", "1800"))


def spawn_ranks(n, argv, timeout_s=SPAWN_TIMEOUT_S):
    """`bench.py --gpus N` started without a launcher: one fresh rank process
    per GPU (this process has made no GPU call and only waits), rank 0's
    JSON line relayed to stdout.  A rank that fails ends the others; the exit
    code is the worst rank's, and no line is printed unless every rank
    succeeded -- never a 1-GPU line for --gpus N."""
    import subprocess
    port = free_port()
    procs = []
    for r, env in enumerate(rank_envs(n, port)):
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out0 = []
    import threading
    rd = threading.Thread(target=lambda: out0.append(procs[0].stdout.read()), daemon=True)
    rd.start()
    t0 = time.monotonic()
    rcs = [None] * n
    while any(rc is None for rc in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
        failed = any(rc not in (None, 0) for rc in rcs)
        if failed or time.monotonic() - t0 > timeout_s:
            time.sleep(5 if failed else 0)  # a failing rank's peers get a moment to report
            for i, p in enumerate(procs):
                if p.poll() is None:
                    p.kill()
                rcs[i] = p.wait()
            break
        time.sleep(0.05)
    rd.join(timeout=10)
    bad = [rc for rc in rcs if rc != 0]
    if bad:
        log(f"bench.py: --gpus {n} ranks exited {rcs}; no line printed")
        return max(abs(rc) for rc in bad) or 1
    lines = [ln for ln in (out0[0] if out0 else b"").decode().splitlines() if ln.startswith("{")]
    if not lines:
        log("bench.py: rank 0 printed no JSON line")
        return 1
    sys.stdout.write(lines[-1] + "\n")
    sys.stdout.flush()
    return 0


# --dump-outputs: at most this many float32 values of the verdict ring are
# written (32 MiB; the counts and counters beside it are a few hundred bytes)
DUMP_MAX_VALUES = 8 << 20


def sample_verdicts(raw, n, vbytes, max_values=DUMP_MAX_VALUES):
    """The [n, vbytes] verdict bytes in @raw (a uint8 array) as float32: all
    of them when they fit @max_values, else the verdicts of a fixed sample
    of packets (indices drawn with replacement from a generator seeded with
    SEED, so every run with the same arguments picks the same packets)."""
    v = np.asarray(raw, dtype=np.uint8)[:n * vbytes].reshape(n, vbytes)
    k = max(1, max_values // vbytes)
    if n > k:
        v = v[np.random.default_rng(SEED).integers(0, n, size=k)]
    return v.astype(np.float32)


def dump_outputs(path, w, rank, world, counts_before_last=None):
    """What the last timed step handed its caller, as @path/<name>.npy: the
    verdict ring (sample_verdicts; one file per rank) and, where the step
    counts into the workload's own vector (no exchange), that step's
    per-runtime packet counts and rx counters: the vector after the step
    less its copy taken on the stream just before it."""
    os.makedirs(path, exist_ok=True)
    nbytes = w.n * w.vbytes
    hv = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    hip_copy(hv, w.verdicts, nbytes)
    suffix = "" if world == 1 else f"_rank{rank}"
    np.save(os.path.join(path, f"verdicts{suffix}.npy"), sample_verdicts(hv.numpy(), w.n, w.vbytes))
    if counts_before_last is not None:
        last = (w.counts - counts_before_last).cpu().numpy().astype(np.float64)
        np.save(os.path.join(path, f"counts{suffix}.npy"), last[:w.R])
        np.save(os.path.join(path, f"stats{suffix}.npy"), last[w.R:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="udp64", choices=sorted(WORKLOADS))
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: 32 Mi packets per GPU; strong: --total-pkts split over the ranks")
    ap.add_argument("--total-pkts", type=int, default=STRONG_TOTAL_PKTS,
                    help="strong scaling: packets per step over all ranks (default 256 Mi)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the layout's ceiling (gcl_access_probe), the gcl_group rows, "
                         "the other verdict widths, hash modes and workloads, the host-memory and rx_burst "
                         "pipeline rows and the CPU baseline (each can be dropped with its --no-* option); "
                         "at N>1 also the kernel-only steps, e2e_multi, group_node and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed to DIR/<name>.npy: "
                         "verdicts (float32 [packets, verdict bytes], a fixed seeded sample of the packets "
                         "when the ring is larger than 32 MiB of float32) and, without an exchange, counts "
                         "and stats (float64: that step's per-runtime packet counts and rx counters)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary rows")
    ap.add_argument("--no-cpu", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-e2e", action="store_true", help="with --full: skip the host-memory rows")
    ap.add_argument("--no-group", action="store_true",
                    help="with --full: skip the gcl_group (C ABI + RCCL) lines at N=1")
    ap.add_argument("--group-node-force", action="store_true",
                    help="run the group_node line (gcl_group over the line's N GPUs) even at N=1")
    ap.add_argument("--group-child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cpu-budget", type=float, default=30.0)
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo only to rehearse N>1 on one GPU")
    ap.add_argument("--allow-shared-gpu", action="store_true",
                    help="rehearsal only: let several ranks share a GPU")
    ap.add_argument("--exchange-every", type=int, default=EXCHANGE_EVERY,
                    help="steps per counts all_gather (multi-GPU exchange period)")
    ap.add_argument("--verdict-bytes", type=int, default=VERDICT_BYTES, choices=[1, 2, 4, 8],
                    help="8: struct gcl_verdict (with the hash); 4: struct gcl_verdict4; "
                         "2: kthread-queue verdict (GCL_CFG_VERDICT2); 1: the same in one "
                         "byte (GCL_CFG_VERDICT1, <= 128 queues: config 2's 16 x 8)")
    ap.add_argument("--force-exchange", action="store_true",
                    help="run the multi-GPU step (RCCL all_gather on a side stream) even at N=1")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and not args.group_child:
        # no launcher: start the N ranks here, before anything touches a GPU
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))
    _claim_stdout()
    if args.cpu_child:  # cpu_child_line's child: no GPU call, one JSON line
        emit_json(cpu_baseline(args.cpu_budget))
        return
    if args.group_child:  # group_node_line's child: one JSON line, nothing else
        emit_json(group_node_bench(args.group_child, args.steps, args.warmup, args.exchange_every,
                                   shared=args.allow_shared_gpu and args.group_child > torch.cuda.device_count()))
        return

    rank, world, local = shard.dist_env()
    if world != args.gpus:
        log(f"note: --gpus {args.gpus} but WORLD_SIZE={world} (set by the launcher); using WORLD_SIZE")
    dev_index = pick_device(local, world, args.allow_shared_gpu)
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist_on = world > 1 or args.force_exchange
    if dist_on:
        shard.init(rank, world, backend=args.dist_backend, device=device)

    vb = args.verdict_bytes
    n_rank = None
    if args.scaling == "strong":
        if args.total_pkts % (world * SHARD_BLOCK):
            raise SystemExit(f"bench.py: --total-pkts {args.total_pkts} is not a multiple of "
                             f"{world} ranks x {SHARD_BLOCK}-packet shard blocks")
        n_rank = args.total_pkts // world
    w = Workload(args.workload, rank, world, device, vbytes=vb, n=n_rank)
    ex = Exchange(w, world, device, args.exchange_every) if dist_on else None
    before_last = counts_before_last = None
    if args.dump_outputs and ex is None:
        counts_before_last = torch.empty_like(w.counts)

        def before_last():
            counts_before_last.copy_(w.counts)
    el, gms = run_timed(w, args.steps, args.warmup, world, ex, before_last)
    settle_steps = run_timed.last_settle
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, w, rank, world, counts_before_last)
    total_pkts = w.n * world * args.steps
    value = total_pkts / el / 1e6
    # correctness spot check: every packet of every step was accounted for
    if ex is not None:
        tot = ex.acc[:w.R].sum().item()
        expect = w.n * world * (args.steps + args.warmup + settle_steps)
    else:
        tot = w.counts[:w.R].sum().item()
        expect = w.n * (args.steps + args.warmup + settle_steps)
    counts_ok = tot == expect
    # kernel-only next to the exchange-inclusive step: the same
    # steps without the all_gather, barrier + max-over-ranks timed (a run of
    # its own: --full)
    if ex is None:
        el_k, gms_k = el, gms
    elif args.full:
        el_k, gms_k = run_timed(w, args.steps, 2, world, None)
    else:
        el_k = gms_k = None
    w_n = w.n
    scaling_desc = (f"weak: {w.n} pkts per GPU" if args.scaling == "weak" else
                    f"strong: {args.total_pkts} pkts per step over {world} GPU(s), {w.n} per GPU")
    result = {
        "metric": METRIC,
        "value": round(value, 1),
        "unit": "Mpkt/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(el / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic",
        "config": {"workload": f"{args.workload}: {w.desc}", "pkts_per_gpu": w.n,
                   "slot_stride": w.stride, "runtimes": w.R, "kthreads": w.T,
                   "hash": "jenkins (lookup3 13-B 5-tuple)",
                   "verdict": VERDICT_NAMES[vb], "scaling": scaling_desc,
                   "parallelism": (f"dp{world}: round-robin 64Ki-pkt shards, {args.dist_backend} "
                                   f"all_gather of per-runtime counts every {args.exchange_every} step(s), overlapped"
                                   if dist_on else "single GPU")},
        "placement": placement(w),
        "counts_check": "ok" if counts_ok else f"MISMATCH {tot} != {expect}",
        "settle": {"steps": settle_steps, "ms_target": SETTLE_MS,
                   "what": ("untimed steps after the warmup, so the timed steps start after "
                            ">= ms_target of continuous launches (DESIGN.md §5)")},
    }
    if gms_k is not None:
        # the roofline of the timed steps' own launch time; the layout's
        # ceiling beside it takes launches of its own (--full)
        result["roofline"] = roofline(w, gms_k)
        if args.full:
            result["roofline"].update(ceiling(w.clf, w.frames, w.n, w.stride, w.verdicts, gms_k))
        result["kernel_only"] = {
            "value": round(w_n * world * args.steps / el_k / 1e6, 1), "unit": "Mpkt/s",
            "ms_per_step": round(el_k / args.steps * 1e3, 4), "gpu_ms_per_step": round(gms_k, 4),
            "what": ("the same classify steps without the counts all_gather, barrier + "
                     "max-over-ranks timed" if ex is not None else
                     "N=1 without an exchange: the step is the classify launch")}
    if ex is not None:
        result["exchange"] = {"gpu_ms_per_step": round(gms, 4), "period_steps": args.exchange_every,
                              "periods": ex.k, "backend": torch.distributed.get_backend(),
                              "ranks": torch.distributed.get_world_size()}
    if world == 1 and args.full and not args.no_group:
        try:
            result["group"] = group_bench(w, args.steps, args.warmup, dev_index, args.exchange_every,
                                          settle=settle_steps)
        except (OSError, ImportError) as e:  # reported, never silently dropped
            result["group"] = {"error": str(e)}
    del w, ex
    torch.cuda.empty_cache()
    if world == 1 and args.full and not args.no_group:
        node = group_node_line(args, 1)
        if node is not None:
            result["group_node"] = node
    torch.cuda.empty_cache()

    if world == 1 and args.full and not args.no_secondary and args.workload == "udp64" and args.scaling == "weak":
        # the same udp64 step with the other verdict formats
        other = []
        for ob in (b for b in (8, 4, 2, 1) if b != vb):
            w4 = Workload(args.workload, rank, world, device, vbytes=ob)
            el4, gms4 = run_timed(w4, args.steps, 3, 1)
            other.append({"verdict": VERDICT_NAMES[ob],
                          "value": round(w4.n * args.steps / el4 / 1e6, 1), "unit": "Mpkt/s",
                          "ms_per_step": round(el4 / args.steps * 1e3, 4), "roofline": roofline(w4, gms4),
                          "placement": placement(w4)})
            del w4
            torch.cuda.empty_cache()
        # the same udp64 step in the NIC-fidelity hash mode: bit-exact
        # do_toeplitz (runtime/net/core.c:120-139) with the 40-B RSS key,
        # 12 LDS LUT reads per packet instead of lookup3
        wt = Workload(args.workload, rank, world, device, hash_mode=g.HASH_TOEPLITZ, vbytes=vb)
        elt, gmst = run_timed(wt, args.steps, 3, 1)
        toeplitz = {"hash": "toeplitz (GCL_HASH_TOEPLITZ, Caladan's RSS key)",
                    "verdict": VERDICT_NAMES[vb],
                    "value": round(wt.n * args.steps / elt / 1e6, 1), "unit": "Mpkt/s",
                    "ms_per_step": round(elt / args.steps * 1e3, 4), "roofline": roofline(wt, gmst),
                    "placement": placement(wt)}
        del wt
        torch.cuda.empty_cache()
        steps2 = max(20, args.steps // 2)
        sec = {}
        # config 3 leads with the 2-byte queue verdict (1024 runtimes x 4
        # kthreads fit thread_bits 2): 174 vs 180 us for the 4-byte one on
        # the same buffers (profiles/archive/r02_defer_ab.jsonl)
        vbt = fit_vbytes(vb, *WORKLOADS["tcp1500"][3:5])
        for vb2 in (SECONDARY_VERDICT_BYTES,) + tuple(b for b in (vbt,) if b != SECONDARY_VERDICT_BYTES):
            w2 = Workload("tcp1500", rank, world, device, vbytes=vb2)
            el2, gms2 = run_timed(w2, steps2, 3, 1)
            rf2 = roofline(w2, gms2)
            rf2.update(ceiling(w2.clf, w2.frames, w2.n, w2.stride, w2.verdicts, gms2))
            sec[vb2] = {"verdict": VERDICT_NAMES[vb2],
                        "value": round(w2.n * steps2 / el2 / 1e6, 1), "unit": "Mpkt/s",
                        "ms_per_step": round(el2 / steps2 * 1e3, 4), "steps": steps2,
                        "roofline": rf2, "placement": placement(w2),
                        "frame_bytes_rate_GBs": round(w2.n * 1500 / (gms2 * 1e-3) / 1e9, 1)}
            del w2
            torch.cuda.empty_cache()
        w3 = Workload("tcp1500_hsplit", rank, world, device,
                      vbytes=fit_vbytes(vb, *WORKLOADS["tcp1500_hsplit"][3:5]))
        el3, gms3 = run_timed(w3, steps2, 2, 1)
        hsplit = {"workload": f"tcp1500_hsplit: {w3.desc}",
                  "value": round(w3.n * steps2 / el3 / 1e6, 1), "unit": "Mpkt/s",
                  "roofline": roofline(w3, gms3), "placement": placement(w3)}
        del w3
        torch.cuda.empty_cache()
        result["secondary"] = {"workload": f"tcp1500: {WORKLOADS['tcp1500'][5]}",
                               **sec[SECONDARY_VERDICT_BYTES],
                               "other_verdicts": [sec[b] for b in sec if b != SECONDARY_VERDICT_BYTES],
                               "header_split_layout": hsplit, "udp64_other_verdicts": other,
                               "udp64_toeplitz": toeplitz}

    if world == 1 and args.full and not args.no_e2e and args.workload == "udp64" and args.scaling == "weak":
        result["e2e"] = e2e_bench(device, vb)

    if world == 1 and args.full and not args.no_cpu:
        cpu = cpu_baseline(args.cpu_budget)
        cpu["gpu_over_1core_nic"] = round(value / cpu["value"], 1)
        result["cpu_baseline"] = cpu
        # each stream's CPU rate beside the line it stands next to
        if "secondary" in result:
            c3 = cpu["streams"]["tcp1500"]
            result["secondary"]["cpu_baseline"] = {
                **c3, "gpu_over_1core_jenkins": round(result["secondary"]["value"] /
                                                       c3["jenkins_mode"]["1core_mpps"], 1)}
        if "e2e" in result:
            result["e2e"]["mixed"]["cpu_baseline"] = cpu["streams"]["mixed"]
    if world > 1 and args.full and not args.no_e2e:
        result["e2e_multi"] = e2e_multi(device, rank, world, vb)
    if dist_on:
        shard.finish()  # every rank's GPU work done (barrier), the process group gone
    if world > 1 and args.full and rank == 0:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        result.update(node_extras(args, world, value))
    if rank == 0:
        emit_result(result)


if __name__ == "__main__":
    main()
