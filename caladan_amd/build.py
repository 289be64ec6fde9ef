"""Build the product shared libraries in-tree for gfx950.

hipcc compiles the HIP kernels + C ABI (csrc/gcl_*.hip: the context, the
batch kernels, the persistent rx loop, the transports and allocation, the
generator); gcc compiles the host-side C (csrc/gcl_host.c, csrc/gcl_pcap.c,
csrc/gcl_sock.c, csrc/gcl_neigh.c);
hipcc links them into caladan_amd/libgclassify.so.  The multi-GPU group (csrc/gcl_group.hip,
include/gcl_group.h) is its own library, caladan_amd/libgclgroup.so, linked
against libgclassify.so and RCCL, so that a single-GPU dataplane does not
load RCCL.  The .so files are git-ignored but travel to the GPU box with the
gpurun snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libgclassify.so")
OUT_GROUP = os.path.join(HERE, "libgclgroup.so")
OBJ = os.path.join(HERE, "_obj")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("GCL_OFFLOAD_ARCH", "gfx950")

SOURCES_HIP = ["gcl_ctx.hip", "gcl_batch.hip", "gcl_loop.hip", "gcl_xfer.hip", "gcl_gen.hip",
               "gcl_plan.hip", "gcl_pack.hip", "gcl_csum.hip", "gcl_copy.hip", "gcl_sock.hip", "gcl_l4.hip",
               "gcl_payload.hip", "gcl_txhdr.hip", "gcl_seg.hip", "gcl_tcprx.hip", "gcl_tcptmr.hip",
               "gcl_txq.hip", "gcl_tcpopen.hip", "gcl_udprx.hip", "gcl_tcpread.hip",
               "gcl_tcpwrite.hip", "gcl_tcpshut.hip"]
SOURCES_C = ["gcl_host.c", "gcl_pcap.c", "gcl_sock.c", "gcl_neigh.c"]
DEPS = ["gcl_device.h", "gcl_kern.h", "gcl_ctx.h", "gcl_sock.h", "gcl_pay.h", "gcl_neigh.h", "gcl_txh.h", "gcl_seg.h",
        "gcl_tcprx.h", "gcl_tcprxf.h", "gcl_tcprxo.h", "gcl_tcprxs.h", "gcl_tcptmr.h", "gcl_txq.h",
        "gcl_tcpopen.h", "gcl_udprx.h", "gcl_tcpread.h", "gcl_tcpwrite.h", "gcl_tcpshut.h", "../../include/gclassify.h",
        "../../include/gcl_host.h", "../../include/gcl_pcap.h"]
SOURCE_GROUP = "gcl_group.hip"
DEPS_GROUP = ["../../include/gclassify.h", "../../include/gcl_group.h"]


def _run(cmd):
    print("+", " ".join(cmd), flush=True)
    subprocess.check_call(cmd)


def _stale(target, inputs):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(i) > t for i in inputs)


def build(force=False, verbose_resources=False):
    os.makedirs(OBJ, exist_ok=True)
    deps = [os.path.join(CSRC, d) for d in DEPS] + [os.path.abspath(__file__)]
    objs, cmds = [], []
    for src in SOURCES_HIP:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src + ".o")
        if force or _stale(o, [s] + deps):
            cmd = [HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC",
                   "-Wall", "-Wno-unused-function", "-c", s, "-o", o]
            if verbose_resources:
                cmd.insert(1, "-Rpass-analysis=kernel-resource-usage")
            cmds.append(cmd)
        objs.append(o)
    # the translation units are independent: compile them side by side
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=min(len(cmds), 4) or 1) as ex:
        list(ex.map(_run, cmds))
    for src in SOURCES_C:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src + ".o")
        if force or _stale(o, [s] + deps):
            _run(["gcc", "-std=gnu11", "-O3", "-fPIC", "-Wall", "-Wextra",
                  "-Wno-unused-parameter", "-c", s, "-o", o])
        objs.append(o)
    if force or _stale(OUT, objs):
        # only the C ABI (gcl_*) is exported; the translation units' shared
        # helpers (namespace gclk) stay internal to the library
        vs = os.path.join(OBJ, "exports.map")
        with open(vs, "w") as f:
            f.write("{ global: gcl_*; local: *; };\n")
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", OUT] + objs +
             ["-lm", "-Wl,--version-script=" + vs])
    build_group(force)
    return OUT


def build_group(force=False):
    """libgclgroup.so: the multi-GPU group over libgclassify.so + RCCL."""
    s = os.path.join(CSRC, SOURCE_GROUP)
    o = os.path.join(OBJ, SOURCE_GROUP + ".o")
    deps = [s, os.path.abspath(__file__)] + [os.path.join(CSRC, d) for d in DEPS_GROUP]
    if force or _stale(o, deps):
        _run([HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall",
              "-c", s, "-o", o])
    if force or _stale(OUT_GROUP, [o, OUT]):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", OUT_GROUP, o,
              "-L" + HERE, "-lgclassify", "-L/opt/rocm/lib", "-lrccl",
              "-Wl,-rpath,$ORIGIN", "-Wl,--no-undefined"])
    return OUT_GROUP


SANITIZE_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                  "-fno-omit-frame-pointer", "-static-libasan", "-g", "-O1"]


def build_sanitized(out_dir=None):
    """Host-only CPU build of the C that parses untrusted input -- the pcap
    loader (csrc/gcl_pcap.c), the verdict post-pass (csrc/gcl_host.c) and the
    oracle's classifier (oracle/orc.c, test infrastructure) -- under ASan +
    UBSan, linked into the fuzz driver tests/fuzz/host_fuzz.c.  No HIP code is
    compiled: GPU code is never built with sanitizers here.  Returns the
    driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "host_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "host_fuzz.c"), os.path.join(CSRC, "gcl_host.c"),
            os.path.join(CSRC, "gcl_pcap.c"), os.path.join(ROOT, "oracle", "orc.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm", "-lpthread"])
    return exe


def build_sanitized_plan(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/plan_fuzz.c: a stand-alone driver of gcl_host_deliver_idx (the
    post-pass over a delivery plan's index lists).  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "plan_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "plan_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_pack(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/pack_fuzz.c: a stand-alone driver of gcl_host_deliver_packed
    (the post-pass over a list's packed records).  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pack_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "pack_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_csum(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/csum_fuzz.c: a stand-alone driver of gcl_rx_csum_flags (the
    checksum rule for one frame) over exactly sized heap frames.  Returns the
    driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "csum_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "csum_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_copy(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/copy_fuzz.c: a stand-alone driver of gcl_copy_batch_host (the
    loopback frame copy on the CPU) over exactly sized heap regions.  Returns
    the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "copy_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "copy_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_sock(out_dir=None):
    """The ASan + UBSan host build of csrc/gcl_sock.c (the socket table, its
    placement and the lookup of a batch on the CPU, with the probe of
    csrc/gcl_sock.h that the GPU kernel shares) and of csrc/gcl_host.c (the
    verdict widening the driver checks against), linked into
    tests/fuzz/sock_fuzz.c: a stand-alone driver over random entry sets,
    exactly sized heap frames and random verdict bytes.  Returns the driver's
    path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "sock_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "sock_fuzz.c"), os.path.join(CSRC, "gcl_sock.c"),
            os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_l4(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/l4_fuzz.c: a stand-alone driver of gcl_l4_csum_host (the TCP/UDP
    checksum verify and fill on the CPU) over exactly sized heap regions with
    hostile offsets and lengths.  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "l4_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "l4_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_pay(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/pay_fuzz.c: a stand-alone driver of gcl_l4_payload_host (the
    payload descriptors and the packed layout on the CPU, with the rule of
    csrc/gcl_pay.h that the GPU kernel shares) over exactly sized heap arrays
    with hostile offsets, lengths, orders and segment starts.  Returns the
    driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pay_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "pay_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_txh(out_dir=None):
    """The ASan + UBSan host build of csrc/gcl_host.c (gcl_tx_hdr_host, with
    the rule of csrc/gcl_txh.h that the GPU kernel shares) and of
    csrc/gcl_neigh.c (the neighbour table, its placement and the probe of
    csrc/gcl_neigh.h), linked into tests/fuzz/txh_fuzz.c: a stand-alone driver
    over exactly sized heap regions with hostile descriptors, offsets, caps
    and table images.  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "txh_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "txh_fuzz.c"), os.path.join(CSRC, "gcl_host.c"),
            os.path.join(CSRC, "gcl_neigh.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_seg(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/seg_fuzz.c: a stand-alone driver of gcl_tx_seg_host (the
    segmenter of a batch of socket writes on the CPU, with the rule of
    csrc/gcl_seg.h that the GPU kernels share) over exactly sized heap arrays
    with hostile writes, caps and layouts.  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "seg_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "seg_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcprx(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcprx_fuzz.c: a stand-alone driver of gcl_tcp_rx_host (the
    established fast path of tcp_rx_conn for a list on the CPU, with the rule
    of csrc/gcl_tcprx.h that the GPU kernels share) over exactly sized heap
    arrays with hostile frames, cookies, connection words and orders.  Returns
    the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcprx_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcprx_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcptmr(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcptmr_fuzz.c: a stand-alone driver of gcl_tcp_tick_host and
    gcl_tcp_rx_acks_host (the timer sweep and the control segments on the CPU,
    with the rules of csrc/gcl_tcptmr.h that the GPU kernels share) over
    exactly sized heap arrays with hostile timer words, connection words,
    cookies, orders, verdicts and caps.  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcptmr_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcptmr_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_txq(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/txq_fuzz.c: a stand-alone driver of gcl_tcp_txq_host (the
    retransmit queues of a batch of connections on the CPU, with the rule of
    csrc/gcl_txq.h that the GPU kernels share) over exactly sized heap arrays
    with garbage queue offsets, entries, connection words, wants and caps.
    Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "txq_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "txq_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcprxf(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcprxf_fuzz.c: a stand-alone driver of gcl_tcp_rx_full_host
    (tcp_rx_conn with the established part of its slow path for a list on the
    CPU, with the rule of csrc/gcl_tcprxf.h that the GPU walk shares) over
    exactly sized heap arrays with garbage frames, cookies, connection words,
    rep_acks, orders and blocks.  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcprxf_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcprxf_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcprxo(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcprxo_fuzz.c: a stand-alone driver of gcl_tcp_rx_ooo_host
    (tcp_rx_conn with its established slow path and the out-of-order queue for
    a list on the CPU, with the rule of csrc/gcl_tcprxo.h that the GPU walk
    shares) over exactly sized heap arrays with hostile q_off, queue entries
    and orders.  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcprxo_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcprxo_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcprxs(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcprxs_fuzz.c: a stand-alone driver of gcl_tcp_rx_states_host and
    gcl_tcp_rx_ctl_host (tcp_rx_conn in every state, and its control segments,
    with the rules of csrc/gcl_tcprxs.h and csrc/gcl_tcptmr.h that the GPU
    shares) over exactly sized heap arrays with random states, flags, queue
    ranges and seg_cap.  Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcprxs_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcprxs_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcpopen(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcpopen_fuzz.c: a stand-alone driver of gcl_tcp_rx_open_host
    (the passive open of a list on the CPU, with the rule and the option walk
    of csrc/gcl_tcpopen.h that the GPU kernels share) over exactly sized heap
    arrays with random frames, options, cookies, backlogs and caps.  Returns
    the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcpopen_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcpopen_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_udprx(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/udprx_fuzz.c: a stand-alone driver of gcl_udp_rx_host
    (udp_conn_recv and udp_par_recv for a list on the CPU, with the rule of
    csrc/gcl_udprx.h that the GPU kernels share) over exactly sized heap
    arrays with random frames, cookies, socket words and caps.  Returns the
    driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "udprx_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "udprx_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcpread(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcpread_fuzz.c: a stand-alone driver of gcl_tcp_read_host
    (tcp_read and tcp_readv for a batch of connections on the CPU, with the
    rule of csrc/gcl_tcpread.h that the GPU kernels share) over exactly sized
    heap arrays with garbage queue and vector offsets, entries, reads and caps.
    Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcpread_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcpread_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcpwrite(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcpwrite_fuzz.c: a stand-alone driver of gcl_tcp_write_host
    (tcp_write and tcp_writev for a batch of connections on the CPU, with the
    rule of csrc/gcl_tcpwrite.h that the GPU kernels share) over exactly sized
    heap arrays with garbage vector offsets, vectors, writes and caps.
    Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcpwrite_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcpwrite_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


def build_sanitized_tcpshut(out_dir=None):
    """The same ASan + UBSan host build of csrc/gcl_host.c, linked into
    tests/fuzz/tcpshut_fuzz.c: a stand-alone driver of gcl_tcp_shut_host
    (tcp_shutdown, tcp_close and tcp_abort for a batch of connections on the
    CPU, with the rule of csrc/gcl_tcpshut.h that the GPU kernels share) over
    exactly sized heap arrays with garbage states, ops, how and caps.
    Returns the driver's path."""
    out_dir = out_dir or os.path.join(ROOT, "build", "sanitize")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "tcpshut_fuzz")
    srcs = [os.path.join(ROOT, "tests", "fuzz", "tcpshut_fuzz.c"), os.path.join(CSRC, "gcl_host.c")]
    if _stale(exe, srcs + [os.path.join(CSRC, d) for d in DEPS]):
        _run(["gcc", "-std=gnu11", "-Wall", "-Wno-unused-parameter", *SANITIZE_FLAGS,
              "-o", exe, *srcs, "-lm"])
    return exe


if __name__ == "__main__":
    if "--sanitize" in sys.argv:
        print(build_sanitized())
        print(build_sanitized_plan())
        print(build_sanitized_pack())
        print(build_sanitized_csum())
        print(build_sanitized_copy())
        print(build_sanitized_sock())
        print(build_sanitized_l4())
        print(build_sanitized_pay())
        print(build_sanitized_txh())
        print(build_sanitized_seg())
        print(build_sanitized_tcprx())
        print(build_sanitized_tcptmr())
        print(build_sanitized_txq())
        print(build_sanitized_tcprxf())
        print(build_sanitized_tcprxo())
        print(build_sanitized_tcprxs())
        print(build_sanitized_tcpopen())
        print(build_sanitized_udprx())
        print(build_sanitized_tcpread())
        print(build_sanitized_tcpwrite())
        print(build_sanitized_tcpshut())
    else:
        build(force="--force" in sys.argv, verbose_resources="--resources" in sys.argv)
