/*
 * gclassify.h - C ABI of the MI355X (gfx950) rx packet classifier.
 *
 * This library replaces the per-packet work that Caladan's IOKernel does in
 * rx_burst()/rx_one_pkt() (iokernel/rx.c:116-233, :270-290): parse the
 * Ethernet/IPv4/ARP header, look the destination IP up in the IP->runtime
 * table (dp.ip_to_proc, an rte_hash keyed by rte_jhash, iokernel/dp_clients.c:
 * 349-363), and steer the packet to a runtime kthread through that runtime's
 * flow table (rx_send_to_runtime, iokernel/rx.c:50-73).  The GPU emits one
 * 8-byte verdict per packet; the host (one dataplane thread, as in the
 * reference) turns verdicts into lrpc_send() calls (see gcl_host.h); gcl_plan
 * (below) partitions a classified batch by runtime on the GPU, so that
 * several host cores can each deliver their own runtimes' packets.
 *
 * Conventions follow the reference: every function returns 0 or -errno
 * (rx_init iokernel/rx.c:398-415, lrpc_init_out base/lrpc.c:38-52), nothing is
 * thread-safe, and one context serves one GPU the way one dataplane core
 * serves one NIC queue (iokernel/dpdk.c:276-280).  There are no per-packet
 * error returns: outcomes are verdict actions plus counters, exactly like the
 * reference's STAT_INC counters (iokernel/defs.h:417-460).
 *
 * All pointers passed to gcl_classify() are DEVICE pointers (HBM); table
 * setters take host pointers.  Table updates are applied on the stream of the
 * next gcl_classify() call, before its kernel, giving the snapshot semantics
 * of the reference's single-threaded dataplane (tables only change between
 * bursts, iokernel/main.c:144-176).
 */
#ifndef GCLASSIFY_H
#define GCLASSIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Limits of the reference data model. */
#define GCL_MAX_PROC      4096  /* IOKERNEL_MAX_PROC, iokernel/defs.h:69 */
#define GCL_NCPU          256   /* NCPU, inc/base/limits.h:7: max threads per proc */
#define GCL_RX_BURST_SIZE 64    /* IOKERNEL_RX_BURST_SIZE, iokernel/defs.h:75 */

/* Header constants parsed on the path (inc/net/ethernet.h, inc/net/arp.h). */
#define GCL_ETHTYPE_IP    0x0800
#define GCL_ETHTYPE_ARP   0x0806
#define GCL_ETHTYPE_IPV6  0x86DD
#define GCL_ARP_OP_REQUEST 1
#define GCL_ARP_OP_REPLY   2
#define GCL_HDR_GRANULE   64    /* bytes of each frame the kernel stages */

/*
 * Per-packet offload flags: one byte that carries the rte_mbuf ol_flags bits
 * rx.c reads (RTE_MBUF_F_RX_RSS_HASH at rx.c:132/:160, RTE_MBUF_F_RX_FDIR_ID at
 * rx.c:131, RTE_MBUF_F_RX_IP_CKSUM_MASK at rx.c:31-35).
 */
#define GCL_F_RSS_HASH           0x01
#define GCL_F_FDIR_ID            0x02
#define GCL_F_IP_CKSUM_MASK      0x0C
#define GCL_F_IP_CKSUM_UNKNOWN   0x00
#define GCL_F_IP_CKSUM_BAD       0x04
#define GCL_F_IP_CKSUM_GOOD      0x08
#define GCL_F_IP_CKSUM_NONE      0x0C

/*
 * Steering-hash source.  The reference steers with buf->hash.rss (rx.c:83),
 * i.e. the NIC's Toeplitz RSS over IPv4 TCP/UDP (iokernel/dpdk.c:67-82).
 *  NIC      - use the per-packet rss[] array, exactly like rx.c.
 *  JENKINS  - compute lookup3 (base/jenkins_hash.c:126-297) over the 13-byte
 *             key {saddr, daddr, dport, sport, proto} (host-order fields).
 *  TOEPLITZ - compute the NIC's Toeplitz hash in software, bit-exact with
 *             do_toeplitz (runtime/net/core.c:120-139) for the configured key.
 * In the two computed modes the hash is 0 unless the frame is IPv4 with
 * IHL >= 5, not a fragment (MF clear, offset 0) and protocol TCP or UDP
 * (the NIC's RTE_ETH_RSS_NONFRAG_IPV4_TCP|UDP, dpdk.c:79).
 */
enum gcl_hash_mode {
	GCL_HASH_NIC = 0,
	GCL_HASH_JENKINS = 1,
	GCL_HASH_TOEPLITZ = 2,
};

/* gcl_cfg.flags */
#define GCL_CFG_AZURE_ARP  0x1  /* cfg.azure_arp_mode: rx.c:171-190, :200-203 */
#define GCL_CFG_HASH16     0x2  /* truncate the steering hash to 16 bits, as the
                                   loopback hint does (runtime/net/core.c:524,
                                   iokernel/tx.c:81-83, inc/iokernel/queue.h:120-134) */
#define GCL_CFG_PROFILE    0x4  /* record HIP events around every classify kernel */
#define GCL_CFG_TRANS_HASH 0x8  /* also compute the destination runtime's transport
                                   demux hashes (gcl_classify_ex, struct gcl_trans) */
#define GCL_CFG_VERDICT4   0x10 /* write 4-byte struct gcl_verdict4 instead of
                                   struct gcl_verdict (see there) */
#define GCL_CFG_VERDICT2   0x20 /* write 2-byte queue verdicts (gcl_verdict2 below);
                                   needs cfg.thread_bits, excludes VERDICT4 and
                                   TRANS_HASH */
#define GCL_CFG_VERDICT1   0x40 /* write 1-byte queue verdicts (gcl_verdict1 below):
                                   needs cfg.thread_bits with max_runtimes <<
                                   thread_bits <= GCL_V1_QUEUES, excludes VERDICT2,
                                   VERDICT4 and TRANS_HASH */

struct gcl_cfg {
	uint32_t max_runtimes;    /* uniqids must be < max_runtimes (<= GCL_MAX_PROC) */
	uint32_t hash_mode;       /* enum gcl_hash_mode */
	uint32_t flags;           /* GCL_CFG_* */
	uint8_t  default_olflags; /* flags of every packet when gcl_batch.olflags == NULL */
	uint8_t  rss_key[40];     /* Toeplitz key (NIC key, dpdk.c:219-228) */
	uint8_t  thread_bits;     /* GCL_CFG_VERDICT2 / VERDICT1: kthread queues per runtime
	                             are 1 << thread_bits (thread_count may not exceed it),
	                             and max_runtimes << thread_bits <= GCL_V2_QUEUES
	                             (GCL_V1_QUEUES) */
	uint8_t  pad[2];
};

/* One batch of received frames, resident in device memory. */
struct gcl_batch {
	const uint8_t  *frames;     /* frame bytes (mbuf data) */
	uint64_t        frames_len; /* readable bytes at frames (< 2^64 - 1, else -EINVAL);
	                               reads past it see 0, at any offset */
	uint64_t        stride;     /* slot stride when offs == NULL (multiple of 16) */
	const uint64_t *offs;       /* optional u64[n] frame start offsets, any alignment:
	                               a 4-B-aligned frame (16-B aligned, or the
	                               reference's mbuf data at element + 344,
	                               iokernel/defs.h:503-506) is staged as the
	                               16-B-aligned 64-B window starting up to 12 B
	                               before it (four 16-B loads), cut at the first
	                               128-B line end when that line holds frame
	                               bytes 0-39; any other alignment is read byte
	                               by byte */
	const uint8_t  *olflags;    /* optional u8[n]  GCL_F_* per packet */
	const uint32_t *rss;        /* optional u32[n] buf->hash.rss (NIC mode) */
	const uint32_t *fdir_hi;    /* optional u32[n] buf->hash.fdir.hi (FDIR mark) */
	const uint16_t *pkt_len;    /* optional u16[n] rte_pktmbuf_pkt_len; NOT read by
	                               the kernel, only by the host post-pass that
	                               builds rxq_cmd (rx_make_cmd, rx.c:24-38) */
	uint64_t        n;          /* packets in the batch */
	const uint32_t *dst_hint;   /* optional u32[n] loopback hint: tx_pktmbuf_priv.dst_ip
	                               (host order, 0 = none).  A hint found in ip_to_proc
	                               marks the packet FDIR with hash.fdir.hi = uniqid
	                               before classification, as rx_loopback does
	                               (iokernel/rx.c:249-262); it overrides fdir_hi[] */
};

/*
 * Verdict actions.  Each is one exit of rx_one_pkt (rx.c:116-233).
 * GCL_ACT_F_FDIR is or-ed in when the runtime was found by the FDIR mark.
 */
enum gcl_action {
	GCL_ACT_DELIVER = 0,       /* rx_send_pkt_to_runtime(p) -> threads[thread] */
	GCL_ACT_WAKE = 1,          /* runtime has no active thread: the host must
	                              replay rx_send_to_runtime (sched_add_core,
	                              rx.c:62-72) in packet order */
	GCL_ACT_DROP_ETHERTYPE = 2,/* rx.c:191-194 -> fail_free, RX_UNHANDLED */
	GCL_ACT_DROP_UNREG = 3,    /* rx.c:198-207: RX_UNREGISTERED_MAC, RX_UNHANDLED */
	GCL_ACT_BROADCAST = 4,     /* azure ARP reply, rx.c:171-190 (host fans out) */
	GCL_ACT_ARP_RESPOND = 5,   /* azure ARP request miss, rx.c:200-203 (host) */
};
#define GCL_ACT_MASK    0x3F
#define GCL_ACT_F_FDIR  0x80
#define GCL_ACT_F_TRANS 0x40  /* struct gcl_trans of this packet is valid */
#define GCL_NO_RUNTIME  0xFFFF
#define GCL_NO_THREAD   0xFF

/*
 * DELIVER and WAKE verdicts name the runtime and its flow-table SLOT,
 * hash % thread_count (rx.c:57, :68), not the kthread: the host post-pass
 * (gcl_host.h) reads p->flow_tbl[slot] and p->active_thread_count when it
 * delivers the packet, as rx_send_to_runtime does (rx.c:55-72), so a
 * scheduler change earlier in the same batch is seen by the later packets.
 * DELIVER means the runtime had an active kthread in the classify snapshot,
 * WAKE that it had none; the post-pass re-checks either way.
 *
 * BREAKING in ABI 4 (round 4): before it, .thread held the kthread
 * (flow_tbl[slot]) in the same layout.  A direct consumer of the verdicts
 * that indexes kthread rings with .thread must check gcl_abi_version() >= 4
 * and read flow_tbl[.thread] itself (or use the gcl_host_deliver* post-pass).
 */
#define GCL_ABI_VERSION 6
/* GCL_ABI_VERSION of the library actually loaded: 4 = verdict .thread is
 * the flow-table slot; 5 = gcl_group_open_v2 and struct gcl_group_cfg.size;
 * 6 = struct gcl_tune / gcl_ctx_tune (the library reads no environment) */
int gcl_abi_version(void);
struct gcl_verdict {
	uint32_t hash;    /* steering hash (hash.rss, or the computed flow hash) */
	uint16_t uniqid;  /* proc->uniqid of the destination, GCL_NO_RUNTIME if none */
	uint8_t  thread;  /* the flow_tbl slot hash % thread_count, GCL_NO_THREAD if none */
	uint8_t  action;  /* enum gcl_action | GCL_ACT_F_FDIR */
};

/*
 * Compact verdict (GCL_CFG_VERDICT4): the last four bytes of gcl_verdict,
 * without the hash.  rx_send_to_runtime uses the hash only as
 * hash % thread_count (rx.c:57, :68), and thread_count is fixed per runtime,
 * so the slot in @thread is all the post-pass needs.  The only other use of
 * the hash is the Azure ARP broadcast fan-out, where it is the mbuf's
 * hash.rss in GCL_HASH_NIC mode and 0 in the computed modes (ARP is not
 * hashed): gcl_host_deliver4 takes it from the caller.
 */
struct gcl_verdict4 {
	uint16_t uniqid;  /* as gcl_verdict */
	uint8_t  thread;  /* DELIVER, WAKE: the flow_tbl slot hash % thread_count;
	                     otherwise GCL_NO_THREAD */
	uint8_t  action;  /* as gcl_verdict */
};

/*
 * 2-byte verdict (GCL_CFG_VERDICT2): a u16 per packet naming a runtime's
 * flow-table slot q = uniqid << thread_bits | slot, one flat index over
 * every runtime's flow_tbl (defs.h:244), slot = hash % thread_count.
 *   DELIVER (any flags)  q
 *   WAKE                 GCL_V2_WAKE | q
 *   every other action   GCL_V2_OTHER | action (DROP_*, BROADCAST, ARP_RESPOND)
 * It drops what gcl_verdict4 keeps beyond that: GCL_ACT_F_FDIR, which the
 * host never reads (RX_FLOW_TAG_MATCH is counted on the device).  Half the
 * verdict stores of the 4-byte form; gcl_verdict2_to4 (gcl_host.h) widens one.
 */
#define GCL_V2_QUEUES   0x4000
#define GCL_V2_Q_MASK   0x3FFF
#define GCL_V2_KIND     0xC000
#define GCL_V2_DELIVER  0x0000
#define GCL_V2_WAKE     0x4000
#define GCL_V2_OTHER    0xC000

/*
 * 1-byte verdict (GCL_CFG_VERDICT1), for contexts whose queues fit 7 bits
 * (max_runtimes << thread_bits <= 128: config 2's 16 runtimes x 8 kthreads):
 *   DELIVER or WAKE      q = uniqid << thread_bits | slot
 *   every other action   GCL_V1_OTHER | action (DROP_*, BROADCAST, ARP_RESPOND)
 * A WAKE is not marked: the post-pass reads the runtime's live
 * active_thread_count at delivery anyway and takes rx.c's wake path when it
 * is 0 (rx.c:55-72), so the mark carried nothing the host uses.  Half the
 * verdict bytes of the 2-byte form; gcl_verdict1_to4 (gcl_host.h) widens one.
 */
#define GCL_V1_QUEUES   0x80
#define GCL_V1_Q_MASK   0x7F
#define GCL_V1_OTHER    0x80

/*
 * Counter slots; indices 0..5 keep the order of the reference enum
 * (iokernel/defs.h:421-426).  The device adds RX_PULLED, RX_FLOW_TAG_MATCH,
 * RX_HASH_MISSING, RX_UNREGISTERED_MAC and RX_UNHANDLED (for its drops); the
 * host adds RX_UNICAST_FAIL / RX_BROADCAST_FAIL (ring full) and the UNHANDLED
 * that goes with them.
 */
enum {
	GCL_RX_UNREGISTERED_MAC = 0,
	GCL_RX_UNICAST_FAIL,
	GCL_RX_BROADCAST_FAIL,
	GCL_RX_FLOW_TAG_MATCH,
	GCL_RX_UNHANDLED,
	GCL_RX_HASH_MISSING,
	GCL_RX_PULLED,
	GCL_NR_STATS = 8, /* padded */
};

struct gcl_ctx;

/*
 * gcl_open - create a classifier context on HIP device @hip_device.
 * Replaces the ip_to_proc creation in dp_clients_init (dp_clients.c:349-363)
 * and the flow tables held in struct proc (defs.h:244).
 * Returns 0, -EINVAL (bad cfg), -ENODEV (no such device) or -ENOMEM.
 */
int gcl_open(int hip_device, const struct gcl_cfg *cfg, struct gcl_ctx **out);
void gcl_close(struct gcl_ctx *ctx);

/*
 * gcl_runtime_set - add or update a runtime (proc).
 * Mirrors dp_clients_add_client (dp_clients.c:156-185: clients_by_id[uniqid],
 * rte_hash_add_key_data(ip)) plus the flow table that sched_steer_flows writes
 * (sched.c:122-147).  @flow_tbl holds @thread_count entries (ignored when
 * @active_count == 0).  Returns -EEXIST if another runtime owns @ip_host
 * (dp_clients.c:174-179), -EINVAL on out-of-range arguments.
 */
int gcl_runtime_set(struct gcl_ctx *ctx, uint16_t uniqid, uint32_t ip_host,
                    uint16_t thread_count, uint16_t active_count,
                    const uint16_t *flow_tbl);

/* gcl_runtime_del - remove a runtime (dp_clients_remove_client,
 * dp_clients.c:230-250).  Returns -ENOENT if @uniqid is not present. */
int gcl_runtime_del(struct gcl_ctx *ctx, uint16_t uniqid);

/*
 * gcl_steer_flows - the flow_tbl rule of sched_steer_flows (sched.c:122-147):
 * identity for the active threads, the rest round-robin over them.  Host-only
 * helper; leaves @flow_tbl untouched when @active_count == 0, like the
 * reference.  @active_idx lists the active thread indices in activation order.
 */
int gcl_steer_flows(uint16_t thread_count, const uint16_t *active_idx,
                    uint16_t active_count, uint16_t *flow_tbl);

/*
 * gcl_classify - classify @b->n packets on @hip_stream (NULL = null stream).
 * @verdicts       device gcl_verdict[n] (gcl_verdict4[n] with GCL_CFG_VERDICT4,
 *                 u16[n] with GCL_CFG_VERDICT2)
 * @runtime_counts device u64[max_runtimes], ACCUMULATED: packets steered to
 *                 each runtime (DELIVER + WAKE), may be NULL
 * @stats          device u64[GCL_NR_STATS], ACCUMULATED, may be NULL
 * Asynchronous; returns -EINVAL for malformed batches (including n > 2^40),
 * -EIO when the table
 * upload fails, -ENOSPC when the IP table cannot place every key (cuckoo
 * placement failed for all 256 seeds: not seen at the table's load <= 1/2).
 * Replaces the rx_one_pkt loop of rx_burst (rx.c:281-287).
 */
int gcl_classify(struct gcl_ctx *ctx, const struct gcl_batch *b,
                 void *verdicts, uint64_t *runtime_counts,
                 uint64_t *stats, void *hip_stream);

/*
 * End-to-end classification of a batch whose frames are in HOST memory (the
 * NIC's mbufs in the iokernel's ingress region), verdicts returned to host
 * memory; synchronous.  Two transports:
 *  GCL_E2E_COPY     the 64-B header granule of every fixed-stride slot is
 *                   DMA-gathered into HBM (hipMemcpy2DAsync), classified, and
 *                   the verdicts copied back; chunks pipelined over nstreams.
 *  GCL_E2E_ZEROCOPY the kernel reads the headers directly from pinned or
 *                   registered host memory over PCIe (gcl_host_register) and
 *                   writes the verdicts directly into host memory.
 * @host_counts / @host_stats are accumulated (may be NULL).
 * Returns -EFAULT when a ZEROCOPY buffer is not pinned/registered.
 */
enum gcl_e2e_mode {
	GCL_E2E_COPY = 0,
	GCL_E2E_ZEROCOPY = 1,
};

struct gcl_e2e_opts {
	uint32_t mode;      /* enum gcl_e2e_mode */
	uint32_t nstreams;  /* COPY: chunks in flight (1..4, 0 = 2) */
	uint64_t chunk;     /* COPY: packets per chunk (0 = 1 Mi) */
};

int gcl_classify_host(struct gcl_ctx *ctx, const struct gcl_batch *host_batch,
                      void *host_verdicts, uint64_t *host_counts,
                      uint64_t *host_stats, const struct gcl_e2e_opts *opts);

/*
 * gcl_header_gather - the COPY transport's gather step over per-packet
 * offsets, as gcl_classify_host uses it (and gcl_group_classify_host, per
 * GPU): on the current HIP device's @hip_stream, row i of @rows (device
 * memory, @n x GCL_GATHER_ROW bytes) gets frame bytes [0, GCL_GATHER_ROW)
 * of the frame at @frames + offs[i], bytes at or past @frames_len reading 0
 * (offsets clamped as gcl_batch's).  @frames and @offs are device-visible
 * pointers (a registered region's mapped address, or HBM).  The rows hold
 * everything rx_one_pkt reads (ports end at byte 78 for IHL 15), so a
 * classify over @rows with stride GCL_GATHER_ROW equals one over the
 * frames.  Asynchronous; 0, -EINVAL or -EIO.
 */
#define GCL_GATHER_ROW 80
int gcl_header_gather(const uint8_t *frames, uint64_t frames_len, const uint64_t *offs, uint64_t n,
                      uint8_t *rows, void *hip_stream);

/* Pin + map host memory for ZEROCOPY / async copies (hipHostRegister). */
int gcl_host_register(void *p, size_t len);
int gcl_host_unregister(void *p);

/*
 * Transport demux pre-hash (runtime/net/transport.c:29-42, :355-398).  For a
 * packet delivered to runtime p that the runtime will hand to trans_lookup
 * -- IPv4, version 4, IHL 5, the MF test of ip_hdr_supported as written
 * (runtime/net/core.c:203-209: IP_MF applied to the network-order field),
 * TCP or UDP -- the GPU computes, with p's trans_seed:
 *   h5 = hash_crc32c_two(seed, laddr.ip | laddr.port << 32,
 *                        raddr.ip | raddr.port << 32 | proto << 48)
 *   h3 = hash_crc32c_one(seed, laddr.ip | laddr.port << 32 | proto << 48)
 * with laddr = (daddr, dport), raddr = (saddr, sport) in host order, i.e.
 * trans_hash_5tuple / trans_hash_3tuple; the runtime's table buckets are
 * h % TRANS_TBL_SIZE.  GCL_ACT_F_TRANS marks valid entries.
 */
struct gcl_trans {
	uint32_t h5;
	uint32_t h3;
};

/* gcl_runtime_set_trans_seed - the runtime's trans_seed (transport.c:27,
 * :459); needs GCL_CFG_TRANS_HASH.  -ENOENT if @uniqid is not present. */
int gcl_runtime_set_trans_seed(struct gcl_ctx *ctx, uint16_t uniqid, uint32_t seed);

/* All outputs of one classify launch (device pointers; NULL = not wanted). */
struct gcl_out {
	void *verdicts;                  /* required: gcl_verdict[n] or gcl_verdict4[n] */
	uint64_t *runtime_counts;        /* accumulated */
	uint64_t *stats;                 /* accumulated */
	struct gcl_trans *trans;         /* GCL_CFG_TRANS_HASH only */
};

int gcl_classify_ex(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_out *out,
                    void *hip_stream);

/*
 * gcl_access_probe - a measurement aid beside the classify kernel's roofline
 * (bench.py roofline.ceiling_ms), not part of the rx path.  Asynchronous on
 * @hip_stream; 0, -EINVAL or -EIO.  @out receives @vbytes (1, 2, 4 or 8)
 * bytes per packet (not verdicts: a fold of the loaded bytes).
 *
 * At the context's own verdict width: the gcl_classify launch itself -- the
 * same kernel and geometry, its loads (tiles staged through LDS with their
 * drains and barriers for a dense batch; lane-pair header loads, offsets and
 * side arrays for a batch with offsets), and the same verdict writes
 * (deferred where the context defers them) -- with rx_one_pkt replaced by a
 * fold of the header words it reads (and the batch's ol_flags, and hash.rss
 * in a NIC-mode context).  So its time is the kernel's memory shape with
 * nothing computed: the kernel's own ceiling.
 *
 * At another width, or with GCL_PROBE_MIN or'ed into @vbytes: the memory requests
 * one launch over @b cannot do without, and nothing else -- the ceiling the
 * frame layout itself sets (e.g. one 128-B line fetched per 64-B header of a
 * 1536-B slot).  One 16-B load per packet of the line holding frame byte 0
 * (plus one of the next line when frame bytes [0, 40) cross into it), @b's
 * offs, olflags and rss when given, and one write-through store per packet.
 */
#define GCL_PROBE_MIN 0x100
int gcl_access_probe(struct gcl_ctx *ctx, const struct gcl_batch *b, void *out, uint32_t vbytes,
                     void *hip_stream);

/*
 * Test and A/B overrides of the library's measured defaults.  A dataplane
 * never needs them: with every field GCL_TUNE_AUTO (gcl_tune_init) the
 * library makes its own choice, and no environment variable changes it.  The
 * parity tests use them to drive every launch shape and loop form through
 * the same code, tools/ for its A/Bs.
 *
 * gcl_tune_init  - every field GCL_TUNE_AUTO, loop_t0 and debug 0, size set.
 * gcl_ctx_tune   - copy @t into @ctx (NULL: back to the defaults); 0, or
 *                  -EINVAL for a wrong size or a field out of its range.  The
 *                  batch fields apply from the next gcl_classify*, the loop
 *                  fields from the next gcl_rxloop_start.
 */
#define GCL_TUNE_AUTO (-1)
struct gcl_tune {
	uint32_t size;           /* sizeof(struct gcl_tune) */
	/* batch kernels */
	int32_t tables;          /* 0: tables in LDS when they fit, 1: in HBM */
	int32_t depth;           /* tiles in flight per block: 1 or 2 */
	int32_t threads;         /* lanes (packets) per block: 256, 512 or 1024 */
	int32_t grid;            /* blocks per launch (default: the persistent grid) */
	int32_t blocks_per_cu;   /* cap on blocks per CU */
	int32_t defer;           /* dense 1-/2-B verdicts: 0 stored per packet, 1 kept in LDS +
	                            registers and written after the reads where that takes
	                            <= 2 writes per block (default), 2 always */
	int32_t pair_lean;       /* classify_pair_kernel: plain-IPv4 waves on the lean path (1) */
	int32_t tile_lean;       /* classify_kernel: plain-IPv4 waves on the lean path (1) */
	/* the persistent loop */
	int32_t loop64;          /* 0: bursts <= 64 through the general loop kernel */
	int32_t loop_lean;       /* plain-IPv4 bursts on the lean path (1) */
	int32_t loop_spec;       /* speculative window in 10-ns ticks (400; 1 ms with <= 2 workers) */
	int32_t loop_phase_max;  /* poll-phase delay: ceiling in ticks (0 off), set with the two below */
	int32_t loop_phase_up;   /* its step up (> 0) */
	int32_t loop_phase_down; /* its step down (<= up) */
	int32_t loop_prefetch;   /* the next ticket's poll during classification (0 / 1) */
	uint32_t debug;          /* 1: loop diagnostics to stderr */
	int32_t rec_prefetch;    /* GCL_LOOP_HDR_RECORDS: frame headers gcl_rxloop_submit keeps
	                            in flight while it writes the records, 0..64 (64) */
	int32_t slot_prefetch;   /* a wait with no later ticket submitted takes the next
	                            ticket's slot lines for writing while it spins (0 / 1; 1) */
	int32_t vstage;          /* deferred verdicts: the register-held part of the last write
	                            staged through LDS and stored 16 B per lane (1, default) or
	                            stored a verdict per lane per tile (0) */
	int32_t pair_i32;        /* classify_pair_kernel: batches within 2 GiB in 32-bit
	                            arithmetic through buffer descriptors (1) */
	int32_t tile_order;      /* classify_kernel: tiles dealt round-robin over the blocks (0)
	                            or one contiguous run of tiles per block (1) */
	uint64_t loop_t0;        /* tickets start after loop_t0 (rounded down to a multiple of the
	                            ring's slots): tests of the stamps' wrap */
};
void gcl_tune_init(struct gcl_tune *t);
int gcl_ctx_tune(struct gcl_ctx *ctx, const struct gcl_tune *t);

/* Host CRC32C step with the crc32q contract (no inversion, inc/asm/ops.h:77-80)
 * and the two transport hashes, for the runtime side. */
uint32_t gcl_crc32c_u64(uint32_t crc, uint64_t val);
void gcl_trans_hash(uint32_t seed, uint8_t proto, uint32_t lip, uint16_t lport, uint32_t rip,
                    uint16_t rport, struct gcl_trans *out);

/* Synchronise the context's last stream. */
int gcl_sync(struct gcl_ctx *ctx);

/*
 * gcl_kernel_time - with GCL_CFG_PROFILE: total milliseconds the classify
 * kernel ran (HIP events around each launch, on its own stream) and the
 * number of launches since the last reset.  Synchronises.
 */
int gcl_kernel_time(struct gcl_ctx *ctx, double *ms, uint64_t *launches, int reset);

/*
 * gcl_profile_sample - with GCL_CFG_PROFILE, time only one classify launch in
 * @every (the first of each run of @every); gcl_kernel_time then reports the
 * timed launches.  A timed HIP event pair costs the stream ~10 us per launch
 * on MI355X; sampling keeps that out of the throughput it measures.
 * Default 1 (every launch).  -EINVAL for @every == 0.
 */
int gcl_profile_sample(struct gcl_ctx *ctx, uint32_t every);

/*
 * Synthetic rx traffic generator (device).  Counter-based: packet g of the
 * global stream depends only on (seed, g), so every rank and the CPU oracle
 * produce identical bytes.  Packet j of this call is global packet
 * ((j / shard_block) * world + rank) * shard_block + j % shard_block
 * (round-robin block sharding across ranks).
 */
enum gcl_workload {
	GCL_WL_UDP64 = 0,       /* 64-B Eth/IPv4/UDP, uniform 5-tuples */
	GCL_WL_TCP1500_ZIPF = 1,/* 1500-B Eth/IPv4/TCP, Zipf flow ranks */
	GCL_WL_MIXED = 2,       /* IPv4 TCP/UDP + IPv6 + ARP, jumbo lengths */
};

struct gcl_gen_params {
	uint32_t workload;      /* enum gcl_workload */
	uint32_t nruntimes;     /* R: destination IPs are gcl_runtime_ip(r), r < R */
	uint64_t seed;
	uint64_t n;             /* packets to generate */
	uint64_t stride;        /* slot stride (>= 64, multiple of 16) */
	uint32_t rank, world;   /* shard position */
	uint64_t shard_block;   /* packets per round-robin block (0 = no sharding) */
	const uint64_t *zipf_cdf; /* device u64[nflows] (TCP1500_ZIPF only) */
	uint32_t nflows;
	uint32_t pad;
	uint16_t *pkt_len;      /* optional device u16[n]: frame length on the wire
	                           (64, 1500, or the mixed stream's IP/ARP length) */
};

/* Write the first GCL_HDR_GRANULE bytes of every slot of @frames (n * stride
 * bytes; the rest of each slot is left as the caller initialised it), and
 * optionally olflags[n] (what the NIC would report) and rss[n] (an arbitrary
 * 32-bit NIC hash value, so NIC mode can be exercised). */
int gcl_generate(const struct gcl_gen_params *p, uint8_t *frames,
                 uint8_t *olflags, uint32_t *rss, void *hip_stream);

/* IP address of runtime r in the synthetic workloads: 10.0.0.0 + r + 1. */
uint32_t gcl_runtime_ip(uint32_t r);

/* Host helper: Zipf(s) CDF over @nflows ranks as u64 fixed point
 * (cdf[k] = floor(P(rank <= k) * 2^64), last entry saturated). */
int gcl_zipf_cdf(uint32_t nflows, double s, uint64_t *cdf_out);

/*
 * Loopback feed helpers (iokernel/tx.c:81-83, iokernel/dma.c:182-185): the rx
 * olflags of a looped-back tx packet (RSS_HASH iff the runtime set
 * TXFLAG_LOCAL_HINT; IP checksum always good after copy_batch), and the 16-bit
 * steering hint carried in bits 48..63 of the txpkt payload
 * (inc/iokernel/queue.h:120-134).
 */
uint8_t gcl_loopback_olflags(uint8_t tx_olflags);
uint32_t gcl_txpkt_rss(uint64_t payload);

/* Host reference of the two hashes the kernel computes (for callers that
 * need the same value on the CPU, e.g. the loopback hint). */
uint32_t gcl_jenkins_hash(const void *key, size_t len);
uint32_t gcl_toeplitz(const uint8_t *key, size_t keylen, const uint8_t *input,
                      size_t len);

/* Device memory for batches (hipMalloc on @hip_device): 0, -ENODEV, -ENOMEM. */
int gcl_dev_alloc(int hip_device, size_t bytes, void **out);
int gcl_dev_free(void *p);

/*
 * Placement-aware device allocation for the two long-lived classify buffers
 * (the frame pool and the verdict ring, the GPU-side counterparts of the
 * iokernel's ingress region and rxq rings, shm.h:14-15, ioqueues.c:31-40).
 * On MI355X the header read stream and the verdict write stream run ~15%
 * slower when the two buffers fall in the same physical placement class
 * (measured: DESIGN.md §4 "Buffer placement", profiles/archive/r01_pair_*.jsonl).
 * The class cannot be read from a virtual address, so this allocates a
 * candidate, times a read+write probe of the classify kernel's access shape
 * over the whole of both buffers (up to 4 GiB read, 256 MiB written) against
 * @partner, and keeps the first candidate whose probe differs from an
 * earlier one by more than the class gap (the faster of the two), trying at
 * most GCL_PAIR_TRIES candidates; losers are freed.  Classes come in runs of
 * consecutive allocations (4-34 GiB of 2-GiB pools in a row were measured,
 * profiles/archive/r02_classmap.jsonl), so after every GCL_PAIR_RUN candidates of one
 * class a spacer of 2, 4, 8, then 16 x @bytes is allocated to step past the
 * run.  Candidates and spacers together hold at most 60% of the free device
 * memory; all but the kept buffer are freed before returning.  When no second
 * class shows up the fastest candidate is kept, @info->classes is 1 and a
 * warning goes to stderr (the GCL_PAIR_QUIET flag silences it;
 * GCL_PAIR_VERBOSE prints every candidate's probe).
 *
 * GCL_PAIR_NEW_READS: the new buffer is the one stream-read (frames) and
 *                     @partner the one written (verdicts);
 * GCL_PAIR_NEW_WRITES: the reverse.
 * OR in GCL_PAIR_VBYTES(1|2|4|8), the verdict width the kernel will write
 * (default 4): the probe stores the same width, so its time tracks the
 * kernel's for every format.
 * The probe WRITES to the written side's first min(bytes, 256 MiB), rounded
 * down to whole 256-verdict tiles (@info->probe_write_bytes), and nothing past it: call it before that buffer
 * holds data.  @info may be NULL.
 * Returns 0, -EINVAL, -ENODEV, -ENOMEM or -EIO.
 */
#define GCL_PAIR_NEW_READS  0x1
#define GCL_PAIR_NEW_WRITES 0x2
#define GCL_PAIR_VBYTES(b)  ((uint32_t)(b) << 8)
#define GCL_PAIR_VBYTES_OF(f) (((f) >> 8) & 0xFF)
#define GCL_PAIR_QUIET      0x10000
#define GCL_PAIR_VERBOSE    0x20000
#define GCL_PAIR_TRIES      24
#define GCL_PAIR_RUN        2
struct gcl_pair_info {
	double   chosen_us;         /* probe time of the buffer kept */
	double   worst_us;          /* slowest candidate probed */
	uint32_t candidates;        /* candidates probed */
	uint32_t classes;           /* placement classes seen: 2, or 1 (kept one may be slow) */
	uint64_t spacer_bytes;      /* spacer memory held during the search */
	uint64_t probe_write_bytes; /* bytes of the written side the probe stored to */
};
int gcl_dev_alloc_paired(int hip_device, size_t bytes, const void *partner, size_t partner_bytes,
                         uint32_t flags, void **out, struct gcl_pair_info *info);

/*
 * Persistent rx loop: the classifier at the reference's own granularity, one
 * rx_burst of <= IOKERNEL_RX_BURST_SIZE mbufs at a time (iokernel/rx.c:270-290,
 * defs.h:75), with microsecond latency instead of batch latency.  A
 * persistent kernel polls a ring of burst slots in coherent host memory,
 * classifies each burst straight from the registered ingress region (the 2
 * GiB mbuf pool, shm.h:14-15) and writes the verdicts back into the slot.
 *
 * gcl_rxloop_start - launch the loop for @ctx.  @cfg->region must be
 *   registered with gcl_host_register; frames are addressed by byte offsets
 *   into it (mbuf data pointer - region base, like ptr_to_shmptr, shm.h:40-47).
 *   The kernel leaves by itself after @cfg->lifetime_ms.  Tables must fit in
 *   LDS (-E2BIG otherwise); with GCL_CFG_TRANS_HASH each burst's transport
 *   demux hashes come back beside its verdicts (gcl_rxloop_trans);
 *   one loop per context (-EBUSY); the region must be shorter than 2^40 - 64
 *   bytes (-EINVAL: offsets share their slot entry with a stamp, so a burst
 *   of <= 64 packets has its offsets with the poll that finds it; offsets at
 *   or past the region's end still read as frames of zeros).  Table changes
 *   made with gcl_runtime_set /
 *   _del apply from the next submitted burst on (snapshot semantics).
 * gcl_rxloop_submit - publish one burst; returns its ticket (> 0), -EAGAIN
 *   when the ring is full (a slot is reused only after gcl_rxloop_wait has
 *   collected the burst it held, as an lrpc ring's consumer frees a slot), -EINVAL, -E2BIG (tables grew past LDS) or
 *   -ESHUTDOWN when the kernel has left.  The arrays are copied; the side
 *   arrays (olflags, rss, fdir_hi, dst_hint) are optional, as in gcl_batch.
 * gcl_rxloop_wait - spin up to @spin_ns for @ticket; 0 and the burst's
 *   verdicts (gcl_verdict or gcl_verdict4 per the context) copied to
 *   @verdicts_out (may be NULL), -EAGAIN if not done yet, -ESTALE if the slot
 *   was already reused, -ESHUTDOWN if the kernel left first.
 * gcl_rxloop_stop - raise the stop flag, wait for the kernel, free the loop.
 * gcl_rxloop_drive - measurement helper: @iters bursts of the same @n offsets
 *   with @depth bursts in flight; lat_ns[i] = submit -> verdicts seen of
 *   burst i, *elapsed_ns the whole run.
 */
struct gcl_rxloop;
struct gcl_rxloop_cfg {
	uint32_t slots;        /* ring depth: power of two, 2..1024 */
	uint32_t max_burst;    /* packets per burst: 1..4096 */
	uint32_t workers;      /* polling workgroups: 1..64 */
	uint32_t lifetime_ms;  /* kernel lifetime bound: 1..600000 */
	const void *region;    /* registered host region holding the frames */
	uint64_t region_len;
	uint64_t *counts;      /* device u64[max_runtimes] (optional), accumulated; the loop
	                          runs on a stream of its own: gcl_rxloop_start waits for the
	                          default stream's work (e.g. their zeroing), work on other
	                          streams must be complete before the call */
	uint64_t *stats;       /* device u64[GCL_NR_STATS] (optional), accumulated, as counts */
	uint32_t flags;        /* GCL_LOOP_INLINE_HDRS or GCL_LOOP_HDR_RECORDS */
	uint32_t pad;
};
/* gcl_rxloop_submit copies each frame's first 64-B header granule into the
 * ring slot (the dataplane core reads the headers, as rx_one_pkt does), so
 * the kernel fetches them with the burst's side arrays instead of one PCIe
 * round trip later from the region.  Since the offsets arrive with the poll
 * the two forms take the same time for one burst; inlining saves the GPU's
 * reads of the region when many workers keep PCIe busy. */
#define GCL_LOOP_INLINE_HDRS 0x1
/* gcl_rxloop_submit writes each packet as one 64-B header record in the
 * slot: the header words rx_one_pkt reads (frame bytes 12-15 and 20-43), its
 * offset and its side fields, every 16-B chunk led by the slot's use count
 * and written with one 16-B store (the four chunks of a record in four
 * planes, so the GPU reads each plane contiguously).  A worker polling a burst of <= 64
 * packets reads the records with the slot word and, when every chunk carries
 * the current count, classifies at once: one PCIe round trip per burst
 * instead of two.  Ports past byte 43 (IHL >= 7) are read from the region.
 * Exclusive with GCL_LOOP_INLINE_HDRS (-EINVAL).  A worker polls the records
 * (or, without this flag, the stamped offsets) during the first 4 us of a
 * wait, or the first 1 ms in a loop of 1 or 2 workers (gcl_tune.loop_spec);
 * a burst found later is read after its word.  In a loop of 1 or 2 workers
 * with bursts of <= 64 a worker issues the first poll of each ticket a
 * little after its last verdict records, the delay following the host's
 * turnaround (up to 1.2 us; gcl_tune.loop_phase_*): a dataplane core that
 * submits once it has seen the last verdicts is sampled just after its
 * submit rather than a round trip later.  In a loop of more than 2 workers
 * without this flag (stamped offsets), a worker whose burst was already
 * there at its first poll issues the next ticket's poll while it classifies
 * that burst (gcl_tune.loop_prefetch). */
#define GCL_LOOP_HDR_RECORDS 0x2
/* Measurement: lane 0 of the worker stores each burst's stage times into
 * the slot header after its records (gcl_rxloop_stamps). */
#define GCL_LOOP_STAMPS 0x4
int gcl_rxloop_start(struct gcl_ctx *ctx, const struct gcl_rxloop_cfg *cfg,
                     struct gcl_rxloop **out);
int64_t gcl_rxloop_submit(struct gcl_rxloop *loop, uint32_t n, const uint64_t *offs,
                          const uint8_t *olflags, const uint32_t *rss, const uint32_t *fdir_hi,
                          const uint32_t *dst_hint);
int gcl_rxloop_wait(struct gcl_rxloop *loop, int64_t ticket, void *verdicts_out, uint64_t spin_ns);
/*
 * gcl_rxloop_peek - gcl_rxloop_wait without the copy: on 0, *@recs points at
 * the burst's @*n verdict records in the ring slot itself (one 16-B record per
 * packet, written by the kernel with one store; @verdict holds the verdict in
 * the context's width -- gcl_verdict4 bytes, the 2-byte queue verdict in the
 * low half, or with 8-byte verdicts {hash, verdict} is the struct gcl_verdict).
 * The records stay valid, and the slot is not reused, until
 * gcl_rxloop_release(@ticket): the post-pass (gcl_host_deliver_recs) reads
 * them in place.  Errors as gcl_rxloop_wait.
 */
struct gcl_loop_rec {
	uint32_t hash;
	uint32_t verdict;
	uint64_t ticket;
};
int gcl_rxloop_peek(struct gcl_rxloop *loop, int64_t ticket, uint64_t spin_ns,
                    const struct gcl_loop_rec **recs, uint32_t *n);
int gcl_rxloop_release(struct gcl_rxloop *loop, int64_t ticket);
/* gcl_rxloop_poll_stats - how the loop's bursts have arrived so far, summed
 * over its workers: @out[0] with the poll that found the burst (offsets or
 * header records already current: one PCIe round trip), @out[1] eligible
 * for that (<= 64 packets, in the speculative window) but an entry still
 * stale, so read after the word, @out[2] read after the word (the window
 * over, a longer burst, or inline granules).  Before gcl_rxloop_stop.
 * The burst-of-64 kernel's writer wave posts these counters (and the lean
 * count below) after the burst's verdict records, so both can lag the bursts
 * a gcl_rxloop_wait has seen complete by up to a few microseconds: poll. */
int gcl_rxloop_poll_stats(struct gcl_rxloop *loop, uint64_t out[3]);
/* gcl_rxloop_lean_bursts - how many of the loop's bursts so far were
 * classified by the burst-of-64 kernel's lean path (every packet plain IPv4:
 * IHL 5, no FDIR mark, no dst_ip hint, no transport pre-hash; the verdicts and
 * counters are classify_core's), summed over its workers, into @out.  Before
 * gcl_rxloop_stop. */
int gcl_rxloop_lean_bursts(struct gcl_rxloop *loop, uint64_t *out);
/* gcl_rxloop_trans - a GCL_CFG_TRANS_HASH context's transport demux hashes
 * of @ticket's burst (struct gcl_trans per packet, as gcl_classify_ex writes
 * them), copied to @out once the burst is complete: after gcl_rxloop_wait
 * and before the slot's next submit, or between gcl_rxloop_peek and
 * _release.  -EINVAL (no transport hashes), -EAGAIN (not complete yet),
 * -ESTALE (the slot was reused). */
int gcl_rxloop_trans(struct gcl_rxloop *loop, int64_t ticket, struct gcl_trans *out);
/* gcl_rxloop_stamps - with GCL_LOOP_STAMPS: @ticket's stage times in ns
 * (s_memrealtime, 10-ns ticks): @out[0] the round trip of the poll that
 * found the burst (its issue to its return), @out[1] from that return to
 * the packets classified, @out[2] to the last verdict record's store issued,
 * @out[3] the polls of that wait, @out[4..6] from the return to past the
 * worker's first, second and third barriers (burst header shared, tables
 * and histogram ready, tile ready), @out[7] 0; with the kernel for bursts of
 * <= 64 (max_burst <= 64), @out[4..6] from the return to the packets in
 * registers, the burst posted to the writer wave, the writer taking it,
 * and @out[7] 1.  -EAGAIN until they land
 * (they are posted after the records), -ESTALE once the slot is reused,
 * -EINVAL without the flag. */
int gcl_rxloop_stamps(struct gcl_rxloop *loop, int64_t ticket, uint64_t out[8]);
int gcl_rxloop_stop(struct gcl_rxloop *loop);
int gcl_rxloop_drive(struct gcl_rxloop *loop, uint32_t n, const uint64_t *offs, uint32_t iters,
                     uint32_t depth, uint64_t *lat_ns, uint64_t *elapsed_ns);

/*
 * Delivery plan: a stable partition of a classified batch by destination, on
 * the GPU.  The host post-pass walks a verdict array in packet order on one
 * core; a plan gives it one packet-index list per runtime (or per flow-table
 * queue) instead, each in ascending packet order, so that disjoint sets of
 * runtimes can be delivered by different cores with gcl_host_deliver_idx
 * (gcl_host.h) and every kthread ring still receives the message sequence it
 * receives from one in-order pass.  The per-bucket counts let a core check
 * ring space before it starts.
 *
 * @verdicts is a device array in the context's own width (8, 4, 2 or 1 B), as
 * gcl_classify wrote it, 16-B aligned.  The last bucket, the host bucket,
 * takes every packet that is not DELIVER or WAKE (DROP_*, BROADCAST,
 * ARP_RESPOND), and every verdict whose key would be >= nbuckets - 1 (a
 * uniqid >= max_runtimes, the undefined 2-B kind 0x8000, garbage): no byte
 * pattern in @verdicts indexes outside the counters or outside order[0, n).
 *  GCL_PLAN_BY_RUNTIME  nbuckets = max_runtimes + 1; the key is the uniqid
 *                       (8-/4-B), or the queue index >> thread_bits (2-/1-B)
 *  GCL_PLAN_BY_QUEUE    nbuckets = (max_runtimes << thread_bits) + 1; the key
 *                       is the queue index q of a 2-/1-B verdict; -EINVAL on
 *                       an 8-/4-B context
 * Result: bucket_off[b] is the number of packets with key < b,
 * bucket_off[nbuckets] = n, and order[bucket_off[b] .. bucket_off[b + 1]) the
 * indices of bucket b's packets, ascending: order is the stable argsort of
 * the keys.
 *
 * gcl_plan_buckets   - nbuckets of @key for this context.
 * gcl_plan_workspace - bytes of device scratch a plan of @n verdicts takes
 *                      (the counters of every packet range: ranges x nbuckets
 *                      x 4 B, at most 16 MiB by the library's own choice of
 *                      ranges, plus the scan's block sums).
 * gcl_plan           - asynchronous on @hip_stream; no host synchronisation
 *                      and no allocation.  @workspace (device, 16-B aligned)
 *                      need not be zeroed and may be reused by the next call
 *                      on the same stream.  @verdicts must not change between
 *                      the call and its completion: the kernels read them
 *                      twice (a caller who breaks this gets a wrong list, never
 *                      a write outside order[0, n)).  n == 0 zeroes
 *                      bucket_off.  -EINVAL for a bad size or key, NULL or
 *                      misaligned pointers, n > 2^31, a workspace that is too
 *                      small, BY_QUEUE on a wide-verdict context, or
 *                      blocks x nbuckets > 2^24; -EIO when a launch fails.
 */
enum gcl_plan_key {
	GCL_PLAN_BY_RUNTIME = 0, /* every verdict width */
	GCL_PLAN_BY_QUEUE   = 1, /* GCL_CFG_VERDICT1 / VERDICT2 contexts only */
};
struct gcl_plan_cfg {
	uint32_t size;    /* sizeof(struct gcl_plan_cfg) */
	uint32_t key;     /* enum gcl_plan_key */
	uint32_t blocks;  /* 0: the library's choice; else the number of contiguous
	                     packet ranges the batch is cut into (tests) */
	uint32_t pad;
};
struct gcl_plan_out {
	uint32_t *order;      /* device u32[n] */
	uint32_t *bucket_off; /* device u32[nbuckets + 1] */
};
int gcl_plan_buckets(const struct gcl_ctx *ctx, uint32_t key, uint32_t *nbuckets);
int gcl_plan_workspace(const struct gcl_ctx *ctx, const struct gcl_plan_cfg *cfg, uint64_t n,
                       size_t *bytes);
int gcl_plan(struct gcl_ctx *ctx, const struct gcl_plan_cfg *cfg, const void *verdicts, uint64_t n,
             const struct gcl_plan_out *out, void *workspace, size_t workspace_bytes,
             void *hip_stream);

/*
 * Packed delivery records: the messages of an index list, ready to send, in
 * list order.  gcl_host_deliver_idx reads verdicts[idx[j]], pkt_len[idx[j]],
 * olflags[idx[j]] and shmptr[idx[j]] for every packet of a list: four
 * dependent reads strided through arrays no core's cache holds.  The GPU
 * holds the same arrays and gathers them here into three dense ones, which
 * gcl_host_deliver_packed (gcl_host.h) walks sequentially.  @order is a
 * plan's order, or one bucket's slice of it (order + bucket_off[b], m =
 * bucket_off[b + 1] - bucket_off[b]); with i = order[j], for j in [0, m):
 *   cmd[j]      gcl_rx_make_cmd(pkt_len ? pkt_len[i] : 0,
 *                               olflags ? olflags[i] : cfg.default_olflags):
 *               len << 16 | csum_type << 48, bit 63 (the ring's parity) clear
 *   payload[j]  shm_base + (offs ? offs[i] : i * stride): the frame's
 *               ptr_to_shmptr (rx.c:82) when the batch's frames lie in the
 *               ingress region at shm_base
 *   v4[j]       verdict i as a gcl_verdict4: the last four bytes of an 8-B
 *               verdict (action flags kept), a 4-B verdict as it is,
 *               gcl_verdict2_to4 / gcl_verdict1_to4 (gcl_host.h) of a 2- / 1-B
 *               verdict with the context's thread_bits
 * An entry order[j] >= n gets cmd = 0, payload = 0 and v4 = {GCL_NO_RUNTIME,
 * GCL_NO_THREAD, GCL_ACT_MASK}, which gcl_host_deliver_packed skips by its
 * index: no content of @order or @verdicts causes a read outside [0, n) of a
 * per-packet array or a write outside [0, m) of the outputs.
 *
 * gcl_plan_pack - asynchronous on @hip_stream; no allocation, no host
 *                 synchronisation; on the same stream it may directly follow
 *                 the gcl_plan that writes @order.  m == 0 is a no-op.
 *                 -EINVAL for a wrong size, a NULL verdicts / order / output,
 *                 an output that is not 16-B aligned, an input that is not
 *                 aligned to its element (verdicts: the context's width), or
 *                 m > 2^31; -EIO when the launch fails.
 */
struct gcl_pack_in {
	uint32_t size;            /* sizeof(struct gcl_pack_in) */
	uint32_t pad;
	const void     *verdicts; /* device, the context's width, n entries */
	uint64_t        n;        /* packets in the batch */
	const uint32_t *order;    /* device u32[m], 4-B aligned */
	uint64_t        m;        /* entries to pack, <= 2^31 */
	const uint16_t *pkt_len;  /* optional device u16[n] */
	const uint8_t  *olflags;  /* optional device u8[n] */
	const uint64_t *offs;     /* optional device u64[n]; else i * stride */
	uint64_t        stride;
	uint64_t        shm_base;
};
struct gcl_pack_out {         /* device, 16-B aligned, m entries each */
	uint64_t *cmd;
	uint64_t *payload;
	struct gcl_verdict4 *v4;
};
int gcl_plan_pack(struct gcl_ctx *ctx, const struct gcl_pack_in *in,
                  const struct gcl_pack_out *out, void *hip_stream);

/*
 * IPv4 header checksum offload: the rx offload a NIC reports in
 * RTE_MBUF_F_RX_IP_CKSUM_*, for batches that arrive without it (a pcap
 * replay, a NIC or virtual function without the offload, ol_flags that say
 * UNKNOWN).  rx_make_cmd (iokernel/rx.c:24-38) sends CHECKSUM_TYPE_UNNECESSARY
 * only for IP_CKSUM_GOOD; for every other packet the receiving runtime runs
 * chksum_internet(iphdr, sizeof(*iphdr)) itself and drops on a non-zero
 * result (net_rx_one, runtime/net/core.c:275-279).  gcl_rx_csum makes that
 * check on the GPU and writes its verdict into the checksum bits of an
 * ol_flags array, which gcl_host_deliver* and gcl_plan_pack then turn into
 * cmd as before.
 *
 * Packet i, with fl = b->olflags[i], or cfg.default_olflags when b->olflags
 * is NULL:
 *   frame bytes 12-13 are not 0x0800        olflags_out[i] = fl    SKIPPED
 *   fl's checksum bits say IP_CKSUM_GOOD    olflags_out[i] = fl    SKIPPED
 *   otherwise (UNKNOWN, BAD or NONE)        CHECKED: the one's-complement sum
 *     of the ten 16-bit words of frame bytes [14, 34) is folded to 16 bits;
 *     the header is good iff it is 0xFFFF (chksum_internet returns 0), and
 *     olflags_out[i] = (fl & ~GCL_F_IP_CKSUM_MASK) |
 *                      (good ? GCL_F_IP_CKSUM_GOOD : GCL_F_IP_CKSUM_BAD),
 *     counted as GOOD or BAD.
 *
 * Guarantee: the reference sends CHECKSUM_TYPE_NEEDED for everything but
 * IP_CKSUM_GOOD and the runtime then decides by this same 20-byte check, so a
 * runtime fed gcl_rx_make_cmd(len, olflags_out[i]) accepts exactly the
 * packets it accepts when fed gcl_rx_make_cmd(len, fl); it only skips the
 * check on those marked GOOD.  Limit: GOOD here means what net_rx_one
 * verifies, the first 20 header bytes whatever the IHL says, not a NIC's
 * whole-header check of a header with options; ip_hdr_supported
 * (runtime/net/core.c:203-209) drops those frames afterwards either way.
 *
 * Frames are addressed as gcl_classify addresses them (frames, frames_len,
 * stride or offs at any byte alignment; an offset at or past frames_len is a
 * frame of zeros and every byte at or past frames_len reads 0, so a frame may
 * be cut anywhere); rss, fdir_hi, dst_hint and pkt_len are ignored.  Every
 * pointer is a device pointer.  @olflags_out (u8[n]) may be exactly
 * b->olflags (in place); any other overlap is the caller's error.  @counts is
 * a device u64[GCL_CSUM_NR], ACCUMULATED, may be NULL; per call CHECKED =
 * GOOD + BAD and CHECKED + SKIPPED = n.  No content of frames, offs or
 * olflags causes a read outside frames[0, frames_len), offs[0, n) or
 * olflags[0, n), or a write outside olflags_out[0, n).
 *
 * Asynchronous on @hip_stream; no allocation, no host synchronisation.
 * n == 0 is a no-op.  -EINVAL for a NULL ctx, b or olflags_out and for the
 * batches gcl_classify refuses (NULL frames, frames_len == UINT64_MAX,
 * n > 2^40, a stride < 16, not a multiple of 16 or > 2^20 when offs is NULL);
 * -EIO when the launch fails.
 */
enum {
	GCL_CSUM_CHECKED = 0, /* packets the check was made for: GOOD + BAD */
	GCL_CSUM_GOOD,
	GCL_CSUM_BAD,
	GCL_CSUM_SKIPPED,     /* not IPv4, or IP_CKSUM_GOOD on entry */
	GCL_CSUM_NR = 4,
};
int gcl_rx_csum(struct gcl_ctx *ctx, const struct gcl_batch *b, uint8_t *olflags_out,
                uint64_t *counts, void *hip_stream);

/*
 * TCP/UDP checksum offload, both directions: what the reference asks of the
 * NIC with IPV4_CKSUM | UDP_CKSUM | TCP_CKSUM (iokernel/dpdk.c:80,
 * iokernel/tx.c:67-70), for batches that have no NIC to do it.
 *
 * GCL_L4_FILL is the transmit side.  With cfg.tx_offloads_disabled
 * (dpdk.c:140-148) every runtime runs ipv4_udptcp_cksum over the whole
 * segment (runtime/net/tcp_out.c:33-39) and ipv4_cksum (runtime/net/core.c:
 * 612-617) on its own cores; FILL writes those two fields for a batch of
 * frames on the GPU.  GCL_L4_VERIFY is the receive side, which the reference
 * leaves to the NIC entirely (nothing under runtime/net checks a TCP or UDP
 * checksum): a pcap replay, a TAP or virtual function, or a looped-back frame
 * (whose TCP field holds only the pseudo-header sum) reaches a socket with
 * its payload unchecked unless somebody sums it.
 *
 * Packet i has o = its offset clamped to frames_len (b->offs[i], or
 * i * b->stride), avail = frames_len - o and L = min(b->pkt_len[i], avail):
 * the mbuf's bytes that exist.  No byte at or past o + L enters any result,
 * and none is written.
 *
 *   IP-eligible: L >= 34, frame bytes 12-13 are 0x0800, version 4 and IHL 5
 *     (ip_hdr_supported, and the fixed l3_len of tx.c:72).
 *   L4-eligible: IP-eligible, not a fragment (MF clear and fragment offset 0,
 *     on the host-order field), protocol 6 or 17, and tot = ntoh16(bytes
 *     16-17) with tot >= 20 + (TCP ? 20 : 8) and 14 + tot <= L (the length
 *     test of net_rx_one, core.c:283-285).  l4len = tot - 20; bytes past
 *     14 + tot (Ethernet padding) are not summed, as after mbuf_trim.
 *   S: the 16-bit end-around-carry fold of the L4 bytes [34, 34 + l4len) as
 *     16-bit words in memory order (an odd last byte is the low byte of a
 *     last word) plus the pseudo-header {saddr, daddr, 0, proto,
 *     hton16(l4len)} of the frame's own addresses: __raw_cksum and
 *     ipv4_phdr_cksum of inc/net/chksum.h.
 *
 * VERIFY writes status and counts only.  status[i] is GCL_L4_NA when the
 * packet is not L4-eligible, GCL_L4_NONE for UDP whose checksum field is 0,
 * GCL_L4_GOOD when S over the bytes as they stand is 0xFFFF, GCL_L4_BAD when
 * it is not; per call GOOD + BAD + NONE + NA = n.
 *
 * FILL, with f = in->tx_olflags ? in->tx_olflags[i] : 3 (txpkt cmd.olflags):
 *   bit 0 (OLFLAG_IP_CHKSUM) and IP-eligible: frame bytes 24-25 become
 *     ipv4_cksum of the header with that field taken as 0; status gets
 *     GCL_L4_FILLED_IP.
 *   bit 1 (OLFLAG_TCP_CHKSUM) and L4-eligible: the L4 checksum field (bytes
 *     50-51 for TCP, 40-41 for UDP) is taken as 0 whatever it held (the
 *     runtime leaves the pseudo-header sum there for the NIC) and becomes
 *     ipv4_udptcp_cksum's value, ~S & 0xFFFF with 0 replaced by 0xFFFF for
 *     both protocols; status gets GCL_L4_FILLED_L4.
 *   The status low nibble is GCL_L4_NA.  The two fills do not feed each
 *   other: the IP field is outside the bytes S covers (the pseudo-header
 *   takes only the addresses) and the L4 field is outside the IP header.
 *   FILL writes through b->frames (the const is the struct's; the caller owns
 *   the memory) and writes only the two or four checksum bytes of a filled
 *   packet, each with a store of its own width or narrower: no wider word is
 *   read-modify-written.  Frames that overlap are the caller's error in FILL
 *   (the fields are then unspecified); nothing is written out of bounds even
 *   so.
 *
 * Frames are addressed as gcl_rx_csum addresses them (frames, frames_len,
 * stride or offs at any byte alignment); b->pkt_len (u16[n], 2-B aligned) is
 * REQUIRED here; rss, fdir_hi, dst_hint and olflags are ignored.  Every
 * pointer is a device pointer.  @status is u8[n].  @counts is a device
 * u64[GCL_L4C_NR], ACCUMULATED, may be NULL: GOOD, BAD, NONE and NA count the
 * status low nibbles (so FILL adds n to NA), FILLED_IP and FILLED_L4 the two
 * bits, and BYTES adds l4len of every packet judged GOOD or BAD (VERIFY) or
 * FILLED_L4 (FILL).  No content of frames,
 * offs, pkt_len or tx_olflags causes a read outside frames[0, frames_len) or
 * the n-element arrays, or a write outside status[0, n), counts and the
 * checksum bytes above, which lie inside [o, o + L).
 *
 * in->group = 0 lets the library choose how many lanes sum one packet from
 * in->len_hint (the typical frame length, 0 = unknown); 4, 16 or 64 force it
 * (tests).  The result does not depend on it.
 *
 * Asynchronous on @hip_stream; no allocation, no host synchronisation.
 * n == 0 is a no-op.  -EINVAL for a NULL ctx, b, in or status, a wrong
 * in->size, a mode other than VERIFY or FILL, a group other than 0, 4, 16 or
 * 64, a NULL pkt_len or one that is not 2-B aligned, and the batches
 * gcl_rx_csum refuses; -EIO when the launch fails.
 */
enum gcl_l4_mode { GCL_L4_VERIFY = 0, GCL_L4_FILL = 1 };
/* status byte, low nibble: the verdict of the L4 check */
#define GCL_L4_NA    0   /* not a datagram this call judges */
#define GCL_L4_GOOD  1
#define GCL_L4_BAD   2
#define GCL_L4_NONE  3   /* VERIFY: UDP with checksum field 0 (no checksum sent) */
/* FILL: or-ed in */
#define GCL_L4_FILLED_IP 0x10
#define GCL_L4_FILLED_L4 0x20
enum {
	GCL_L4C_GOOD = 0,
	GCL_L4C_BAD,
	GCL_L4C_NONE,
	GCL_L4C_NA,
	GCL_L4C_FILLED_IP,
	GCL_L4C_FILLED_L4,
	GCL_L4C_BYTES,        /* L4 bytes of the packets whose S was used */
	GCL_L4C_NR = 8,
};
struct gcl_l4_in {
	uint32_t size;      /* sizeof(struct gcl_l4_in) */
	uint32_t mode;      /* enum gcl_l4_mode */
	uint32_t group;     /* 0: the library's choice; else lanes per packet: 4, 16 or 64 (tests) */
	uint32_t len_hint;  /* typical frame length, only steers the choice of group; 0 = unknown */
	const uint8_t *tx_olflags; /* FILL: optional u8[n] txpkt cmd.olflags; NULL = IP and L4 for every packet */
};
int gcl_l4_csum(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_l4_in *in,
                uint8_t *status, uint64_t *counts, void *hip_stream);

/*
 * The loopback frame copy: copy_batch(src_bufs, rx_bufs, n_bufs, rx_one_pkt)
 * of rx_loopback (iokernel/rx.c:264, iokernel/dma.c:167-191), the step between
 * the dst_ip lookups (gcl_batch.dst_hint) and rx_one_pkt (gcl_classify).  For
 * every tx packet the reference appends rte_pktmbuf_pkt_len(src) bytes to a
 * fresh rx mbuf and copies the frame into it, copies ol_flags, ORs in
 * RTE_MBUF_F_RX_IP_CKSUM_GOOD and copies hash; where an idxd engine is present
 * it hands the copy to it (copy_batch_dma, dma.c:140-165).  gcl_copy_batch
 * makes that copy for a batch on the GPU: @n frames of any length at any byte
 * alignment out of the tx region into the rx pool that gcl_classify then
 * reads, with the three per-packet fields the classify batch takes
 * (gcl_batch.pkt_len is what the post-pass sends, olflags and rss feed
 * rx_one_pkt).
 *
 * Packet i, with L = in->len[i] and d = out->dst_off ? out->dst_off[i] :
 * i * out->dst_stride:
 *   REFUSED when in->dst_cap != 0 and L > in->dst_cap, when out->dst_off is
 *     NULL and L > out->dst_stride, or when the range does not fit the pool:
 *     d > dst_len or L > dst_len - d (no sum is formed, so any d up to
 *     UINT64_MAX is judged rightly).  No destination byte is written,
 *     pkt_len[i] = 0.  This is the rte_pktmbuf_append the reference asserts
 *     on: a caller drops such a packet (a batch entry with pkt_len 0 is not to
 *     be classified or delivered) or copies it by other means.
 *   COPIED otherwise: dst[d + j] = src[src_off[i] + j] for j in [0, L), where
 *     a source byte at or past src_len reads 0 (src_off[i] + j is never formed
 *     where it could overflow: an offset at or past src_len is a frame of
 *     zeros); pkt_len[i] = L; L is added to BYTES.  L == 0 is COPIED and
 *     writes no byte.
 *   For every i < n, copied or refused: out->olflags[i] =
 *     gcl_loopback_olflags(in->tx_olflags ? in->tx_olflags[i] : 0) and
 *     out->rss[i] = in->hash ? in->hash[i] : 0, each when the output array is
 *     given.
 *
 * @counts is a device u64[GCL_COPY_NR], ACCUMULATED, may be NULL; per call
 * COPIED + REFUSED = n and BYTES is the sum of pkt_len.
 *
 * @src is device-visible memory: HBM, or a tx region registered with
 * gcl_host_register, given by its host address and read in place over PCIe
 * (the call looks its device address up; that is a table lookup, no
 * synchronisation).  Every other pointer is a device pointer.  The u64, u32 and u16 arrays are aligned to their element;
 * src, dst and the offsets may have any byte alignment.
 *
 * Guarantee: no content of src_off, len or dst_off causes a read outside
 * src[0, src_len) or the n-element input arrays, or a write outside
 * dst[0, dst_len) or the n-element output arrays; and no destination byte
 * outside the [d, d + L) of a copied packet is written, not even with the
 * value it already had: neighbouring mbufs belong to other packets, which
 * other lanes may be writing at the same time, so there is no
 * read-modify-write of a wider word.  Two copied packets whose destination
 * ranges overlap, or any overlap of src and dst, are the caller's error (the
 * bytes there are then unspecified); nothing is written out of bounds even so.
 *
 * in->group = 0 lets the library choose how many lanes copy one packet from
 * in->len_hint (the typical frame length, 0 = unknown); 4, 16 or 64 force it
 * (tests).  The result does not depend on it.
 *
 * Asynchronous on @hip_stream; no allocation, no host synchronisation.
 * n == 0 is a no-op.  -EINVAL for a wrong in->size, a NULL ctx, in, out, src,
 * src_off, len, dst or pkt_len, src_len or dst_len == UINT64_MAX, n > 2^40,
 * a dst_stride < 16, not a multiple of 16 or > 2^20 when dst_off is NULL, a
 * group other than 0, 4, 16 or 64, or an element array that is not aligned to
 * its element; -EIO when the launch fails.
 */
enum {
	GCL_COPY_COPIED = 0,
	GCL_COPY_REFUSED,     /* the frame does not fit its destination */
	GCL_COPY_BYTES,       /* frame bytes of the copied packets */
	GCL_COPY_NR = 4,
};
struct gcl_copy_in {
	uint32_t size;              /* sizeof(struct gcl_copy_in) */
	uint32_t group;             /* 0: the library's choice; else lanes per packet: 4, 16 or 64 (tests) */
	const uint8_t  *src;        /* device-visible: HBM, or a gcl_host_register'ed tx region */
	uint64_t        src_len;    /* bytes at or past it read as 0, at any offset */
	const uint64_t *src_off;    /* u64[n], any byte alignment */
	const uint16_t *len;        /* u16[n]: txpkt cmd.len, tx.c:61-63 */
	const uint8_t  *tx_olflags; /* optional u8[n]: txpkt cmd.olflags (OLFLAG_*, TXFLAG_*) */
	const uint32_t *hash;       /* optional u32[n]: pkt->hash, tx.c:82 */
	uint64_t        n;
	uint32_t        len_hint;   /* typical frame length, only steers the library's choice of group; 0 = unknown */
	uint32_t        dst_cap;    /* a frame longer than this is refused; 0 = no cap of its own */
};
struct gcl_copy_out {
	uint8_t        *dst;        /* device: the rx pool (gcl_batch.frames of the batch to classify) */
	uint64_t        dst_len;
	const uint64_t *dst_off;    /* optional u64[n], any alignment; else i * dst_stride */
	uint64_t        dst_stride; /* dst_off == NULL: multiple of 16, 16..2^20, as gcl_batch.stride */
	uint16_t       *pkt_len;    /* u16[n]: len[i] when copied, 0 when refused */
	uint8_t        *olflags;    /* optional u8[n]: gcl_loopback_olflags(tx_olflags ? tx_olflags[i] : 0) */
	uint32_t       *rss;        /* optional u32[n]: hash ? hash[i] : 0 */
};
int gcl_copy_batch(struct gcl_ctx *ctx, const struct gcl_copy_in *in,
                   const struct gcl_copy_out *out, uint64_t *counts, void *hip_stream);

/*
 * Socket demux: trans_lookup (runtime/net/transport.c:341-397), the step that
 * ends the receive path.  Every TCP or UDP frame net_rx_one hands to
 * net_rx_trans is matched against the receiving runtime's 5-tuple entries
 * (its connections), then its 3-tuple entries (its listeners), then its
 * listeners bound to address 0.  The classify kernel's GCL_CFG_TRANS_HASH
 * gives a runtime the two bucket hashes; the runtime still walks its hash
 * chains for every packet on its own cores, and the 2- and 1-byte verdict
 * contexts have no hashes at all.  gcl_sock_lookup makes the whole lookup for
 * a classified batch on the GPU, on every context: sock[i] is the cookie (the
 * runtime's own name) of the entry trans_lookup would return for packet i.
 *
 * The table.  A context holds a set of entries per runtime, exact-match on
 * (uniqid, match, proto, laddr[, raddr]), hashed by a hash of the library's
 * own: the result depends on the keys only, never on trans_seed.
 *
 * gcl_sock_set - replace the whole entry set of runtime @uniqid (@n == 0
 *   clears it); on any error the previous set stays in place.  Works on every
 *   context, whatever its verdict width, and needs no GCL_CFG_TRANS_HASH.
 *   -ENOENT: the runtime is not present.  -EINVAL: a NULL ctx, a NULL @e with
 *   @n > 0, lport == 0 (port zero is reserved, transport.c:185), a match
 *   other than GCL_SOCK_MATCH_*, a proto other than 6 or 17, or a cookie
 *   above GCL_SOCK_COOKIE_MAX.  -EADDRINUSE: two 5-tuple entries with the
 *   same key (the conflict check of __trans_table_add, transport.c:202-214).
 *   -ENOSPC: the context would hold more than GCL_SOCK_MAX_ENTRIES, or the
 *   table could not place every key (not seen at its load of <= 1/2).
 *   -ENOMEM.  Several 3-tuple entries with the same key are allowed: they are
 *   the reference's reuse_port listeners, among which trans_lookup picks by
 *   this_thread_id() (transport.c:392-396); a lookup that matches them
 *   answers GCL_SOCK_MULTI and the runtime makes that choice itself.
 *   rip, rport and pad of a 3-tuple entry are ignored.
 *   gcl_runtime_del drops the runtime's entries.  Changes are applied on the
 *   stream of the next gcl_sock_lookup, before its kernel (the snapshot
 *   semantics of the runtime tables); the classify tables and their upload
 *   are not touched.
 *
 * gcl_sock_lookup - asynchronous on @hip_stream.  Frames are addressed
 *   exactly as gcl_rx_csum addresses them (frames, frames_len, stride or offs
 *   at any byte alignment; a byte at or past frames_len reads 0, an offset at
 *   or past frames_len is a frame of zeros); the side arrays of @b are
 *   ignored.  @verdicts is a device array in the context's own width (8, 4, 2
 *   or 1 B) as gcl_classify wrote it, aligned to its element; @sock a device
 *   u32[n], 4-B aligned; @counts a device u64[GCL_SOCK_NR], ACCUMULATED, may
 *   be NULL; per call the six counters sum to n.
 *
 *   Packet i.  u is the verdict's runtime for a DELIVER or WAKE verdict:
 *   uniqid (8- and 4-byte verdicts), or q >> thread_bits of the 2- and 1-byte
 *   forms (gcl_verdict2_to4 / gcl_verdict1_to4, gcl_host.h).
 *     GCL_SOCK_NA (N_NA) when the verdict is any other action (the undefined
 *       2-B kind 0x8000 included), when u >= max_runtimes, or when the frame
 *       fails the predicate that sets GCL_ACT_F_TRANS (struct gcl_trans):
 *       bytes 12-13 0x0800, version 4, IHL 5, the MF test of ip_hdr_supported
 *       as written, protocol 6 or 17.
 *     Otherwise, as transport.c:361-391, with proto = byte 23, laddr = (bytes
 *       30-33, bytes 36-37) and raddr = (bytes 26-29, bytes 34-35) in host
 *       order, the first of:
 *         the cookie of u's 5-tuple entry (proto, laddr, raddr)      HIT5
 *         the cookie of u's 3-tuple entry (proto, laddr)             HIT3
 *         the cookie of u's 3-tuple entry (proto, (0, laddr.port))   HIT3_ANY
 *         GCL_SOCK_MISS (trans_lookup returns NULL)                  N_MISS
 *       A 3-tuple step that finds several listeners on its key answers
 *       GCL_SOCK_MULTI, counted N_MULTI and not as a hit, and ends the
 *       search as transport.c:384-396 does.
 *
 *   Guarantee: no content of frames, offs, verdicts or the entries causes a
 *   read outside frames[0, frames_len), the n-element arrays or the table
 *   image, or a write outside sock[0, n).  A lookup reads a fixed number of
 *   table words (twelve 16-B keys and one cookie).
 *
 *   No allocation and no host synchronisation beyond the table upload after
 *   a change.  n == 0 is a no-op.  -EINVAL for a NULL ctx, b, verdicts or
 *   sock, a misaligned verdicts or sock, and the batches gcl_rx_csum refuses;
 *   -ENOMEM or -EIO when the table upload fails, -EIO when the launch fails.
 */
#define GCL_SOCK_MATCH_3TUPLE 3   /* listener: (proto, laddr)            */
#define GCL_SOCK_MATCH_5TUPLE 5   /* connection: (proto, laddr, raddr)   */
#define GCL_SOCK_MAX_ENTRIES (1u << 20)   /* per context, all runtimes   */
#define GCL_SOCK_NA    0xFFFFFFFFu  /* not a packet net_rx_trans sees     */
#define GCL_SOCK_MISS  0xFFFFFFFEu  /* trans_lookup returns NULL          */
#define GCL_SOCK_MULTI 0xFFFFFFFDu  /* >= 2 listeners share the 3-tuple   */
#define GCL_SOCK_COOKIE_MAX 0xFFFFFFEFu
struct gcl_sock_entry {            /* host order, as struct netaddr      */
	uint32_t lip, rip;             /* rip/rport ignored for 3TUPLE       */
	uint16_t lport, rport;
	uint8_t  proto;                /* 6 or 17                            */
	uint8_t  match;                /* GCL_SOCK_MATCH_*                   */
	uint16_t pad;
	uint32_t cookie;               /* the runtime's own name for the entry */
};
int gcl_sock_set(struct gcl_ctx *ctx, uint16_t uniqid, const struct gcl_sock_entry *e, uint32_t n);

enum {
	GCL_SOCK_HIT5 = 0,    /* a connection */
	GCL_SOCK_HIT3,        /* a listener on the packet's own address */
	GCL_SOCK_HIT3_ANY,    /* a listener on address 0 */
	GCL_SOCK_N_MULTI,
	GCL_SOCK_N_MISS,
	GCL_SOCK_N_NA,
	GCL_SOCK_NR = 8,      /* padded */
};
int gcl_sock_lookup(struct gcl_ctx *ctx, const struct gcl_batch *b, const void *verdicts,
                    uint32_t *sock, uint64_t *counts, void *hip_stream);

/*
 * Payload descriptors and a packed receive layout: the step that ends the
 * receive path in the reference.  Once trans_lookup has an entry,
 * udp_conn_recv / udp_par_recv pull the 8-byte UDP header and hand on
 * mbuf_data, mbuf_length -- frame bytes [42, 14 + tot) after net_rx_one's trim
 * (runtime/net/udp.c:79-107, :811-840, runtime/net/core.c:283-287);
 * tcp_rx_conn reads seq, ack, the flags and hdr_len = off * 4, drops
 * hdr_len < 20 and takes len = tot - 20 - hdr_len bytes behind the header
 * (runtime/net/tcp_in.c:182-218); udp_read_from / tcp_read then memcpy those
 * bytes into the application's buffer on a runtime core (udp.c:373-379).
 * gcl_l4_payload says, for every entry of a list of packets, where the
 * payload starts, how long it is and where it goes in a dense receive buffer:
 * the src_off[], len[] and dst_off[] that gcl_copy_batch takes, so that the
 * chain classify -> sock_lookup -> l4_csum VERIFY -> plan -> l4_payload ->
 * copy_batch leaves, per runtime, one dense payload stream in HBM plus a
 * descriptor per datagram.  tcp_rx_conn's state machine (sequence checks,
 * reassembly, ACKs) stays with the runtime: meta[] carries what it reads.
 *
 * List entry j names packet i = in->order ? in->order[j] : j.  Packet i has
 * o, avail and L = min(b->pkt_len[i], avail) exactly as gcl_l4_csum defines
 * them, and is L4-eligible exactly as there (b->pkt_len is REQUIRED).  The
 * first line that matches decides:
 *   i >= b->n                                              GCL_PAY_OOR
 *   the packet is not L4-eligible                          GCL_PAY_NA
 *   TCP with hl = 4 * (byte 46 >> 4), when hl < 20 or
 *     hl > tot - 20 (UDP has hl = 8)                       GCL_PAY_NA
 *   in->l4_status given and (l4_status[i] & 0xF) ==
 *     GCL_L4_BAD (the FILLED bits are ignored)             GCL_PAY_BADCSUM
 *   in->sock given and sock[i] > GCL_SOCK_COOKIE_MAX
 *     (NA, MISS, MULTI, the reserved values)               GCL_PAY_NOSOCK
 *   otherwise the entry is KEPT: kind[j] is GCL_PAY_UDP or GCL_PAY_TCP,
 *     len[j] = tot - 20 - hl (it may be 0: a pure ACK, an empty datagram),
 *     src_off[j] = o + 34 + hl, an offset into b->frames that lies inside
 *     [o, o + L] and is directly usable as gcl_copy_in.src_off, and meta[j]
 *     is filled from the frame.
 * Every entry that is not kept gets len = 0, src_off = 0 and an all-zero meta
 * (proto 0).
 *
 * The layout, with pad(x) = x rounded up to in->align (0 or 1: dense):
 *   dst_off[j]   = the sum of pad(len[j']) over j' < j
 *   *total       = that sum over all m entries
 *   seg_bytes[s] = seg_off[s] < m ? dst_off[seg_off[s]] : *total, s <= nseg
 * With a plan's order and seg_off = its bucket_off (nseg = nbuckets),
 * runtime r's stream is therefore bytes [seg_bytes[r], seg_bytes[r + 1]) of
 * the receive buffer.  Garbage in seg_off gives garbage values, never a read
 * out of range.  The copy that follows is
 *   gcl_copy_in  { .src = b->frames, .src_len = b->frames_len,
 *                  .src_off = out->src_off, .len = out->len, .n = m }
 *   gcl_copy_out { .dst_off = out->dst_off, ... }.
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * meta to 16 B.  @counts is a device u64[GCL_PAYC_NR], ACCUMULATED, may be
 * NULL: per call the six kind counters sum to m, and BYTES adds the unpadded
 * len of every entry.  Frames are addressed as gcl_rx_csum addresses them;
 * rss, fdir_hi, dst_hint and olflags are ignored.
 *
 * Guarantee: no content of frames, offs, pkt_len, order, sock, l4_status or
 * seg_off causes a read outside frames[0, frames_len) or the given arrays
 * (order[0, m), seg_off[0, nseg], the n-element per-packet arrays), or a
 * write outside the m-element outputs, seg_bytes[0, nseg], total and counts.
 *
 * gcl_l4_payload_workspace - bytes of device scratch a call takes: one u64
 *   per contiguous range the list is cut into (in->blocks of them, or the
 *   cap GCL_PAY_MAX_BLOCKS when in->blocks is 0).  -EINVAL for a NULL @bytes,
 *   m > 2^31 or blocks > GCL_PAY_MAX_BLOCKS.
 * gcl_l4_payload - asynchronous on @hip_stream: three launches (four with
 *   seg_off), none of which waits for another block.  No allocation, no host
 *   synchronisation.  @workspace (device, 16-B aligned) need not be zeroed and
 *   may be reused by the next call on the same stream.  m == 0 writes
 *   *total = 0 and zero seg_bytes, and nothing else.  -EINVAL for a NULL ctx,
 *   b, in or out; a wrong in->size; an align that is not 0 or a power of two
 *   <= 256; order == NULL with m != b->n; m > 2^31; a NULL src_off, len,
 *   dst_off, kind or total; seg_off without seg_bytes or seg_bytes without
 *   seg_off; any given array that is not aligned to its element (meta: 16 B);
 *   blocks > GCL_PAY_MAX_BLOCKS; a NULL workspace, one that is not 16-B
 *   aligned or one smaller than gcl_l4_payload_workspace says; and, when
 *   m > 0, a NULL or misaligned b->pkt_len and the batches gcl_rx_csum
 *   refuses.  -EIO when a launch fails.
 */
/* kind[j] */
#define GCL_PAY_NA      0  /* not a datagram this call describes */
#define GCL_PAY_UDP     1
#define GCL_PAY_TCP     2
#define GCL_PAY_NOSOCK  3  /* in->sock given and sock[i] > GCL_SOCK_COOKIE_MAX */
#define GCL_PAY_BADCSUM 4  /* in->l4_status given and (l4_status[i] & 0xF) == GCL_L4_BAD */
#define GCL_PAY_OOR     5  /* order[j] >= n */
#define GCL_PAY_MAX_BLOCKS 1024  /* the cap on in->blocks */
enum { GCL_PAYC_UDP = 0, GCL_PAYC_TCP, GCL_PAYC_NA, GCL_PAYC_NOSOCK, GCL_PAYC_BADCSUM,
       GCL_PAYC_OOR, GCL_PAYC_BYTES, GCL_PAYC_NR = 8 };
struct gcl_pay_meta {            /* 16 B, host order */
	uint32_t rip;                /* the sender: frame bytes 26-29 */
	uint16_t rport;              /* bytes 34-35 */
	uint8_t  proto;              /* 6 or 17; 0: the entry is not kept */
	uint8_t  tcp_flags;          /* byte 47, 0 for UDP */
	uint32_t seq, ack;           /* TCP bytes 38-41, 42-45; 0 for UDP */
};
struct gcl_pay_in {
	uint32_t size, align;        /* sizeof(struct gcl_pay_in); align: 0 or 1 = dense, else a
	                                power of two <= 256 */
	const uint32_t *order;       /* optional u32[m]; NULL: m == b->n and i = j */
	uint64_t m;                  /* list entries, <= 2^31 */
	const uint32_t *sock;        /* optional u32[n], as gcl_sock_lookup wrote it */
	const uint8_t  *l4_status;   /* optional u8[n], as GCL_L4_VERIFY wrote it */
	const uint32_t *seg_off;     /* optional u32[nseg + 1], e.g. a plan's bucket_off */
	uint32_t nseg;
	uint32_t blocks;             /* 0: the library's choice; else the number of contiguous
	                                list ranges the scan is cut into (tests) */
};
struct gcl_pay_out {             /* device; m entries each, aligned to their element */
	uint64_t *src_off;           /* required */
	uint16_t *len;               /* required */
	uint64_t *dst_off;           /* required */
	uint8_t  *kind;              /* required */
	struct gcl_pay_meta *meta;   /* optional, 16-B aligned */
	uint64_t *seg_bytes;         /* u64[nseg + 1], required iff seg_off */
	uint64_t *total;             /* u64[1], required */
};
int gcl_l4_payload_workspace(uint64_t m, uint32_t blocks, size_t *bytes);
int gcl_l4_payload(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_pay_in *in,
                   const struct gcl_pay_out *out, uint64_t *counts,
                   void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * Transmit headers: what the runtime does to a segment between its socket and
 * its txpkt queue, for a batch whose payloads already sit in the tx region
 * behind their headroom.  udp_send_raw (runtime/net/udp.c:24-40) or
 * __tcp_add_tcphdr (runtime/net/tcp_out.c:54-81) writes the L4 header,
 * net_tx_ip (runtime/net/core.c:686-737) the IPv4 header, the route, the ARP
 * hit (arp_lookup's hot path, runtime/net/arp.c:331-344), the loopback hint
 * and through net_tx_eth (core.c:581-590) the Ethernet header, and
 * net_tx_iokernel (core.c:504-538) the padding, the txpkt_xmit_cmd and its
 * payload word.  gcl_tx_hdr does all of that for m segments of one runtime on
 * the GPU.  The transmit chain on one stream:
 *
 *   gcl_copy_batch (payloads to their place behind the headroom)
 *   -> gcl_tx_hdr -> gcl_l4_csum GCL_L4_FILL (offs = frame_off, pkt_len and
 *   tx_olflags as written here) -> the NIC, or gcl_copy_batch (src_off =
 *   frame_off, len = pkt_len, tx_olflags, hash) + gcl_classify for frames to
 *   a runtime on the same machine.
 *
 * The neighbour table is a context's ARP cache.  gcl_neigh_set replaces the
 * whole set (n == 0 clears it); an entry stands for an arp_entry whose state
 * is not ARP_STATE_PROBING: only resolved addresses are given.  -EINVAL for a
 * NULL ctx, or a NULL @e with n > 0; -EEXIST when two entries share their ip;
 * -ENOSPC for more than GCL_NEIGH_MAX_ENTRIES or when the placement failed;
 * -ENOMEM.  On any error the previous set stays in place.  A change reaches
 * the device on the stream of the next gcl_tx_hdr, before its kernel (the
 * snapshot semantics of gcl_sock_set); the classify and socket tables and
 * their uploads are not touched.  It works on every context, whatever its
 * verdict width.
 *
 * Entry j, with o = frame_off[j], hl = 8 for UDP and 4 * tcp_off for TCP,
 * tot = 20 + hl + paylen, len = 14 + tot and elen = max(len,
 * net.min_pkt_size); the first status that matches decides:
 *
 *   GCL_TXH_REFUSED when proto is not 6 or 17, when the segment is TCP and
 *     tcp_off is outside 5..15, when len > 65535, when cap != 0 and
 *     elen > cap, or when o > frames_len or elen > frames_len - o (no sum is
 *     formed, so any o is judged rightly).  No frame byte is written; cmd =
 *     payload = 0, pkt_len = 0, tx_olflags = 0, hash = 0.
 *   Otherwise the L4 and IP headers are written.  saddr = lip, or when lip is
 *     0: 127.0.0.1 if rip is 127.0.0.1, else net.addr (core.c:693-698).
 *     UDP, bytes 34-41: sport, dport, hton16(paylen + 8), checksum 0.
 *     TCP, bytes 34-53: sport, dport, seq, ack, off << 4, flags, win, the
 *     non-complemented ipv4_phdr_cksum(6, saddr, rip, hl + paylen) as
 *     inc/net/chksum.h:110-126 stores it (the value the runtime leaves for
 *     the NIC, and the one FILL overwrites), urgent 0.  Bytes [54, 34 + hl),
 *     the options, are the caller's and are NOT written.
 *     IPv4, bytes 14-33: 0x45, tos = has_ecn ? ecn & 3 : 0, hton16(tot),
 *     id 0, hton16(IP_DF), ttl 64, the protocol, checksum 0 (ipv4_cksum with
 *     GCL_TXH_IP_CSUM), saddr, daddr = rip.
 *   GCL_TXH_SELF when rip == net.addr or rip is 127.0.0.1
 *     (net_tx_local_loopback, core.c:705-706: the runtime handles the segment
 *     itself).  The Ethernet header is not written; cmd = payload = 0,
 *     pkt_len = len, tx_olflags = 0, hash = 0.
 *   Otherwise nh = rip when (rip & netmask) == (addr & netmask), else gateway,
 *     and nh is looked up in the neighbour table.
 *   GCL_TXH_NONEIGH on a miss (the -EINPROGRESS path: the host's ARP code
 *     takes the frame).  The Ethernet header is not written; cmd = payload =
 *     0, pkt_len = len, hash = 0, tx_olflags = IP_CHKSUM | IPV4 | (TCP ?
 *     TCP_CHKSUM : 0) (core.c:709 sets them before the lookup).
 *   GCL_TXH_OK on a hit.  Bytes 0-13: dhost = the entry's mac, shost =
 *     net.mac, type 0x0800.  local = (mac == net.mac) (is_local, arp.c:62-65);
 *     tx_olflags is the flags above plus TXFLAG_LOCAL | TXFLAG_LOCAL_HINT when
 *     local.  When local, hash = do_toeplitz(net.addr, nh, lport, rport) with
 *     the context's cfg.rss_key (net.addr, not saddr, as core.c:730) and
 *     dst_ip = nh; else hash = 0 and dst_ip = 0.  When len < min_pkt_size,
 *     bytes [len, min_pkt_size) become 0 and pkt_len = min_pkt_size
 *     (core.c:513-517); else pkt_len = len.  cmd = dst_ip | (u64)pkt_len << 32
 *     | (u64)tx_olflags << 48 (txcmd is TXPKT_NET_XMIT = 0: the top bit is
 *     clear); payload = (shm_base + o) | (u64)(hash & 0xFFFF) << 48.
 *
 * @counts is a device u64[GCL_TXHC_NR], ACCUMULATED, may be NULL: OK, SELF,
 * NONEIGH, REFUSED, LOCAL (the OK entries that got the hint) and BYTES
 * (pkt_len of the OK entries); per call the first four sum to m.
 *
 * Guarantee: no content of desc, frame_off or the table causes a read outside
 * the m-element arrays or the table image, or a write outside the m-element
 * outputs, counts and the bytes named above, which lie inside [o, o + elen) of
 * a frame that was not refused.  The TCP option bytes, the payload behind the
 * header and every byte outside the frame are not written, not even with the
 * value they already had: neighbouring frames belong to other lanes, so each
 * store has the width of what it writes or less and no wider word is
 * read-modify-written (gcl_copy_batch's discipline).  Frames that overlap are
 * the caller's error; nothing is written out of bounds even so.
 *
 * Asynchronous on @hip_stream; no allocation and no host synchronisation
 * beyond the table upload after a change.  m == 0 is a no-op.  -EINVAL for a
 * NULL ctx, in, out, desc, frame_off, frames, cmd, payload, pkt_len,
 * tx_olflags or status; a wrong in->size; m > 2^31; frames_len == UINT64_MAX;
 * an array that is not aligned to its element (desc: 16 B).  -EIO when the
 * launch fails; -ENOMEM or -EIO when the table upload fails.
 */
#define GCL_NEIGH_MAX_ENTRIES (1u << 16)
struct gcl_neigh_entry { uint32_t ip; uint8_t mac[6]; uint16_t pad; };  /* ip in host order */
int gcl_neigh_set(struct gcl_ctx *ctx, const struct gcl_neigh_entry *e, uint32_t n);

/* status[j] and the first four counter slots */
#define GCL_TXH_OK       0
#define GCL_TXH_SELF     1
#define GCL_TXH_NONEIGH  2
#define GCL_TXH_REFUSED  3
enum { GCL_TXHC_OK = 0, GCL_TXHC_SELF, GCL_TXHC_NONEIGH, GCL_TXHC_REFUSED, GCL_TXHC_LOCAL,
       GCL_TXHC_BYTES, GCL_TXHC_NR = 8 };
#define GCL_TXH_IP_CSUM  0x01    /* gcl_txh_net.flags */
struct gcl_txh_desc {          /* 32 B, 16-B aligned, host order: what the runtime knows of a segment */
	uint32_t lip, rip;         /* laddr.ip (0: see above), raddr.ip */
	uint16_t lport, rport;
	uint8_t  proto;            /* 6 or 17 */
	uint8_t  tcp_flags;        /* TCP byte 13; ignored for UDP */
	uint8_t  tcp_off;          /* TCP data offset in words, 5..15; ignored for UDP */
	uint8_t  ecn;              /* bit 7: has_ecn; bits 0-1: the ECN codepoint (core.c:602-606) */
	uint32_t seq, ack;         /* TCP; ignored for UDP */
	uint16_t win;              /* TCP window as it goes on the wire (already scaled) */
	uint16_t paylen;           /* bytes behind the L4 header (UDP: behind its 8 B; TCP: behind 4 * tcp_off) */
	uint32_t pad;
};
struct gcl_txh_net {           /* one runtime's netcfg */
	uint32_t addr, netmask, gateway;   /* host order */
	uint8_t  mac[6];
	uint8_t  min_pkt_size;     /* netcfg.min_pkt_size, 0 = none */
	uint8_t  flags;            /* GCL_TXH_IP_CSUM: write ipv4_cksum into the header (netcfg.no_tx_offloads) */
};
struct gcl_txh_in {
	uint32_t size, pad;                /* sizeof(struct gcl_txh_in) */
	const struct gcl_txh_desc *desc;   /* device [m] */
	const uint64_t *frame_off;         /* device u64[m]: where each frame's Ethernet header starts in @frames, any byte alignment */
	uint64_t m;                        /* <= 2^31 */
	uint8_t *frames; uint64_t frames_len;   /* the tx region (device) */
	uint64_t shm_base;                 /* payload[j] = shm_base + frame_off[j] | hash16 << 48 */
	uint32_t cap;                      /* a frame longer than this is refused; 0 = no cap of its own */
	uint32_t pad2;
	struct gcl_txh_net net;
};
struct gcl_txh_out {                   /* device, m entries each, aligned to their element */
	uint64_t *cmd;       /* required: txpkt_xmit_cmd.lrpc_cmd (inc/iokernel/queue.h:82-93) */
	uint64_t *payload;   /* required: txpkt_to_payload(shmptr, (uint16_t)hash) (queue.h:120-124) */
	uint16_t *pkt_len;   /* required: cmd.len; with frame_off it is gcl_batch.offs/pkt_len of FILL and src_off/len of gcl_copy_batch */
	uint8_t  *tx_olflags;/* required: cmd.olflags, the tx_olflags of gcl_l4_in and gcl_copy_in */
	uint32_t *hash;      /* optional: m->hash (gcl_copy_in.hash) */
	uint8_t  *status;    /* required */
};
int gcl_tx_hdr(struct gcl_ctx *ctx, const struct gcl_txh_in *in, const struct gcl_txh_out *out,
               uint64_t *counts, void *hip_stream);

/*
 * Transmit segmentation: the first step of the transmit chain.  A runtime that
 * writes to a socket cuts the bytes into segments on a core, one write at a
 * time: tcp_write3 clamps the length to the send window (runtime/net/tcp.c:
 * 1362-1380) and "the main TCP segmenter loop" of tcp_tx_send cuts it into
 * mss-sized segments, the last one pushed (runtime/net/tcp_out.c:313-386);
 * udp_write_to refuses a datagram above udp_get_payload_size() and sends one
 * segment (runtime/net/udp.c:590-591).  gcl_tx_seg does that for m writes of
 * one runtime on the GPU and writes, per segment and in send order, the inputs
 * of the calls that follow:
 *
 *   gcl_tx_seg -> gcl_copy_batch (src = the writers' buffers; src_off, len and
 *   dst_off as written here) -> gcl_tx_hdr (desc and frame_off as written
 *   here) -> gcl_l4_csum GCL_L4_FILL -> the NIC or the loopback.
 *
 * It works on every context, whatever its verdict width, and touches no table.
 *
 * The rule for write i is the closed form of the reference's loop with
 * push == true (tcp_write3 always passes it) and no tx_pending:
 *   TCP (proto 6): L = min(len, winlen), nseg = max(1, ceil(L / mss)): the loop
 *     is a do ... while, so L == 0 still sends one empty ACK|PSH segment and
 *     the write returns 0.  Segment k has seq = snd_nxt + k * mss (mod 2^32),
 *     paylen = min(mss, L - k * mss), tcp_off = 5, tcp_flags = ACK (0x10), plus
 *     PSH (0x08) on the last segment; ack, win and ecn are the write's.
 *   UDP (proto 17): L = len, nseg = 1, one datagram of L bytes (L == 0 is a
 *     valid empty datagram); tcp_flags, tcp_off, seq, ack and win are 0.
 *   GCL_SEG_REFUSED when proto is not 6 or 17; for TCP when mss == 0; for UDP
 *     when len > udp_max (the runtime's -EMSGSIZE); and with slots (below) when
 *     the write's largest frame does not fit one:
 *     lead + 34 + hl + min(L, mss) > stride (UDP: L for min(L, mss); hl is 20
 *     for TCP, 8 for UDP).  A refused write has no segments.
 *
 * The frame layout, both forms taken from one scan.  Every write that is not
 * refused has a segment count n_i = nseg above and layout bytes w_i:
 *   slots (stride != 0): w_i = n_i * stride, and
 *     frame_off[g] = frame_base + g * stride + lead.
 *   packed (stride == 0): frames go back to back, each padded to 16 B:
 *     w_i = the sum of pad16(34 + hl + paylen) over the write's segments, and
 *     segment k of write i lies at frame_base + lead + B_i +
 *     k * pad16(34 + hl + mss) (all segments of a write but the last have the
 *     same length).
 * S_i and B_i are the sums of n and w over the writes before i that were not
 * refused.  Write i, not refused, is GCL_SEG_NOSPACE when
 *   S_i + n_i > seg_cap, or, when frames_len != 0, its frames would end past
 *   it: B_i + w_i > frames_len - frame_base - (packed: lead), a test made
 *   without forming a sum that can wrap (a frames_len below frame_base, or
 *   below frame_base + lead when packed, leaves no room at all).
 * Both sums count the NOSPACE writes too and only grow, so the NOSPACE writes
 * are a suffix of the writes that were not refused: once one write does not
 * fit, no later one is sent, as a runtime stops at a full queue.  A NOSPACE
 * write writes no segment at all.  Otherwise the write is GCL_SEG_OK.
 *
 * Per-write outputs (m entries): status; sent = L and snd_nxt_out = snd_nxt + L
 * (mod 2^32) for an OK write, sent = 0 and snd_nxt_out = snd_nxt otherwise
 * (for UDP snd_nxt is just carried); nseg = the segments written for the write
 * (n_i when OK, else 0); seg_first = min(S_i, seg_cap): where the write's
 * segments start.  It never decreases with i, and for the OK writes it is
 * exact.
 * *total_segs = the sum of nseg[]: the m to give the three calls that follow.
 * *total_bytes = the sum of w_i over the OK writes (slots: *total_segs *
 * stride): the next frame would start at frame_base + *total_bytes (+ lead).
 *
 * Per-segment outputs, for g = seg_first[i] + k of an OK write i:
 *   desc[g]     a full gcl_txh_desc: the write's tuple and ecn, the fields
 *               above, paylen, pad 0.
 *   frame_off[g] as the layout says (mod 2^64 when frames_len == 0 and the
 *               caller's frame_base is absurd).
 *   src_off[g]  = send.src_off + k * mss, a u64 sum mod 2^64 (gcl_copy_batch
 *               reads an offset past its src_len as zeros).
 *   len[g]      = paylen.
 *   dst_off[g]  = frame_off[g] + 14 + 20 + hl.
 *   send_idx[g] = i (optional: lets a completion find its write).
 * Entries at and past *total_segs are not written, not even with the value
 * they had.  gcl_tx_hdr refuses a frame above 65535 bytes: a TCP segment whose
 * mss exceeds 65481 comes out of this call and is refused there.
 *
 * @counts is a device u64[GCL_SEGC_NR], ACCUMULATED, may be NULL: OK, REFUSED
 * and NOSPACE writes (per call the three sum to m), SEGS (*total_segs), BYTES
 * (the sum of sent[]) and PUSH (segments carrying PSH: one per OK TCP write).
 *
 * Guarantee: no content of the writes causes a read outside send[0, m) or the
 * workspace, or a write outside the first min(*total_segs, seg_cap) entries of
 * the per-segment arrays, the m-element per-write arrays, the two totals,
 * counts and the workspace.
 *
 * Out of scope, and left with the runtime: push == false and tx_pending (the
 * held tail of tcp_writev2's inner iovecs), retransmission, the SYN, FIN and
 * RST segments, tx_exclusive and the wait queues.  Several writes of one
 * connection may share a batch only when the caller gives each its own
 * snd_nxt (and winlen): the call does not chain them.
 *
 * gcl_tx_seg_workspace - bytes of device scratch a call takes: 16 per write
 *   plus 32 per contiguous range the writes are cut into (in->blocks of them,
 *   or the cap GCL_SEG_MAX_BLOCKS when blocks is 0) plus 16.  -EINVAL for a
 *   NULL @bytes, m > 2^31 or blocks > GCL_SEG_MAX_BLOCKS.
 * gcl_tx_seg - asynchronous on @hip_stream: four launches ordered by the
 *   stream alone; no block waits for another.  No allocation, no host
 *   synchronisation.  @workspace (device, 16-B aligned) need not be zeroed and
 *   may be reused by the next call on the same stream.  m == 0 writes the two
 *   totals as 0 and nothing else.  -EINVAL for a NULL ctx, in or out; a wrong
 *   in->size; m or seg_cap > 2^31; stride > 2^20; lead > 65535; udp_max >
 *   65507; blocks > GCL_SEG_MAX_BLOCKS; a NULL total_segs or total_bytes; with
 *   m > 0 a NULL send, status, sent, snd_nxt_out, seg_first or nseg; with m > 0
 *   and seg_cap > 0 a NULL desc, frame_off, src_off, len or dst_off; any given
 *   array that is not aligned to its element (send and desc: 16 B); a NULL
 *   workspace, one that is not 16-B aligned or one smaller than
 *   gcl_tx_seg_workspace says.  -EIO when a launch fails.
 */
/* status[i] and the first three counter slots */
#define GCL_SEG_OK       0
#define GCL_SEG_REFUSED  1
#define GCL_SEG_NOSPACE  2
#define GCL_SEG_MAX_BLOCKS 1024  /* the cap on in->blocks */
enum { GCL_SEGC_OK = 0, GCL_SEGC_REFUSED, GCL_SEGC_NOSPACE, GCL_SEGC_SEGS, GCL_SEGC_BYTES,
       GCL_SEGC_PUSH, GCL_SEGC_NR = 8 };
struct gcl_seg_send {          /* 48 B, 16-B aligned, host order: one socket write */
	uint32_t lip, rip;         /* as in gcl_txh_desc */
	uint16_t lport, rport;
	uint8_t  proto;            /* 6 or 17 */
	uint8_t  ecn;              /* as in gcl_txh_desc */
	uint16_t mss;              /* TCP: pcb.snd_mss */
	uint32_t snd_nxt, ack;     /* TCP: pcb.snd_nxt, tx_last_ack */
	uint16_t win, pad;         /* TCP: the window as __tcp_add_tcphdr would write it */
	uint32_t len;              /* the write's length */
	uint32_t winlen;           /* TCP: snd_una + snd_wnd - snd_nxt; ignored for UDP */
	uint32_t pad2;
	uint64_t src_off;          /* where the write's bytes start in the source region of the later gcl_copy_batch */
};
struct gcl_seg_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_seg_in); blocks: 0 = the library's choice, else
	                                      the number of contiguous ranges the scan is cut into (tests) */
	const struct gcl_seg_send *send;   /* device [m] */
	uint64_t m;                        /* <= 2^31 */
	uint64_t seg_cap;                  /* <= 2^31: the length of every per-segment output array */
	uint64_t frame_base;               /* where the layout starts in the tx region */
	uint64_t frames_len;               /* the tx region's length; 0: no limit */
	uint32_t stride;                   /* != 0: slots of this many bytes; 0: packed */
	uint32_t lead;                     /* bytes in front of every frame (slots) or of the first (packed) */
	uint32_t udp_max;                  /* udp_get_payload_size() */
	uint32_t pad;
};
struct gcl_seg_out {                   /* device, aligned to their element */
	uint8_t  *status;                  /* [m] */
	uint32_t *sent, *snd_nxt_out, *seg_first, *nseg;   /* [m] */
	struct gcl_txh_desc *desc;         /* [seg_cap], 16-B aligned */
	uint64_t *frame_off, *src_off;     /* [seg_cap] */
	uint16_t *len;                     /* [seg_cap] */
	uint64_t *dst_off;                 /* [seg_cap] */
	uint32_t *send_idx;                /* [seg_cap], optional */
	uint64_t *total_segs, *total_bytes;/* u64[1] each, required */
};
int gcl_tx_seg_workspace(uint64_t m, uint32_t blocks, size_t *bytes);
int gcl_tx_seg(struct gcl_ctx *ctx, const struct gcl_seg_in *in, const struct gcl_seg_out *out,
               uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * TCP receive, the established fast path: the step behind gcl_l4_payload for
 * TCP.  tcp_rx_conn (runtime/net/tcp_in.c:172-296) is written as a fast path:
 * an established connection, the next in-order segment, one that fits the
 * receive window, no FIN / RST / URG; everything else leaves through
 * __tcp_rx_conn.  Under the connection lock it compares seq with rcv_nxt,
 * moves the windows and counts delayed ACKs, once per segment on a core.
 * gcl_tcp_rx runs every connection's segments of one runtime's list, in
 * arrival order, through that fast path on the GPU, and lays the bytes each
 * connection accepted out contiguously and in sequence order:
 *
 *   gcl_classify -> gcl_sock_lookup -> gcl_l4_csum VERIFY -> gcl_plan ->
 *   gcl_l4_payload -> gcl_tcp_rx -> gcl_copy_batch (src_off from
 *   gcl_l4_payload; len = copy_len and dst_off from this call).
 *
 * A connection stops at its first segment that needs __tcp_rx_conn; the
 * runtime gets, per connection, the new PCB words, a byte range and the list
 * position of the first segment it must still look at itself.  One call
 * serves ONE runtime, because cookies are per runtime (as gcl_tx_hdr serves
 * one): @in->order / m are that runtime's range of a plan, @in->conn its
 * connections indexed by cookie.  It works on every context and touches no
 * table.
 *
 * List entry j names packet i = in->order ? in->order[j] : j.  It is a TCP
 * SEGMENT exactly when gcl_l4_payload, given the same sock and l4_status,
 * keeps it as GCL_PAY_TCP (the very function decides, gcl_pay_rule), with
 * c = sock[i] its connection; len is gcl_l4_payload's len, and seq, ack, flags
 * and win are frame bytes 38-41, 42-45, 47 and 48-49 (a kept TCP entry has
 * L >= 54).  The verdict of entry j is the first line that matches, the
 * entries of a connection taken in list order:
 *   not a TCP segment (OOR, NA, UDP, BADCSUM, NOSOCK)       GCL_TCPRX_NA
 *   c >= nconn                                               GCL_TCPRX_NOCONN
 *   len > conn[c].rcv_mss (tcp_in.c:207: freed before the
 *     lock is taken; it neither reads nor changes state and
 *     does not stop the connection)                          GCL_TCPRX_DROP
 *   the connection has stopped earlier in this call, or
 *     slow_path of :221-239 holds for its current state:
 *     flags & (FIN | RST | URG), len == 0,
 *     wraps_gt(ack, snd_nxt), not GCL_TCPC_ELIGIBLE,
 *     wraps_lte(snd_una + snd_wnd, snd_nxt), seq != rcv_nxt,
 *     rcv_wnd < len                                          GCL_TCPRX_SLOW
 *     (the first such segment STOPS the connection: its state
 *     is frozen as it stood before that segment)
 *   otherwise                                                GCL_TCPRX_FAST
 * SYN is not a slow-path flag and the ACK flag is not tested: both as in the
 * reference.  A FAST segment applies :246-287 to the connection's state:
 *   if wraps_lte(snd_una, ack):
 *     if snd_una != ack: snd_una = ack (sflags ACKED; rep_acks = 0)
 *     if wraps_lt(snd_wl1, seq) or (snd_wl1 == seq and wraps_lte(snd_wl2, ack)):
 *       snd_wnd = win << snd_wscale, snd_wl1 = seq, snd_wl2 = ack
 *       (sflags WND; rep_acks = 0)
 *   rcv_nxt += len, rcv_wnd -= len
 *   wake (sflags WAKE) when GCL_TCPC_RXQ is set or the segment carries PSH
 *   if ++acks_delayed_cnt >= 2: do_ack (sflags ACK_NOW), the counter 0 and
 *     ACK_DELAYED cleared; else if ACK_DELAYED is clear: it is set and the
 *     timer armed (out flags TIMER_ARMED)
 *   GCL_TCPC_RXQ is set (the mbuf joined rxq).
 * All arithmetic is mod 2^32 with the reference's wraps_* comparisons
 * ((int32_t)(a - b) < 0 and its kin); acks_delayed_cnt is taken as the
 * reference's int, so a counter of 1 or more on entry gives do_ack.
 *
 * Per-entry outputs (m elements each): verdict; sflags; rcv_nxt_after, the
 * number tcp_tx_ack would carry after a FAST segment, 0 otherwise; copy_len
 * and dst_off (below).  Per connection, out_conn[c] holds the six words that
 * move, acks_delayed_cnt and flags as they stand after the list, nfast / nslow
 * (FAST and SLOW verdicts of the connection) / nacks (ACK_NOW segments), and
 * first_slow, the list position j of the stopping segment or 0xFFFFFFFF.  A
 * connection with no segment in the list gets its input back with zero counts.
 *
 * The in-order layout, with pad() as in gcl_l4_payload and in->align:
 *   fast_bytes[c] = out_conn[c].rcv_nxt - conn[c].rcv_nxt (mod 2^32)
 *   conn_off[c]   = the sum of pad(fast_bytes[c']) over c' < c, c <= nconn:
 *                   conn_off[nconn] is the total
 *   a FAST entry:  copy_len = len, dst_off = conn_off[c] + (seq - conn[c].rcv_nxt)
 *   every other:   copy_len = 0,   dst_off = 0.
 * gcl_copy_batch with these then leaves connection c's accepted bytes at
 * [conn_off[c], conn_off[c] + fast_bytes[c]) in sequence order; the SLOW
 * entries stay reachable through gcl_l4_payload's own layout.
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * conn and out_conn to 16 B.  @counts is a device u64[GCL_TCPRXC_NR],
 * ACCUMULATED, may be NULL: FAST, SLOW, DROP, NOCONN and NA entries (per call
 * the five sum to m), BYTES (the sum of copy_len), ACKS (ACK_NOW) and WAKES.
 * Frames are addressed as gcl_l4_payload addresses them.
 *
 * Guarantee: no content of frames, offs, pkt_len, order, sock, l4_status or
 * conn causes a read outside frames[0, frames_len) or the given arrays
 * (order[0, m), the n-element per-packet arrays, conn[0, nconn)), or a write
 * outside the m-element outputs, out_conn[0, nconn), conn_off[0, nconn],
 * counts and the workspace.
 *
 * What stays with the runtime: all of __tcp_rx_conn (every SLOW segment and
 * what follows it on its connection), the out-of-order queue, tcp_conn_ack's
 * mbuf frees (ACKED says when), the wake-ups (WAKE), sending the ACKs
 * (ACK_NOW, with rcv_nxt_after), ack_ts and next_timeout (TIMER_ARMED), the
 * timers, and the lock: conn must be a snapshot no core changes meanwhile.
 *
 * gcl_tcp_rx_workspace - bytes of device scratch a call takes for m entries,
 *   nconn connections and in->blocks = @blocks.  -EINVAL for a NULL @bytes,
 *   m > 2^31, nconn > 2^20 or blocks > GCL_TCPRX_MAX_BLOCKS.
 * gcl_tcp_rx - asynchronous on @hip_stream: launches ordered by the stream
 *   alone; no block waits for another and no atomic's order decides a result.
 *   No allocation, no host synchronisation.  @workspace (device, 16-B aligned)
 *   need not be zeroed and may be reused by the next call on the same stream.
 *   m == 0 still writes out_conn and conn_off.  -EINVAL for a NULL ctx, b, in
 *   or out; a wrong in->size; a bad align; order == NULL with m != b->n;
 *   m > 2^31; nconn > 2^20; a NULL sock; with nconn > 0 a NULL conn or
 *   out_conn; a NULL conn_off; with m > 0 a NULL verdict, sflags,
 *   rcv_nxt_after, copy_len or dst_off; any given array that is not aligned to
 *   its element (conn, out_conn: 16 B); blocks > GCL_TCPRX_MAX_BLOCKS; a NULL
 *   workspace, one that is not 16-B aligned or one smaller than
 *   gcl_tcp_rx_workspace says; and, when m > 0, what gcl_l4_payload refuses of
 *   a batch.  -EIO when a launch fails.
 */
/* verdict[j], and the first five counter slots */
#define GCL_TCPRX_FAST   0
#define GCL_TCPRX_SLOW   1
#define GCL_TCPRX_DROP   2
#define GCL_TCPRX_NOCONN 3
#define GCL_TCPRX_NA     4
#define GCL_TCPRX_MAX_BLOCKS 1024  /* the cap on in->blocks */
#define GCL_TCPRX_MAX_CONN (1u << 20)
enum { GCL_TCPRXC_FAST = 0, GCL_TCPRXC_SLOW, GCL_TCPRXC_DROP, GCL_TCPRXC_NOCONN, GCL_TCPRXC_NA,
       GCL_TCPRXC_BYTES, GCL_TCPRXC_ACKS, GCL_TCPRXC_WAKES, GCL_TCPRXC_NR = 8 };
/* sflags[j] */
#define GCL_TCPRX_SF_WAKE    0x01  /* waitq_signal + POLLIN */
#define GCL_TCPRX_SF_ACK_NOW 0x02  /* do_ack: tcp_tx_ack with rcv_nxt_after[j] */
#define GCL_TCPRX_SF_ACKED   0x04  /* snd_una moved: run tcp_conn_ack */
#define GCL_TCPRX_SF_WND     0x08  /* snd_wnd, snd_wl1 and snd_wl2 were rewritten */
/* gcl_tcp_conn.flags */
#define GCL_TCPC_ELIGIBLE    0x01  /* state == ESTABLISHED && list_empty(&rxq_ooo) */
#define GCL_TCPC_RXQ         0x02  /* !list_empty(&rxq) */
#define GCL_TCPC_ACK_DELAYED 0x04  /* c->ack_delayed */
/* gcl_tcp_conn_out.flags: RXQ and ACK_DELAYED as above, and */
#define GCL_TCPO_STOPPED        0x08  /* first_slow is valid */
#define GCL_TCPO_WOKEN          0x10  /* some segment had WAKE */
#define GCL_TCPO_TIMER_ARMED    0x20  /* set ack_ts = microtime(), lower next_timeout */
#define GCL_TCPO_REP_ACKS_RESET 0x40  /* rep_acks = 0 */
struct gcl_tcp_conn {      /* 48 B, 16-B aligned, host order: the PCB words the fast path reads */
	uint32_t snd_una, snd_nxt, snd_wnd, snd_wl1, snd_wl2, rcv_nxt, rcv_wnd;
	uint16_t rcv_mss;
	uint8_t  snd_wscale;   /* the low five bits are used: a shift of 0..31 */
	uint8_t  flags;        /* GCL_TCPC_* */
	uint8_t  acks_delayed_cnt, pad[15];
};
struct gcl_tcp_conn_out {  /* 48 B, 16-B aligned */
	uint32_t snd_una, snd_wnd, snd_wl1, snd_wl2, rcv_nxt, rcv_wnd;
	uint32_t nfast, nslow, nacks;
	uint32_t first_slow;   /* list position, or 0xFFFFFFFF */
	uint8_t  acks_delayed_cnt;
	uint8_t  flags;        /* GCL_TCPC_RXQ, GCL_TCPC_ACK_DELAYED, GCL_TCPO_* */
	uint8_t  pad[6];
};
struct gcl_tcprx_in {
	uint32_t size, align;            /* sizeof(struct gcl_tcprx_in); align as in gcl_pay_in */
	const uint32_t *order;           /* optional u32[m]; NULL: m == b->n and i = j */
	uint64_t m;                      /* list entries, <= 2^31 */
	const uint32_t *sock;            /* REQUIRED u32[n], as gcl_sock_lookup wrote it */
	const uint8_t  *l4_status;       /* optional u8[n], as GCL_L4_VERIFY wrote it */
	const struct gcl_tcp_conn *conn; /* [nconn], indexed by cookie */
	uint32_t nconn;                  /* <= 2^20 */
	uint32_t blocks;                 /* 0: the library's choice; else the number of contiguous
	                                    list ranges the grouping is cut into (tests) */
};
struct gcl_tcprx_out {               /* device, aligned to their element */
	uint8_t  *verdict, *sflags;      /* [m] */
	uint32_t *rcv_nxt_after;         /* [m] */
	uint16_t *copy_len;              /* [m] */
	uint64_t *dst_off;               /* [m] */
	struct gcl_tcp_conn_out *out_conn; /* [nconn] */
	uint64_t *conn_off;              /* u64[nconn + 1] */
};
int gcl_tcp_rx_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, size_t *bytes);
int gcl_tcp_rx(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_tcprx_in *in,
               const struct gcl_tcprx_out *out, uint64_t *counts,
               void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * TCP receive with the established slow path: gcl_tcp_rx_full stands where
 * gcl_tcp_rx stands and takes, besides the fast path, the part of
 * __tcp_rx_conn (runtime/net/tcp_in.c:352-611) that a connection in
 * ESTABLISHED with an empty out-of-order queue needs: acceptability, the ACK
 * and window update, the sender wake-up, duplicate-ACK counting and in-order
 * text under the slow rule's own wake and delayed-ACK steps.  gcl_tcp_rx stops
 * a connection at its first pure ACK (len == 0 is slow, :222), so it does
 * nothing for a connection that mostly sends; this call keeps going.
 *
 *   gcl_l4_payload -> gcl_tcp_rx_full -> gcl_copy_batch
 *                  -> gcl_tcp_rx_acks -> gcl_tx_hdr
 *                  -> gcl_tcp_txq (snd_una from out_conn, GCL_TXQ_W_FAST for a
 *                     connection whose out_ext has GCL_TCPX_FASTRTX)
 *
 * Lists, segments, one runtime per call, arithmetic (mod 2^32, wraps_*; win
 * shifted by snd_wscale & 31; snd_nxt the snapshot's) and the lines NA, NOCONN
 * and DROP are gcl_tcp_rx's.  Then, for one segment of connection c, the
 * entries of a connection in list order:
 *  1. The connection has not stopped and gcl_tcp_rx's rule says FAST: the fast
 *     path as there; its ACKED or WND also sets rep_acks = 0.
 *  2. Otherwise the segment is __tcp_rx_conn's.  It STOPS the connection
 *     (verdict SLOW, the state frozen as it stood before the segment,
 *     first_slow set, every later segment SLOW, as in gcl_tcp_rx) when the
 *     connection has stopped already, is not GCL_TCPC_ELIGIBLE, the segment
 *     carries FIN, RST, URG or SYN, or it is acceptable text (len > 0,
 *     is_acceptable) with seq != rcv_nxt: the out-of-order queue or a head
 *     clip.
 *  3. Every other segment is HANDLED (sflags RULE2), in the reference's order:
 *     is_acceptable (:27-51) false: do_ack, done.
 *     no ACK flag: done.
 *     snd_was_full = wraps_lte(snd_una + snd_wnd, snd_nxt).
 *     if wraps_lte(snd_una, ack) and wraps_lte(ack, snd_nxt):
 *       snd_una != ack: snd_una = ack (ACKED); else ack_same.
 *       if wraps_lt(snd_wl1, seq) or (snd_wl1 == seq and wraps_lte(snd_wl2, ack)),
 *       and (!ack_same or snd_wnd <= win): wnd_updated when snd_wnd != win or
 *       snd_wl2 != ack; snd_wnd = win, snd_wl1 = seq, snd_wl2 = ack (WND).
 *     else if wraps_gt(ack, snd_nxt): do_ack, done.
 *     snd_was_full and no longer full: TXWAKE.
 *     if ack_same and snd_una != snd_nxt and len == 0 and !wnd_updated:
 *       rep_acks++ (the reference's int; counted in DUPACKS); at 3 or more
 *       FASTRTX, fast_rtx_ack = ack, rep_acks = 0.
 *     else if snd_una == ack: rep_acks = 0.
 *     len > 0 (the text starts at rcv_nxt and rcv_wnd > 0): wake on PSH or
 *       GCL_TCPC_RXQ; the tail is clipped to rcv_wnd; rcv_nxt and rcv_wnd move
 *       by the accepted bytes; GCL_TCPC_RXQ is set; wake when rcv_wnd reached
 *       0 (WAKE); ++acks_delayed_cnt >= 2: do_ack, else if ACK_DELAYED is
 *       clear it is set (TIMER_ARMED).  do_drop = false.
 *     done: do_ack clears ACK_DELAYED and the counter (ACK_NOW), so a segment
 *       that is not acceptable cancels a pending delayed ACK; do_drop as it
 *       stands (DROPPED): every handled segment that left no text.
 *     GCL_TCPO_REP_ACKS_RESET is set whenever some segment set rep_acks = 0.
 *
 * Per-entry outputs are gcl_tcprx_out's arrays: verdict GCL_TCPRX_FAST for
 * every handled segment, by either rule, so that gcl_tcp_rx_acks takes
 * verdict, sflags and rcv_nxt_after of this call unchanged; rcv_nxt_after =
 * rcv_nxt after the segment for every handled one (rcv_wnd falls only by
 * accepted bytes, so the window follows from it), 0 otherwise; sflags with
 * four more bits; copy_len the accepted byte count (0 for pure ACKs and drops,
 * the clipped length after a tail clip); dst_off = conn_off[c] + (seq -
 * conn[c].rcv_nxt) where copy_len > 0, else 0.  Accepted text always starts at
 * rcv_nxt, so fast_bytes, conn_off and the layout are gcl_tcp_rx's.
 * out_conn[c] as there, nfast counting the handled segments; out_ext[c] adds
 * nrule2 and ndropped (handled under rule 2; DROPPED among them),
 * fast_rtx_ack (the ack of the last FASTRTX, for fast_retransmit_last_ack; 0
 * without one), rep_acks as it stands after the list and xflags.  A
 * connection with no segment in the list gets its input back.
 *
 * @in is gcl_tcprx_in's fields with its own size and rep_acks: an optional
 * device u8[nconn], c->rep_acks per connection, NULL meaning zeros.  @counts
 * is a device u64[GCL_TCPRXFC_NR], ACCUMULATED, may be NULL: the first eight
 * slots as gcl_tcp_rx (FAST: handled), then RULE2, TXWAKES, FASTRTX, DUPACKS
 * (rep_acks++ events) and DROPPED.  The bounds guarantee is gcl_tcp_rx's, with
 * rep_acks[0, nconn) among the reads and out_ext[0, nconn) among the writes.
 *
 * What stays with the runtime: every SLOW segment and what follows it (the
 * out-of-order queue, head-clipped text, FIN / RST / URG / SYN, every other
 * state), tcp_timer_update at done, tcp_conn_ack's frees (ACKED), the
 * wake-ups (WAKE; TXWAKE: POLLOUT and waitq_release of tx_wq), the fast
 * retransmit itself (FASTRTX: do_fast_retransmit with tx_exclusive, else
 * tcp_tx_fast_retransmit_start, or GCL_TXQ_W_FAST for gcl_tcp_txq), freeing
 * the mbufs (DROPPED), sending the ACKs, and the lock.
 *
 * gcl_tcp_rx_full_workspace, gcl_tcp_rx_full - as gcl_tcp_rx_workspace and
 *   gcl_tcp_rx: asynchronous, launches ordered by the stream alone, no block
 *   waits for another, no atomic's order decides a result, no allocation, no
 *   host synchronisation, a workspace that need not be zeroed.  -EINVAL for
 *   what gcl_tcp_rx refuses, and with nconn > 0 for an out_ext that is NULL or
 *   not 16-B aligned.
 */
#define GCL_TCPRX_SF_RULE2   0x10  /* went through __tcp_rx_conn */
#define GCL_TCPRX_SF_TXWAKE  0x20  /* POLLOUT + waitq_release of tx_wq */
#define GCL_TCPRX_SF_FASTRTX 0x40  /* rep_acks reached TCP_FAST_RETRANSMIT_THRESH */
#define GCL_TCPRX_SF_DROPPED 0x80  /* do_drop: the mbuf is freed */
/* gcl_tcp_conn_ext.xflags */
#define GCL_TCPX_TXWAKE  0x01  /* some segment had TXWAKE */
#define GCL_TCPX_FASTRTX 0x02  /* some segment had FASTRTX */
enum { GCL_TCPRXFC_RULE2 = 8, GCL_TCPRXFC_TXWAKES, GCL_TCPRXFC_FASTRTX, GCL_TCPRXFC_DUPACKS,
       GCL_TCPRXFC_DROPPED, GCL_TCPRXFC_NR = 13 };
struct gcl_tcp_conn_ext {  /* 16 B, 16-B aligned */
	uint32_t nrule2, ndropped;
	uint32_t fast_rtx_ack;
	uint8_t  rep_acks;
	uint8_t  xflags;       /* GCL_TCPX_* */
	uint8_t  pad[2];       /* written 0 */
};
struct gcl_tcprxf_in {
	uint32_t size, align;            /* sizeof(struct gcl_tcprxf_in) */
	const uint32_t *order;
	uint64_t m;
	const uint32_t *sock;
	const uint8_t  *l4_status;
	const struct gcl_tcp_conn *conn;
	uint32_t nconn;
	uint32_t blocks;
	const uint8_t  *rep_acks;        /* optional u8[nconn]; NULL: zeros */
};
int gcl_tcp_rx_full_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, size_t *bytes);
int gcl_tcp_rx_full(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_tcprxf_in *in,
                    const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext, uint64_t *counts,
                    void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * TCP receive with the out-of-order queue: gcl_tcp_rx_ooo stands where
 * gcl_tcp_rx_full stands, takes the same inputs and behaves exactly as it
 * does, except that out-of-order and head-clipped text is handled instead of
 * stopping the connection: tcp_rx_text and tcp_rx_append_text
 * (runtime/net/tcp_in.c:64-169) with c->rxq_ooo.  Every connection brings its
 * queue in and gets it back as it stands after the list.  This closes the
 * established-state data path of tcp_in.c.
 *
 *   gcl_l4_payload -> gcl_tcp_rx_ooo -> gcl_copy_batch (src_off + skip)
 *                  -> gcl_tcp_rx_acks (the duplicate ACKs of :574 among them)
 *                  -> gcl_tcp_txq
 *
 * The queue of a connection is an ordered array of at most GCL_TCPOOO_CAP
 * entries {seq, end, ref, flags, src}, the head first.  Connection c's input
 * queue is q[min(q_off[c], nq), min(q_off[c + 1], nq)), empty when that range
 * is reversed; q_off == NULL means every queue is empty.  The input queue
 * itself, not GCL_TCPC_ELIGIBLE, says whether the queue is empty.  No order is
 * assumed on it: the result is what the reference's walk gives on that list.
 * A connection is TAKEN when its flags have GCL_TCPC_ELIGIBLE or
 * GCL_TCPC_ESTABLISHED (state == ESTABLISHED whatever the queue holds; never
 * set in out_conn.flags), its input queue has at most GCL_TCPOOO_CAP entries
 * and none of them carries FIN (flags & 0x01: a drained FIN would change state
 * in mid-segment).  The queue of a connection whose flags have neither bit is
 * not looked at, nor are more than GCL_TCPOOO_CAP entries.  A connection that
 * is not taken stops at its first segment as in gcl_tcp_rx_full, gets an empty
 * output queue and GCL_OOOQ_UNTOUCHED on its input entries, and, when its
 * input range was not empty, GCL_TCPX_QSKIP in xflags: the runtime still holds
 * that queue (this departs from marking every connection that is not taken:
 * one without a queue gets gcl_tcp_rx_full's out_ext byte for byte).  The
 * ranges of two connections must not overlap; they may follow each other in
 * any order (q_off need not be non-decreasing).  Where they do overlap, the
 * outputs of those connections and of the shared entries are unspecified, and
 * still in bounds.
 *
 * For one segment of connection c, in list order, after the lines NA, NOCONN
 * and DROP of gcl_tcp_rx:
 *  1. The fast path, exactly when gcl_tcp_rx's rule says FAST and the LIVE
 *     queue is empty (:233): the queue as it stands now, so a connection whose
 *     queue drains empty in mid-list goes back to the fast path.
 *  2. The segment STOPS the connection (verdict SLOW, state and queue frozen as
 *     before the segment) when the connection has stopped already, is not
 *     taken, the segment carries FIN, RST, URG or SYN, or it would be inserted
 *     (:124-135) while the live queue holds GCL_TCPOOO_CAP entries.  The
 *     reference's own bound, TCP_OOO_MAX_SIZE = 2048, cannot be reached below
 *     this cap; the cap stops the connection, it does not drop the segment.
 *  3. Every other segment runs gcl_tcp_rx_full's step 3 unchanged up to the
 *     text; for len > 0 the text step is tcp_rx_text:
 *     wraps_lte(seq, rcv_nxt), the in-order branch: wake on PSH or
 *       GCL_TCPC_RXQ; the head is clipped by rcv_nxt - seq bytes, then the tail
 *       to the window; rcv_nxt and rcv_wnd move.
 *     else the out-of-order branch: walk the queue from its tail; the first
 *       entry e with wraps_gt(end, e.end): insert after it; an entry with
 *       wraps_gte(seq, e.seq) before that: the segment is refused (DROPPED),
 *       no drain runs and the delayed-ACK lines below still run; no such
 *       entry: insert at the head.
 *     the drain (:140-163), from the head: free every entry with
 *       wraps_lte(e.end, rcv_nxt); stop at wraps_gt(e.seq, rcv_nxt); else pop
 *       the entry, wake, and append it with both clips, also when the window
 *       has reached 0 and clips it to zero bytes.
 *     then: wake when rcv_wnd == 0; ++acks_delayed_cnt >= 2: do_ack, else arm
 *       the delayed ACK; do_ack also when the queue is not empty (:574).
 *     WAKE, ACK_NOW and rcv_nxt_after belong to the segment being processed,
 *     its drain included.
 *
 * Outputs.  @out and @out_ext are gcl_tcp_rx_full's.  All accepted bytes of a
 * connection still form [conn[c].rcv_nxt, out_conn[c].rcv_nxt), so fast_bytes,
 * conn_off and the layout are gcl_tcp_rx's; copy_len is the accepted byte
 * count after both clips and dst_off = conn_off[c] + (clipped seq -
 * conn[c].rcv_nxt) where copy_len > 0.  @ooo adds, per list entry, oflags[j]
 * (GCL_OOOF_*) and skip[j], the head bytes to add to gcl_l4_payload's src_off;
 * gcl_copy_batch with src_off + skip, copy_len and dst_off leaves the stream
 * contiguous and in sequence order.  An entry queued in this call and drained
 * later in it gets its copy_len, skip and dst_off then (LATE_DRAINED), one
 * freed as already received LATE_FREED, one still queued at the end HELD with
 * copy_len = 0: the runtime keeps the frame.  Per input queue entry i < nq:
 * qin_state[i] (GCL_OOOQ_*), and for a DRAINED one qin_skip[i], qin_len[i]
 * (each saturates at 65535, more than any frame holds) and qin_dst_off[i], its
 * place in the same layout; else 0.  The output queues: qout_off[c], c <=
 * nconn, is the whole prefix sum of the final queue lengths, and entry k of
 * connection c's queue is qout[qout_off[c] + k]: seq, end, flags as they
 * stand (unclipped), src 0 with the input's ref for one carried over from the
 * input, src 1 with ref = j for list entry j of this call.  Entries at and
 * past q_out_cap are not written; totals[0] = qout_off[nconn], the entries
 * wanted (what q_out_cap should have been).
 *
 * @counts is a device u64[GCL_TCPRXOC_NR], ACCUMULATED, may be NULL: the
 * thirteen of gcl_tcp_rx_full (BYTES: every accepted byte, the drained input
 * entries' among them), then OOO (segments that took the out-of-order branch),
 * QUEUED (inserted), DRAINED and FREED (entries, of either source), HEADCLIP
 * (appends that lost head bytes) and HELD.
 *
 * Guarantee: gcl_tcp_rx_full's, and no content of q_off or q causes an access
 * outside q_off[0, nconn], q[0, nq), the outputs (@ooo's per-entry arrays m
 * elements, its per-queue-entry arrays nq, qout_off[0, nconn], qout[0,
 * q_out_cap), totals[0]) and the workspace.
 *
 * What stays with the runtime: FIN / RST / URG / SYN and every other state,
 * which need the connection object itself; the mbufs (ref is the handle:
 * free the FREED, DROPPED and LATE_FREED ones, keep the HELD ones, relink
 * rxq_ooo from qout); the wake-ups, the ACKs, the timers and the lock, as for
 * gcl_tcp_rx_full.
 *
 * gcl_tcp_rx_ooo_workspace, gcl_tcp_rx_ooo - as gcl_tcp_rx_full's, the
 *   workspace also sized by nq: asynchronous, launches ordered by the stream
 *   alone, no block waits for another, no atomic's order decides a result, no
 *   allocation, no host synchronisation.  -EINVAL for what gcl_tcp_rx_full
 *   refuses; nq > 2^31; a NULL ooo, qout_off or totals; with m > 0 a NULL
 *   oflags or skip; with nq > 0 a NULL q, qin_state, qin_skip, qin_len or
 *   qin_dst_off; with q_out_cap > 0 a NULL qout; any of them not aligned to
 *   its element (q, qout: 16 B).
 */
#define GCL_TCPOOO_CAP 64            /* queue entries per connection: one per lane of a wave */
#define GCL_TCPC_ESTABLISHED 0x80    /* gcl_tcp_conn.flags: state == ESTABLISHED, whatever rxq_ooo holds */
#define GCL_TCPX_QSKIP 0x04          /* gcl_tcp_conn_ext.xflags: the input queue was not taken */
/* oflags[j] */
#define GCL_OOOF_OOO          0x01   /* took tcp_rx_text's out-of-order branch */
#define GCL_OOOF_QUEUED       0x02   /* was inserted into the queue */
#define GCL_OOOF_HEADCLIP     0x04   /* skip[j] > 0 */
#define GCL_OOOF_LATE_DRAINED 0x08   /* queued here, appended by a later drain of this call */
#define GCL_OOOF_LATE_FREED   0x10   /* queued here, freed as already received */
#define GCL_OOOF_HELD         0x20   /* queued here and still queued: in qout */
/* qin_state[i] */
#define GCL_OOOQ_UNTOUCHED 0         /* of no taken connection */
#define GCL_OOOQ_KEPT      1         /* still queued: in qout */
#define GCL_OOOQ_FREED     2
#define GCL_OOOQ_DRAINED   3
enum { GCL_TCPRXOC_OOO = 13, GCL_TCPRXOC_QUEUED, GCL_TCPRXOC_DRAINED, GCL_TCPRXOC_FREED,
       GCL_TCPRXOC_HEADCLIP, GCL_TCPRXOC_HELD, GCL_TCPRXOC_NR = 19 };
struct gcl_tcp_ooo_ent {   /* 16 B, 16-B aligned */
	uint32_t seq, end;     /* m->seg_seq, m->seg_end */
	uint32_t ref;          /* input: opaque (the mbuf's handle); output: that, or j with src 1 */
	uint16_t flags;        /* m->flags */
	uint16_t src;          /* output: 0 carried over from the input, 1 list entry ref of this call */
};
struct gcl_tcprxo_in {
	uint32_t size, align;            /* sizeof(struct gcl_tcprxo_in) */
	const uint32_t *order;
	uint64_t m;
	const uint32_t *sock;
	const uint8_t  *l4_status;
	const struct gcl_tcp_conn *conn;
	uint32_t nconn;
	uint32_t blocks;
	const uint8_t  *rep_acks;        /* optional u8[nconn]; NULL: zeros */
	const uint32_t *q_off;           /* optional u32[nconn + 1]; NULL: every queue is empty */
	const struct gcl_tcp_ooo_ent *q; /* [nq] */
	uint32_t nq;                     /* <= 2^31 */
	uint32_t q_out_cap;              /* entries qout can hold */
};
struct gcl_tcprxo_out {              /* device, aligned to their element */
	uint8_t  *oflags;                /* [m] */
	uint16_t *skip;                  /* [m] */
	uint8_t  *qin_state;             /* [nq] */
	uint16_t *qin_skip, *qin_len;    /* [nq] */
	uint64_t *qin_dst_off;           /* [nq] */
	uint32_t *qout_off;              /* u32[nconn + 1] */
	struct gcl_tcp_ooo_ent *qout;    /* [q_out_cap] */
	uint64_t *totals;                /* u64[1]: the entries wanted */
};
int gcl_tcp_rx_ooo_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, uint32_t nq, size_t *bytes);
int gcl_tcp_rx_ooo(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_tcprxo_in *in,
                   const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                   const struct gcl_tcprxo_out *ooo, uint64_t *counts,
                   void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * TCP receive in every state: gcl_tcp_rx_states stands where gcl_tcp_rx_ooo
 * stands, takes the same inputs and one more, the connections' states, and
 * finishes __tcp_rx_conn (runtime/net/tcp_in.c:352-611): FIN, RST, SYN and URG
 * segments no longer stop a connection, and a connection in SYN_RECEIVED,
 * FIN_WAIT1, FIN_WAIT2, CLOSE_WAIT, CLOSING, LAST_ACK, TIME_WAIT or CLOSED is
 * walked as one in ESTABLISHED is.
 *
 *   gcl_l4_payload -> gcl_tcp_rx_states -> gcl_copy_batch (src_off + skip)
 *                  -> gcl_tcp_rx_ctl (the ACKs of ACK_NOW and the RSTs of ev / rst_seq)
 *                  -> gcl_tcp_txq
 *
 * @in is gcl_tcprxo_in's fields with its own size and state: an optional
 * device u8[nconn], enum tcp state (runtime/net/tcp.h:41-52, GCL_TCP_STATE_*).
 * With state == NULL a connection is in ESTABLISHED exactly when its flags
 * have GCL_TCPC_ELIGIBLE or GCL_TCPC_ESTABLISHED and is otherwise not taken:
 * gcl_tcp_rx_ooo's meaning.  With state given, state[c] decides and the two
 * flag bits are ignored.  A connection is TAKEN when its state is 1..9 and its
 * input queue has at most GCL_TCPOOO_CAP entries; FIN entries in the queue no
 * longer bar it.  SYN_SENT (0) and values above 9 are not taken.
 *
 * For one segment of a taken connection that has not stopped, in list order,
 * after the lines NA, NOCONN and DROP of gcl_tcp_rx; `state` is the LIVE one:
 *  1. The fast path, exactly when gcl_tcp_rx's rule says FAST, the live state
 *     is ESTABLISHED and the live queue is empty.  A connection that becomes
 *     ESTABLISHED in mid-list may take it for its later segments.
 *  2. Otherwise __tcp_rx_conn (sflags RULE2), with len counting a FIN as one
 *     (:369-370) in the acceptability test, in the duplicate-ACK test len == 0
 *     and in seg_end (:552):
 *     state CLOSED (:372-376): RST|ACK with seq 0 and ack seq + len unless the
 *       segment carries RST; done.
 *     not acceptable: do_ack unless the segment carries RST (:439); done.
 *     RST (:444): FAIL; done.
 *     SYN (:452): RST with seq = ack when the segment carries ACK, else RST|ACK
 *       with ack = seq + len; FAIL; done.
 *     no ACK flag: done.
 *     SYN_RECEIVED (:462-473): not snd_una <= ack <= snd_nxt: RST with seq =
 *       ack, done; else snd_wnd, snd_wl1, snd_wl2 = win, seq, ack (WND) and the
 *       state is ESTABLISHED (GCL_TCPX_OPENED: tcp_conn_set_state's
 *       waitq_release of tx_wq and POLLOUT, tcp.c:254-258).
 *     gcl_tcp_rx_full's ACK, window, TXWAKE and duplicate-ACK lines.
 *     snd_una == snd_nxt (:530-542): FIN_WAIT1 -> FIN_WAIT2; CLOSING ->
 *       TIME_WAIT (GCL_TCPX_TIMEWAIT: time_wait_ts = microtime()); LAST_ACK ->
 *       CLOSED, PUT (tcp_conn_put), done.
 *     len > 0 and the state is ESTABLISHED, FIN_WAIT1 or FIN_WAIT2: the text
 *       step of gcl_tcp_rx_ooo; fin is set by an in-order segment that carries
 *       FIN (:114) and by every drained entry that does (:161), and the drain
 *       goes on behind such an entry.  In the other states acceptable text is
 *       dropped and the delayed-ACK lines do not run.
 *     fin (:578-590): ESTABLISHED -> CLOSE_WAIT; FIN_WAIT1 -> CLOSING;
 *       FIN_WAIT2 -> TIME_WAIT with do_ack and GCL_TCPX_TIMEWAIT.
 *     done as in gcl_tcp_rx_full.  URG is not looked at (step 6 is skipped).
 *  3. A segment with FAIL or PUT is handled and is the last one of its
 *     connection the call takes: the next one STOPS it (verdict SLOW,
 *     first_slow).  FAIL leaves the state as it was: tcp_conn_fail is the
 *     runtime's.  A connection that ENTERS in CLOSED is walked to the end.
 *     The stop at the 65th insert is gcl_tcp_rx_ooo's, with every word of the
 *     connection, its state among them, as before the segment.
 *
 * Kept as the reference has them.  A FIN's octet is part of seg_end, so
 * tcp_rx_append_text's tail clip (:83-87) trims the mbuf by a length that
 * counts it: FIN + 6 bytes into rcv_wnd = 3 links 2 bytes while rcv_nxt moves
 * by 3.  copy_len[j] (qin_len[i]) is the mbuf length the reference leaves:
 * the text length - the head pull - the trim, not below 0; an input queue
 * entry with FIN holds end - seq - 1 bytes of text.  rcv_nxt, rcv_wnd and the
 * layout stay in sequence space: conn_off[c + 1] - conn_off[c] spans
 * out_conn[c].rcv_nxt - conn[c].rcv_nxt and dst_off = conn_off[c] + (clipped
 * seq - conn[c].rcv_nxt), so an accepted FIN leaves one byte of the region
 * unwritten (THE FIN GAP), and a tail-clipped FIN segment a second one, the
 * lost tail byte.  After a FIN the state leaves the text states, so only
 * entries drained behind a FIN entry in the same tcp_rx_text call land behind
 * that gap.  fin is set even where the clip removed the FIN's own octet.
 *
 * Outputs: @out, @out_ext and @ooo are gcl_tcp_rx_ooo's; out_ext.xflags may
 * also hold GCL_TCPX_FAILED, _PUT, _TIMEWAIT and _OPENED.  @st adds per list
 * entry ev[j] (GCL_TCPS_*), rst_seq[j] (the seq of a RST, the ack of a
 * RST|ACK, else 0) and state_after[j], all 0 for an entry that was not
 * handled; and per connection state_out[c]: the live state after the list,
 * for a connection that was not taken state[c] as given, or GCL_TCPS_NOSTATE
 * without a state array.  An entry has at most one of RST and RST_ACK, and
 * never with ACK_NOW.  @counts is a device u64[GCL_TCPRXSC_NR], ACCUMULATED,
 * may be NULL: the nineteen of gcl_tcp_rx_ooo, then RSTS (either kind), FAILS,
 * FINS and STATE_CHANGES (entries with GCL_TCPS_STATE).
 *
 * Guarantee: gcl_tcp_rx_ooo's, with state[0, nconn) among the reads and ev,
 * rst_seq, state_after (m elements) and state_out[0, nconn) among the writes.
 *
 * What stays with the runtime: SYN_SENT, which needs iss, winmax and the
 * options and answers with tcp_tx_ctl(SYN|ACK); tcp_rx_listener and
 * tcp_rx_closed, the segments with no connection; tcp_timer_update;
 * tcp_conn_fail's frees and wake-ups and its state CLOSED (FAIL), tcp_conn_put
 * (PUT), time_wait_ts (TIMEWAIT), the wake of OPENED; and what gcl_tcp_rx_ooo
 * leaves.  The RSTs are gcl_tcp_rx_ctl's.
 *
 * gcl_tcp_rx_states_workspace, gcl_tcp_rx_states - as gcl_tcp_rx_ooo's, the
 *   same bytes: asynchronous, launches ordered by the stream alone, no block
 *   waits for another, atomics only add to counts, no allocation, no host
 *   synchronisation.  -EINVAL for what gcl_tcp_rx_ooo refuses; a NULL st; with
 *   m > 0 a NULL ev, rst_seq or state_after, or a rst_seq not 4-B aligned; with
 *   nconn > 0 a NULL state_out.
 */
/* enum tcp state: ESTABLISHED 2, TIME_WAIT 8 and CLOSED 9 are defined with gcl_tcp_tmr below */
#define GCL_TCP_STATE_SYN_SENT     0
#define GCL_TCP_STATE_SYN_RECEIVED 1
#define GCL_TCP_STATE_FIN_WAIT1    3
#define GCL_TCP_STATE_FIN_WAIT2    4
#define GCL_TCP_STATE_CLOSE_WAIT   5
#define GCL_TCP_STATE_CLOSING      6
#define GCL_TCP_STATE_LAST_ACK     7
#define GCL_TCPS_NOSTATE 0xFF        /* state_out[c] of a connection that is not taken when state == NULL */
/* ev[j] */
#define GCL_TCPS_RST     0x01        /* tcp_tx_raw_rst(seq = rst_seq[j]) */
#define GCL_TCPS_RST_ACK 0x02        /* tcp_tx_raw_rst_ack(seq = 0, ack = rst_seq[j]) */
#define GCL_TCPS_FAIL    0x04        /* tcp_conn_fail(c, ECONNRESET) */
#define GCL_TCPS_STATE   0x08        /* tcp_conn_set_state ran: state_after[j] differs from the state before */
#define GCL_TCPS_FIN     0x10        /* step 8 ran: a FIN was consumed */
#define GCL_TCPS_PUT     0x20        /* LAST_ACK -> CLOSED: tcp_conn_put, :540 */
/* gcl_tcp_conn_ext.xflags */
#define GCL_TCPX_FAILED   0x08       /* some segment had FAIL */
#define GCL_TCPX_PUT      0x10       /* some segment had PUT */
#define GCL_TCPX_TIMEWAIT 0x20       /* set time_wait_ts = microtime(), :535 and :587 */
#define GCL_TCPX_OPENED   0x40       /* SYN_RECEIVED -> ESTABLISHED: waitq_release(tx_wq) + POLLOUT */
enum { GCL_TCPRXSC_RSTS = 19, GCL_TCPRXSC_FAILS, GCL_TCPRXSC_FINS, GCL_TCPRXSC_STATE_CHANGES,
       GCL_TCPRXSC_NR = 23 };
struct gcl_tcprxs_in {
	uint32_t size, align;            /* sizeof(struct gcl_tcprxs_in) */
	const uint32_t *order;
	uint64_t m;
	const uint32_t *sock;
	const uint8_t  *l4_status;
	const struct gcl_tcp_conn *conn;
	uint32_t nconn;
	uint32_t blocks;
	const uint8_t  *rep_acks;
	const uint32_t *q_off;
	const struct gcl_tcp_ooo_ent *q;
	uint32_t nq;
	uint32_t q_out_cap;
	const uint8_t  *state;           /* optional u8[nconn]: enum tcp state; NULL: the flags decide */
};
struct gcl_tcprxs_out {              /* device, aligned to their element */
	uint8_t  *ev;                    /* [m] */
	uint32_t *rst_seq;               /* [m] */
	uint8_t  *state_after;           /* [m] */
	uint8_t  *state_out;             /* [nconn] */
};
int gcl_tcp_rx_states_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, uint32_t nq, size_t *bytes);
int gcl_tcp_rx_states(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_tcprxs_in *in,
                      const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                      const struct gcl_tcprxo_out *ooo, const struct gcl_tcprxs_out *st, uint64_t *counts,
                      void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * TCP control segments: the timer sweep, and the ACKs of a gcl_tcp_rx call.
 * Both chains end where TCP asks for a segment that carries no data.  In the
 * reference that is per-connection work on a core: tcp_worker
 * (runtime/net/tcp.c:143-174) wakes every 10 ms, walks the list of all
 * connections under tcp_lock and runs tcp_handle_timeouts (tcp.c:80-140) and
 * tcp_timer_update (tcp.c:46-77) on every one whose next_timeout has passed,
 * which ends in tcp_tx_ack or tcp_tx_probe_window (tcp_out.c:178-228); and
 * tcp_rx_conn sends one ACK after every do_ack of its fast path
 * (tcp_in.c:289-290).  gcl_tcp_tick is the sweep of all connections of one
 * runtime at one clock reading, gcl_tcp_rx_acks the ACKs of one gcl_tcp_rx
 * call; both write gcl_txh_desc records in send order, so that
 *
 *   gcl_tcp_tick -> gcl_tx_hdr -> gcl_l4_csum GCL_L4_FILL, and
 *   gcl_tcp_rx -> gcl_tcp_rx_acks -> gcl_tx_hdr -> gcl_l4_csum GCL_L4_FILL
 *
 * run on one stream.  They work on every context and touch no table.
 *
 * The sweep of connection c at @now, on tmr[c].  All time arithmetic is
 * uint64_t mod 2^64 and every comparison unsigned, as `now - ts >= T` reads in
 * the reference (a ts ahead of now gives a huge difference: the timeout
 * fires).  T in microseconds: ACK 10000, CONNECT 5000000, TIME_WAIT 1000000,
 * ZERO_WND 300000, RETRANSMIT 300000, OOQ_ACK 300000.
 *   1. GCL_TMR_LIVE clear, or next_timeout > now: nothing.  action = 0 and
 *      out_tmr[c] repeats the input words (tcp.c:166).
 *   2. action FIRED.  state == CLOSED: done, the timer is not recomputed
 *      (:85-88).
 *   3. state < ESTABLISHED and now - attach_ts >= CONNECT: action FAIL, the out
 *      state is CLOSED, done (:90-95).
 *   4. state == TIME_WAIT and now - time_wait_ts >= TIME_WAIT: action CLOSE,
 *      the out state is CLOSED, done (:97-104).
 *   5. ACK_DELAYED and now - ack_ts >= ACK: ACK_DELAYED is cleared, action ACK.
 *   6. ZERO_WND and now - zero_wnd_ts >= ZERO_WND: zero_wnd_ts = now, action
 *      PROBE.
 *   7. not TX_EXCLUSIVE, TXQ and now - txq_ts >= RETRANSMIT: action RETRANSMIT.
 *   8. OOO: action ACK.
 *   9. tcp_timer_update on the words as they now stand: nt = UINT64_MAX;
 *      TIME_WAIT: nt = time_wait_ts + TIME_WAIT; state < ESTABLISHED: nt =
 *      attach_ts + CONNECT (it overrides the line before, as in the
 *      reference); ACK_DELAYED: nt = min(nt, ack_ts + ACK); ZERO_WND: nt =
 *      min(nt, zero_wnd_ts + ZERO_WND); not TX_EXCLUSIVE and TXQ: nt = min(nt,
 *      txq_ts + RETRANSMIT); OOO: nt = min(nt, now + OOQ_ACK).
 * In the last term the reference reads microtime() a second time; a sweep has
 * one clock reading, @now.  That is the one departure.
 *
 * A control segment of connection c is a gcl_txh_desc with proto 6, tcp_flags
 * 0x10 (ACK), tcp_off 5, ecn 0 (net_tx_ip is given a NULL aux), paylen 0, pad
 * 0, the tuple of addr[c], the given ack, win = (uint16_t)(rcv_wnd >>
 * (rcv_wscale & 31)) (the truncation is hton16 of a uint32_t's, as
 * __tcp_add_tcphdr, tcp_out.c:74), and seq = conn[c].snd_nxt for an ACK,
 * conn[c].snd_una - 1 for a window probe.
 *
 * Segments of a sweep come in connection order, and inside a connection the
 * ACK before the probe (the order of tcp.c:134-137); both take ack =
 * conn[c].rcv_nxt and rcv_wnd = conn[c].rcv_wnd.  Segment k is written exactly
 * when k < seg_cap; a connection with a segment that was not written gets
 * action NOSPACE.  Its timer words change all the same, as a tcp_tx_ack that
 * returns -ENOMEM loses the ACK after ack_delayed was cleared.
 *
 * Segments of a gcl_tcp_rx call: list entry j emits one ACK exactly when
 * verdict[j] == GCL_TCPRX_FAST, sflags[j] has GCL_TCPRX_SF_ACK_NOW,
 * i = order ? order[j] : j is below n and c = sock[i] is below nconn.  They
 * come in list order, with ack = rcv_nxt_after[j], rcv_wnd = conn[c].rcv_wnd -
 * (rcv_nxt_after[j] - conn[c].rcv_nxt) mod 2^32 (the window as it stood after
 * that segment) and seq = conn[c].snd_nxt.  order, n, sock, conn and nconn are
 * those given to gcl_tcp_rx: conn is the same snapshot.
 *
 * Per segment k < min(wanted, seg_cap): desc[k]; frame_off[k] = frame_base +
 * k * frame_stride (mod 2^64); seg_conn[k] = c; seg_kind[k] = GCL_CTL_ACK or
 * GCL_CTL_PROBE; seg_src[k] = c for a sweep and the list position j for
 * gcl_tcp_rx_acks.  Entries at and past that are not written.  totals[0] = the
 * segments wanted, totals[1] = min(wanted, seg_cap), the m of gcl_tx_hdr.
 * frame_stride is the caller's slot size: at least 54, and at least
 * net.min_pkt_size when gcl_tx_hdr is to pad.
 *
 * @counts is a device u64[GCL_TICKC_NR], ACCUMULATED, may be NULL.  A sweep:
 * FIRED, ACK, PROBE, RETRANSMIT, FAIL, CLOSE and NOSPACE connections, and SEGS,
 * the segments written.  gcl_tcp_rx_acks: GCL_RXACKC_WANTED, _WRITTEN and
 * _SKIPPED (FAST | ACK_NOW entries whose i or c is out of range).
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * tmr, conn, addr, out_tmr and desc to 16 B.  Asynchronous on @hip_stream:
 * three launches (decide, the scan of the block sums, emit) ordered by the
 * stream alone; no block waits for another, and no atomic hands out a
 * position: atomics only add to counts.  No allocation, no host
 * synchronisation.  @workspace (device, 16-B aligned) need not be zeroed and
 * may be reused by the next call on the same stream.  nconn == 0 or m == 0
 * still writes totals.
 *
 * Guarantee: no content of tmr, conn, addr, order, sock, verdict, sflags or
 * rcv_nxt_after causes a read outside the given arrays, or a write outside the
 * first seg_cap elements of the per-segment outputs, out_tmr[0, nconn),
 * totals, counts and the workspace.
 *
 * What stays with the runtime: tcp_retransmit itself (RETRANSMIT says when),
 * tcp_conn_fail's frees and wake-ups (FAIL), tcp_conn_put (CLOSE), writing
 * out_tmr's words back under the connection lock, and the second clock
 * reading.
 *
 * gcl_tcp_tick_workspace / gcl_tcp_rx_acks_workspace - bytes of device scratch
 *   a call takes: 4 per block (in->blocks, or the cap GCL_TICK_MAX_BLOCKS when
 *   blocks is 0), rounded up to 16.  -EINVAL for a NULL @bytes, nconn > 2^20 or
 *   m > 2^31, or blocks > GCL_TICK_MAX_BLOCKS.
 * gcl_tcp_tick - -EINVAL for a NULL ctx, in or out; a wrong in->size; nconn >
 *   2^20; seg_cap > 2^31; blocks > GCL_TICK_MAX_BLOCKS; frame_stride < 54; a
 *   NULL totals; with nconn > 0 a NULL tmr, conn, addr or out_tmr; with
 *   nconn > 0 and seg_cap > 0 a NULL desc, frame_off, seg_conn, seg_kind or
 *   seg_src; any given array that is not aligned to its element; a NULL
 *   workspace, one that is not 16-B aligned or one smaller than
 *   gcl_tcp_tick_workspace says.  -EIO when a launch fails.
 * gcl_tcp_rx_acks - -EINVAL for the same of its own structs, with m > 2^31 and
 *   nconn > 2^20 as the caps; with m > 0 a NULL sock, verdict, sflags or
 *   rcv_nxt_after; with m > 0 and nconn > 0 a NULL conn or addr; with m > 0 and
 *   seg_cap > 0 a NULL per-segment output.  -EIO when a launch fails.
 */
/* enum tcp state (runtime/net/tcp.h) as gcl_tcp_tmr.state holds it */
#define GCL_TCP_STATE_ESTABLISHED 2
#define GCL_TCP_STATE_TIME_WAIT   8
#define GCL_TCP_STATE_CLOSED      9
/* gcl_tcp_tmr.flags */
#define GCL_TMR_LIVE         0x01  /* the slot holds a connection that is on tcp_conns */
#define GCL_TMR_ACK_DELAYED  0x02  /* c->ack_delayed */
#define GCL_TMR_ZERO_WND     0x04  /* c->zero_wnd */
#define GCL_TMR_TX_EXCLUSIVE 0x08  /* c->tx_exclusive */
#define GCL_TMR_TXQ          0x10  /* !list_empty(&c->txq); txq_ts = its head's timestamp */
#define GCL_TMR_OOO          0x20  /* !list_empty(&c->rxq_ooo) */
/* gcl_tcp_tmr_out.action */
#define GCL_TMRA_FIRED       0x01  /* next_timeout <= now: tcp_handle_timeouts ran */
#define GCL_TMRA_ACK         0x02  /* tcp_tx_ack */
#define GCL_TMRA_PROBE       0x04  /* tcp_tx_probe_window */
#define GCL_TMRA_RETRANSMIT  0x08  /* thread_spawn(tcp_retransmit): no segment comes from this call */
#define GCL_TMRA_FAIL        0x10  /* tcp_conn_fail(c, ETIMEDOUT) */
#define GCL_TMRA_CLOSE       0x20  /* TIME_WAIT ran out: tcp_conn_put */
#define GCL_TMRA_NOSPACE     0x40  /* a segment of the connection lay at or past seg_cap */
/* seg_kind[k] */
#define GCL_CTL_ACK   0
#define GCL_CTL_PROBE 1
#define GCL_TICK_MAX_BLOCKS 1024   /* the cap on in->blocks */
#define GCL_TICK_MAX_CONN (1u << 20)
#define GCL_CTL_MIN_STRIDE 54      /* Ethernet + IPv4 + TCP without options */
enum { GCL_TICKC_FIRED = 0, GCL_TICKC_ACK, GCL_TICKC_PROBE, GCL_TICKC_RETRANSMIT, GCL_TICKC_FAIL,
       GCL_TICKC_CLOSE, GCL_TICKC_NOSPACE, GCL_TICKC_SEGS, GCL_TICKC_NR = 8 };
enum { GCL_RXACKC_WANTED = 0, GCL_RXACKC_WRITTEN, GCL_RXACKC_SKIPPED };
struct gcl_tcp_tmr {       /* 64 B, 16-B aligned, host order: the timer words of a connection */
	uint64_t next_timeout, attach_ts, time_wait_ts, ack_ts, zero_wnd_ts, txq_ts;  /* us, as microtime() */
	uint8_t  state;        /* enum tcp state: SYN_SENT 0, SYN_RECEIVED 1, ESTABLISHED 2, ... */
	uint8_t  flags;        /* GCL_TMR_* */
	uint8_t  pad[14];
};
struct gcl_tcp_tmr_out {   /* 32 B, 16-B aligned */
	uint64_t next_timeout, zero_wnd_ts;
	uint8_t  state, flags;
	uint8_t  action;       /* GCL_TMRA_* */
	uint8_t  pad[13];      /* written as 0 */
};
struct gcl_tcp_addr {      /* 16 B: the tuple of a connection's segments, host order */
	uint32_t lip, rip;     /* as in gcl_txh_desc */
	uint16_t lport, rport;
	uint8_t  rcv_wscale;   /* the low five bits are used */
	uint8_t  pad[3];
};
struct gcl_ctlseg_out {                /* device, seg_cap elements each, aligned to their element */
	struct gcl_txh_desc *desc;         /* 16-B aligned */
	uint64_t *frame_off;
	uint32_t *seg_conn;
	uint8_t  *seg_kind;
	uint32_t *seg_src;
	uint64_t *totals;                  /* u64[2], required: wanted, written */
};
struct gcl_tick_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_tick_in); blocks: 0 = the library's choice, else
	                                      the number of contiguous ranges the connections are cut into (tests) */
	uint64_t now;                      /* us: the sweep's one clock reading */
	const struct gcl_tcp_tmr *tmr;     /* [nconn] */
	const struct gcl_tcp_conn *conn;   /* [nconn] */
	const struct gcl_tcp_addr *addr;   /* [nconn] */
	uint32_t nconn;                    /* <= 2^20 */
	uint32_t frame_stride;             /* bytes, >= GCL_CTL_MIN_STRIDE */
	uint64_t seg_cap;                  /* <= 2^31: the length of every per-segment output array */
	uint64_t frame_base;
};
struct gcl_tick_out {
	struct gcl_tcp_tmr_out *out_tmr;   /* [nconn] */
	struct gcl_ctlseg_out seg;
};
struct gcl_rxack_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_rxack_in); blocks as in gcl_tick_in */
	const uint32_t *order;             /* optional u32[m], as given to gcl_tcp_rx */
	uint64_t m;                        /* list entries, <= 2^31 */
	uint64_t n;                        /* the batch's packets: the length of sock */
	const uint32_t *sock;              /* u32[n] */
	const uint8_t  *verdict, *sflags;  /* u8[m], as gcl_tcp_rx wrote them */
	const uint32_t *rcv_nxt_after;     /* u32[m], as gcl_tcp_rx wrote it */
	const struct gcl_tcp_conn *conn;   /* [nconn]: the snapshot gcl_tcp_rx was given */
	const struct gcl_tcp_addr *addr;   /* [nconn] */
	uint32_t nconn;                    /* <= 2^20 */
	uint32_t frame_stride;             /* bytes, >= GCL_CTL_MIN_STRIDE */
	uint64_t seg_cap;                  /* <= 2^31 */
	uint64_t frame_base;
};
int gcl_tcp_tick_workspace(uint32_t nconn, uint32_t blocks, size_t *bytes);
int gcl_tcp_tick(struct gcl_ctx *ctx, const struct gcl_tick_in *in, const struct gcl_tick_out *out,
                 uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);
int gcl_tcp_rx_acks_workspace(uint64_t m, uint32_t blocks, size_t *bytes);
int gcl_tcp_rx_acks(struct gcl_ctx *ctx, const struct gcl_rxack_in *in, const struct gcl_ctlseg_out *out,
                    uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The control segments of a gcl_tcp_rx_states call: gcl_tcp_rx_ctl stands
 * where gcl_tcp_rx_acks stands and also emits the RSTs that send_rst
 * (runtime/net/tcp_in.c:54-62) sends, in list order:
 *
 *   gcl_tcp_rx_states -> gcl_tcp_rx_ctl -> gcl_tx_hdr -> gcl_l4_csum GCL_L4_FILL
 *
 * @in is gcl_rxack_in's fields with its own size and ev and rst_seq as
 * gcl_tcp_rx_states wrote them.  List entry j with verdict[j] ==
 * GCL_TCPRX_FAST emits at most one segment (every send_rst path goes to done
 * with do_ack false): an ACK when sflags[j] has GCL_TCPRX_SF_ACK_NOW, exactly
 * as gcl_tcp_rx_acks writes it; else with GCL_TCPS_RST in ev[j] a gcl_txh_desc
 * with proto 6, tcp_off 5, win 0, paylen 0, the tuple of addr[c], tcp_flags
 * 0x04, seq = rst_seq[j] and ack 0 (tcp_tx_raw_rst, tcp_out.c:98-128), seg_kind
 * GCL_CTL_RST; else with GCL_TCPS_RST_ACK tcp_flags 0x14, seq 0 and ack =
 * rst_seq[j] (tcp_tx_raw_rst_ack, :139-170), seg_kind GCL_CTL_RST_ACK.  The
 * guards (i below n, c below nconn), frame_off, seg_conn, seg_src = j, totals,
 * seg_cap, the workspace, the three launches (decide, the scan of the block
 * sums, emit) and @counts (GCL_RXACKC_WANTED, _WRITTEN, _SKIPPED) are
 * gcl_tcp_rx_acks': on a list without RSTs the two calls write the same bytes.
 * ev and rst_seq are among the arrays whose content causes no access outside
 * the given arrays.  -EINVAL for what gcl_tcp_rx_acks refuses, and with m > 0
 * a NULL ev or rst_seq, or a rst_seq that is not 4-B aligned.
 */
#define GCL_CTL_RST     2
#define GCL_CTL_RST_ACK 3
struct gcl_rxctl_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_rxctl_in) */
	const uint32_t *order;
	uint64_t m;
	uint64_t n;
	const uint32_t *sock;
	const uint8_t  *verdict, *sflags;
	const uint32_t *rcv_nxt_after;
	const struct gcl_tcp_conn *conn;
	const struct gcl_tcp_addr *addr;
	uint32_t nconn;
	uint32_t frame_stride;
	uint64_t seg_cap;
	uint64_t frame_base;
	const uint8_t  *ev;                /* u8[m], as gcl_tcp_rx_states wrote it */
	const uint32_t *rst_seq;           /* u32[m], as gcl_tcp_rx_states wrote it */
};
int gcl_tcp_rx_ctl_workspace(uint64_t m, uint32_t blocks, size_t *bytes);
int gcl_tcp_rx_ctl(struct gcl_ctx *ctx, const struct gcl_rxctl_in *in, const struct gcl_ctlseg_out *out,
                   uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The TCP retransmit queue: where the three TCP chains meet.  gcl_tx_seg cuts
 * segments to link into c->txq, gcl_tcp_rx moves snd_una (GCL_TCPRX_SF_ACKED)
 * and gcl_tcp_tick says when tcp_retransmit is due (GCL_TMRA_RETRANSMIT).  In
 * the reference the queue of sent but unacknowledged segments is then walked
 * one connection at a time under the connection lock: tcp_conn_ack
 * (runtime/net/tcp.c:217-238), tcp_tx_retransmit with tcp_tx_retransmit_one
 * (runtime/net/tcp_out.c:480-506, :388-444) and tcp_tx_fast_retransmit_start
 * (tcp_out.c:450-466).  gcl_tcp_txq does those walks for all connections of
 * one runtime at one clock reading and writes the retransmitted segments as
 * gcl_txh_desc records, so that
 *
 *   gcl_tx_seg -> (txq) -> gcl_tcp_rx / gcl_tcp_tick -> gcl_tcp_txq ->
 *   gcl_copy_batch -> gcl_tx_hdr -> gcl_l4_csum GCL_L4_FILL
 *
 * run on one stream.  It works on every context and touches no table.
 *
 * The queues come as a CSR: connection c owns entries [qoff[c], qoff[c + 1])
 * of ent and cold, in queue order (qoff non-decreasing, qoff[nconn] == nent).
 * ent holds what the walks read of every entry (m->seg_seq, m->seg_end,
 * m->timestamp), cold what only a retransmitted entry needs.  conn[c] gives
 * snd_una, rcv_nxt and rcv_wnd, addr[c] the tuple, want[c] (optional; NULL:
 * pops only) what the runtime would run: GCL_TXQ_W_RTO tcp_retransmit,
 * GCL_TXQ_W_FAST tcp_tx_fast_retransmit_start, GCL_TXQ_W_EXCL c->tx_exclusive.
 * wraps_* are those of inc/base/stddef.h: wraps_gt(a, b) is (int32_t)(b - a)
 * < 0.
 *
 * One connection, in the reference's order: tcp_retransmit runs
 * tcp_tx_retransmit over the whole queue and only then does tcp_write_finish
 * pop (tcp.c:1425-1444, :1309-1349).
 *   1. W_EXCL: nothing happens: no pops (tcp.c:224), no walk (tcp.c:1431
 *      waits), no fast retransmit (tcp_out.c:456).  GCL_TXQO_DEFERRED.
 *   2. W_RTO, the walk from entry 0: break at the first entry with now - ts <
 *      300000 (uint64_t arithmetic: ts > now counts as due, as in C);
 *      wraps_gte(snd_una, seg_end) means continue; otherwise the entry is
 *      WANTED: its timestamp becomes now and it is retransmitted (5).  The
 *      walk ends after the 16th segment (TCP_RETRANSMIT_BATCH:
 *      GCL_TXQO_BATCH), and at the first wanted entry whose segment would lie
 *      at or past seg_cap: that entry is GCL_TXQS_NOSPACE, its timestamp has
 *      moved, as after the -ENOMEM of tcp_out.c:410, and nothing is sent for
 *      it.
 *   3. Pops: nacked = the number of leading entries with !wraps_gt(seg_end,
 *      snd_una).
 *   4. W_FAST: entry nacked, the head after the pops, when there is one.  If
 *      the walk did not send it, its timestamp becomes now and it is sent BY
 *      COPY (tcp_out.c:462 raises ref, so :407 always copies); without room it
 *      is NOSPACE.
 *   5. A wanted entry (tcp_tx_retransmit_one): trim = wraps_lt(seg_seq,
 *      snd_una) ? snd_una - seg_seq : 0; seq = seg_seq + trim; paylen =
 *      seg_end - seq - ((tcp_flags & (SYN | FIN)) ? 1 : 0).  Its descriptor:
 *      the tuple of addr[c], proto 6, ecn 0, tcp_flags and tcp_off of the
 *      entry, seq, ack = rcv_nxt, win as a control segment's (above: the
 *      "fresher ack" of :435), paylen, pad 0.  With k its output position:
 *        in place (not GCL_TXQE_INFLIGHT, not the fast retransmit):
 *          frame_off[k] = cold.frame_off + trim: the headers go back in front
 *          of the bytes that stay; len[k] = 0, src_off[k] = cold.frame_off +
 *          54 + trim, dst_off[k] = frame_off[k] + 54 (nothing moves).
 *        by copy: frame_off[k] = frame_base + k * frame_stride, src_off[k] =
 *          cold.frame_off + 54 + trim, len[k] = 4 * (tcp_off - 5) + paylen,
 *          dst_off[k] = frame_off[k] + 54.
 *      REFUSED (GCL_TXQS_REFUSED: nothing is emitted, its timestamp has moved,
 *      it does not count towards the 16 and the walk goes on, like the
 *      mbuf_free; return 0 of :428): tcp_off outside 5..15; paylen, or a
 *      copy's len, above 65535; trim > 0 with tcp_off > 5; a copied frame (54
 *      + len) longer than frame_stride.  A refused entry asks for no room: it
 *      is REFUSED, not NOSPACE, wherever seg_cap lies.
 * Two departures from the reference.  It computes l4len before the partial-ACK
 * pull and never again (:395 against :431) and so seeds the checksum with the
 * untrimmed length: the descriptor carries the trimmed one.  And with options
 * and a partial ACK it pulls option bytes: such an entry is refused here (only
 * a SYN carries options and a SYN has sequence length 1, so consistent input
 * never gets there).  The test of :427 can hold for a wanted entry only when
 * seg_end lies exactly 2^31 past snd_una, which no consistent queue has: such
 * an entry is sent by the rules above and reported ACKED.
 *
 * Per connection out_conn[c], every byte written: nacked; nretx, the segments
 * written for it; first = min(the segments wanted by the connections before
 * it, seg_cap), the position of its first segment; head_ts, the timestamp of
 * entry nacked after the call (0 without one): the txq_ts of the next
 * gcl_tcp_tmr; flags: GCL_TXQO_EMPTY (nacked is the whole queue: clear
 * GCL_TMR_TXQ), DEFERRED, NOSPACE, BATCH, and GCL_TXQO_BADRANGE: a range that
 * is inverted or not inside [0, nent] is treated as an empty queue.
 * Per entry state[e], for every e of a valid range (an entry no range covers
 * is not written): GCL_TXQS_KEPT, ACKED (free it), RETX, RETX_COPY, NOSPACE or
 * REFUSED, the sent ones ORed with GCL_TXQS_TRIMMED when trim > 0 (the host
 * sets m->seg_seq = snd_una); every state from RETX on means m->timestamp =
 * now.  An ACKED entry that was also retransmitted is ACKED.
 * Per segment k < totals[1], in connection order and then queue order: desc,
 * frame_off, src_off, len and dst_off as above (the types of gcl_seg_out:
 * gcl_copy_batch passes over len 0), seg_conn[k] = c and seg_ent[k] = e.
 * Entries at and past totals[1] are not written.  totals[0] = the segments
 * wanted (what seg_cap should have been), totals[1] = min(wanted, seg_cap),
 * totals[2] = the sum of len[].
 *
 * @counts is a device u64[GCL_TXQC_NR], ACCUMULATED, may be NULL: ACKED
 * entries, RETX segments written, those COPIED and those TRIMMED, REFUSED
 * entries, NOSPACE and DEFERRED connections, and BYTES (totals[2]).
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * ent, cold, conn, addr, out_conn and desc to 16 B.  Asynchronous on
 * @hip_stream: three launches (decide, the scan of the block sums, emit)
 * ordered by the stream alone; no block waits for another and no atomic hands
 * out a position: atomics only add to counts and to the byte sum totals[2].
 * No allocation, no host synchronisation.  @workspace (device, 16-B aligned)
 * need not be zeroed and may be reused by the next call on the same stream.
 * nconn == 0 still writes totals.
 *
 * Guarantee: no content of qoff, ent, cold, conn, addr or want causes a read
 * outside the given arrays, or a write outside the first seg_cap elements of
 * the per-segment outputs, out_conn[0, nconn), state[0, nent), totals, counts
 * and the workspace.  Garbage qoff is included: decreasing values, or values
 * past nent.  Ranges that overlap, which only a decreasing qoff produces, are
 * each walked; state[e] of an entry two of them share is that of either.
 *
 * What stays with the runtime: the frees themselves, tcp_write_finish's
 * wake-ups, do_fast_retransmit's bookkeeping (the caller decides W_FAST;
 * gcl_tcp_rx_full's GCL_TCPX_FASTRTX says when),
 * writing the timestamps and seg_seq back, and the lock.
 *
 * gcl_tcp_txq_workspace - bytes of device scratch a call takes: 4 per block
 *   (in->blocks, or the cap GCL_TXQ_MAX_BLOCKS when blocks is 0), rounded up
 *   to 16.  -EINVAL for a NULL @bytes, nconn > 2^20 or blocks >
 *   GCL_TXQ_MAX_BLOCKS.
 * gcl_tcp_txq - -EINVAL for a NULL ctx, in or out; a wrong in->size; nconn >
 *   2^20; nent or seg_cap > 2^31; blocks > GCL_TXQ_MAX_BLOCKS; frame_stride <
 *   54; a NULL totals; with nconn > 0 a NULL qoff, conn, addr or out_conn; with
 *   nent > 0 a NULL ent, cold or state; with nconn > 0 and seg_cap > 0 a NULL
 *   per-segment output; any given array that is not aligned to its element; a
 *   NULL workspace, one that is not 16-B aligned or one smaller than
 *   gcl_tcp_txq_workspace says.  -EIO when a launch fails.
 */
/* want[c] */
#define GCL_TXQ_W_RTO      0x01  /* GCL_TMRA_RETRANSMIT fired: tcp_retransmit */
#define GCL_TXQ_W_FAST     0x02  /* tcp_tx_fast_retransmit_start */
#define GCL_TXQ_W_EXCL     0x04  /* c->tx_exclusive */
/* gcl_txq_cold.flags */
#define GCL_TXQE_INFLIGHT  0x01  /* atomic_read(&m->ref) != 1 */
/* state[e] */
#define GCL_TXQS_KEPT      0
#define GCL_TXQS_ACKED     1
#define GCL_TXQS_RETX      2
#define GCL_TXQS_RETX_COPY 3
#define GCL_TXQS_NOSPACE   4
#define GCL_TXQS_REFUSED   5
#define GCL_TXQS_TRIMMED   0x80
/* gcl_txq_conn_out.flags */
#define GCL_TXQO_EMPTY     0x01
#define GCL_TXQO_DEFERRED  0x02
#define GCL_TXQO_NOSPACE   0x04
#define GCL_TXQO_BATCH     0x08
#define GCL_TXQO_BADRANGE  0x10
#define GCL_TXQ_MAX_BLOCKS 1024    /* the cap on in->blocks */
#define GCL_TXQ_MAX_CONN (1u << 20)
enum { GCL_TXQC_ACKED = 0, GCL_TXQC_RETX, GCL_TXQC_COPIED, GCL_TXQC_TRIMMED, GCL_TXQC_REFUSED,
       GCL_TXQC_NOSPACE, GCL_TXQC_DEFERRED, GCL_TXQC_BYTES, GCL_TXQC_NR = 8 };
struct gcl_txq_ent {       /* 16 B: m->seg_seq, m->seg_end, m->timestamp */
	uint32_t seg_seq, seg_end;
	uint64_t ts;
};
struct gcl_txq_cold {      /* 16 B */
	uint64_t frame_off;    /* where the segment's Ethernet header lies in the tx region */
	uint8_t  tcp_flags, tcp_off;
	uint8_t  flags;        /* GCL_TXQE_* */
	uint8_t  pad[5];
};
struct gcl_txq_conn_out {  /* 32 B, 16-B aligned */
	uint64_t head_ts;
	uint32_t nacked, nretx, first;
	uint8_t  flags;        /* GCL_TXQO_* */
	uint8_t  pad[11];      /* written as 0 */
};
struct gcl_txq_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_txq_in); blocks as in gcl_tick_in */
	uint64_t now;                      /* us: the call's one clock reading */
	const uint32_t *qoff;              /* u32[nconn + 1] */
	const struct gcl_txq_ent *ent;     /* [nent] */
	const struct gcl_txq_cold *cold;   /* [nent] */
	uint64_t nent;                     /* <= 2^31 */
	const struct gcl_tcp_conn *conn;   /* [nconn] */
	const struct gcl_tcp_addr *addr;   /* [nconn] */
	const uint8_t *want;               /* optional u8[nconn] */
	uint32_t nconn;                    /* <= 2^20 */
	uint32_t frame_stride;             /* bytes, >= GCL_CTL_MIN_STRIDE: the slots of copied segments */
	uint64_t seg_cap;                  /* <= 2^31: the length of every per-segment output array */
	uint64_t frame_base;
};
struct gcl_txq_out {                   /* device, aligned to their element */
	struct gcl_txq_conn_out *out_conn; /* [nconn] */
	uint8_t  *state;                   /* [nent] */
	struct gcl_txh_desc *desc;         /* [seg_cap], 16-B aligned */
	uint64_t *frame_off, *src_off;     /* [seg_cap] */
	uint16_t *len;                     /* [seg_cap] */
	uint64_t *dst_off;                 /* [seg_cap] */
	uint32_t *seg_conn, *seg_ent;      /* [seg_cap] */
	uint64_t *totals;                  /* u64[3], required: wanted, written, bytes to copy */
};
int gcl_tcp_txq_workspace(uint32_t nconn, uint32_t blocks, size_t *bytes);
int gcl_tcp_txq(struct gcl_ctx *ctx, const struct gcl_txq_in *in, const struct gcl_txq_out *out,
                uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The passive open: the two answers of gcl_sock_lookup that no other call
 * takes.  A TCP packet whose cookie is a listener goes to tcp_queue_recv ->
 * tcp_rx_listener (runtime/net/tcp.c:488-522, runtime/net/tcp_in.c:614-694),
 * one whose lookup missed to net_rx_trans -> tcp_rx_closed (runtime/net/
 * transport.c:413-419, tcp_in.c:696-723).  gcl_tcp_rx_open runs one runtime's
 * list through both and writes the new connections, their SYN|ACKs with the
 * option bytes, and the RSTs a closed port or a listener answers:
 *
 *   gcl_classify -> gcl_sock_lookup -> gcl_l4_csum VERIFY -> gcl_plan ->
 *   { gcl_tcp_rx_states -> gcl_tcp_rx_ctl,  gcl_tcp_rx_open } -> gcl_tx_hdr ->
 *   gcl_l4_csum GCL_L4_FILL
 *
 * List entry j names packet i = in->order ? in->order[j] : j.  o, avail, L and
 * tot are gcl_l4_csum's, frames are addressed as gcl_l4_payload addresses them
 * (b->pkt_len REQUIRED), a byte at or past frames_len reads 0.  A packet is
 * TCP-ELIGIBLE when it is L4-eligible as gcl_l4_csum says with protocol 6,
 * except that tot need only be 20 (net_rx_one's length test): line 3 is where
 * the reference finds the TCP header too short.  Cookie c with listen_base <=
 * c < listen_base + nlisten (and c <= GCL_SOCK_COOKIE_MAX) is listener
 * c - listen_base; the cookie namespace is the caller's.  seq, ack, off and
 * flags are frame bytes 38-41, 42-45, 46 >> 4 and 47; lip / lport are the
 * packet's daddr / dport, rip / rport its saddr / sport.  verdict[j] is the
 * first line that matches:
 *   1. i >= b->n                                              GCL_OPEN_OOR
 *   2. sock[i] is neither GCL_SOCK_MISS nor a listener cookie
 *      (GCL_SOCK_NA, connections, GCL_SOCK_MULTI: the runtime
 *      picks among reuse_port listeners by thread id), the
 *      packet is not TCP-eligible, or l4_status is given and
 *      says GCL_L4_BAD (what gcl_tcp_rx would not take)       GCL_OPEN_NA
 *   3. tot - 20 < 20 or L < 54: mbuf_pull_hdr_or_null fails   GCL_OPEN_SHORT
 *   4. GCL_SOCK_MISS, tcp_rx_closed (tcp_in.c:708-722):
 *      RST                                                    GCL_OPEN_CLOSED_DROP
 *      ACK: rst_seq[j] = ack                                  GCL_OPEN_CLOSED_RST
 *      else: rst_seq[j] = seq + (tot - 20 - 4 * off) mod 2^32,
 *        as written: not checked against wrap, SYN and FIN
 *        not counted                                          GCL_OPEN_CLOSED_RST_ACK
 *   5. listener l, the entries taken in list order:
 *      a. an earlier entry k < j with verdict ACCEPT has the
 *         same (lip, lport, rip, rport) and listener:
 *         later_of[j] = k.  tcp_conn_attach made k's connection
 *         the 5-tuple match of this packet, whatever its flags;
 *         the backlog is not touched.  The caller runs it
 *         through gcl_tcp_rx_states once open[] is installed    GCL_OPEN_LATER
 *      b. GCL_LISTEN_SHUTDOWN, or the running backlog is 0
 *         (tcp.c:496): listen[l].backlog minus the ACCEPTs of l
 *         before j; every other outcome gives its slot back
 *         (:505-509).  Silent: an ACK gets no RST here          GCL_OPEN_FULL
 *      c. tcp_rx_listener (tcp_in.c:638-656): RST               GCL_OPEN_DROP
 *         ACK: rst_seq[j] = ack                                 GCL_OPEN_RST
 *         no SYN; tot - 20 != 4 * off (off < 5, or a SYN with
 *         data); an option byte at or past L                    GCL_OPEN_DROP
 *      d. tcp_parse_options meets an option other than EOL or
 *         NOP whose length byte is 0                            GCL_OPEN_BADOPT
 *      e. otherwise                                             GCL_OPEN_ACCEPT
 * (The listener is part of 5a's comparison.  gcl_sock_lookup gives one tuple
 * one listener, so this matters only for a sock array that is not its.)
 * Line 5d is the ONE PLACE THE CALL DECLINES TO FOLLOW THE REFERENCE: on that
 * input tcp_parse_options does not return (ptr += opsize - 2; len -= opsize
 * makes no progress), so there is nothing to follow.
 *
 * The option walk is tcp_parse_options (tcp_in.c:298-348) as written over the
 * 4 * off - 20 option bytes: EOL stops it, NOP takes one byte, MSS counts only
 * with length 4, WSCALE only with length 3 and is clamped to 14, any other
 * length still advances by that length (a length of 1 steps back onto the
 * length byte), the last occurrence wins, len may go negative and that ends
 * the walk.  A read at or past the end of the option bytes reads 0 (the
 * reference reads what follows in the mbuf; the two differ only on malformed
 * options), so an opcode in the last byte is line 5d.  Then snd_mss =
 * min(max(mss, 88), rcv_mss), or 1460 (tcp_calculate_mss(ETH_DEFAULT_MTU))
 * when no MSS counted; snd_wscale the clamped value or 0; without WSCALE
 * rcv_wnd = winmax = min(winmax, 65535) and rcv_wscale = 0, with it rcv_wnd =
 * winmax and rcv_wscale as the listener gives it; opt_en the options that
 * counted.  snd_wscale and the WSCALE bit are pinned to the reference's own
 * tcp_in.c; snd_mss is not visible through that driver and rests on the tests'
 * independent model and hand-derived cases.
 *
 * An ACCEPT writes open[k], k counting the ACCEPTs in list order: src = j,
 * irs = seq, rcv_nxt = irs + 1, iss = in->iss[j] (read only for an ACCEPT),
 * snd_una = iss, snd_nxt = iss + 1 (after tcp_tx_ctl), state SYN_RECEIVED, pad
 * 0: what gcl_sock_entry, gcl_tcp_conn, gcl_tcp_addr and gcl_tcp_tmr.state
 * need to install the connection before the next batch.  totals[0] = the
 * ACCEPTs, totals[1] = min(ACCEPTs, open_cap); a record at or past open_cap
 * is not written, its entry is an ACCEPT all the same and counts in
 * GCL_OPENC_NOSPACE.  backlog_out[l] = listen[l].backlog minus l's ACCEPTs.
 * later_of[j] is 0xFFFFFFFF and rst_seq[j] 0 where the rule names none.
 *
 * Segments go through @seg in list order, at most one per entry, segment k at
 * frame_off = frame_base + k * frame_stride (mod 2^64), seg_src = j:
 *   GCL_OPEN_RST, GCL_OPEN_CLOSED_RST      GCL_CTL_RST, and
 *   GCL_OPEN_CLOSED_RST_ACK                GCL_CTL_RST_ACK, the gcl_txh_desc
 *     exactly as gcl_tcp_rx_ctl writes the two kinds, with lip = the packet's
 *     own daddr and rip its saddr; seg_conn 0xFFFFFFFF
 *   GCL_OPEN_ACCEPT                        GCL_CTL_SYNACK: proto 6, tcp_flags
 *     0x12, seq = iss, ack = irs + 1, paylen 0, tcp_off = 5 + the options in
 *     opt_en, win = (uint16_t)(rcv_wnd >> (rcv_wscale & 31)) (tcp_out.c:74);
 *     seg_conn = the index into open[].  gcl_tx_hdr leaves the option bytes
 *     to its caller, so this call writes them at tx_frames[frame_off + 54 ..]
 *     in tcp_put_options' order (tcp_out.c:230-251): 01 03 03 rcv_wscale when
 *     WSCALE is enabled, then 02 04 hi(rcv_mss) lo(rcv_mss) when MSS is; one
 *     byte store each, and nothing else in the frame.
 * Segment k is written exactly when k < seg_cap and its slot [frame_off,
 * frame_off + frame_stride) lies inside tx_frames_len, which with an
 * increasing frame_off is k < (tx_frames_len - frame_base) / frame_stride; a
 * frame_base past tx_frames_len writes none.  seg->totals[0] = the segments
 * wanted, [1] = those written, the m of gcl_tx_hdr; the others count in
 * GCL_OPENC_SEGSKIP.  frame_stride is at least GCL_CTL_MIN_STRIDE + 8.
 *
 * @counts is a device u64[GCL_OPENC_NR], ACCUMULATED, may be NULL: one slot
 * per verdict (slot = verdict; per call they sum to m), SEGS (written),
 * SEGSKIP and NOSPACE.  in->blocks: 0 is the library's choice, else the number
 * of contiguous ranges the list is cut into; in->hash_slots: 0 is the
 * library's choice, else the power-of-two size of the tuple table, at least
 * 2 * m (both for tests).  The result depends on neither,
 * nor on which lane wins a race: the tuple table keeps the smallest list
 * index of every tuple, per-listener counts are sums, and positions come from
 * scans.
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * listen and open to 16 B.  Asynchronous on @hip_stream, launches ordered by
 * the stream alone, no allocation, no host synchronisation.  @workspace
 * (device, 16-B aligned) need not be zeroed.  m == 0 is a no-op.
 *
 * Guarantee: no content of frames, offs, pkt_len, order, sock, l4_status,
 * listen or iss causes a read outside frames[0, frames_len) and the given
 * arrays, or a write outside the m-element outputs, open[0, open_cap),
 * backlog_out[0, nlisten), the first seg_cap elements of the segment arrays,
 * the totals, counts, the workspace and the option bytes named above.  The
 * walk is bounded: at most 40 option bytes.
 *
 * What stays with the runtime: tcp_conn_alloc's memory and iss, installing
 * open[] (gcl_sock_set, the conn / addr / tmr arrays, the accept queue and its
 * wake-up), replaying LATER entries, SYN_SENT (the active open), and reuse_port.
 *
 * gcl_tcp_rx_open_workspace - bytes of device scratch a call takes.  -EINVAL
 *   for a NULL @bytes, m > 2^31, nlisten > GCL_OPEN_MAX_LISTEN, blocks >
 *   GCL_OPEN_MAX_BLOCKS, or a hash_slots that is neither 0 nor a power of two
 *   of at least 2 * m.
 * gcl_tcp_rx_open - -EINVAL for a NULL ctx, b, in, out or seg; a wrong
 *   in->size; order == NULL with m != b->n; what the workspace call refuses;
 *   seg_cap or open_cap > 2^31; frame_stride < GCL_CTL_MIN_STRIDE + 8; a NULL
 *   seg->totals or out->totals; with nlisten > 0 a NULL listen or
 *   backlog_out; with m > 0 a NULL sock, iss, verdict, later_of or rst_seq,
 *   with open_cap > 0 also a NULL open, with seg_cap > 0 a NULL per-segment
 *   array, with tx_frames_len > 0 a NULL tx_frames; any given array that is
 *   not aligned to its element; a NULL workspace, one that is not 16-B
 *   aligned or one that is too small; and, when m > 0, what gcl_l4_payload
 *   refuses of a batch.  -EIO when a launch fails.
 */
/* verdict[j], and the counter slot of each */
#define GCL_OPEN_NA             0
#define GCL_OPEN_OOR            1
#define GCL_OPEN_SHORT          2
#define GCL_OPEN_CLOSED_DROP    3
#define GCL_OPEN_CLOSED_RST     4
#define GCL_OPEN_CLOSED_RST_ACK 5
#define GCL_OPEN_LATER          6
#define GCL_OPEN_FULL           7
#define GCL_OPEN_DROP           8
#define GCL_OPEN_RST            9
#define GCL_OPEN_BADOPT         10
#define GCL_OPEN_ACCEPT         11
#define GCL_OPEN_NR_VERDICTS    12
enum { GCL_OPENC_SEGS = 12, GCL_OPENC_SEGSKIP, GCL_OPENC_NOSPACE, GCL_OPENC_NR = 16 };
#define GCL_OPEN_MAX_LISTEN 4096   /* the cap on in->nlisten */
#define GCL_OPEN_MAX_BLOCKS 1024   /* the cap on in->blocks */
#define GCL_CTL_SYNACK      4      /* seg_kind[k] beside GCL_CTL_ACK .. GCL_CTL_RST_ACK */
#define GCL_TCP_STATE_SYN_RECEIVED 1
#define GCL_LISTEN_SHUTDOWN 0x01   /* gcl_tcp_listen.flags: q->shutdown */
/* gcl_tcp_open.opt_en: TCP_OPTION_MSS and TCP_OPTION_WSCALE (runtime/net/tcp.h:165-166) */
#define GCL_OPEN_OPT_MSS    0x01
#define GCL_OPEN_OPT_WSCALE 0x02
struct gcl_tcp_listen {    /* 16 B, 16-B aligned, host order: one listener */
	uint32_t backlog;      /* q->backlog on entry */
	uint32_t winmax;       /* tcp_default_win */
	uint16_t rcv_mss;      /* tcp_calculate_mss(net_get_mtu()) */
	uint8_t  rcv_wscale;   /* tcp_scale_window(winmax) */
	uint8_t  flags;        /* GCL_LISTEN_* */
	uint32_t pad;
};
struct gcl_tcp_open {      /* 64 B, 16-B aligned, host order: the connection an ACCEPT opens */
	uint32_t src;          /* the list position j of its SYN */
	uint32_t listener;
	uint32_t lip, rip;
	uint16_t lport, rport;
	uint32_t irs, rcv_nxt, iss;
	uint32_t snd_una, snd_nxt, rcv_wnd, winmax;
	uint16_t snd_mss;
	uint8_t  snd_wscale, rcv_wscale;
	uint8_t  opt_en;       /* GCL_OPEN_OPT_* */
	uint8_t  state;        /* GCL_TCP_STATE_SYN_RECEIVED */
	uint8_t  pad[10];      /* written as 0 */
};
struct gcl_tcpopen_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_tcpopen_in) */
	const uint32_t *order;             /* optional u32[m]; NULL: m == b->n and i = j */
	uint64_t m;                        /* list entries, <= 2^31 */
	const uint32_t *sock;              /* u32[b->n], as gcl_sock_lookup wrote it */
	const uint8_t  *l4_status;         /* optional u8[b->n], as GCL_L4_VERIFY wrote it */
	uint32_t hash_slots;               /* 0: the library's choice */
	uint32_t listen_base, nlisten;
	uint32_t frame_stride;             /* bytes, >= GCL_CTL_MIN_STRIDE + 8 */
	const struct gcl_tcp_listen *listen; /* [nlisten] */
	const uint32_t *iss;               /* u32[m]: the pcb.iss tcp_conn_alloc would draw for entry j */
	uint64_t seg_cap, frame_base;      /* as in gcl_rxctl_in */
	uint64_t open_cap;                 /* <= 2^31: the length of open[] */
	uint8_t *tx_frames;                /* the tx region gcl_tx_hdr will be given */
	uint64_t tx_frames_len;
};
struct gcl_tcpopen_out {               /* device, aligned to their element */
	uint8_t  *verdict;                 /* [m] */
	uint32_t *later_of, *rst_seq;      /* [m] */
	struct gcl_tcp_open *open;         /* [open_cap] */
	uint32_t *backlog_out;             /* [nlisten] */
	uint64_t *totals;                  /* u64[2], required: opens wanted, written */
};
int gcl_tcp_rx_open_workspace(uint64_t m, uint32_t nlisten, uint32_t blocks, uint32_t hash_slots, size_t *bytes);
int gcl_tcp_rx_open(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_tcpopen_in *in,
                    const struct gcl_tcpopen_out *out, const struct gcl_ctlseg_out *seg, uint64_t *counts,
                    void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * UDP receive: the step behind gcl_l4_payload for UDP.  udp_conn_recv
 * (runtime/net/udp.c:79-107) takes inq_lock, drops the datagram when the
 * socket's ingress queue is full, in error or shut down, and otherwise pushes
 * it, sets POLLIN when the queue was empty and signals a waiter;
 * udp_par_recv (udp.c:811-840) hands a spawner's datagram to a new thread.
 * gcl_udp_rx runs every UDP socket's datagrams of one runtime's list, in
 * arrival order, through that step on the GPU, and lays the datagrams each
 * socket took out contiguously and in arrival order:
 *
 *   gcl_classify -> gcl_sock_lookup -> gcl_l4_csum VERIFY -> gcl_plan ->
 *   gcl_l4_payload -> gcl_udp_rx -> gcl_copy_batch (src_off from
 *   gcl_l4_payload; len = copy_len and dst_off from this call).
 *
 * One call serves ONE runtime, as gcl_tcp_rx does: @in->order / m are that
 * runtime's range of a plan.  A runtime's cookies are shared by its TCP
 * connections, its listeners and its UDP sockets, so cookie c with
 * sock_base <= c < sock_base + nsock names @in->usock[c - sock_base] (as
 * gcl_tcp_rx_open has listen_base).  It works on every context and touches no
 * table.
 *
 * List entry j names packet i = in->order ? in->order[j] : j.  It is a
 * DATAGRAM exactly when gcl_l4_payload, given the same sock and l4_status,
 * keeps it as GCL_PAY_UDP (the very function decides, gcl_pay_rule; it keeps no
 * UDP packet with tot < 28, which is mbuf_pull_hdr_or_null failing, udp.c:84
 * and :820); len is gcl_l4_payload's len.  The verdict of entry j is the first
 * line that matches, the entries of a socket taken in list order:
 *   not a datagram (OOR, NA, TCP, BADCSUM, NOSOCK)           GCL_UDPRX_NA
 *   the cookie lies outside [sock_base, sock_base + nsock)   GCL_UDPRX_NOSOCK
 *   GCL_UDPS_SPAWNER (udp_par_recv: no cap; ERR and
 *     SHUTDOWN are not looked at)                            GCL_UDPRX_SPAWN
 *   GCL_UDPS_ERR or GCL_UDPS_SHUTDOWN (udp.c:91, mbuf_drop)  GCL_UDPRX_CLOSED
 *   the running inq_len >= inq_cap (udp.c:91)                GCL_UDPRX_FULL
 *   otherwise: pushed, the running inq_len++                 GCL_UDPRX_QUEUED
 * The running inq_len starts at usock[s].inq_len and only a QUEUED entry moves
 * it; both words are the reference's ints and are compared as signed, so a
 * socket that enters with inq_cap <= inq_len (negative values included) has
 * every entry FULL, and nothing overflows.  The call works on a snapshot: no
 * udp_read pops during it.  A datagram of len 0 is a datagram and takes a slot.
 *
 * Per-entry outputs (m elements each): verdict; sflags, GCL_UDPRX_SF_POLLIN on
 * the QUEUED entry that found the running inq_len == 0 (udp.c:99-100);
 * copy_len, len for QUEUED and SPAWN and 0 otherwise; dst_off (0 when nothing
 * is copied); rec_idx, the entry's record or 0xFFFFFFFF.  Per socket,
 * out_sock[s] holds inq_len after the list, ntaken (QUEUED or SPAWN: the
 * runtime signals inq_wq that many times), ndropped (FULL + CLOSED) and
 * GCL_UDPRX_SF_POLLIN in flags when some entry set it; a socket with no entry
 * gets its inq_len back with zero counts.  rec_off[0, nsock] and
 * sock_off[0, nsock] are the prefix sums over the sockets of ntaken and of the
 * padded bytes taken, the last element the total.
 *
 * The layout, with pad() as in gcl_l4_payload and in->align: the k-th taken
 * datagram of socket s, in arrival order, is rec[rec_off[s] + k] (dst_off,
 * rip and rport in host order, len: what udp_read_from, udp.c:373-379, and
 * udp_spawn_data, :833-838, need), and its bytes go to dst_off = sock_off[s] +
 * the sum of pad(len) over the k taken before it.  gcl_copy_batch with
 * copy_len and dst_off then leaves every socket's queue as one contiguous run
 * of datagrams in arrival order; a dropped datagram is not copied.  Records at
 * and past rec_off[nsock] are not written.
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * usock, out_sock and rec to 16 B.  @counts is a device u64[GCL_UDPRXC_NR],
 * ACCUMULATED, may be NULL: the six verdicts (per call they sum to m), BYTES
 * (the sum of copy_len) and POLLINS.  Frames are addressed as gcl_l4_payload
 * addresses them.
 *
 * Guarantee: no content of frames, offs, pkt_len, order, sock, l4_status or
 * usock causes a read outside frames[0, frames_len) or the given arrays
 * (order[0, m), the n-element per-packet arrays, usock[0, nsock)), or a write
 * outside the m-element outputs, out_sock[0, nsock), rec_off[0, nsock],
 * sock_off[0, nsock], counts and the workspace.
 *
 * What stays with the runtime: inq_lock and writing inq_len back (usock must
 * be a snapshot no core changes meanwhile), linking the mbufs, the
 * waitq_signals (ntaken) and poll_set (POLLIN), thread_create_with_buf and its
 * failure drop for a spawner's datagrams, udp_conn_err, and the reads.
 *
 * gcl_udp_rx_workspace - bytes of device scratch a call takes for m entries,
 *   nsock sockets and in->blocks = @blocks.  -EINVAL for a NULL @bytes,
 *   m > 2^31, nsock > GCL_SOCK_MAX_ENTRIES or blocks > GCL_UDPRX_MAX_BLOCKS.
 * gcl_udp_rx - asynchronous on @hip_stream: launches ordered by the stream
 *   alone; no block waits for another and no atomic's order decides a result.
 *   No allocation, no host synchronisation.  @workspace (device, 16-B aligned)
 *   need not be zeroed and may be reused by the next call on the same stream.
 *   m == 0 still writes out_sock, rec_off and sock_off.  -EINVAL for a NULL
 *   ctx, b, in or out; a wrong in->size; a bad align; order == NULL with
 *   m != b->n; m > 2^31; nsock > GCL_SOCK_MAX_ENTRIES; a NULL sock; with
 *   nsock > 0 a NULL usock or out_sock; a NULL rec_off or sock_off; with m > 0
 *   a NULL verdict, sflags, copy_len, dst_off, rec_idx or rec; any given array
 *   that is not aligned to its element (usock, out_sock, rec: 16 B);
 *   blocks > GCL_UDPRX_MAX_BLOCKS; a NULL workspace, one that is not 16-B
 *   aligned or one smaller than gcl_udp_rx_workspace says; and, when m > 0,
 *   what gcl_l4_payload refuses of a batch.  -EIO when a launch fails.
 */
/* verdict[j], and the first six counter slots */
#define GCL_UDPRX_QUEUED 0
#define GCL_UDPRX_SPAWN  1
#define GCL_UDPRX_FULL   2
#define GCL_UDPRX_CLOSED 3
#define GCL_UDPRX_NOSOCK 4
#define GCL_UDPRX_NA     5
#define GCL_UDPRX_NR_VERDICTS 6
#define GCL_UDPRX_MAX_BLOCKS 1024  /* the cap on in->blocks */
enum { GCL_UDPRXC_BYTES = 6, GCL_UDPRXC_POLLINS = 7, GCL_UDPRXC_NR = 8 };
/* sflags[j] and gcl_udp_sock_out.flags */
#define GCL_UDPRX_SF_POLLIN 0x01   /* poll_set(&c->poll_src, POLLIN) */
/* gcl_udp_sock.flags */
#define GCL_UDPS_SHUTDOWN 0x01     /* c->shutdown */
#define GCL_UDPS_ERR      0x02     /* c->inq_err != 0 */
#define GCL_UDPS_SPAWNER  0x04     /* the entry is a udpspawner_t */
struct gcl_udp_sock {      /* 16 B, 16-B aligned, host order: what udp_conn_recv reads */
	int32_t inq_len, inq_cap;
	uint8_t flags;         /* GCL_UDPS_* */
	uint8_t pad[7];
};
struct gcl_udp_sock_out {  /* 16 B, 16-B aligned */
	int32_t  inq_len;      /* after the list */
	uint32_t ntaken;       /* QUEUED or SPAWN */
	uint32_t ndropped;     /* FULL + CLOSED */
	uint8_t  flags;        /* GCL_UDPRX_SF_POLLIN */
	uint8_t  pad[3];       /* written as 0 */
};
struct gcl_udp_rec {       /* 16 B, 16-B aligned, host order: one taken datagram */
	uint64_t dst_off;
	uint32_t rip;
	uint16_t rport, len;
};
struct gcl_udprx_in {
	uint32_t size, align;            /* sizeof(struct gcl_udprx_in); align as in gcl_pay_in */
	const uint32_t *order;           /* optional u32[m]; NULL: m == b->n and i = j */
	uint64_t m;                      /* list entries, <= 2^31 */
	const uint32_t *sock;            /* REQUIRED u32[n], as gcl_sock_lookup wrote it */
	const uint8_t  *l4_status;       /* optional u8[n], as GCL_L4_VERIFY wrote it */
	const struct gcl_udp_sock *usock; /* [nsock] */
	uint32_t nsock;                  /* <= GCL_SOCK_MAX_ENTRIES */
	uint32_t sock_base;              /* the cookie of usock[0] */
	uint32_t blocks;                 /* 0: the library's choice; else the number of contiguous
	                                    list ranges the grouping is cut into (tests) */
	uint32_t pad;
};
struct gcl_udprx_out {               /* device, aligned to their element */
	uint8_t  *verdict, *sflags;      /* [m] */
	uint16_t *copy_len;              /* [m] */
	uint64_t *dst_off;               /* [m] */
	uint32_t *rec_idx;               /* [m] */
	struct gcl_udp_rec *rec;         /* [m]; rec_off[nsock] of them are written */
	struct gcl_udp_sock_out *out_sock; /* [nsock] */
	uint32_t *rec_off;               /* u32[nsock + 1] */
	uint64_t *sock_off;              /* u64[nsock + 1] */
};
int gcl_udp_rx_workspace(uint64_t m, uint32_t nsock, uint32_t blocks, size_t *bytes);
int gcl_udp_rx(struct gcl_ctx *ctx, const struct gcl_batch *b, const struct gcl_udprx_in *in,
               const struct gcl_udprx_out *out, uint64_t *counts,
               void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The socket reads of TCP: the step between the receive chain and the
 * application.  The gcl_tcp_rx* calls decide which segments a connection
 * accepts and gcl_copy_batch leaves their bytes lying in sequence order;
 * tcp_read / tcp_readv (runtime/net/tcp.c: tcp_wait_rx :850-876, tcp_read_wait
 * :878-934, tcp_read_wait_peek :963-988, copy_mbufs_to_buf :1013-1038,
 * copy_into_iov :1133-1185, tcp_conn_shutdown_rx :1492-1502) then take them
 * off c->rxq into the application's buffer, give the window back and send the
 * window-update ACK (tcp_tx_ack with __tcp_add_tcphdr's tx_last_ack and
 * tx_last_win, tcp_out.c:59-61).  gcl_tcp_read does that for every connection
 * of one runtime at one instant, on a snapshot:
 *
 *   gcl_tcp_rx* -> gcl_copy_batch -> (rxq) -> gcl_tcp_read -> gcl_copy_batch
 *   (src_off, len, dst_off) ; the ACKs -> gcl_tx_hdr -> gcl_l4_csum GCL_L4_FILL
 *
 * It works on every context and touches no table.
 *
 * The receive queues come as a CSR like gcl_tcp_txq's: connection c owns
 * entries [qoff[c], qoff[c + 1]) of ent in queue order; an entry says where
 * the mbuf's data lies in the source region (off), mbuf_length (len) and
 * GCL_RDQE_FIN for m->flags & TCP_FIN.  dst_off[j] and copy_len[j] of a
 * gcl_tcp_rx* call become off and len directly.  The read of connection c is
 * rd[c]: flags (GCL_RD_*), the words of the ACK test, c->err, and its buffer
 * (dst_off, len).  With voff given the buffer is instead the vectors
 * [voff[c], voff[c + 1]) of iov, the read's length L their summed len
 * (iov_len()), and rd[c].dst_off and rd[c].len are ignored.  A range of qoff
 * or voff that is inverted or not inside [0, nent] ([0, nvec]) makes the
 * connection GCL_RDS_BADRANGE: it is not read, as if GCL_RD_WANT were clear.
 *
 * One connection; n is its queue's length, A_i the summed len of its first i
 * entries, L the read's length:
 *   1. no GCL_RD_WANT: status NONE, nothing changes.
 *   2. tcp_wait_rx: not RX_CLOSED, and RX_EXCL or n == 0: with NONBLOCK status
 *      AGAIN, ret -11 (-EAGAIN); else status BLOCK, ret 0 (the waitq_wait
 *      stays with the runtime).  Nothing changes.
 *   3. RX_CLOSED: status CLOSED, ret = -(int64_t)err, nothing changes.
 *   4. GCL_RD_PEEK (tcp_read_wait_peek): ret = min(A_n, L); FIN flags are not
 *      looked at, nothing is popped, rcv_wnd stays and no ACK is sent; the
 *      bytes are copied (5d); GCL_RDO_RXWAKE (tcp_exclusive_finish).  With
 *      ret == 0 the reference returns with rx_exclusive set and never clears
 *      it: that case reports GCL_RDO_EXCL_LEFT instead of RXWAKE.  Status DONE.
 *   5. tcp_read_wait, as the host twin walks it:
 *      a. while readlen < L: take the top entry, with none stop.  With FIN:
 *         tcp_conn_shutdown_rx (GCL_RDO_RX_CLOSED), and if its len is 0 stop,
 *         the entry stays queued.  If L - readlen < len the entry is pulled by
 *         pull = L - readlen (GCL_RDO_PARTIAL and RXWAKE), readlen = L, stop.
 *         Otherwise pop it (npop) and add its len.
 *      b. rcv_wnd += readlen (mod 2^32); GCL_RDO_ACK iff wraps_gte(rcv_nxt +
 *         rcv_wnd, tx_last_ack + tx_last_win + winmax / 4), for L == 0 too.
 *      c. GCL_RDO_POLLIN_CLEAR iff npop == n.
 *      d. The copy items.  With ret > 0: ne is the smallest i >= 1 with A_i >=
 *         ret, nv the same over the vectors' running sums B_j (without voff
 *         the one vector (rd.dst_off, rd.len)).  The cuts are the multiset
 *         {A_1..A_{ne-1}} + {B_1..B_{nv-1}}, sorted, an entry cut before an
 *         equal vector cut; with 0 in front and ret behind they bound exactly
 *         ne + nv - 1 items.  Item t spans [c_t, c_{t+1}) of the stream and
 *         lies in entry i and vector j: src_off = ent.off + (c_t - A_i),
 *         dst_off = iov.off + (c_t - B_j), len = c_{t+1} - c_t (it fits a
 *         uint16_t: an item lies in one entry), item_conn = c, item_ent = the
 *         entry's index in ent.  Coinciding cuts and zero-length entries and
 *         vectors give len 0 items, which gcl_copy_batch passes over.  With
 *         ret == 0 there are none.  A connection takes at most n + its vector
 *         count, so item_cap = nent + max(nvec, nconn) always suffices.
 *      e. status DONE, ret = readlen.
 *    The kernels use 5a's closed form: z = the first zero-length FIN entry or
 *    n; if A_z >= L, npop = the smallest i with A_i >= L and pull = 0, except
 *    that with A_i > L npop = i - 1 and pull = L - A_{i-1}; else npop = z and
 *    ret = A_z.  RX_CLOSED iff an entry examined as top has FIN: entries
 *    0..npop-1, and entry npop when it exists and the walk did not end on
 *    readlen >= L right after a pop.  L == 0 examines none.
 *
 * A connection with GCL_RDO_ACK emits one control segment (the rule of
 * gcl_tcp_tick above), in connection order: tcp_flags 0x10, seq =
 * conn[c].snd_nxt, ack = conn[c].rcv_nxt, win from rcv_wnd AFTER the read,
 * seg_kind GCL_CTL_ACK, seg_src = seg_conn = c, frame_off = frame_base + k *
 * frame_stride.  A written segment implies tx_last_ack = rcv_nxt and
 * tx_last_win = the new rcv_wnd for the host to store.  A connection whose
 * ACK lies at or past seg_cap gets GCL_RDO_SEG_NOSPACE; its other words
 * change all the same, like the -ENOMEM of tcp_tx_ack.
 *
 * out_conn[c], every byte written: ret; npop and pull (the host pops npop
 * entries and pulls pull bytes off the next: mbuf_pull, seg_seq += pull);
 * rcv_wnd after the read; first_item = min(the items wanted by the
 * connections before it, item_cap); nitems, the items written for it; status;
 * flags.  Per item k < min(wanted, item_cap), in connection order and then
 * stream order: src_off, len, dst_off (the types gcl_copy_batch takes),
 * item_conn, item_ent; items at and past item_cap are not written and the
 * connection gets GCL_RDO_ITEM_NOSPACE.  totals u64[4]: items wanted, items
 * written, the bytes of the written items, the sum of the DONE connections'
 * ret (a CLOSED connection's -err is no length, whatever its sign).
 * seg.totals u64[2] as for every control-segment call.
 *
 * @counts is a device u64[GCL_RDC_NR], ACCUMULATED, may be NULL: DONE, AGAIN,
 * BLOCK and CLOSED connections, PEEKS, POPPED entries, PARTIAL and RX_CLOSED
 * connections, ACKS written, ITEMS written, their BYTES, and NOSPACE
 * connections (either NOSPACE flag).
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * conn, addr, rd, ent, iov, out_conn and desc to 16 B.  Asynchronous on
 * @hip_stream: launches ordered by the stream alone (two three-launch prefix
 * scans over ent and iov, decide, the scan of the block sums, emit); no block
 * waits for another, no launch walks a connection's queue serially, and no
 * atomic hands out a position: atomics only add to counts and totals.  No
 * allocation, no host synchronisation.  @workspace (device, 16-B aligned) need
 * not be zeroed and may be reused by the next call on the same stream.
 * nconn == 0 still writes both totals.
 *
 * Guarantee: no content of qoff, ent, voff, iov, rd, conn or addr causes a
 * read outside the given arrays, or a write outside the first item_cap
 * elements of the per-item outputs, the first seg_cap elements of the
 * per-segment outputs, out_conn[0, nconn), both totals, counts and the
 * workspace.  Garbage qoff and voff are included: decreasing values, or values
 * past nent or nvec.  Ranges that overlap are each read.
 *
 * What stays with the runtime: the connection lock and waitq_wait (BLOCK), the
 * waitq_releases and poll_set / poll_clear themselves, mbuf_list_free, and
 * writing rcv_wnd, tx_last_ack, tx_last_win, rx_exclusive and rx_closed back.
 *
 * gcl_tcp_read_workspace - bytes of device scratch a call takes: 16 per queue
 *   entry and 8 per vector plus a fixed part.  -EINVAL for a NULL @bytes,
 *   nconn > 2^20, nent or nvec > 2^31 or blocks > GCL_RD_MAX_BLOCKS.
 * gcl_tcp_read - -EINVAL for a NULL ctx, in or out; a wrong in->size; nconn >
 *   2^20; nent, nvec, item_cap or seg_cap > 2^31; blocks > GCL_RD_MAX_BLOCKS;
 *   frame_stride < 54; a NULL totals or seg.totals; with nconn > 0 a NULL qoff,
 *   rd, conn, addr or out_conn; with nent > 0 a NULL ent; with voff and nvec > 0
 *   a NULL iov (without voff neither iov nor nvec is looked at); with nconn > 0 and item_cap > 0 a NULL per-item output; with
 *   nconn > 0 and seg_cap > 0 a NULL per-segment output; any given array that
 *   is not aligned to its element; a NULL workspace, one that is not 16-B
 *   aligned or one smaller than gcl_tcp_read_workspace says.  -EIO when a
 *   launch fails.
 */
/* gcl_tcp_rd.flags */
#define GCL_RD_WANT       0x01  /* a read is issued on this connection */
#define GCL_RD_PEEK       0x02
#define GCL_RD_NONBLOCK   0x04  /* the call's or c->nonblocking */
#define GCL_RD_RX_CLOSED  0x08  /* c->rx_closed */
#define GCL_RD_RX_EXCL    0x10  /* c->rx_exclusive */
/* gcl_rdq_ent.flags */
#define GCL_RDQE_FIN      0x01  /* m->flags & TCP_FIN */
/* gcl_rd_conn_out.status */
#define GCL_RDS_NONE      0
#define GCL_RDS_DONE      1
#define GCL_RDS_AGAIN     2
#define GCL_RDS_BLOCK     3
#define GCL_RDS_CLOSED    4
#define GCL_RDS_BADRANGE  5
/* gcl_rd_conn_out.flags */
#define GCL_RDO_RXWAKE        0x01  /* tcp_exclusive_finish: rx_exclusive = false, release rx_wq */
#define GCL_RDO_EXCL_LEFT     0x02  /* a peek of 0 bytes: rx_exclusive stays set */
#define GCL_RDO_RX_CLOSED     0x04  /* tcp_conn_shutdown_rx: rx_closed, POLLRDHUP | POLLIN, release rx_wq */
#define GCL_RDO_PARTIAL       0x08  /* entry npop is pulled by `pull` bytes */
#define GCL_RDO_ACK           0x10  /* tcp_tx_ack */
#define GCL_RDO_POLLIN_CLEAR  0x20  /* poll_clear(&c->poll_src, POLLIN) */
#define GCL_RDO_SEG_NOSPACE   0x40  /* its ACK lay at or past seg_cap */
#define GCL_RDO_ITEM_NOSPACE  0x80  /* an item of it lay at or past item_cap */
#define GCL_RD_MAX_BLOCKS 1024      /* the cap on in->blocks */
#define GCL_RD_MAX_CONN (1u << 20)
enum { GCL_RDC_DONE = 0, GCL_RDC_AGAIN, GCL_RDC_BLOCK, GCL_RDC_CLOSED, GCL_RDC_PEEKS, GCL_RDC_POPPED,
       GCL_RDC_PARTIAL, GCL_RDC_RX_CLOSED, GCL_RDC_ACKS, GCL_RDC_ITEMS, GCL_RDC_BYTES, GCL_RDC_NOSPACE,
       GCL_RDC_NR = 12 };
struct gcl_tcp_rd {        /* 32 B, 16-B aligned, host order: one read and what the ACK test reads */
	uint64_t dst_off;      /* without voff: the buffer */
	uint32_t len;
	uint32_t tx_last_ack, tx_last_win, winmax;
	int32_t  err;          /* c->err */
	uint8_t  flags;        /* GCL_RD_* */
	uint8_t  pad[3];
};
struct gcl_rdq_ent {       /* 16 B: one mbuf of c->rxq */
	uint64_t off;          /* where its data lies in the source region */
	uint16_t len;          /* mbuf_length */
	uint8_t  flags;        /* GCL_RDQE_* */
	uint8_t  pad[5];
};
struct gcl_rd_iov {        /* 16 B: one struct iovec */
	uint64_t off;
	uint32_t len;
	uint8_t  pad[4];
};
struct gcl_rd_conn_out {   /* 32 B, 16-B aligned */
	int64_t  ret;
	uint32_t npop, pull, rcv_wnd, first_item, nitems;
	uint8_t  status;       /* GCL_RDS_* */
	uint8_t  flags;        /* GCL_RDO_* */
	uint8_t  pad[2];       /* written as 0 */
};
struct gcl_rd_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_rd_in); blocks as in gcl_tick_in: the ranges of
	                                      every scan and sweep of the call */
	const uint32_t *qoff;              /* u32[nconn + 1] */
	const struct gcl_rdq_ent *ent;     /* [nent] */
	uint64_t nent;                     /* <= 2^31 */
	const uint32_t *voff;              /* optional u32[nconn + 1] */
	const struct gcl_rd_iov *iov;      /* [nvec] */
	uint64_t nvec;                     /* <= 2^31; not looked at without voff */
	const struct gcl_tcp_rd *rd;       /* [nconn] */
	const struct gcl_tcp_conn *conn;   /* [nconn]: rcv_nxt, rcv_wnd and snd_nxt are read */
	const struct gcl_tcp_addr *addr;   /* [nconn] */
	uint32_t nconn;                    /* <= 2^20 */
	uint32_t frame_stride;             /* bytes, >= GCL_CTL_MIN_STRIDE */
	uint64_t item_cap;                 /* <= 2^31: the length of every per-item output array */
	uint64_t seg_cap;                  /* <= 2^31: the length of every per-segment output array */
	uint64_t frame_base;
};
struct gcl_rd_out {                    /* device, aligned to their element */
	struct gcl_rd_conn_out *out_conn;  /* [nconn] */
	uint64_t *src_off;                 /* [item_cap] */
	uint16_t *len;                     /* [item_cap] */
	uint64_t *dst_off;                 /* [item_cap] */
	uint32_t *item_conn, *item_ent;    /* [item_cap] */
	uint64_t *totals;                  /* u64[4], required: items wanted, written, their bytes, bytes read */
	struct gcl_ctlseg_out seg;         /* the ACKs; seg.totals required */
};
int gcl_tcp_read_workspace(uint32_t nconn, uint64_t nent, uint64_t nvec, uint32_t blocks, size_t *bytes);
int gcl_tcp_read(struct gcl_ctx *ctx, const struct gcl_rd_in *in, const struct gcl_rd_out *out,
                 uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The socket writes of TCP: the step between the application and the transmit
 * chain.  gcl_tx_seg cuts a write whose winlen and snd_nxt someone else worked
 * out and always pushes; tcp_write3 / tcp_writev2 (runtime/net/tcp.c:
 * tcp_write_wait :1259-1307, tcp_write_finish :1309-1349, :1362-1422) with
 * tcp_tx_send (tcp_out.c:313-386) decide whether a write goes ahead at all,
 * work the window out, gather the bytes of several iovecs into one segment and
 * hold the unfinished tail in c->tx_pending.  gcl_tcp_write does that for
 * every connection of one runtime at one instant, on a snapshot:
 *
 *   gcl_tcp_write -> gcl_copy_batch (src_off, len, dst_off) -> gcl_tx_hdr (desc,
 *   frame_off) -> gcl_l4_csum GCL_L4_FILL ; (txq_ent, txq_cold appended to the
 *   connection's queue) -> gcl_tcp_txq
 *
 * It works on every context and touches no table.
 *
 * The write of connection c is wr[c]: flags (GCL_WR_*), c->err, snd_mss, the
 * ecn byte of its descriptors, tx_last_ack, the held c->tx_pending (pend_len
 * bytes of payload in the frame at pend_frame_off, its seg_seq = snd_nxt -
 * pend_len; pend_len 0: none) and, without GCL_WR_VEC, its buffer (src_off,
 * len).  With GCL_WR_VEC the buffer is the vectors [voff[c], voff[c + 1]) of
 * iov (struct gcl_rd_iov), and GCL_WR_NO_PARTIAL is ignored: tcp_write3 takes
 * no vectors.  conn[c] gives snd_una, snd_wnd, snd_nxt, rcv_nxt and rcv_wnd,
 * addr[c] the tuple and rcv_wscale, in->now the call's one clock reading.
 *
 * One connection; full(x) = wraps_lte(snd_una + snd_wnd, x):
 *   1. no GCL_WR_WANT: status NONE, nothing changes.
 *   2. status REFUSED, not written, when GCL_WR_VEC is set and there is no voff,
 *      or its voff range is inverted or not inside [0, nvec], or holds more
 *      than GCL_WR_MAX_IOV vectors, or the vectors named by the wanted vector
 *      writes before it and its own are more than nvec (ranges that overlap:
 *      never with a consistent CSR); when snd_mss == 0; when pend_len >
 *      snd_mss; when 54 + snd_mss > frame_stride.
 *   3. tcp_write_wait: not TX_CLOSED, and BELOW_EST or TX_EXCL or
 *      full(snd_nxt): GCL_WRO_ZWND_ARM iff full(snd_nxt) and not ZERO_WND (the
 *      host stores zero_wnd = true, zero_wnd_ts = now and runs the timer update
 *      again); with NONBLOCK status AGAIN, ret -11, else status BLOCK, ret 0.
 *      Nothing else changes.
 *   4. Otherwise GCL_WRO_ZWND_CLEAR iff ZERO_WND was set (tcp.c:1285 runs before
 *      the closed test).  TX_CLOSED: status CLOSED, ret = err ? -err : -32.
 *      winlen = snd_una + snd_wnd - snd_nxt (mod 2^32; 1 .. 2^31 - 1 here).
 *      Without VEC, with NO_PARTIAL and winlen < len: status NOSPC, ret -28.
 *   5. The write goes ahead: GCL_WRO_ACKS_RESET (acks_delayed_cnt = 0,
 *      ack_delayed = false) and GCL_WRO_TXWAKE.  Without VEC one
 *      tcp_tx_send(min(len, winlen), push).  With VEC the vectors are walked
 *      with the window that is left: stop at 0, skip an empty vector, send
 *      min(iov_len, left) with push = (it is the last vector and iov_len <=
 *      left).
 *   6. tcp_tx_send(X, push) with h bytes held makes one pass per segment it
 *      touches, at least one.  A held segment continues with min(rest, mss - h)
 *      bytes (0 when it is full); otherwise a new segment takes min(rest, mss)
 *      with seg_seq = snd_nxt and flags ACK.  snd_nxt advances.  With !push,
 *      rest == 0 and (size_t)(fill - 20) < mss the segment is held: mbuf_length
 *      does not hold the TCP header yet, so it is held iff fill >= 20; a tail of
 *      1..19 bytes is sent short and without PSH (counted as SHORT), a tail of
 *      exactly mss bytes is held.  Otherwise it is sent, with PSH iff push and
 *      rest == 0.  X == 0 occurs for a plain write of len 0 alone: a held
 *      segment is flushed with PSH, or an empty ACK|PSH segment is sent.
 *   7. ret = the bytes taken = min(total, winlen); snd_nxt as the passes leave
 *      it.  A vector write of no bytes (no vectors, or all of them empty) makes
 *      no pass: ret 0, no segment and no item.
 *   8. tcp_write_finish: GCL_WRO_ACK_TS iff rcv_nxt != tx_last_ack, where
 *      tx_last_ack is rcv_nxt once a segment was sent (tcp_out.c:60);
 *      GCL_WRO_POLLOUT_CLEAR iff full(snd_nxt after).  Status DONE.
 *
 * Every pass is one copy item: src_off = the vector's (buffer's) off + the
 * bytes of it sent before, len (<= mss), dst_off = the segment's frame_off + 54
 * + the bytes already in it, item_conn = c, item_seg = the index of the
 * segment in the per-segment outputs, 0xFFFFFFFF for the one that is held when
 * the call ends.  A pass that takes nothing gives an item of len 0.
 *
 * Every new segment, sent or held, takes the next slot frame_base + k *
 * frame_stride, k counted over the call in connection and send order; the
 * continued tx_pending keeps pend_frame_off and takes none.  Per sent segment,
 * in connection order and then send order: desc (proto 6, the flags above,
 * tcp_off 5, seq, ack = rcv_nxt, win = (rcv_wnd >> rcv_wscale) & 0xFFFF as on
 * the wire, paylen, ecn), frame_off, seg_conn, txq_ent {seg_seq, seg_end =
 * seg_seq + paylen, ts = now} and txq_cold {frame_off, tcp_flags, tcp_off 5,
 * GCL_TXQE_INFLIGHT}: what the connection's queue of gcl_tcp_txq gains.  A sent
 * segment implies tx_last_ack = rcv_nxt and tx_last_win = rcv_wnd for the host
 * to store.
 *
 * Caps.  S_c, I_c and K_c are the segments, items and slots wanted by the
 * connections before c that went ahead.  Connection c that goes ahead is
 * status NOSPACE, ret -105 (-ENOBUFS), when S_c + its segments > seg_cap, I_c +
 * its items > item_cap or, with frames_len != 0, (K_c + its slots) *
 * frame_stride > frames_len - frame_base (no room at all below frame_base).
 * It writes nothing and changes nothing: flags 0, snd_nxt and the pending
 * words as they came.  The sums count those connections too and only grow, so
 * the NOSPACE connections are a suffix of those that went ahead: no later
 * connection is sent once one does not fit, not even a vector write of no
 * bytes, which wants nothing.
 *
 * out_conn[c], every byte written: ret; snd_nxt; first_seg = min(S_c, seg_cap)
 * and nseg, first_item = min(I_c, item_cap) and nitems (0 unless DONE);
 * pend_len and pend_frame_off after the call (0 and 0 when a DONE write leaves
 * nothing held); status; flags.  totals u64[6]:
 * segments wanted, written, items wanted, written, slots used, the sum of the
 * DONE connections' ret.
 *
 * @counts is a device u64[GCL_WRC_NR], ACCUMULATED, may be NULL: one slot per
 * status (GCL_WRS_* is its index), SEGS written, PUSH (segments with PSH), HELD
 * (DONE connections that leave a tx_pending), SHORT, ITEMS written and BYTES
 * (totals[5]).
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * conn, addr, wr, iov, out_conn, desc, txq_ent and txq_cold to 16 B.
 * Asynchronous on @hip_stream, six launches ordered by the stream alone: the
 * prefix sums of the vectors the writes name (two launches), one lane per
 * connection walks its vectors (at most GCL_WR_MAX_IOV; the walk has a true
 * serial dependency, a short tail resets the segment phase), the scan of the
 * block sums, one lane per connection places it, and one lane per segment and
 * per item emits, from the prefix sums and a search: nothing that grows with
 * the bytes runs serially.  No block waits for another and no atomic hands
 * out a position: atomics only add to counts and totals.  No allocation, no
 * host synchronisation.  @workspace (device, 16-B aligned) need not be zeroed
 * and may be reused by the next call on the same stream.  nconn == 0 still
 * writes totals.
 *
 * Guarantee: no content of voff, iov, wr, conn or addr causes a read outside
 * the given arrays, or a write outside the first seg_cap elements of the
 * per-segment outputs, the first item_cap elements of the per-item outputs,
 * out_conn[0, nconn), totals, counts and the workspace.  Garbage voff is
 * included: decreasing values, or values past nvec.  Ranges that overlap are
 * each read.  The call writes no frame: the offsets it emits are the
 * caller's to bound (frames_len).
 *
 * What stays with the runtime: the connection lock and waitq_wait (BLOCK),
 * tx_exclusive, the waitq_release, poll_clear, tcp_conn_ack and the fast
 * retransmit of tcp_write_finish, storing the words back and appending the
 * queue records.
 *
 * gcl_tcp_write_workspace - bytes of device scratch a call takes: 32 per
 *   vector and 36 per connection plus a fixed part.  -EINVAL for a NULL
 *   @bytes, nconn > 2^20, nvec > 2^31 or blocks > GCL_WR_MAX_BLOCKS.
 * gcl_tcp_write - -EINVAL for a NULL ctx, in or out; a wrong in->size; nconn >
 *   2^20; nvec (with voff), seg_cap or item_cap > 2^31; blocks >
 *   GCL_WR_MAX_BLOCKS; frame_stride < 54 or > 2^20; a NULL totals; with nconn >
 *   0 a NULL wr, conn, addr or out_conn; with voff and nvec > 0 a NULL iov
 *   (without voff neither iov nor nvec is looked at); with nconn > 0 and
 *   seg_cap > 0 a NULL per-segment output; with nconn > 0 and item_cap > 0 a
 *   NULL per-item output; any given array that is not aligned to its element;
 *   a NULL workspace, one that is not 16-B aligned or one smaller than
 *   gcl_tcp_write_workspace says.  -EIO when a launch fails.
 */
/* gcl_tcp_wr.flags */
#define GCL_WR_WANT        0x01  /* a write is issued on this connection */
#define GCL_WR_VEC         0x02  /* tcp_writev2 over its voff range; else tcp_write3 over (src_off, len) */
#define GCL_WR_NONBLOCK    0x04  /* the call's or c->nonblocking */
#define GCL_WR_NO_PARTIAL  0x08  /* tcp_write3's no_partial_write */
#define GCL_WR_TX_CLOSED   0x10  /* c->tx_closed */
#define GCL_WR_TX_EXCL     0x20  /* c->tx_exclusive */
#define GCL_WR_ZERO_WND    0x40  /* c->zero_wnd */
#define GCL_WR_BELOW_EST   0x80  /* pcb.state < TCP_STATE_ESTABLISHED */
/* gcl_wr_conn_out.status, and the first counter slots */
#define GCL_WRS_NONE     0
#define GCL_WRS_DONE     1
#define GCL_WRS_AGAIN    2
#define GCL_WRS_BLOCK    3
#define GCL_WRS_CLOSED   4
#define GCL_WRS_NOSPC    5   /* -ENOSPC: no_partial_write and the window is shorter */
#define GCL_WRS_REFUSED  6
#define GCL_WRS_NOSPACE  7   /* a cap: -ENOBUFS */
/* gcl_wr_conn_out.flags */
#define GCL_WRO_ZWND_ARM       0x01  /* zero_wnd = true, zero_wnd_ts = now, tcp_timer_update */
#define GCL_WRO_ZWND_CLEAR     0x02  /* zero_wnd = false */
#define GCL_WRO_ACKS_RESET     0x04  /* acks_delayed_cnt = 0, ack_delayed = false */
#define GCL_WRO_TXWAKE         0x08  /* tx_exclusive = false, release tx_wq */
#define GCL_WRO_ACK_TS         0x10  /* ack_ts = now; clear: ack_delayed = false */
#define GCL_WRO_POLLOUT_CLEAR  0x20  /* poll_clear(&c->poll_src, POLLOUT) */
#define GCL_WR_MAX_IOV    1024       /* vectors of one write */
#define GCL_WR_MAX_BLOCKS 1024       /* the cap on in->blocks */
#define GCL_WR_MAX_CONN   (1u << 20)
#define GCL_WR_MAX_STRIDE (1u << 20)
#define GCL_WR_SEG_HELD   0xFFFFFFFFu /* item_seg of the segment that stays in tx_pending */
enum { GCL_WRC_SEGS = 8, GCL_WRC_PUSH, GCL_WRC_HELD, GCL_WRC_SHORT, GCL_WRC_ITEMS, GCL_WRC_BYTES, GCL_WRC_NR = 14 };
struct gcl_tcp_wr {        /* 48 B, 16-B aligned, host order: one write and the words of the connection it reads */
	uint64_t src_off;      /* without GCL_WR_VEC: the buffer */
	uint32_t len;
	uint32_t tx_last_ack;
	uint64_t pend_frame_off; /* c->tx_pending: where its Ethernet header lies */
	uint32_t pend_len;     /* its payload bytes; 0: none */
	int32_t  err;          /* c->err */
	uint16_t snd_mss;
	uint8_t  ecn;          /* as gcl_txh_desc.ecn */
	uint8_t  flags;        /* GCL_WR_* */
	uint8_t  pad[12];
};
struct gcl_wr_conn_out {   /* 48 B, 16-B aligned */
	int64_t  ret;
	uint32_t snd_nxt;
	uint32_t first_seg, nseg, first_item, nitems;
	uint32_t pend_len;
	uint64_t pend_frame_off;
	uint8_t  status;       /* GCL_WRS_* */
	uint8_t  flags;        /* GCL_WRO_* */
	uint8_t  pad[6];       /* written as 0 */
};
struct gcl_wr_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_wr_in); blocks as in gcl_tick_in */
	uint64_t now;                      /* us: the call's one clock reading */
	const uint32_t *voff;              /* optional u32[nconn + 1] */
	const struct gcl_rd_iov *iov;      /* [nvec] */
	uint64_t nvec;                     /* <= 2^31; not looked at without voff */
	const struct gcl_tcp_wr *wr;       /* [nconn] */
	const struct gcl_tcp_conn *conn;   /* [nconn] */
	const struct gcl_tcp_addr *addr;   /* [nconn] */
	uint32_t nconn;                    /* <= 2^20 */
	uint32_t frame_stride;             /* bytes, 54 .. 2^20 */
	uint64_t seg_cap;                  /* <= 2^31: the length of every per-segment output array */
	uint64_t item_cap;                 /* <= 2^31: the length of every per-item output array */
	uint64_t frame_base;
	uint64_t frames_len;               /* 0: no limit */
};
struct gcl_wr_out {                    /* device, aligned to their element */
	struct gcl_wr_conn_out *out_conn;  /* [nconn] */
	struct gcl_txh_desc *desc;         /* [seg_cap] */
	uint64_t *frame_off;               /* [seg_cap] */
	uint32_t *seg_conn;                /* [seg_cap] */
	struct gcl_txq_ent *txq_ent;       /* [seg_cap] */
	struct gcl_txq_cold *txq_cold;     /* [seg_cap] */
	uint64_t *src_off;                 /* [item_cap] */
	uint16_t *len;                     /* [item_cap] */
	uint64_t *dst_off;                 /* [item_cap] */
	uint32_t *item_conn, *item_seg;    /* [item_cap] */
	uint64_t *totals;                  /* u64[6], required */
};
int gcl_tcp_write_workspace(uint32_t nconn, uint64_t nvec, uint32_t blocks, size_t *bytes);
int gcl_tcp_write(struct gcl_ctx *ctx, const struct gcl_wr_in *in, const struct gcl_wr_out *out,
                  uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The end of a TCP connection as the application asks for it: tcp_shutdown,
 * tcp_close and tcp_abort (runtime/net/tcp.c:1555-1633, with
 * tcp_conn_shutdown_tx :1504-1546, tcp_conn_shutdown_rx :1492-1502 and
 * tcp_conn_fail :1453-1484) for every connection of one runtime at one clock
 * reading, on a snapshot, with the FIN of tcp_tx_ctl(FIN | ACK)
 * (tcp_out.c:264-295) and the RST of tcp_tx_raw_rst (:98-128):
 *
 *   gcl_tcp_shut -> gcl_tx_hdr (desc, frame_off) -> gcl_l4_csum GCL_L4_FILL ;
 *   (txq_ent, txq_cold of a FIN appended to the connection's queue) ->
 *   gcl_tcp_txq ; state, tmr_flags, next_timeout stored -> gcl_tcp_rx_states,
 *   gcl_tcp_tick
 *
 * It works on every context and touches no table.
 *
 * The request of connection c is shut[c]: op (GCL_SHUT_OP_*), how (the raw
 * argument of tcp_shutdown: 0 SHUT_RD, 1 SHUT_WR, 2 SHUT_RDWR; read for
 * SHUTDOWN alone) and flags (c->tx_closed, c->rx_closed, c->rx_exclusive).
 * tmr[c] gives state, GCL_TMR_LIVE, _TX_EXCLUSIVE (X below), _TXQ, _OOO,
 * _ACK_DELAYED, _ZERO_WND and the timestamps; conn[c] snd_nxt, rcv_nxt and
 * rcv_wnd; addr[c] the tuple and rcv_wscale; in->now the one clock reading.
 *
 * One connection, S its state:
 *   1. op NONE, or LIVE clear: status NONE; out_conn[c] repeats the input
 *      words, err 0, flags 0.  Otherwise an op above ABORT or S > 9: status
 *      REFUSED, nothing changes.
 *   2. SHUTDOWN with how not 0, 1 or 2: status EINVAL, ret -22, nothing changes
 *      (tcp.c:1560).
 *   3. The tx part, for SHUTDOWN with how 1 or 2 and for CLOSE, in the
 *      reference's order:
 *      a. TX_CLOSED: nothing (:1510).
 *      b. S < ESTABLISHED: FAIL(103, ECONNABORTED) and one RST with seq =
 *         snd_nxt (:1513-1517).  The reference does not wait for X here, and
 *         with X the fail does not free the txq.
 *      c. X: status BLOCK, ret 0, nothing changes; the rx part and CLOSE's put
 *         do not run either: the reference sleeps here before them (:1519).
 *      d. Otherwise one FIN|ACK: seq = snd_nxt, ack = rcv_nxt, win = (rcv_wnd >>
 *         rcv_wscale) & 0xFFFF, tcp_flags 0x11, tcp_off 5, no payload, ecn 0.
 *         snd_nxt + 1.  The queue gains {seg_seq, seg_end = seg_seq + 1, ts =
 *         now} and {frame_off, 0x11, 5, GCL_TXQE_INFLIGHT}: GCL_TMR_TXQ is set
 *         in tmr_flags, and txq_ts becomes now unless TXQ was set already (the
 *         FIN is the new head).  ESTABLISHED -> FIN_WAIT1, CLOSE_WAIT ->
 *         LAST_ACK, and tcp_conn_set_state's tcp_timer_update gives
 *         next_timeout by rule 9 of gcl_tcp_tick on the new state, the new TXQ
 *         and now.  Any other state is the reference's WARN(): the FIN is sent
 *         all the same, state and next_timeout stay, GCL_SHO_WARN.  Then
 *         POLLHUP, TX_CLOSED_SET and TXWAKE.  A sent FIN implies tx_last_ack =
 *         rcv_nxt and tx_last_win = rcv_wnd for the host to store.
 *   4. The rx part, for SHUTDOWN with how 0 or 2 and for CLOSE: unless
 *      RX_CLOSED is set or a FAIL of 3b has set it, POLLRDHUP_IN, RX_CLOSED_SET
 *      and RXWAKE.
 *   5. CLOSE: DETACH_POLL (poll_src.set_fn = clear_fn = NULL) and one
 *      tcp_conn_put.
 *   6. ABORT: S == CLOSED is status DONE with nothing.  Otherwise FAIL(103);
 *      with X status ABORT_WAIT: the fail's effects are reported and no RST is
 *      emitted, since the reference sends it with the snd_nxt the writer
 *      leaves; without X one RST with seq = snd_nxt.
 *   7. FAIL(e) is tcp_conn_fail: err = e, state CLOSED; from S < ESTABLISHED
 *      tcp_conn_set_state's GCL_SHO_POLLOUT; next_timeout by rule 9 on state
 *      CLOSED and the input flags, since the timer update (:1459) runs before
 *      the frees (:1471-1479): it still counts the txq head and the OOO term
 *      and is not recomputed afterwards.  The rx part as in 4.  Without
 *      TX_CLOSED: TX_CLOSED_SET, TXWAKE, POLLHUP.  Without X: FREE_TXQ,
 *      FREE_PEND, and GCL_TMR_TXQ cleared in tmr_flags.  Without RX_EXCL:
 *      FREE_RXQ.  FREE_OOO always, GCL_TMR_OOO cleared.  One put if S was not
 *      CLOSED.
 *   8. nput (0..2) counts the puts of 5 and 7.  status DONE unless said
 *      otherwise; ret 0 in every status but EINVAL and NOSPACE.
 * Not modelled: the interrupted wait of tcp_shutdown (-EINTR).  tx_pending is
 * left as the reference leaves it: a FIN neither flushes nor frees it (its
 * bytes are below snd_nxt already); only FREE_PEND frees it.
 *
 * Segments.  A connection wants at most one.  cap = seg_cap, or with
 * frames_len != 0 min(seg_cap, (frames_len - frame_base) / frame_stride), 0
 * when frames_len < frame_base: gcl_tcp_write's fit test.  Let W_c be the
 * connections before c that want one, k = min(W_c, cap).  A connection that
 * wants one with W_c >= cap is status NOSPACE, ret -105 (-ENOBUFS), nothing
 * changed: tcp_tx_ctl's -ENOMEM path is not played out.  Those are a suffix of
 * the wanting connections; one that wants none is never NOSPACE.  Otherwise
 * its segment is segment k of the call: desc[k]; frame_off[k] = frame_base + k
 * * frame_stride; seg_conn[k] = seg_src[k] = c; seg_kind[k] = GCL_CTL_FIN or
 * GCL_CTL_RST (the descriptor gcl_tcp_rx_ctl writes for rst_seq = snd_nxt);
 * txq_ent[k] and txq_cold[k] the records of 3d for a FIN, all-zero bytes for
 * an RST.  totals[0] = segments wanted, totals[1] = min(wanted, cap), the m of
 * gcl_tx_hdr.
 *
 * out_conn[c], every byte written: next_timeout, txq_ts, ret, err (0: c->err
 * stays), snd_nxt, first_seg (k when nseg is 1, else 0), the flag word
 * (GCL_SHO_*), status, state, tmr_flags (the input byte with TXQ and OOO as
 * above), nseg (0 or 1), nput, and zero padding.
 *
 * @counts is a device u64[GCL_SHUTC_NR], ACCUMULATED, may be NULL: one slot
 * per status (GCL_SHUTS_* is its index), FIN and RST segments written, FAIL
 * (connections failed), PUT (the sum of nput) and WARN.
 *
 * Every pointer is a device pointer; each array is aligned to its element,
 * shut, tmr, conn, addr, out_conn, desc, txq_ent and txq_cold to 16 B.
 * Asynchronous on @hip_stream, three launches ordered by the stream alone: one
 * lane per connection decides and writes out_conn, the per-block counts are
 * scanned, and one lane per connection emits its own segment (or takes its
 * decision back as NOSPACE).  No block waits for another and no atomic hands
 * out a position: atomics only add to counts.  No allocation, no host
 * synchronisation.  @workspace (device, 16-B aligned) need not be zeroed and
 * may be reused by the next call on the same stream.  nconn == 0 still writes
 * totals.
 *
 * Guarantee: no content of shut, tmr, conn or addr causes a read outside the
 * given arrays, or a write outside the first seg_cap elements of the
 * per-segment outputs, out_conn[0, nconn), totals, counts and the workspace.
 *
 * What stays with the runtime: the connection lock; the sleeps behind BLOCK
 * and ABORT_WAIT (and calling again when the writer is done); the delayed RST
 * of ABORT_WAIT, with the writer's snd_nxt; the actual frees (FREE_*); the
 * wake-ups and poll_set (the flag word says which); the puts; storing state,
 * err, snd_nxt, next_timeout, txq_ts and the flags back; appending the FIN's
 * record to the queue.
 *
 * gcl_tcp_shut_workspace - bytes of device scratch a call takes: 4 per block
 *   (in->blocks, or the cap GCL_SHUT_MAX_BLOCKS when blocks is 0) and 1 per
 *   connection, each rounded up to 16.  -EINVAL for a NULL @bytes, nconn > 2^20
 *   or blocks > GCL_SHUT_MAX_BLOCKS.
 * gcl_tcp_shut - -EINVAL for a NULL ctx, in or out; a wrong in->size; nconn >
 *   2^20; seg_cap > 2^31; blocks > GCL_SHUT_MAX_BLOCKS; frame_stride < 54; a
 *   NULL totals; with nconn > 0 a NULL shut, tmr, conn, addr or out_conn; with
 *   nconn > 0 and seg_cap > 0 a NULL per-segment output; any given array that
 *   is not aligned to its element; a NULL workspace, one that is not 16-B
 *   aligned or one smaller than gcl_tcp_shut_workspace says.  -EIO when a
 *   launch fails.
 */
/* gcl_tcp_shut.op */
#define GCL_SHUT_OP_NONE     0
#define GCL_SHUT_OP_SHUTDOWN 1   /* tcp_shutdown(c, how) */
#define GCL_SHUT_OP_CLOSE    2   /* tcp_close(c) */
#define GCL_SHUT_OP_ABORT    3   /* tcp_abort(c) */
/* gcl_tcp_shut.flags */
#define GCL_SHUT_TX_CLOSED   0x01  /* c->tx_closed */
#define GCL_SHUT_RX_CLOSED   0x02  /* c->rx_closed */
#define GCL_SHUT_RX_EXCL     0x04  /* c->rx_exclusive */
/* gcl_shut_conn_out.status, and the first counter slots */
#define GCL_SHUTS_NONE       0
#define GCL_SHUTS_DONE       1
#define GCL_SHUTS_BLOCK      2   /* the writer is busy: wait on tx_wq, call again */
#define GCL_SHUTS_ABORT_WAIT 3   /* failed; the RST waits for the writer */
#define GCL_SHUTS_EINVAL     4
#define GCL_SHUTS_REFUSED    5
#define GCL_SHUTS_NOSPACE    6   /* a cap: -ENOBUFS */
#define GCL_SHUTS_NR         7
/* gcl_shut_conn_out.flags */
#define GCL_SHO_POLLHUP        0x0001  /* poll_set(&c->poll_src, POLLHUP) */
#define GCL_SHO_TX_CLOSED_SET  0x0002  /* c->tx_closed = true */
#define GCL_SHO_TXWAKE         0x0004  /* waitq_release(&c->tx_wq) */
#define GCL_SHO_POLLRDHUP_IN   0x0008  /* poll_set(&c->poll_src, POLLRDHUP | POLLIN) */
#define GCL_SHO_RX_CLOSED_SET  0x0010  /* c->rx_closed = true */
#define GCL_SHO_RXWAKE         0x0020  /* waitq_release(&c->rx_wq) */
#define GCL_SHO_DETACH_POLL    0x0040  /* poll_src.set_fn = clear_fn = NULL */
#define GCL_SHO_FREE_TXQ       0x0080  /* mbuf_list_free(&c->txq) */
#define GCL_SHO_FREE_PEND      0x0100  /* mbuf_free(c->tx_pending), if any */
#define GCL_SHO_FREE_RXQ       0x0200  /* mbuf_list_free(&c->rxq) */
#define GCL_SHO_FREE_OOO       0x0400  /* mbuf_list_free(&c->rxq_ooo) */
#define GCL_SHO_WARN           0x0800  /* a FIN from a state other than ESTABLISHED and CLOSE_WAIT */
#define GCL_SHO_POLLOUT        0x1000  /* tcp_conn_set_state from below ESTABLISHED: release tx_wq, POLLOUT */
#define GCL_CTL_FIN          5      /* seg_kind[k] beside GCL_CTL_ACK .. GCL_CTL_SYNACK */
#define GCL_SHUT_MAX_BLOCKS 1024    /* the cap on in->blocks */
#define GCL_SHUT_MAX_CONN (1u << 20)
enum { GCL_SHUTC_FIN = 7, GCL_SHUTC_RST, GCL_SHUTC_FAIL, GCL_SHUTC_PUT, GCL_SHUTC_WARN, GCL_SHUTC_NR = 12 };
struct gcl_tcp_shut {      /* 16 B, 16-B aligned, host order: what the application asks of one connection */
	int32_t  how;          /* tcp_shutdown's argument as it came */
	uint8_t  op;           /* GCL_SHUT_OP_* */
	uint8_t  flags;        /* GCL_SHUT_* */
	uint8_t  pad[10];
};
struct gcl_shut_conn_out { /* 48 B, 16-B aligned */
	uint64_t next_timeout, txq_ts;
	int32_t  ret;
	int32_t  err;          /* 0: c->err stays */
	uint32_t snd_nxt;
	uint32_t first_seg;    /* the index of its segment when nseg is 1, else 0 */
	uint32_t flags;        /* GCL_SHO_* */
	uint8_t  status;       /* GCL_SHUTS_* */
	uint8_t  state;        /* enum tcp state */
	uint8_t  tmr_flags;    /* GCL_TMR_* */
	uint8_t  nseg;
	uint8_t  nput;
	uint8_t  pad[7];       /* written as 0 */
};
struct gcl_shut_in {
	uint32_t size, blocks;             /* sizeof(struct gcl_shut_in); blocks as in gcl_tick_in */
	uint64_t now;                      /* us: the call's one clock reading */
	const struct gcl_tcp_shut *shut;   /* [nconn] */
	const struct gcl_tcp_tmr *tmr;     /* [nconn] */
	const struct gcl_tcp_conn *conn;   /* [nconn] */
	const struct gcl_tcp_addr *addr;   /* [nconn] */
	uint32_t nconn;                    /* <= 2^20 */
	uint32_t frame_stride;             /* bytes, >= GCL_CTL_MIN_STRIDE */
	uint64_t seg_cap;                  /* <= 2^31: the length of every per-segment output array */
	uint64_t frame_base;
	uint64_t frames_len;               /* 0: no limit */
};
struct gcl_shut_out {                  /* device, aligned to their element */
	struct gcl_shut_conn_out *out_conn; /* [nconn] */
	struct gcl_ctlseg_out seg;         /* [seg_cap] each; totals u64[2]: wanted, written */
	struct gcl_txq_ent *txq_ent;       /* [seg_cap] */
	struct gcl_txq_cold *txq_cold;     /* [seg_cap] */
};
int gcl_tcp_shut_workspace(uint32_t nconn, uint32_t blocks, size_t *bytes);
int gcl_tcp_shut(struct gcl_ctx *ctx, const struct gcl_shut_in *in, const struct gcl_shut_out *out,
                 uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream);

/* Library version string. */
const char *gcl_version(void);

#ifdef __cplusplus
}
#endif

#endif /* GCLASSIFY_H */
