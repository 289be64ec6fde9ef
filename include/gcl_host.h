/*
 * gcl_host.h - host (CPU, C) side of the rx path that stays on the dataplane
 * core: turning GPU verdicts into lrpc messages for the runtimes.
 *
 * This is the part of rx_one_pkt that cannot run on the GPU
 * (iokernel/rx.c:50-92, :171-233): lrpc_send into the runtime's shared-memory
 * ring (inc/base/lrpc.h:48-63, base/lrpc.c:10-27), ownership bookkeeping of
 * the mbuf (rx.c:86-90), the sched_add_core wake path for runtimes with no
 * active kthread (rx.c:62-72), the Azure ARP broadcast/response, and the
 * ring-full counters RX_UNICAST_FAIL / RX_BROADCAST_FAIL.  Verdicts are
 * consumed in packet order and every DELIVER / WAKE verdict's flow_tbl slot
 * is resolved against p->flow_tbl and p->active_thread_count as they stand
 * when that packet is delivered (rx.c:55-72): a wake earlier in the batch
 * whose sched_add_core activated a kthread, or disabled another runtime's
 * (sched.c:208-216), steers the later packets exactly as in the reference.
 */
#ifndef GCL_HOST_H
#define GCL_HOST_H

#include <stdbool.h>
#include <stdint.h>

#include "gclassify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Same layout as struct lrpc_msg / struct lrpc_chan_out
 * (inc/base/lrpc.h:15-35), so a reference thread's &th->rxq can be passed. */
struct gcl_lrpc_msg {
	uint64_t cmd;
	unsigned long payload;
};

struct gcl_lrpc_chan_out {
	uint32_t send_head;
	uint32_t send_tail;
	struct gcl_lrpc_msg *tbl;
	uint32_t *recv_head_wb;
	uint32_t size;
	uint32_t pad;
};

#define GCL_LRPC_DONE_PARITY (1ULL << 63)

/* lrpc_init_out (base/lrpc.c:38-52): -EINVAL unless @size is a power of 2 */
int gcl_lrpc_init_out(struct gcl_lrpc_chan_out *chan, struct gcl_lrpc_msg *tbl,
                      unsigned int size, uint32_t *recv_head_wb);
/* lrpc_send / __lrpc_send: false when the ring is full */
bool gcl_lrpc_send(struct gcl_lrpc_chan_out *chan, uint64_t cmd, unsigned long payload);

/* The slice of struct proc (iokernel/defs.h:187-251) the rx path touches. */
struct gcl_host_proc {
	uint16_t uniqid;
	uint16_t thread_count;
	uint16_t active_thread_count;
	int16_t  idle_top;                 /* list_top(&p->idle_threads), -1 if empty */
	uint16_t flow_tbl[GCL_NCPU];
	struct gcl_lrpc_chan_out *rxq[GCL_NCPU]; /* &p->threads[i].rxq */
};

/* Callbacks into the surrounding dataplane (all optional). */
struct gcl_host_ops {
	void *arg;
	/* sched_add_core(p) (sched.c:870-878): may activate threads and rewrite
	 * p->flow_tbl / active_thread_count / idle_top before returning. */
	void (*sched_add_core)(void *arg, struct gcl_host_proc *p);
	/* thread_enable_sched_poll(th) (rx.c:58, :71) */
	void (*enable_poll)(void *arg, struct gcl_host_proc *p, unsigned int thread);
	/* rte_pktmbuf_free(buf) of packet i (rx.c:231) */
	void (*free_pkt)(void *arg, uint64_t i);
	/* pdata->owner = p; list_add_tail(&p->owned_rx_bufs) (rx.c:86-90) */
	void (*owned)(void *arg, struct gcl_host_proc *p, uint64_t i);
	/* rte_mbuf_refcnt_update(buf, delta) (rx.c:188) */
	void (*refcnt_update)(void *arg, uint64_t i, int delta);
	/* azure_arp_response(buf) (rx.c:94-114): true if transmitted */
	bool (*arp_respond)(void *arg, uint64_t i);
};

/* rx_make_cmd (rx.c:24-38): RX_NET_RECV | len << 16 | csum_type << 48 */
uint64_t gcl_rx_make_cmd(uint16_t pkt_len, uint8_t olflags);

/*
 * gcl_rx_csum_flags - the rule of gcl_rx_csum (gclassify.h) for one frame on
 * the CPU, for the packets the GPU did not see: the ol_flags of a frame of
 * @len bytes that arrived with @olflags, its IPv4 header checksum resolved.
 * Bytes at or past @len read 0 (@frame may be NULL when @len is 0).  A frame
 * whose bytes 12-13 are not 0x0800, or that is already IP_CKSUM_GOOD, keeps
 * @olflags; any other gets IP_CKSUM_GOOD when the one's-complement sum of
 * frame bytes [14, 34) folds to 0xFFFF (chksum_internet returns 0) and
 * IP_CKSUM_BAD when it does not, every other bit unchanged.
 */
uint8_t gcl_rx_csum_flags(const uint8_t *frame, size_t len, uint8_t olflags);

/*
 * gcl_copy_batch_host - the rule of gcl_copy_batch (gclassify.h) on the CPU
 * over host pointers, for the packets the GPU did not see: the copy_batch
 * loop of iokernel/dma.c:179-188 with the rte_pktmbuf_append check made a
 * refusal.  @in and @out are gcl_copy_batch's structs with every pointer a
 * host pointer (in->group and in->len_hint are not looked at); @counts is a
 * host u64[GCL_COPY_NR],
 * ACCUMULATED, may be NULL.  The same packets are refused, the same bytes
 * written and the same guarantee holds.  0, or -EINVAL for a wrong in->size,
 * a NULL in, out, src, src_off, len, dst or pkt_len, src_len or dst_len ==
 * UINT64_MAX, n > 2^40, or a dst_stride < 16, not a multiple of 16 or > 2^20
 * when dst_off is NULL.  n == 0 is a no-op.
 */
int gcl_copy_batch_host(const struct gcl_copy_in *in, const struct gcl_copy_out *out,
                        uint64_t *counts);

/*
 * gcl_l4_csum_host - the rule of gcl_l4_csum (gclassify.h) on the CPU over
 * host pointers, for the batches the GPU did not see: the runtime's own
 * ipv4_cksum and ipv4_udptcp_cksum fill (runtime/net/core.c:612-617,
 * runtime/net/tcp_out.c:33-39) in GCL_L4_FILL, the check of the same sum in
 * GCL_L4_VERIFY.  @b and @in are gcl_l4_csum's structs with every pointer a
 * host pointer (in->group is checked, in->len_hint not looked at); @status is
 * u8[n]; @counts is a host u64[GCL_L4C_NR], ACCUMULATED, may be NULL.  The
 * same status bytes and counts, the same bytes written by FILL and the same
 * guarantee.  0, or -EINVAL for what gcl_l4_csum refuses (the ctx apart).
 * n == 0 is a no-op.
 */
int gcl_l4_csum_host(const struct gcl_batch *b, const struct gcl_l4_in *in, uint8_t *status,
                     uint64_t *counts);

/*
 * gcl_l4_payload_host - the rule of gcl_l4_payload (gclassify.h) on the CPU
 * over host pointers, for the batches the GPU did not see: what udp_conn_recv
 * and tcp_rx_conn find out about each datagram of a list (runtime/net/udp.c:
 * 79-107, runtime/net/tcp_in.c:182-218) and the dense layout of the kept
 * payloads, sequential plain C with no workspace.  @b, @in and @out are
 * gcl_l4_payload's structs with every pointer a host pointer (in->blocks is
 * checked against GCL_PAY_MAX_BLOCKS and otherwise not looked at); @counts is
 * a host u64[GCL_PAYC_NR], ACCUMULATED, may be NULL.  The same outputs, the
 * same counts and the same guarantee.  0, or -EINVAL for what gcl_l4_payload
 * refuses (the ctx and the workspace apart).  m == 0 writes *total = 0 and
 * zero seg_bytes, and nothing else.
 */
int gcl_l4_payload_host(const struct gcl_batch *b, const struct gcl_pay_in *in,
                        const struct gcl_pay_out *out, uint64_t *counts);

/*
 * The socket table of gcl_sock_set / gcl_sock_lookup (gclassify.h) as a
 * host-only object: the same entry checks, the same table image and the same
 * probe (one shared inline function), with no GPU.  A context embeds one.
 *
 * gcl_sock_tbl_new    - an empty table, or NULL (no memory).
 * gcl_sock_tbl_set    - gcl_sock_set without -ENOENT: any @uniqid <
 *                       GCL_MAX_PROC may hold entries (-EINVAL past it).
 * gcl_sock_tbl_del    - drop @uniqid's entries; 0, or -EINVAL.
 * gcl_sock_tbl_hash_bits - a test knob: use only the low @bits (1..32) of the
 *                       table's internal hash from the next gcl_sock_tbl_set
 *                       on, so that every key falls into a few home buckets:
 *                       the longest kick chains, and the placement failure
 *                       (-ENOSPC from gcl_sock_tbl_set, the previous set
 *                       kept).  32 is the production value.  0 or -EINVAL.
 * gcl_sock_tbl_lookup_host - the rule of gcl_sock_lookup over host pointers:
 *                       @b, @verdicts (@vbytes wide: 8, 4, 2 or 1), @sock
 *                       (u32[n]) and @counts (u64[GCL_SOCK_NR], ACCUMULATED,
 *                       may be NULL) as there, @thread_bits and
 *                       @max_runtimes what the context would have.  Any byte
 *                       alignment of verdicts and sock is accepted.  0, or
 *                       -EINVAL for a NULL tbl, b, verdicts or sock, a bad
 *                       @vbytes, @thread_bits > 8, and the batches
 *                       gcl_rx_csum refuses.  n == 0 is a no-op.
 */
struct gcl_sock_tbl;
struct gcl_sock_tbl *gcl_sock_tbl_new(void);
void gcl_sock_tbl_free(struct gcl_sock_tbl *tbl);
int gcl_sock_tbl_set(struct gcl_sock_tbl *tbl, uint16_t uniqid, const struct gcl_sock_entry *e,
                     uint32_t n);
int gcl_sock_tbl_del(struct gcl_sock_tbl *tbl, uint16_t uniqid);
int gcl_sock_tbl_hash_bits(struct gcl_sock_tbl *tbl, uint32_t bits);
int gcl_sock_tbl_lookup_host(const struct gcl_sock_tbl *tbl, uint8_t vbytes, uint8_t thread_bits,
                             uint32_t max_runtimes, const struct gcl_batch *b, const void *verdicts,
                             uint32_t *sock, uint64_t *counts);

/*
 * The neighbour table of gcl_neigh_set / gcl_tx_hdr (gclassify.h) as a
 * host-only object: the same entry checks, the same table image and the same
 * probe (one shared inline function), with no GPU.  A context embeds one.
 *
 * gcl_neigh_tbl_new    - an empty table, or NULL (no memory).
 * gcl_neigh_tbl_set    - gcl_neigh_set: replace the whole set; the same
 *                        errors, the previous set kept on any of them.
 * gcl_neigh_tbl_hash_bits - a test knob: use only the low @bits (1..32) of the
 *                        table's internal hash from the next gcl_neigh_tbl_set
 *                        on, so that both buckets of many addresses collide:
 *                        the longest kick chains, and the placement failure
 *                        (-ENOSPC).  32 is the production value.  0 or -EINVAL.
 * gcl_neigh_tbl_count  - entries in the table.
 * gcl_neigh_tbl_lookup - 1 and @mac filled when @ip is in the table, 0 when it
 *                        is not, -EINVAL for a NULL tbl or mac.
 *
 * gcl_tx_hdr_host - the rule of gcl_tx_hdr (gclassify.h) on the CPU over host
 * pointers, for the segments the GPU did not see: sequential plain C with the
 * per-entry rule the kernel shares.  @tbl is the neighbour table (NULL: an
 * empty one), @rss_key the 40-byte key a context would have in cfg.rss_key;
 * @in and @out are gcl_tx_hdr's structs with every pointer a host pointer, and
 * any byte alignment of the arrays is accepted; @counts is a host
 * u64[GCL_TXHC_NR], ACCUMULATED, may be NULL.  The same outputs, the same
 * bytes written and the same guarantee.  0, or -EINVAL for a NULL rss_key and
 * for what gcl_tx_hdr refuses (the ctx and the alignments apart).  m == 0 is a
 * no-op.
 */
struct gcl_neigh_tbl;
struct gcl_neigh_tbl *gcl_neigh_tbl_new(void);
void gcl_neigh_tbl_free(struct gcl_neigh_tbl *tbl);
int gcl_neigh_tbl_set(struct gcl_neigh_tbl *tbl, const struct gcl_neigh_entry *e, uint32_t n);
int gcl_neigh_tbl_hash_bits(struct gcl_neigh_tbl *tbl, uint32_t bits);
uint32_t gcl_neigh_tbl_count(const struct gcl_neigh_tbl *tbl);
int gcl_neigh_tbl_lookup(const struct gcl_neigh_tbl *tbl, uint32_t ip, uint8_t mac[6]);
int gcl_tx_hdr_host(const struct gcl_neigh_tbl *tbl, const uint8_t rss_key[40],
                    const struct gcl_txh_in *in, const struct gcl_txh_out *out, uint64_t *counts);

/*
 * gcl_tx_seg_host - the rule of gcl_tx_seg (gclassify.h) on the CPU over host
 * pointers, for the writes the GPU did not see: tcp_write3's window clamp and
 * tcp_tx_send's segmenter loop (runtime/net/tcp.c:1362-1380, tcp_out.c:
 * 313-386) and udp_write_to's size check (udp.c:590-591) in their closed form,
 * sequential plain C with the per-write and per-segment rule the kernels
 * share and no workspace.  @in and @out are gcl_tx_seg's structs with every
 * pointer a host pointer (in->blocks is checked against GCL_SEG_MAX_BLOCKS and
 * otherwise not looked at); @counts is a host u64[GCL_SEGC_NR], ACCUMULATED,
 * may be NULL.  The same outputs, the same counts and the same guarantee.  0,
 * or -EINVAL for what gcl_tx_seg refuses (the ctx and the workspace apart).
 * m == 0 writes the two totals as 0 and nothing else.
 */
int gcl_tx_seg_host(const struct gcl_seg_in *in, const struct gcl_seg_out *out, uint64_t *counts);

/*
 * gcl_tcp_rx_host - the rule of gcl_tcp_rx (gclassify.h) on the CPU over host
 * pointers, for the lists the GPU did not see: tcp_rx_conn's established fast
 * path (runtime/net/tcp_in.c:197-296) for every connection's segments in
 * arrival order, sequential plain C with the rule the kernels share
 * (csrc/gcl_tcprx.h).  It walks the list once and keeps every connection's
 * live words in out_conn, so it needs no grouping and no workspace; a second
 * walk adds conn_off to the FAST entries' dst_off.  @b, @in and @out are
 * gcl_tcp_rx's structs with every pointer a host pointer (in->blocks is
 * checked against GCL_TCPRX_MAX_BLOCKS and otherwise not looked at); @counts
 * is a host u64[GCL_TCPRXC_NR], ACCUMULATED, may be NULL.  The same outputs
 * byte for byte, the same counts and the same guarantee.  0, or -EINVAL for
 * what gcl_tcp_rx refuses (the ctx and the workspace apart).
 */
int gcl_tcp_rx_host(const struct gcl_batch *b, const struct gcl_tcprx_in *in,
                    const struct gcl_tcprx_out *out, uint64_t *counts);

/*
 * gcl_tcp_rx_full_host - the rule of gcl_tcp_rx_full (gclassify.h) on the CPU
 * over host pointers: gcl_tcp_rx_host's walk with the fast path and the
 * established part of __tcp_rx_conn (runtime/net/tcp_in.c:352-611), the rule
 * the kernel shares (csrc/gcl_tcprxf.h).  Every connection's live words are
 * kept in out_conn and out_ext; no grouping and no workspace.  @counts is a
 * host u64[GCL_TCPRXFC_NR], ACCUMULATED, may be NULL.  The same outputs byte
 * for byte, the same counts and the same guarantee.  0, or -EINVAL for what
 * gcl_tcp_rx_full refuses (the ctx and the workspace apart).
 */
int gcl_tcp_rx_full_host(const struct gcl_batch *b, const struct gcl_tcprxf_in *in,
                         const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext, uint64_t *counts);

/*
 * gcl_tcp_rx_ooo_host - the rule of gcl_tcp_rx_ooo (gclassify.h) on the CPU
 * over host pointers: the list is threaded per connection, then every
 * connection walks its segments in list order with its out-of-order queue in a
 * local array, composed of the pieces of csrc/gcl_tcprxo.h that the kernel
 * composes.  It allocates 4 (m + 2 nconn) bytes for the threading and frees
 * them before it returns; no workspace.  @counts is a host
 * u64[GCL_TCPRXOC_NR], ACCUMULATED, may be NULL.  The same outputs byte for
 * byte, the same counts and the same guarantee.  0, -EINVAL for what
 * gcl_tcp_rx_ooo refuses (the ctx and the workspace apart), or -ENOMEM.
 */
int gcl_tcp_rx_ooo_host(const struct gcl_batch *b, const struct gcl_tcprxo_in *in,
                        const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                        const struct gcl_tcprxo_out *ooo, uint64_t *counts);

/*
 * gcl_tcp_rx_states_host - the rule of gcl_tcp_rx_states (gclassify.h) on the
 * CPU over host pointers: gcl_tcp_rx_ooo_host's threading and walk with every
 * connection's live state beside its queue, composed of the pieces of
 * csrc/gcl_tcprxs.h that the kernel composes.  It allocates 4 (m + 2 nconn)
 * bytes for the threading and frees them before it returns; no workspace.
 * @counts is a host u64[GCL_TCPRXSC_NR], ACCUMULATED, may be NULL.  The same
 * outputs byte for byte, the same counts and the same guarantee.  0, -EINVAL
 * for what gcl_tcp_rx_states refuses (the ctx and the workspace apart), or
 * -ENOMEM.
 */
int gcl_tcp_rx_states_host(const struct gcl_batch *b, const struct gcl_tcprxs_in *in,
                           const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                           const struct gcl_tcprxo_out *ooo, const struct gcl_tcprxs_out *st, uint64_t *counts);

/*
 * gcl_tcp_tick_host, gcl_tcp_rx_acks_host - the rules of gcl_tcp_tick and
 * gcl_tcp_rx_acks (gclassify.h) on the CPU over host pointers, for the sweeps
 * and lists the GPU did not see: tcp_worker's walk with tcp_handle_timeouts and
 * tcp_timer_update (runtime/net/tcp.c:46-174) at one clock reading, and the
 * segments of tcp_tx_ack and tcp_tx_probe_window (runtime/net/tcp_out.c:
 * 178-228), sequential plain C with the rules the kernels share
 * (csrc/gcl_tcptmr.h) and no workspace.  @in and @out are the calls' structs
 * with every pointer a host pointer (in->blocks is checked against
 * GCL_TICK_MAX_BLOCKS and otherwise not looked at); @counts is a host
 * u64[GCL_TICKC_NR], ACCUMULATED, may be NULL.  The same outputs byte for
 * byte, the same counts and the same guarantee.  0, or -EINVAL for what the
 * calls refuse (the ctx and the workspace apart).
 */
int gcl_tcp_tick_host(const struct gcl_tick_in *in, const struct gcl_tick_out *out, uint64_t *counts);
/*
 * gcl_tcp_rx_ctl_host - the rule of gcl_tcp_rx_ctl (gclassify.h) on the CPU
 * over host pointers: one walk over the list with gcl_rxctl_kind and
 * gcl_ctl_rst_desc of csrc/gcl_tcptmr.h.  @counts is a host u64[GCL_TICKC_NR],
 * ACCUMULATED (GCL_RXACKC_* slots), may be NULL.  The same outputs byte for
 * byte.  0, or -EINVAL for what gcl_tcp_rx_ctl refuses (the ctx and the
 * workspace apart).
 */
int gcl_tcp_rx_ctl_host(const struct gcl_rxctl_in *in, const struct gcl_ctlseg_out *out, uint64_t *counts);
int gcl_tcp_rx_acks_host(const struct gcl_rxack_in *in, const struct gcl_ctlseg_out *out, uint64_t *counts);

/*
 * gcl_tcp_rx_open_host - the rule of gcl_tcp_rx_open (gclassify.h) on the CPU
 * over host pointers, taken literally: one walk over the list in order with
 * the running backlog and a table of the tuples accepted so far, the
 * per-entry rule and the option walk being the inline code of
 * csrc/gcl_tcpopen.h that the kernels run.  in->blocks and in->hash_slots are
 * checked (hash_slots sizes the twin's own table too).  @counts is a host
 * u64[GCL_OPENC_NR], ACCUMULATED, may be NULL.  The same outputs byte for
 * byte, the same counts and the same guarantee.  0, -EINVAL for what the call
 * refuses (the ctx and the workspace apart), or -ENOMEM.
 */
int gcl_tcp_rx_open_host(const struct gcl_batch *b, const struct gcl_tcpopen_in *in,
                         const struct gcl_tcpopen_out *out, const struct gcl_ctlseg_out *seg, uint64_t *counts);

/*
 * gcl_udp_rx_host - the rule of gcl_udp_rx (gclassify.h) on the CPU over host
 * pointers, taken literally: one walk over the list in order with every
 * socket's running inq_len kept in out_sock, each datagram compared and pushed
 * as udp_conn_recv does it under inq_lock (runtime/net/udp.c:89-100,
 * gcl_udprx_step of csrc/gcl_udprx.h).  It does NOT use the closed form the
 * kernels use (rank against inq_cap - inq_len), so the twin and the kernels
 * check each other.  No grouping and no workspace; a second walk adds
 * sock_off and rec_off and writes the records.  @b, @in and @out are
 * gcl_udp_rx's structs with every pointer a host pointer (in->blocks is
 * checked against GCL_UDPRX_MAX_BLOCKS and otherwise not looked at); @counts
 * is a host u64[GCL_UDPRXC_NR], ACCUMULATED, may be NULL.  The same outputs
 * byte for byte, the same counts and the same guarantee.  0, or -EINVAL for
 * what gcl_udp_rx refuses (the ctx and the workspace apart).
 */
int gcl_udp_rx_host(const struct gcl_batch *b, const struct gcl_udprx_in *in,
                    const struct gcl_udprx_out *out, uint64_t *counts);

/*
 * gcl_tcp_txq_host - the rule of gcl_tcp_txq (gclassify.h) on the CPU over
 * host pointers, for the queues the GPU did not see: tcp_conn_ack
 * (runtime/net/tcp.c:217-238), tcp_tx_retransmit with tcp_tx_retransmit_one
 * (runtime/net/tcp_out.c:480-506, :388-444) and tcp_tx_fast_retransmit_start
 * (tcp_out.c:450-466) for every connection at one clock reading.  The rule is
 * the inline code of csrc/gcl_txq.h that the kernels run, so the same inputs
 * give the same out_conn, state, per-segment arrays and totals byte for byte,
 * the same counts and the same guarantee.  in->blocks is checked and otherwise
 * ignored.  0, or -EINVAL for what the call refuses (the ctx and the workspace
 * apart).
 */
int gcl_tcp_txq_host(const struct gcl_txq_in *in, const struct gcl_txq_out *out, uint64_t *counts);

/*
 * gcl_tcp_read_host - the rule of gcl_tcp_read (gclassify.h) on the CPU over
 * host pointers, on one core: tcp_wait_rx, then tcp_read_wait's or
 * tcp_read_wait_peek's loop over the connection's queue (runtime/net/tcp.c:
 * 850-934, :963-988) taken literally, and copy_into_iov's two cursors
 * (:1133-1185) for the copy items.  The GPU reaches the same numbers through
 * prefix sums and searches, so the twin and the kernels check each other; the
 * wait, the ACK test, the flags and an item's words are the inline code of
 * csrc/gcl_tcpread.h that both run.  The same out_conn, items, segments and
 * totals byte for byte, the same counts and the same guarantee.  in->blocks is
 * checked and otherwise ignored.  0, or -EINVAL for what the call refuses (the
 * ctx and the workspace apart).
 */
int gcl_tcp_read_host(const struct gcl_rd_in *in, const struct gcl_rd_out *out, uint64_t *counts);

/*
 * gcl_tcp_write_host - the rule of gcl_tcp_write (gclassify.h) on the CPU over
 * host pointers, on one core: the wait of csrc/gcl_tcpwrite.h, then
 * tcp_writev2's loop over the vectors (runtime/net/tcp.c:1405-1416) and
 * tcp_tx_send's do ... while (tcp_out.c:329-380) over a simulated mbuf, taken
 * literally, with (size_t)(fill - 20) < mss as the hold test.  A connection is
 * run once to count and, when its segments, items and slots fit, once more to
 * write.  The GPU reaches the same numbers through closed forms, so the twin
 * and the kernels check each other.  The same out_conn, segments, items and
 * totals byte for byte, the same counts and the same guarantee.  in->blocks is
 * checked and otherwise ignored.  The time grows with the segments: a window
 * of 2^31 - 1 bytes at mss 1 is that many passes.  0, or -EINVAL for what the
 * call refuses (the ctx and the workspace apart).
 */
int gcl_tcp_write_host(const struct gcl_wr_in *in, const struct gcl_wr_out *out, uint64_t *counts);

/*
 * gcl_tcp_shut_host - the rule of gcl_tcp_shut (gclassify.h) on the CPU over
 * host pointers, on one core: gcl_shut_rule of csrc/gcl_tcpshut.h for every
 * connection in turn, the count of wanted segments running.  The same
 * out_conn, segments, queue records and totals byte for byte, the same counts
 * and the same guarantee.  in->blocks is checked and otherwise ignored.  0, or
 * -EINVAL for what the call refuses (the ctx and the workspace apart).
 */
int gcl_tcp_shut_host(const struct gcl_shut_in *in, const struct gcl_shut_out *out, uint64_t *counts);

/*
 * gcl_host_deliver - consume @n verdicts in order.
 * @clients_by_id  dp.clients_by_id (iokernel/defs.h:386), @max_runtimes long
 * @clients        dp.clients[0..nr_clients) (broadcast order, rx.c:175)
 * @pkt_len/@olflags per-packet mbuf metadata (olflags NULL: @default_olflags)
 * @shmptr         per-packet ptr_to_shmptr(ingress region, data) (rx.c:82)
 * @stats          u64[GCL_NR_STATS], accumulated (host-side counters only)
 * Returns the number of packets handed to a runtime.
 */
uint64_t gcl_host_deliver(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                          struct gcl_host_proc *const *clients, int nr_clients,
                          const struct gcl_verdict *v, const uint16_t *pkt_len,
                          const uint8_t *olflags, uint8_t default_olflags,
                          const uint64_t *shmptr, uint64_t n,
                          const struct gcl_host_ops *ops, uint64_t *stats);

/*
 * gcl_host_deliver4 - the same over compact verdicts (GCL_CFG_VERDICT4), whose
 * @thread is the flow_tbl slot (hash % thread_count) like gcl_verdict's.
 * @bcast_hash     per-packet hash for GCL_ACT_BROADCAST fan-out: in
 *                 GCL_HASH_NIC mode the mbuf hash.rss array the batch was
 *                 classified with (masked to 16 bits under GCL_CFG_HASH16);
 *                 NULL in the computed modes, where ARP hashes to 0.
 */
uint64_t gcl_host_deliver4(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                           struct gcl_host_proc *const *clients, int nr_clients,
                           const struct gcl_verdict4 *v, const uint32_t *bcast_hash,
                           const uint16_t *pkt_len, const uint8_t *olflags,
                           uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                           const struct gcl_host_ops *ops, uint64_t *stats);

/* gcl_verdict2_to4 - widen a GCL_CFG_VERDICT2 verdict of a context opened
 * with @thread_bits to the gcl_verdict4 the same packet gets under
 * GCL_CFG_VERDICT4 (GCL_ACT_F_FDIR aside, which the 2-byte form drops). */
struct gcl_verdict4 gcl_verdict2_to4(uint16_t v, uint8_t thread_bits);

/*
 * gcl_host_deliver2 - gcl_host_deliver4 over 2-byte verdicts: the same
 * replay of rx_send_pkt_to_runtime / rx_send_to_runtime (rx.c:50-92),
 * packet by packet, of @v widened by gcl_verdict2_to4.  The DELIVER
 * fast path reads flow_tbl[slot] of the runtime the queue index names.
 */
uint64_t gcl_host_deliver2(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                           struct gcl_host_proc *const *clients, int nr_clients,
                           const uint16_t *v, uint8_t thread_bits, const uint32_t *bcast_hash,
                           const uint16_t *pkt_len, const uint8_t *olflags,
                           uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                           const struct gcl_host_ops *ops, uint64_t *stats);

/* gcl_verdict1_to4 - widen a GCL_CFG_VERDICT1 verdict of a context opened
 * with @thread_bits: a queue verdict becomes DELIVER of that flow_tbl slot
 * (the post-pass takes rx.c's wake path itself when the runtime has no
 * active kthread), any other its action. */
struct gcl_verdict4 gcl_verdict1_to4(uint8_t v, uint8_t thread_bits);

/*
 * gcl_host_deliver1 - gcl_host_deliver2 over 1-byte verdicts (GCL_CFG_VERDICT1),
 * with the same outcome packet by packet.
 */
uint64_t gcl_host_deliver1(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                           struct gcl_host_proc *const *clients, int nr_clients,
                           const uint8_t *v, uint8_t thread_bits, const uint32_t *bcast_hash,
                           const uint16_t *pkt_len, const uint8_t *olflags,
                           uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                           const struct gcl_host_ops *ops, uint64_t *stats);

/*
 * gcl_host_deliver_recs - the same post-pass straight over a burst's verdict
 * records in the persistent loop's ring slot (gcl_rxloop_peek), without
 * copying them out: @vbytes is the context's verdict width (1, 2, 4 or 8)
 * and @thread_bits its GclCfg.thread_bits (1- and 2-byte verdicts).
 * Returns 0 for a bad @vbytes / @thread_bits.
 */
uint64_t gcl_host_deliver_recs(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                               struct gcl_host_proc *const *clients, int nr_clients,
                               const struct gcl_loop_rec *recs, uint8_t vbytes,
                               uint8_t thread_bits, const uint32_t *bcast_hash,
                               const uint16_t *pkt_len, const uint8_t *olflags,
                               uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                               const struct gcl_host_ops *ops, uint64_t *stats);

/*
 * gcl_host_deliver_idx - the same post-pass over the packets @idx[0..m) of a
 * batch, in list order: one list of a delivery plan (gcl_plan, gclassify.h).
 * @v is the batch's whole verdict array in the context's width @vbytes (1, 2,
 * 4 or 8; @thread_bits as gcl_host_deliver2 / 1); every per-packet array
 * (@v, @bcast_hash, @pkt_len, @olflags, @shmptr) is indexed by idx[j], and
 * every callback is given idx[j].  The per-packet work is that of
 * gcl_host_deliver{,4,2,1}.  Returns 0 for a bad @vbytes / @thread_bits.
 *
 * Guarantee: delivering the per-runtime lists of a GCL_PLAN_BY_RUNTIME plan
 * one after another (in any order of runtimes, from any cores, as long as one
 * runtime's list is delivered by one core) puts the same message sequence
 * into every kthread ring as gcl_host_deliver* does over the whole batch,
 * with the same counters in sum -- provided no callback during the batch
 * changes ANOTHER runtime's flow_tbl or active_thread_count: inside one
 * runtime's list the packet order is the batch's, and a runtime's steering
 * depends on nothing else.  A sched_add_core that preempts another runtime to
 * find a core (sched.c:208-216) is outside the guarantee.  The lists of a
 * GCL_PLAN_BY_QUEUE plan keep the order within a queue only.  The host bucket
 * (BROADCAST, ARP_RESPOND, drops) touches every client's rings: it is
 * delivered by whichever core owns dp.clients, and never while another core
 * delivers (rings are single-producer); an Azure ARP broadcast's messages
 * then sit before or after the batch's unicast messages instead of between
 * them.
 */
uint64_t gcl_host_deliver_idx(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                              struct gcl_host_proc *const *clients, int nr_clients,
                              const void *v, uint8_t vbytes, uint8_t thread_bits,
                              const uint32_t *bcast_hash, const uint16_t *pkt_len,
                              const uint8_t *olflags, uint8_t default_olflags,
                              const uint64_t *shmptr, const uint32_t *idx, uint64_t m,
                              const struct gcl_host_ops *ops, uint64_t *stats);

/*
 * gcl_host_deliver_packed - gcl_host_deliver_idx over the same list @idx[0..m)
 * of a batch of @n packets, fed by the list's packed records (gcl_plan_pack,
 * gclassify.h) instead of the per-packet arrays: @cmd[j], @payload[j] and
 * @v4[j] are the message and the widened verdict of packet idx[j], read
 * sequentially at the list position j.  idx[j] itself is only the packet
 * number given to the callbacks and the index into @bcast_hash (NULL: hash 0,
 * as gcl_host_deliver4).  @cmd[j] has bit 63, the ring's parity bit, clear, as
 * gcl_rx_make_cmd leaves it.  The DELIVER fast path and every other path are
 * gcl_host_deliver4's.  An entry with idx[j] >= n (gcl_plan_pack gave it the
 * empty record) is skipped: no callback, no counter.  Returns 0 when @cmd,
 * @payload, @v4 or @idx is NULL.
 *
 * Guarantee: for 4-, 2- and 1-byte contexts every list leaves the ring
 * messages, callbacks, counters and return value of gcl_host_deliver_idx over
 * that list, so the guarantee above carries over.  For 8-byte contexts the
 * same holds for the runtime lists; their host bucket stays with
 * gcl_host_deliver_idx, because an Azure ARP broadcast fans out by the
 * verdict's own hash, which the packed records do not carry.
 */
uint64_t gcl_host_deliver_packed(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                                 struct gcl_host_proc *const *clients, int nr_clients,
                                 const uint64_t *cmd, const uint64_t *payload,
                                 const struct gcl_verdict4 *v4, const uint32_t *idx,
                                 uint64_t m, uint64_t n, const uint32_t *bcast_hash,
                                 const struct gcl_host_ops *ops, uint64_t *stats);

/*
 * gcl_host_prefetch_rxq - a hint for a dataplane thread with time to spare
 * (waiting for a burst's verdicts): the ring slot each kthread's next message
 * lands in, and the channel state, taken for writing, so that the post-pass
 * after the wait writes lines it owns.  No effect on results.
 */
void gcl_host_prefetch_rxq(struct gcl_host_proc *const *clients, int nr_clients);

#ifdef __cplusplus
}
#endif

#endif
