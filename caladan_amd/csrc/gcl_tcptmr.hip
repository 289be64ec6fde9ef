/*
 * gcl_tcptmr.hip - the TCP timer sweep and the control segments it and a
 * gcl_tcp_rx call ask for (gcl_tcp_tick, gcl_tcp_rx_acks, gclassify.h):
 * tcp_worker's walk over all connections with tcp_handle_timeouts and
 * tcp_timer_update (runtime/net/tcp.c:46-174), and tcp_tx_ack /
 * tcp_tx_probe_window (runtime/net/tcp_out.c:178-228) as gcl_txh_desc records
 * in send order.  The rules are those of gcl_tcptmr.h, the same inline code the
 * host twins run.
 *
 * Both calls are an ordered compaction: item i (a connection, or a list entry)
 * asks for 0..2 segments, and segment k of the call lies at the sum of the
 * items before it.  Three launches on the stream, and no block ever waits for
 * another: no look-back, no flag, no cooperative launch; no atomic hands out a
 * position.  The items are cut into `blocks` contiguous ranges of whole
 * 256-item tiles (the library's choice, or in->blocks), as gcl_tx_seg cuts its
 * writes.
 *
 *   decide   block r walks range r, one lane per item.  The sweep: the 64-B
 *            timer record as four 16-B loads, the rule, out_tmr as two 16-B
 *            stores (NOSPACE is not known yet).  The ACKs of a list: verdict,
 *            sflags and the two guards.  A lane's segments are two bits, so
 *            the wave's count is the population count of two ballots; the
 *            range's sum goes to workspace word r, and every block stores it.
 *   top      one block turns the range sums into their exclusive prefix sums
 *            in place and writes totals (and the two segment counters).
 *   emit     block r walks range r again tile by tile.  A lane gets its two
 *            bits back (the sweep: from out_tmr's action byte; a list: from
 *            the same test), its position is the range's base + the tiles
 *            before + the waves before (LDS, two buffers in turn: one barrier
 *            per tile) + the population count of the ballots below its lane.
 *            A segment below seg_cap is written: desc as two 16-B stores,
 *            frame_off, seg_conn, seg_kind, seg_src; a connection with one at
 *            or past seg_cap gets NOSPACE, a one-byte store into out_tmr.
 *
 * Bounds.  An item index is used only below nconn or m, a packet index only
 * below n, a cookie only below nconn, a segment index only below seg_cap, a
 * workspace word only below blocks.  Nothing is written outside the first
 * seg_cap entries of the per-segment arrays, out_tmr[0, nconn), totals, counts
 * and the workspace.  No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_tcptmr.h"

namespace gclk {

constexpr uint32_t kTmrThreads = 256;
constexpr uint32_t kTmrWaves = kTmrThreads / 64;
constexpr uint32_t kTmrBlocksPerCu = 4;
constexpr uint32_t kTmrTopPer = GCL_TICK_MAX_BLOCKS / kTmrThreads;
static_assert(kTmrTopPer * kTmrThreads == GCL_TICK_MAX_BLOCKS, "the top kernel is one block");
static_assert(sizeof(struct gcl_tcp_tmr) == 64 && sizeof(struct gcl_tcp_tmr_out) == 32 &&
              sizeof(struct gcl_tcp_addr) == 16, "records as 16-B words");

/* what both calls share: the compaction and the per-segment outputs */
struct CtlParams {
	uint4 *desc;
	uint64_t *frame_off;
	uint32_t *seg_conn;
	uint8_t *seg_kind;
	uint32_t *seg_src;
	unsigned long long *totals;
	unsigned long long *counts;
	uint32_t *bsum;            /* workspace: [blocks], a range's segments, then the segments before it */
	const uint4 *conn;         /* struct gcl_tcp_conn as three 16-B words */
	const uint4 *addr;
	uint64_t items, per;       /* per: items per range, a multiple of kTmrThreads */
	uint64_t seg_cap, frame_base;
	uint32_t nconn, frame_stride, blocks;
	uint32_t cnt_wanted, cnt_written; /* counter slots of the top kernel; >= GCL_TICKC_NR: none */
};

struct TickParams {
	const uint4 *tmr;
	uint4 *out_tmr;
	uint64_t now;
};

struct RxackParams {
	const uint32_t *order, *sock;
	const uint8_t *verdict, *sflags;
	const uint32_t *after;
	uint64_t n;
};

/* the range's segments -> bsum[blockIdx.x]; @wave_sum: this wave's, summed over its tiles (wave-uniform) */
__device__ __forceinline__ void ctl_store_sum(const CtlParams &k, uint32_t wave_sum)
{
	__shared__ uint32_t ws[kTmrWaves];

	if ((threadIdx.x & 63) == 0)
		ws[threadIdx.x >> 6] = wave_sum;
	__syncthreads();
	if (threadIdx.x == 0)
		k.bsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ void __launch_bounds__(kTmrThreads) tick_decide_kernel(CtlParams k, TickParams p)
{
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.items ? lo + k.per : k.items; /* lo >= items: an empty range */
	uint32_t segs = 0, cnt[6] = {0, 0, 0, 0, 0, 0};                  /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kTmrThreads) { /* uniform: every lane reaches the ballots */
		const uint64_t c = j0 + threadIdx.x;
		uint32_t action = 0;
		if (c < hi) {
			const uint4 a = p.tmr[4 * c], b = p.tmr[4 * c + 1], d = p.tmr[4 * c + 2], e = p.tmr[4 * c + 3];
			struct gcl_tcp_tmr t;
			struct gcl_tcp_tmr_out o;
			t.next_timeout = (uint64_t)a.y << 32 | a.x;
			t.attach_ts = (uint64_t)a.w << 32 | a.z;
			t.time_wait_ts = (uint64_t)b.y << 32 | b.x;
			t.ack_ts = (uint64_t)b.w << 32 | b.z;
			t.zero_wnd_ts = (uint64_t)d.y << 32 | d.x;
			t.txq_ts = (uint64_t)d.w << 32 | d.z;
			t.state = (uint8_t)e.x;
			t.flags = (uint8_t)(e.x >> 8);
			action = gcl_tmr_sweep(&t, p.now, &o);
			p.out_tmr[2 * c] = make_uint4((uint32_t)o.next_timeout, (uint32_t)(o.next_timeout >> 32),
			                              (uint32_t)o.zero_wnd_ts, (uint32_t)(o.zero_wnd_ts >> 32));
			p.out_tmr[2 * c + 1] = make_uint4((uint32_t)o.state | (uint32_t)o.flags << 8 | action << 16, 0, 0, 0);
		}
		const uint32_t sg = gcl_tmr_segs(action);
		segs += (uint32_t)__popcll(__ballot(sg & 1u)) + (uint32_t)__popcll(__ballot(sg & 2u));
		if (k.counts) {
#pragma unroll
			for (uint32_t x = 0; x < 6; x++)
				cnt[x] += (uint32_t)__popcll(__ballot((action >> x) & 1u)); /* FIRED .. CLOSE: bits 0..5 */
		}
	}
	if (k.counts && (threadIdx.x & 63) == 0) {
#pragma unroll
		for (uint32_t x = 0; x < 6; x++)
			if (cnt[x])
				atomicAdd(k.counts + GCL_TICKC_FIRED + x, (unsigned long long)cnt[x]);
	}
	ctl_store_sum(k, segs);
}

/* list entry j: 1 when it emits an ACK, with its connection; 2 when only the guards keep it from one */
__device__ __forceinline__ uint32_t rxack_want(const CtlParams &k, const RxackParams &p, uint64_t j, uint32_t *conn)
{
	*conn = 0;
	if (!gcl_rxack_asked(p.verdict[j], p.sflags[j]))
		return 0;
	const uint64_t i = p.order ? p.order[j] : j;
	if (i >= p.n)
		return 2;
	const uint32_t c = p.sock[i];
	if (c >= k.nconn)
		return 2;
	*conn = c;
	return 1;
}

__global__ void __launch_bounds__(kTmrThreads) rxack_decide_kernel(CtlParams k, RxackParams p)
{
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.items ? lo + k.per : k.items;
	uint32_t segs = 0, skipped = 0; /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kTmrThreads) {
		const uint64_t j = j0 + threadIdx.x;
		uint32_t c;
		const uint32_t w = j < hi ? rxack_want(k, p, j, &c) : 0;
		segs += (uint32_t)__popcll(__ballot(w == 1));
		skipped += (uint32_t)__popcll(__ballot(w == 2));
	}
	if (k.counts && (threadIdx.x & 63) == 0 && skipped)
		atomicAdd(k.counts + GCL_RXACKC_SKIPPED, (unsigned long long)skipped);
	ctl_store_sum(k, segs);
}

/* bsum[0, blocks) -> its exclusive prefix sums; totals; one block.  A call's segments are <= 2^31. */
__global__ void __launch_bounds__(kTmrThreads) ctl_top_kernel(CtlParams k)
{
	__shared__ uint32_t sc[2][kTmrThreads];
	const uint32_t t = threadIdx.x;
	uint32_t v[kTmrTopPer], sum = 0;

#pragma unroll
	for (uint32_t x = 0; x < kTmrTopPer; x++) {
		const uint32_t r = t * kTmrTopPer + x;
		v[x] = r < k.blocks ? k.bsum[r] : 0;
		sum += v[x];
	}
	/* inclusive scan of the lanes' sums, ping-pong: one barrier per step */
	uint32_t cur = 0;
	sc[0][t] = sum;
	__syncthreads();
	for (uint32_t step = 1; step < kTmrThreads; step <<= 1) {
		const uint32_t a = t >= step ? sc[cur][t - step] + sc[cur][t] : sc[cur][t];
		sc[cur ^ 1][t] = a;
		cur ^= 1;
		__syncthreads();
	}
	uint32_t base = t ? sc[cur][t - 1] : 0;
#pragma unroll
	for (uint32_t x = 0; x < kTmrTopPer; x++) {
		const uint32_t r = t * kTmrTopPer + x;
		if (r < k.blocks)
			k.bsum[r] = base;
		base += v[x];
	}
	if (t == kTmrThreads - 1) {
		const unsigned long long wanted = base, written = wanted < k.seg_cap ? wanted : k.seg_cap;
		k.totals[0] = wanted;
		k.totals[1] = written;
		if (k.counts) {
			if (k.cnt_wanted < GCL_TICKC_NR && wanted)
				atomicAdd(k.counts + k.cnt_wanted, wanted);
			if (k.cnt_written < GCL_TICKC_NR && written)
				atomicAdd(k.counts + k.cnt_written, written);
		}
	}
}

/* segment @at < seg_cap of connection @c < nconn */
__device__ __forceinline__ void ctl_store(const CtlParams &k, uint64_t at, uint32_t c, uint32_t kind, uint32_t src,
                                          uint32_t ack, uint32_t rcv_wnd, const uint4 &c0, const uint4 &ad)
{
	const uint32_t a[4] = {ad.x, ad.y, ad.z, ad.w};
	uint32_t d[8];

	gcl_ctl_desc(a, gcl_ctl_seq(kind, c0.x, c0.y), ack, rcv_wnd, d); /* snd_una, snd_nxt: words 0, 1 */
	k.desc[2 * at] = make_uint4(d[0], d[1], d[2], d[3]);
	k.desc[2 * at + 1] = make_uint4(d[4], d[5], d[6], d[7]);
	k.frame_off[at] = k.frame_base + at * k.frame_stride;
	k.seg_conn[at] = c;
	k.seg_kind[at] = (uint8_t)kind;
	k.seg_src[at] = src;
}

/* the sweep's source of segments: out_tmr's action byte, as tick_decide_kernel left it */
struct TickSrc {
	TickParams p;
	__device__ uint32_t segs(const CtlParams &k, uint64_t c, uint32_t *conn) const
	{
		*conn = (uint32_t)c;
		return gcl_tmr_segs(p.out_tmr[2 * c + 1].x >> 16);
	}
	/* rcv_nxt, rcv_wnd: words 5, 6 */
	__device__ void ack_wnd(uint64_t, const uint4 &c1, uint32_t *ack, uint32_t *wnd) const
	{
		*ack = c1.y;
		*wnd = c1.z;
	}
	__device__ void nospace(uint64_t c) const
	{
		((uint8_t *)&p.out_tmr[2 * c + 1])[2] |= GCL_TMRA_NOSPACE; /* the action byte: this lane's alone */
	}
	static constexpr uint32_t kNospaceSlot = GCL_TICKC_NOSPACE;
};

/* a list's: the same test as rxack_decide_kernel */
struct RxackSrc {
	RxackParams p;
	__device__ uint32_t segs(const CtlParams &k, uint64_t j, uint32_t *conn) const
	{
		return rxack_want(k, p, j, conn) == 1 ? 1u : 0u;
	}
	__device__ void ack_wnd(uint64_t j, const uint4 &c1, uint32_t *ack, uint32_t *wnd) const
	{
		*ack = p.after[j];
		*wnd = gcl_rxack_wnd(c1.z, c1.y, *ack);
	}
	__device__ void nospace(uint64_t) const {}
	static constexpr uint32_t kNospaceSlot = GCL_TICKC_NR; /* no such counter */
};

template <typename Src>
__global__ void __launch_bounds__(kTmrThreads) ctl_emit_kernel(CtlParams k, Src src)
{
	__shared__ uint32_t wt[2][kTmrWaves];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.items ? lo + k.per : k.items;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t below = (1ull << lane) - 1;
	uint64_t carry = lo < hi ? k.bsum[blockIdx.x] : 0; /* the range's base, then the tiles before */
	uint32_t nospace = 0, par = 0;                     /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kTmrThreads, par ^= 1) { /* uniform: every lane active */
		const uint64_t i = j0 + threadIdx.x;
		uint32_t c = 0;
		const uint32_t sg = i < hi ? src.segs(k, i, &c) : 0;
		const uint64_t m0 = __ballot(sg & 1u), m1 = __ballot(sg & 2u);
		const uint32_t ex = (uint32_t)__popcll(m0 & below) + (uint32_t)__popcll(m1 & below);

		if (lane == 0)
			wt[par][wave] = (uint32_t)__popcll(m0) + (uint32_t)__popcll(m1);
		__syncthreads();
		const uint32_t w0 = wt[par][0], w1 = wt[par][1], w2 = wt[par][2], w3 = wt[par][3];
		uint64_t at = carry + ex;
		if (wave > 0)
			at += w0;
		if (wave > 1)
			at += w1;
		if (wave > 2)
			at += w2;
		carry += (uint64_t)w0 + w1 + w2 + w3;

		bool lost = false;
		if (sg && c < k.nconn) {
			if (at + (sg == 3 ? 2 : 1) > k.seg_cap)
				lost = true;
			if (at < k.seg_cap) {
				const uint4 c0 = k.conn[3 * (size_t)c], c1 = k.conn[3 * (size_t)c + 1], ad = k.addr[c];
				uint32_t ack, wnd;
				src.ack_wnd(i, c1, &ack, &wnd);
				/* a lane's segments in send order: the ACK, then the probe */
				ctl_store(k, at, c, (sg & 1u) ? GCL_CTL_ACK : GCL_CTL_PROBE, (uint32_t)i, ack, wnd, c0, ad);
				if (sg == 3 && at + 1 < k.seg_cap)
					ctl_store(k, at + 1, c, GCL_CTL_PROBE, (uint32_t)i, ack, wnd, c0, ad);
			}
			if (lost)
				src.nospace(i);
		}
		nospace += (uint32_t)__popcll(__ballot(lost));
	}
	if (Src::kNospaceSlot < GCL_TICKC_NR && k.counts && lane == 0 && nospace)
		atomicAdd(k.counts + Src::kNospaceSlot, (unsigned long long)nospace);
}

/* ---- gcl_tcp_rx_ctl: gcl_tcp_rx_acks' three launches with the RSTs of a gcl_tcp_rx_states call ---- */

struct RxctlParams {
	RxackParams a;
	const uint8_t *ev;
	const uint32_t *rst_seq;
};

/* list entry j: its kind and connection when it emits a segment; GCL_RXCTL_NONE, @skip set when only the guards keep it from one */
__device__ __forceinline__ uint32_t rxctl_want(const CtlParams &k, const RxctlParams &p, uint64_t j, uint32_t *conn,
                                               bool *skip)
{
	*conn = 0;
	*skip = false;
	const uint32_t kind = gcl_rxctl_kind(p.a.verdict[j], p.a.sflags[j], p.ev[j]);
	if (kind == GCL_RXCTL_NONE)
		return kind;
	const uint64_t i = p.a.order ? p.a.order[j] : j;
	const uint32_t c = i < p.a.n ? p.a.sock[i] : 0xFFFFFFFFu;
	if (c >= k.nconn) {
		*skip = true;
		return GCL_RXCTL_NONE;
	}
	*conn = c;
	return kind;
}

__global__ void __launch_bounds__(kTmrThreads) rxctl_decide_kernel(CtlParams k, RxctlParams p)
{
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.items ? lo + k.per : k.items;
	uint32_t segs = 0, skipped = 0; /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kTmrThreads) { /* uniform: every lane reaches the ballots */
		const uint64_t j = j0 + threadIdx.x;
		uint32_t c;
		bool skip = false;
		const uint32_t kind = j < hi ? rxctl_want(k, p, j, &c, &skip) : GCL_RXCTL_NONE;
		segs += (uint32_t)__popcll(__ballot(kind != GCL_RXCTL_NONE));
		skipped += (uint32_t)__popcll(__ballot(skip));
	}
	if (k.counts && (threadIdx.x & 63) == 0 && skipped)
		atomicAdd(k.counts + GCL_RXACKC_SKIPPED, (unsigned long long)skipped);
	ctl_store_sum(k, segs);
}

/* ctl_emit_kernel's positions for one segment a lane at the most; segment at < seg_cap of connection c < nconn */
__global__ void __launch_bounds__(kTmrThreads) rxctl_emit_kernel(CtlParams k, RxctlParams p)
{
	__shared__ uint32_t wt[2][kTmrWaves];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.items ? lo + k.per : k.items;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t below = (1ull << lane) - 1;
	uint64_t carry = lo < hi ? k.bsum[blockIdx.x] : 0; /* the range's base, then the tiles before */
	uint32_t par = 0;

	for (uint64_t j0 = lo; j0 < hi; j0 += kTmrThreads, par ^= 1) { /* uniform: every lane active */
		const uint64_t j = j0 + threadIdx.x;
		uint32_t c = 0;
		bool skip = false;
		const uint32_t kind = j < hi ? rxctl_want(k, p, j, &c, &skip) : GCL_RXCTL_NONE;
		const uint64_t m0 = __ballot(kind != GCL_RXCTL_NONE);

		if (lane == 0)
			wt[par][wave] = (uint32_t)__popcll(m0);
		__syncthreads();
		const uint32_t w0 = wt[par][0], w1 = wt[par][1], w2 = wt[par][2], w3 = wt[par][3];
		uint64_t at = carry + (uint32_t)__popcll(m0 & below);
		if (wave > 0)
			at += w0;
		if (wave > 1)
			at += w1;
		if (wave > 2)
			at += w2;
		carry += (uint64_t)w0 + w1 + w2 + w3;

		if (kind != GCL_RXCTL_NONE && c < k.nconn && at < k.seg_cap) {
			const uint4 ad = k.addr[c];
			if (kind == GCL_CTL_ACK) {
				const uint4 c0 = k.conn[3 * (size_t)c], c1 = k.conn[3 * (size_t)c + 1];
				const uint32_t ack = p.a.after[j];
				ctl_store(k, at, c, GCL_CTL_ACK, (uint32_t)j, ack, gcl_rxack_wnd(c1.z, c1.y, ack), c0, ad);
			} else {
				const uint32_t a[4] = {ad.x, ad.y, ad.z, ad.w};
				uint32_t d[8];

				gcl_ctl_rst_desc(a, kind, p.rst_seq[j], d);
				k.desc[2 * at] = make_uint4(d[0], d[1], d[2], d[3]);
				k.desc[2 * at + 1] = make_uint4(d[4], d[5], d[6], d[7]);
				k.frame_off[at] = k.frame_base + at * k.frame_stride;
				k.seg_conn[at] = c;
				k.seg_kind[at] = (uint8_t)kind;
				k.seg_src[at] = (uint32_t)j;
			}
		}
	}
}

static bool tmr_misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

static size_t tmr_workspace(uint32_t blocks)
{
	return ((size_t)4 * (blocks ? blocks : GCL_TICK_MAX_BLOCKS) + 15) & ~(size_t)15;
}

/* what both calls refuse of the shared fields */
static bool ctl_refused(uint32_t nconn, uint32_t blocks, uint64_t seg_cap, uint32_t frame_stride, uint64_t items,
                        const struct gcl_ctlseg_out *o, const uint64_t *counts, const void *workspace,
                        size_t workspace_bytes)
{
	if (nconn > GCL_TICK_MAX_CONN || blocks > GCL_TICK_MAX_BLOCKS || seg_cap > (1ull << 31) ||
	    frame_stride < GCL_CTL_MIN_STRIDE || !o->totals)
		return true;
	if (items && seg_cap && (!o->desc || !o->frame_off || !o->seg_conn || !o->seg_kind || !o->seg_src))
		return true;
	if (tmr_misaligned(o->desc, 16) || tmr_misaligned(o->frame_off, 8) || tmr_misaligned(o->seg_conn, 4) ||
	    tmr_misaligned(o->seg_src, 4) || tmr_misaligned(o->totals, 8) || tmr_misaligned(counts, 8))
		return true;
	return !workspace || tmr_misaligned(workspace, 16) || workspace_bytes < tmr_workspace(blocks);
}

static void ctl_fill(CtlParams *k, const struct gcl_ctx *c, const struct gcl_ctlseg_out *o, uint64_t *counts,
                     void *workspace, uint64_t items, uint32_t blocks)
{
	const uint64_t tiles = (items + kTmrThreads - 1) / kTmrThreads;
	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);

	k->desc = (uint4 *)o->desc;
	k->frame_off = o->frame_off;
	k->seg_conn = o->seg_conn;
	k->seg_kind = o->seg_kind;
	k->seg_src = o->seg_src;
	k->totals = (unsigned long long *)o->totals;
	k->counts = (unsigned long long *)counts;
	k->bsum = (uint32_t *)workspace;
	k->items = items;
	k->blocks = blocks ? blocks :
	            (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::min<uint32_t>(cus * kTmrBlocksPerCu,
	                                                                                       GCL_TICK_MAX_BLOCKS)));
	/* whole tiles per range, so that every range starts at a multiple of 256 */
	k->per = std::max<uint64_t>(1, (tiles + k->blocks - 1) / k->blocks) * kTmrThreads;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tcp_tick_workspace(uint32_t nconn, uint32_t blocks, size_t *bytes)
{
	if (!bytes || nconn > GCL_TICK_MAX_CONN || blocks > GCL_TICK_MAX_BLOCKS)
		return -EINVAL;
	*bytes = tmr_workspace(blocks);
	return 0;
}

extern "C" int gcl_tcp_rx_acks_workspace(uint64_t m, uint32_t blocks, size_t *bytes)
{
	if (!bytes || m > (1ull << 31) || blocks > GCL_TICK_MAX_BLOCKS)
		return -EINVAL;
	*bytes = tmr_workspace(blocks);
	return 0;
}

extern "C" int gcl_tcp_tick(struct gcl_ctx *c, const struct gcl_tick_in *in, const struct gcl_tick_out *out,
                            uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !in || !out || in->size != sizeof(*in) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->nconn, &out->seg, counts, workspace,
	                workspace_bytes))
		return -EINVAL;
	if (in->nconn && (!in->tmr || !in->conn || !in->addr || !out->out_tmr))
		return -EINVAL;
	if (tmr_misaligned(in->tmr, 16) || tmr_misaligned(in->conn, 16) || tmr_misaligned(in->addr, 16) ||
	    tmr_misaligned(out->out_tmr, 16))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->nconn == 0)
		return hipMemsetAsync(out->seg.totals, 0, 2 * sizeof(uint64_t), s) == hipSuccess ? 0 : -EIO;

	CtlParams k;
	ctl_fill(&k, c, &out->seg, counts, workspace, in->nconn, in->blocks);
	k.conn = (const uint4 *)in->conn;
	k.addr = (const uint4 *)in->addr;
	k.nconn = in->nconn;
	k.seg_cap = in->seg_cap;
	k.frame_base = in->frame_base;
	k.frame_stride = in->frame_stride;
	k.cnt_wanted = GCL_TICKC_NR;
	k.cnt_written = GCL_TICKC_SEGS;
	const TickParams p = {(const uint4 *)in->tmr, (uint4 *)out->out_tmr, in->now};
	const TickSrc src = {p};

	hipLaunchKernelGGL(tick_decide_kernel, dim3(k.blocks), dim3(kTmrThreads), 0, s, k, p);
	hipLaunchKernelGGL(ctl_top_kernel, dim3(1), dim3(kTmrThreads), 0, s, k);
	hipLaunchKernelGGL(ctl_emit_kernel<TickSrc>, dim3(k.blocks), dim3(kTmrThreads), 0, s, k, src);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int gcl_tcp_rx_acks(struct gcl_ctx *c, const struct gcl_rxack_in *in, const struct gcl_ctlseg_out *out,
                               uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !in || !out || in->size != sizeof(*in) || in->m > (1ull << 31) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->m, out, counts, workspace,
	                workspace_bytes))
		return -EINVAL;
	if (in->m && (!in->sock || !in->verdict || !in->sflags || !in->rcv_nxt_after))
		return -EINVAL;
	if (in->m && in->nconn && (!in->conn || !in->addr))
		return -EINVAL;
	if (tmr_misaligned(in->order, 4) || tmr_misaligned(in->sock, 4) || tmr_misaligned(in->rcv_nxt_after, 4) ||
	    tmr_misaligned(in->conn, 16) || tmr_misaligned(in->addr, 16))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->m == 0)
		return hipMemsetAsync(out->totals, 0, 2 * sizeof(uint64_t), s) == hipSuccess ? 0 : -EIO;

	CtlParams k;
	ctl_fill(&k, c, out, counts, workspace, in->m, in->blocks);
	k.conn = (const uint4 *)in->conn;
	k.addr = (const uint4 *)in->addr;
	k.nconn = in->nconn;
	k.seg_cap = in->seg_cap;
	k.frame_base = in->frame_base;
	k.frame_stride = in->frame_stride;
	k.cnt_wanted = GCL_RXACKC_WANTED;
	k.cnt_written = GCL_RXACKC_WRITTEN;
	const RxackParams p = {in->order, in->sock, in->verdict, in->sflags, in->rcv_nxt_after, in->n};
	const RxackSrc src = {p};

	hipLaunchKernelGGL(rxack_decide_kernel, dim3(k.blocks), dim3(kTmrThreads), 0, s, k, p);
	hipLaunchKernelGGL(ctl_top_kernel, dim3(1), dim3(kTmrThreads), 0, s, k);
	hipLaunchKernelGGL(ctl_emit_kernel<RxackSrc>, dim3(k.blocks), dim3(kTmrThreads), 0, s, k, src);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int gcl_tcp_rx_ctl_workspace(uint64_t m, uint32_t blocks, size_t *bytes)
{
	return gcl_tcp_rx_acks_workspace(m, blocks, bytes);
}

extern "C" int gcl_tcp_rx_ctl(struct gcl_ctx *c, const struct gcl_rxctl_in *in, const struct gcl_ctlseg_out *out,
                              uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !in || !out || in->size != sizeof(*in) || in->m > (1ull << 31) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->m, out, counts, workspace,
	                workspace_bytes))
		return -EINVAL;
	if (in->m && (!in->sock || !in->verdict || !in->sflags || !in->rcv_nxt_after || !in->ev || !in->rst_seq))
		return -EINVAL;
	if (in->m && in->nconn && (!in->conn || !in->addr))
		return -EINVAL;
	if (tmr_misaligned(in->order, 4) || tmr_misaligned(in->sock, 4) || tmr_misaligned(in->rcv_nxt_after, 4) ||
	    tmr_misaligned(in->conn, 16) || tmr_misaligned(in->addr, 16) || tmr_misaligned(in->rst_seq, 4))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->m == 0)
		return hipMemsetAsync(out->totals, 0, 2 * sizeof(uint64_t), s) == hipSuccess ? 0 : -EIO;

	CtlParams k;
	ctl_fill(&k, c, out, counts, workspace, in->m, in->blocks);
	k.conn = (const uint4 *)in->conn;
	k.addr = (const uint4 *)in->addr;
	k.nconn = in->nconn;
	k.seg_cap = in->seg_cap;
	k.frame_base = in->frame_base;
	k.frame_stride = in->frame_stride;
	k.cnt_wanted = GCL_RXACKC_WANTED;
	k.cnt_written = GCL_RXACKC_WRITTEN;
	const RxctlParams p = {{in->order, in->sock, in->verdict, in->sflags, in->rcv_nxt_after, in->n}, in->ev,
	                       in->rst_seq};

	hipLaunchKernelGGL(rxctl_decide_kernel, dim3(k.blocks), dim3(kTmrThreads), 0, s, k, p);
	hipLaunchKernelGGL(ctl_top_kernel, dim3(1), dim3(kTmrThreads), 0, s, k);
	hipLaunchKernelGGL(rxctl_emit_kernel, dim3(k.blocks), dim3(kTmrThreads), 0, s, k, p);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
