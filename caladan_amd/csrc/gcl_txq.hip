/*
 * gcl_txq.hip - the TCP retransmit queue of a batch of connections
 * (gcl_tcp_txq, gclassify.h): tcp_conn_ack's pops (runtime/net/tcp.c:217-238),
 * tcp_tx_retransmit's walk with tcp_tx_retransmit_one
 * (runtime/net/tcp_out.c:480-506, :388-444) and tcp_tx_fast_retransmit_start
 * (tcp_out.c:450-466) for every connection of one runtime at one clock
 * reading, the retransmitted segments as gcl_txh_desc records in send order.
 * The rule is that of gcl_txq.h, the same inline code the host twin runs.
 *
 * The call is an ordered compaction, the shape of gcl_tcptmr.hip: connection c
 * asks for 0..17 segments and segment k of the call lies at the sum of the
 * connections before it.  Three launches on the stream, and no block ever
 * waits for another; no atomic hands out a position.  The connections are cut
 * into `blocks` contiguous ranges of whole 256-connection tiles.
 *
 *   decide   block r walks range r, one lane per connection, as if seg_cap
 *            were unbounded: state[] of its whole queue, out_conn[c] with the
 *            count of its segments in nretx.  A lane walks a queue shorter
 *            than kTxqLong itself with gcl_txq_conn; neighbouring lanes' queues
 *            are neighbouring memory.  Then the wave takes up its long queues
 *            one at a time (txq_wave): a ballot finds them, shuffles broadcast
 *            the connection, and the wave strides through 64 entries a step.
 *            Ballots and their first set bits find the first young entry, the
 *            first unacknowledged one, the 16th segment and the first without
 *            room; population counts number the segments.  The walk needs
 *            tcp_off and tcp_flags of a wanted entry to know whether it is
 *            refused (a refused one does not count towards the 16), so the
 *            cold array is read for wanted entries and for no others.  The
 *            range's sum goes to workspace word r.
 *   top      one block turns the range sums into their exclusive prefix sums
 *            in place, writes totals[0..1] and zeroes totals[2].
 *   emit     block r walks range r again.  A lane gets its count back from
 *            out_conn, its position is the range's base + the tiles before +
 *            the waves before (LDS, two buffers in turn: one barrier per tile)
 *            + the counts of the lanes below (five ballots: a count is below
 *            32).  It stores `first`; a connection that asked for segments is
 *            walked once more, by the same two paths, now with the room its
 *            position leaves it and with the stores of its segments: that
 *            rewrites its state[] and out_conn[c], which differ from decide's
 *            only where seg_cap cut the walk short.
 *
 * Every store has the width of what it writes: a descriptor is two 16-B
 * stores, out_conn two 16-B stores (`first` alone: 4 B), a state one byte.
 *
 * Bounds.  A connection index is used only below nconn; an entry index only
 * inside a range that gcl_txq_range found inside [0, nent]; a segment index
 * only below seg_cap (room = seg_cap - first, first <= seg_cap); a workspace
 * word only below blocks.  No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_txq.h"

namespace gclk {

constexpr uint32_t kTxqThreads = 256;
constexpr uint32_t kTxqWaves = kTxqThreads / 64;
constexpr uint32_t kTxqBlocksPerCu = 4;
constexpr uint32_t kTxqTopPer = GCL_TXQ_MAX_BLOCKS / kTxqThreads;
/* a queue of this many entries or more is walked by the whole wave: one cooperative stride */
constexpr uint32_t kTxqLong = 64;
static_assert(kTxqTopPer * kTxqThreads == GCL_TXQ_MAX_BLOCKS, "the top kernel is one block");
static_assert(sizeof(struct gcl_txq_ent) == 16 && sizeof(struct gcl_txq_cold) == 16 &&
              sizeof(struct gcl_txq_conn_out) == 32 && sizeof(struct gcl_tcp_conn) == 48 &&
              sizeof(struct gcl_tcp_addr) == 16 && sizeof(struct gcl_txh_desc) == 32, "records as 16-B words");

struct TxqParams {
	struct gcl_txq_out out;
	const uint32_t *qoff;
	const uint4 *ent;  /* struct gcl_txq_ent and gcl_txq_cold as 16-B words */
	const uint4 *cold;
	const uint4 *conn; /* struct gcl_tcp_conn as three 16-B words */
	const uint4 *addr;
	const uint8_t *want;
	unsigned long long *counts;
	uint32_t *bsum;    /* workspace: [blocks], a range's segments, then the segments before it */
	uint64_t nent, seg_cap, frame_base, now;
	uint64_t per;      /* connections per range, a multiple of kTxqThreads */
	uint32_t nconn, frame_stride, blocks;
};

__device__ __forceinline__ struct gcl_txq_ent txq_ent(const uint4 &v)
{
	struct gcl_txq_ent h;
	h.seg_seq = v.x;
	h.seg_end = v.y;
	h.ts = (uint64_t)v.w << 32 | v.z;
	return h;
}

__device__ __forceinline__ struct gcl_txq_cold txq_cold(const uint4 &v)
{
	struct gcl_txq_cold q = {};
	q.frame_off = (uint64_t)v.y << 32 | v.x;
	q.tcp_flags = (uint8_t)v.z;
	q.tcp_off = (uint8_t)(v.z >> 8);
	q.flags = (uint8_t)(v.z >> 16);
	return q;
}

__device__ __forceinline__ uint64_t txq_shfl64(uint64_t v, uint32_t src)
{
	return (uint64_t)__shfl((uint32_t)(v >> 32), src) << 32 | __shfl((uint32_t)v, src);
}

__device__ __forceinline__ uint64_t txq_wave_sum(uint64_t v)
{
#pragma unroll
	for (int s = 32; s; s >>= 1)
		v += (uint64_t)__shfl_xor((uint32_t)(v >> 32), s) << 32 | __shfl_xor((uint32_t)v, s);
	return v;
}

/* a connection as a lane holds it */
struct TxqConn {
	struct gcl_txq_cx x;
	uint32_t e0, n, bad;
};

__device__ __forceinline__ TxqConn txq_load(const TxqParams &p, uint32_t c)
{
	TxqConn t;
	const uint4 c0 = p.conn[3 * (size_t)c], c1 = p.conn[3 * (size_t)c + 1], ad = p.addr[c];
	const uint32_t a[4] = {ad.x, ad.y, ad.z, ad.w};

	t.n = gcl_txq_range(p.qoff[c], p.qoff[c + 1], p.nent, &t.e0, &t.bad);
	gcl_txq_cx_fill(&t.x, c, c0.x, c1.y, c1.z, a, p.want ? p.want[c] : 0); /* snd_una; rcv_nxt, rcv_wnd: words 5, 6 */
	return t;
}

__device__ __forceinline__ TxqConn txq_bcast(const TxqConn &t, uint32_t src)
{
	TxqConn b;
	b.x.c = __shfl(t.x.c, src);
	b.x.snd_una = __shfl(t.x.snd_una, src);
	b.x.ack = __shfl(t.x.ack, src);
	b.x.win = __shfl(t.x.win, src);
	b.x.a[0] = __shfl(t.x.a[0], src);
	b.x.a[1] = __shfl(t.x.a[1], src);
	b.x.a[2] = __shfl(t.x.a[2], src);
	b.x.want = __shfl(t.x.want, src);
	b.e0 = __shfl(t.e0, src);
	b.n = __shfl(t.n, src);
	b.bad = __shfl(t.bad, src);
	return b;
}

__device__ __forceinline__ void txq_store_conn(const TxqParams &p, uint32_t c, const struct gcl_txq_res &r, uint32_t bad,
                                               uint64_t first)
{
	uint4 *o = (uint4 *)&p.out.out_conn[c];

	o[0] = make_uint4((uint32_t)r.head_ts, (uint32_t)(r.head_ts >> 32), r.nacked, r.nretx);
	o[1] = make_uint4((uint32_t)first, (r.flags | bad) & 0xFFu, 0, 0);
}

/*
 * gcl_txq_conn by the whole wave: every argument is wave-uniform, every lane
 * is active, and *@r comes out the same in every lane.  Lane l looks at entry
 * base + l of each 64-entry step.
 */
__device__ void txq_wave(const TxqParams &p, const struct gcl_txq_call &kc, const TxqConn &t, uint64_t first,
                         uint64_t room, int emit, struct gcl_txq_res *r)
{
	const uint32_t lane = threadIdx.x & 63, una = t.x.snd_una, n = t.n;
	const uint64_t below = (1ull << lane) - 1;
	uint8_t *state = p.out.state;
	bool walking = (t.x.want & GCL_TXQ_W_RTO) != 0, popping = true;
	const bool fast = (t.x.want & GCL_TXQ_W_FAST) != 0;
	uint32_t head_st = GCL_TXQS_KEPT;
	uint64_t head_ts0 = 0;

	gcl_txq_res_zero(r);
	if (t.x.want & GCL_TXQ_W_EXCL) {
		for (uint32_t base = 0; base < n; base += 64)
			if (base + lane < n)
				state[t.e0 + base + lane] = GCL_TXQS_KEPT;
		r->flags = GCL_TXQO_DEFERRED;
		gcl_txq_finish(r, n, GCL_TXQS_KEPT, n ? txq_ent(p.ent[t.e0]).ts : 0, kc.now);
		return;
	}
	for (uint32_t base = 0; base < n; base += 64) { /* uniform: every lane reaches the ballots */
		const uint32_t i = base + lane, e = t.e0 + i;
		const bool in = i < n;
		uint32_t st = GCL_TXQS_KEPT, head_lane = 64;

		if (walking || popping) {
			struct gcl_txq_ent h = {0, 0, 0};
			if (in)
				h = txq_ent(p.ent[e]);
			if (walking) {
				const uint32_t due = in ? gcl_txq_due(&h, una, kc.now) : 1;
				const uint64_t ym = __ballot(due == 0);
				const uint64_t reach = ym ? (ym & (0 - ym)) - 1 : ~0ull; /* the lanes before the first young entry */
				const bool wanted = due == 2 && ((reach >> lane) & 1);
				struct gcl_txq_cold q = {};
				struct gcl_txq_pick pk = {0, 0, 0, 0, 0};
				bool ok = false;

				if (wanted) {
					q = txq_cold(p.cold[e]);
					ok = gcl_txq_one(&h, &q, una, 0, kc.frame_stride, &pk) != 0;
				}
				const uint64_t cm = __ballot(ok);
				const uint64_t pos = (uint64_t)r->nretx + (uint32_t)__popcll(cm & below); /* the count as the walk gets here */
				const uint64_t nsm = __ballot(ok && pos >= room);
				const uint64_t bm = __ballot(ok && pos + 1 >= GCL_TXQ_BATCH);
				const uint32_t ns_l = nsm ? (uint32_t)__builtin_ctzll(nsm) : 64;
				const uint32_t b_l = bm ? (uint32_t)__builtin_ctzll(bm) : 64;
				const bool ns_stop = ns_l < 64 && ns_l <= b_l; /* the same entry: the room is asked first */
				const uint32_t stop = ns_l < b_l ? ns_l : b_l;  /* the walk's last entry of this step, or 64 */
				const bool mine = wanted && lane <= stop;
				const bool sent = mine && ok && !(ns_stop && lane == stop);

				if (mine) {
					if (!ok)
						st = GCL_TXQS_REFUSED;
					else if (!sent)
						st = GCL_TXQS_NOSPACE;
					else {
						st = (pk.copy ? GCL_TXQS_RETX_COPY : GCL_TXQS_RETX) | (pk.trim ? GCL_TXQS_TRIMMED : 0u);
						if (emit)
							gcl_txq_store(&kc, first + pos, &t.x, e, &q, &pk);
					}
				}
				const uint64_t cpm = __ballot(sent && pk.copy);
				r->nretx += (uint32_t)__popcll(__ballot(sent));
				r->refused += (uint32_t)__popcll(__ballot(mine && !ok));
				r->copied += (uint32_t)__popcll(cpm);
				r->trimmed += (uint32_t)__popcll(__ballot(sent && pk.trim));
				if (cpm)
					r->bytes += txq_wave_sum(sent ? pk.len : 0);
				if (ns_stop) {
					r->flags |= GCL_TXQO_NOSPACE;
					walking = false;
				} else if (stop < 64) {
					r->flags |= GCL_TXQO_BATCH;
					walking = false;
				} else if (ym) {
					walking = false;
				}
			}
			if (popping) {
				const uint64_t um = __ballot(in && gcl_txq_wraps_gt(h.seg_end, una));
				const uint32_t left = n - base < 64 ? n - base : 64;
				const uint32_t k = um ? (uint32_t)__builtin_ctzll(um) : left;

				if (lane < k && in)
					st = GCL_TXQS_ACKED;
				r->nacked += k;
				if (um) {
					popping = false;
					head_lane = k;
					head_st = __shfl(st, k);
					head_ts0 = txq_shfl64(h.ts, k);
				}
			}
		}
		/* with W_FAST the head's state is stored once, below */
		if (in && !(fast && lane == head_lane))
			state[e] = (uint8_t)st;
	}
	if (fast && r->nacked < n) {
		const uint32_t e = t.e0 + r->nacked;
		const struct gcl_txq_ent h = txq_ent(p.ent[e]);
		const struct gcl_txq_cold q = txq_cold(p.cold[e]);

		head_st = gcl_txq_fast(&kc, &t.x, &h, &q, e, head_st, first, room, emit && lane == 0, r);
		if (lane == 0)
			state[e] = (uint8_t)head_st;
	}
	gcl_txq_finish(r, n, head_st, head_ts0, kc.now);
}

/* a connection's final result into the lane's counters */
__device__ __forceinline__ void txq_count(uint64_t cnt[GCL_TXQC_NR], const struct gcl_txq_res &r)
{
	cnt[GCL_TXQC_ACKED] += r.nacked;
	cnt[GCL_TXQC_RETX] += r.nretx;
	cnt[GCL_TXQC_COPIED] += r.copied;
	cnt[GCL_TXQC_TRIMMED] += r.trimmed;
	cnt[GCL_TXQC_REFUSED] += r.refused;
	cnt[GCL_TXQC_NOSPACE] += (r.flags & GCL_TXQO_NOSPACE) ? 1 : 0;
	cnt[GCL_TXQC_DEFERRED] += (r.flags & GCL_TXQO_DEFERRED) ? 1 : 0;
	cnt[GCL_TXQC_BYTES] += r.bytes;
}

/* the lanes' counters -> counts; totals[2] when @bytes */
__device__ __forceinline__ void txq_flush(const TxqParams &p, uint64_t cnt[GCL_TXQC_NR], bool bytes)
{
#pragma unroll
	for (uint32_t x = 0; x < GCL_TXQC_NR; x++) {
		const uint64_t s = txq_wave_sum(cnt[x]);
		if ((threadIdx.x & 63) == 0 && s) {
			if (p.counts)
				atomicAdd(p.counts + x, (unsigned long long)s);
			if (bytes && x == GCL_TXQC_BYTES)
				atomicAdd((unsigned long long *)p.out.totals + 2, (unsigned long long)s);
		}
	}
}

/*
 * One tile's connections through the rule: a lane's own short queue, then the
 * wave's long ones.  @live: the lane has a connection to walk; @first, @room:
 * the lane's.  The lane's result comes out in *@r (zero when !@live).
 */
__device__ __forceinline__ void txq_tile(const TxqParams &p, const struct gcl_txq_call &kc, const TxqConn &t, bool live,
                                         uint64_t first, uint64_t room, int emit, struct gcl_txq_res *r)
{
	const uint32_t lane = threadIdx.x & 63;
	const bool lng = live && t.n >= kTxqLong;

	gcl_txq_res_zero(r);
	if (live && !lng)
		gcl_txq_conn(&kc, &t.x, (const struct gcl_txq_ent *)p.ent, (const struct gcl_txq_cold *)p.cold, t.e0, t.n,
		             first, room, emit, r);
	for (uint64_t lm = __ballot(lng); lm; lm &= lm - 1) { /* uniform */
		const uint32_t src = (uint32_t)__builtin_ctzll(lm);
		const TxqConn b = txq_bcast(t, src);
		struct gcl_txq_res rb;

		txq_wave(p, kc, b, txq_shfl64(first, src), txq_shfl64(room, src), emit, &rb);
		if (lane == src)
			*r = rb;
	}
}

/* the wave's count -> the range's sum in bsum[blockIdx.x]; @wave_sum: summed over its tiles (wave-uniform) */
__device__ __forceinline__ void txq_store_sum(const TxqParams &p, uint32_t wave_sum)
{
	__shared__ uint32_t ws[kTxqWaves];

	if ((threadIdx.x & 63) == 0)
		ws[threadIdx.x >> 6] = wave_sum;
	__syncthreads();
	if (threadIdx.x == 0)
		p.bsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

/* a count is 0..17: the wave's sum, and the sum of the lanes below, from five ballots */
__device__ __forceinline__ uint32_t txq_count_scan(uint32_t v, uint64_t below, uint32_t *ex)
{
	uint32_t sum = 0, e = 0;
#pragma unroll
	for (uint32_t b = 0; b < 5; b++) {
		const uint64_t m = __ballot((v >> b) & 1u);
		sum += (uint32_t)__popcll(m) << b;
		e += (uint32_t)__popcll(m & below) << b;
	}
	*ex = e;
	return sum;
}

__global__ void __launch_bounds__(kTxqThreads) txq_decide_kernel(TxqParams p)
{
	const uint64_t lo = (uint64_t)blockIdx.x * p.per;
	const uint64_t hi = lo + p.per < p.nconn ? lo + p.per : p.nconn; /* lo >= nconn: an empty range */
	const struct gcl_txq_call kc = {&p.out, p.now, p.frame_base, p.frame_stride};
	uint64_t cnt[GCL_TXQC_NR] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t segs = 0; /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kTxqThreads) { /* uniform: every lane reaches the ballots */
		const uint64_t c = j0 + threadIdx.x;
		const bool live = c < hi;
		TxqConn t = {};
		struct gcl_txq_res r;
		uint32_t ex;

		if (live)
			t = txq_load(p, (uint32_t)c);
		txq_tile(p, kc, t, live, 0, GCL_TXQ_NOROOM, 0, &r);
		if (live) {
			txq_store_conn(p, (uint32_t)c, r, t.bad, 0);
			if (r.nretx == 0) /* final: emit does not walk it again */
				txq_count(cnt, r);
		}
		segs += txq_count_scan(r.nretx, 0, &ex);
	}
	txq_flush(p, cnt, false);
	txq_store_sum(p, segs);
}

/* bsum[0, blocks) -> its exclusive prefix sums; totals; one block.  A call's segments are <= 17 * 2^20. */
__global__ void __launch_bounds__(kTxqThreads) txq_top_kernel(TxqParams p)
{
	__shared__ uint32_t sc[2][kTxqThreads];
	const uint32_t t = threadIdx.x;
	uint32_t v[kTxqTopPer], sum = 0;

#pragma unroll
	for (uint32_t x = 0; x < kTxqTopPer; x++) {
		const uint32_t r = t * kTxqTopPer + x;
		v[x] = r < p.blocks ? p.bsum[r] : 0;
		sum += v[x];
	}
	/* inclusive scan of the lanes' sums, ping-pong: one barrier per step */
	uint32_t cur = 0;
	sc[0][t] = sum;
	__syncthreads();
	for (uint32_t step = 1; step < kTxqThreads; step <<= 1) {
		const uint32_t a = t >= step ? sc[cur][t - step] + sc[cur][t] : sc[cur][t];
		sc[cur ^ 1][t] = a;
		cur ^= 1;
		__syncthreads();
	}
	uint32_t base = t ? sc[cur][t - 1] : 0;
#pragma unroll
	for (uint32_t x = 0; x < kTxqTopPer; x++) {
		const uint32_t r = t * kTxqTopPer + x;
		if (r < p.blocks)
			p.bsum[r] = base;
		base += v[x];
	}
	if (t == kTxqThreads - 1) {
		const uint64_t wanted = base;
		p.out.totals[0] = wanted;
		p.out.totals[1] = wanted < p.seg_cap ? wanted : p.seg_cap;
		p.out.totals[2] = 0; /* emit adds the bytes */
	}
}

__global__ void __launch_bounds__(kTxqThreads) txq_emit_kernel(TxqParams p)
{
	__shared__ uint32_t wt[2][kTxqWaves];
	const uint64_t lo = (uint64_t)blockIdx.x * p.per;
	const uint64_t hi = lo + p.per < p.nconn ? lo + p.per : p.nconn;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t below = (1ull << lane) - 1;
	const struct gcl_txq_call kc = {&p.out, p.now, p.frame_base, p.frame_stride};
	uint64_t carry = lo < hi ? p.bsum[blockIdx.x] : 0; /* the range's base, then the tiles before */
	uint64_t cnt[GCL_TXQC_NR] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t par = 0;

	for (uint64_t j0 = lo; j0 < hi; j0 += kTxqThreads, par ^= 1) { /* uniform: every lane active */
		const uint64_t c = j0 + threadIdx.x;
		const bool live = c < hi;
		const uint32_t want = live ? p.out.out_conn[c].nretx : 0; /* decide's count */
		uint32_t ex;
		const uint32_t wsum = txq_count_scan(want, below, &ex);

		if (lane == 0)
			wt[par][wave] = wsum;
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

		const uint64_t first = at < p.seg_cap ? at : p.seg_cap;
		const bool again = live && want != 0;
		TxqConn t = {};
		struct gcl_txq_res r;

		if (again)
			t = txq_load(p, (uint32_t)c);
		txq_tile(p, kc, t, again, first, p.seg_cap - first, 1, &r);
		if (again) {
			txq_store_conn(p, (uint32_t)c, r, t.bad, first);
			txq_count(cnt, r);
		} else if (live) {
			p.out.out_conn[c].first = (uint32_t)first;
		}
	}
	txq_flush(p, cnt, true);
}

static bool txq_misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

static size_t txq_workspace(uint32_t blocks)
{
	return ((size_t)4 * (blocks ? blocks : GCL_TXQ_MAX_BLOCKS) + 15) & ~(size_t)15;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tcp_txq_workspace(uint32_t nconn, uint32_t blocks, size_t *bytes)
{
	if (!bytes || nconn > GCL_TXQ_MAX_CONN || blocks > GCL_TXQ_MAX_BLOCKS)
		return -EINVAL;
	*bytes = txq_workspace(blocks);
	return 0;
}

extern "C" int gcl_tcp_txq(struct gcl_ctx *c, const struct gcl_txq_in *in, const struct gcl_txq_out *out,
                           uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !in || !out || in->size != sizeof(*in) || in->nconn > GCL_TXQ_MAX_CONN ||
	    in->blocks > GCL_TXQ_MAX_BLOCKS || in->nent > (1ull << 31) || in->seg_cap > (1ull << 31) ||
	    in->frame_stride < GCL_CTL_MIN_STRIDE || !out->totals)
		return -EINVAL;
	if (in->nconn && (!in->qoff || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if (in->nent && (!in->ent || !in->cold || !out->state))
		return -EINVAL;
	if (in->nconn && in->seg_cap && (!out->desc || !out->frame_off || !out->src_off || !out->len || !out->dst_off ||
	                                 !out->seg_conn || !out->seg_ent))
		return -EINVAL;
	if (txq_misaligned(in->qoff, 4) || txq_misaligned(in->ent, 16) || txq_misaligned(in->cold, 16) ||
	    txq_misaligned(in->conn, 16) || txq_misaligned(in->addr, 16) || txq_misaligned(out->out_conn, 16) ||
	    txq_misaligned(out->desc, 16) || txq_misaligned(out->frame_off, 8) || txq_misaligned(out->src_off, 8) ||
	    txq_misaligned(out->len, 2) || txq_misaligned(out->dst_off, 8) || txq_misaligned(out->seg_conn, 4) ||
	    txq_misaligned(out->seg_ent, 4) || txq_misaligned(out->totals, 8) || txq_misaligned(counts, 8))
		return -EINVAL;
	if (!workspace || txq_misaligned(workspace, 16) || workspace_bytes < txq_workspace(in->blocks))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->nconn == 0)
		return hipMemsetAsync(out->totals, 0, 3 * sizeof(uint64_t), s) == hipSuccess ? 0 : -EIO;

	const uint64_t tiles = ((uint64_t)in->nconn + kTxqThreads - 1) / kTxqThreads;
	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);
	TxqParams p;

	p.out = *out;
	p.qoff = in->qoff;
	p.ent = (const uint4 *)in->ent;
	p.cold = (const uint4 *)in->cold;
	p.conn = (const uint4 *)in->conn;
	p.addr = (const uint4 *)in->addr;
	p.want = in->want;
	p.counts = (unsigned long long *)counts;
	p.bsum = (uint32_t *)workspace;
	p.nent = in->nent;
	p.seg_cap = in->seg_cap;
	p.frame_base = in->frame_base;
	p.now = in->now;
	p.nconn = in->nconn;
	p.frame_stride = in->frame_stride;
	p.blocks = in->blocks ? in->blocks :
	           (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::min<uint32_t>(cus * kTxqBlocksPerCu,
	                                                                                      GCL_TXQ_MAX_BLOCKS)));
	/* whole tiles per range, so that every range starts at a multiple of 256 */
	p.per = std::max<uint64_t>(1, (tiles + p.blocks - 1) / p.blocks) * kTxqThreads;

	hipLaunchKernelGGL(txq_decide_kernel, dim3(p.blocks), dim3(kTxqThreads), 0, s, p);
	hipLaunchKernelGGL(txq_top_kernel, dim3(1), dim3(kTxqThreads), 0, s, p);
	hipLaunchKernelGGL(txq_emit_kernel, dim3(p.blocks), dim3(kTxqThreads), 0, s, p);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
