/*
 * gcl_tcprx.hip - tcp_rx_conn's established fast path for one runtime's list
 * of packets (gcl_tcp_rx, gclassify.h; runtime/net/tcp_in.c:197-296): every
 * connection's segments, in arrival order, through the rule of gcl_tcprx.h,
 * the same inline code the host twin runs, and the layout that puts the bytes
 * a connection accepted in one piece.
 *
 * Launches on the stream, ordered by the stream alone: no block waits for
 * another, there is no look-back, flag or cooperative launch, and the only
 * atomics are counter additions whose order changes nothing.
 *
 *   parse    one lane per list entry: order[j], the per-packet arrays, the
 *            frame's bytes [12, 52) with gcl_payload.hip's loads (the 16-B
 *            chunks of an aligned 64-B window, else byte by byte), then
 *            gcl_pay_rule.  An entry that is NA, NOCONN or DROP gets its final
 *            outputs here and the cookie GCL_TCPRX_NONE in the workspace; a
 *            segment that takes part gets its cookie and one 16-B record
 *            (seq, ack, win | flags << 16, len).
 *   group    a stable LSD counting sort of the list positions that take part
 *            by cookie, 11 bits a pass: one pass for nconn <= 2048, two up to
 *            2^20.  As in gcl_plan.hip a pass is count (a wave per contiguous
 *            range, its counters in LDS), three scan launches over
 *            hist[digit][range], and scatter: a wave re-reads its range in
 *            order, a lane's rank among the equal keys of its 64 entries is a
 *            ballot population count, and the wave's leader lanes move its
 *            counters on.  No atomic hands out a position, so arrival order
 *            inside a connection is exact.  The first pass skips the entries
 *            that do not take part, so the second runs over T <= m positions.
 *   runs     one lane per sorted position: a position whose neighbour has
 *            another cookie stores its connection's run start or end (one
 *            writer each; the array is cleared by a memset on the stream).
 *   walk     one wave per connection.  It gathers up to 64 records of the run
 *            at once, evaluates the terms nothing moves in parallel, forms the
 *            expected seq and the remaining window by a wave prefix sum of len
 *            and finds the first lane that breaks the chain; only the send
 *            window words and the delayed-ACK counter are carried serially,
 *            wave-uniform, across that FAST prefix, with the segment's words
 *            read out of their lane.  Longer runs loop in chunks of 64.  It
 *            writes the per-entry outputs (dst_off relative to the run), the
 *            connection's out_conn and its WAKE count; a connection without a
 *            run writes its input back.
 *   layout   three scan launches over pad(fast_bytes) write conn_off, one
 *            launch adds conn_off[c] to the FAST entries' dst_off, and one
 *            (only with counts) sums the connections' counters: an add per
 *            counter per block.
 *
 * The four calls (gcl_tcp_rx, _full, _ooo, _states) go through one driver,
 * rx_run.  Shared by all: parse, group, runs and the layout scan.  A call's
 * own:
 *   walk     gcl_tcp_rx: rx_walk_kernel.  _full: rxf_walk_kernel, serial over
 *            the chunk (gcl_tcprxf.h).  _ooo and _states: the two
 *            instantiations of rxq_walk_kernel, which lists what differs
 *            between them; then a scan of the final queue lengths.
 *   fix-up   rx_fix_kernel keyed on the verdict for gcl_tcp_rx, on copy_len
 *            for the other three.
 *   queues   _ooo and _states: rxo_qout_kernel.
 *   counters rx_counts_kernel over 5, 10 or 16 counters (_ooo and _states
 *            share the 16; _states' four more are added by its walk).
 * The walks share the connection load, the run bounds, the chunk gather and
 * the per-connection stores; the three serial walks also the chunk's end.
 *
 * Bounds.  A list index is used only below m, a packet index only below n, a
 * cookie only below nconn (parse leaves no other in the workspace, and every
 * later use clamps again); sorted positions are stored only below m; the
 * frame is read as in gcl_payload.hip: an aligned window only when it lies
 * inside frames[0, frames_len), else every byte's index is tested.  Nothing is
 * written outside the m-element outputs, out_conn[0, nconn), conn_off[0,
 * nconn], counts and the workspace.  No inline assembly beyond compiler
 * barriers.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_pay.h"
#include "gcl_tcprx.h"
#include "gcl_tcprxf.h"
#include "gcl_tcprxo.h"
#include "gcl_tcprxs.h"

namespace gclk {

constexpr uint32_t kRxThreads = 256;
constexpr uint32_t kRxWaves = kRxThreads / 64;
constexpr uint32_t kRxDigitBits = 11;
constexpr uint32_t kRxDigits = 1u << kRxDigitBits; /* counters of one wave */
constexpr uint32_t kRxChunk = 2048;                /* entries per scan block */
constexpr uint32_t kRxTopThreads = 1024;
constexpr uint32_t kRxBlocksPerCu = 4;

struct RxParams {
	const uint8_t *frames;
	uint64_t frames_len;
	uint64_t stride;
	const uint64_t *offs;
	const uint16_t *pkt_len;
	uint64_t n;
	const uint32_t *order;
	const uint32_t *sock;
	const uint8_t *l4_status;
	const uint4 *conn;      /* struct gcl_tcp_conn as three 16-B words */
	uint8_t *verdict, *sflags;
	uint32_t *after;
	uint16_t *copy_len;
	uint64_t *dst_off;
	uint4 *out_conn;        /* struct gcl_tcp_conn_out as three 16-B words */
	unsigned long long *conn_off;
	unsigned long long *counts;
	/* the workspace */
	uint4 *rec;             /* [m] */
	uint32_t *cookie;       /* [m] */
	uint32_t *idx[2];       /* [m] each: the sorted list positions of pass 0 and 1 */
	uint32_t *hist;         /* [digits][ranges] */
	uint32_t *csum;         /* [scan blocks] */
	unsigned long long *lsum; /* [layout scan blocks] */
	uint32_t *tot;          /* the number of entries that take part */
	uint2 *run;             /* [nconn]: a connection's sorted positions [x, y) */
	uint32_t *wakes;        /* [nconn] */
	uint64_t m;             /* <= 2^31 */
	uint32_t nconn;
	uint32_t ranges, range_len; /* range_len: a multiple of 64 */
	uint32_t amask;
};

/* ---- the exclusive scan of io.load(0 .. total), kRxChunk entries per block ---- */

template <typename T, int NT>
__device__ __forceinline__ T rx_block_scan(T x, T *total)
{
	__shared__ T sh[NT];
	const uint32_t t = threadIdx.x;
	T acc = x;

	sh[t] = acc;
	__syncthreads();
	for (uint32_t d = 1; d < NT; d <<= 1) {
		const T y = t >= d ? sh[t - d] : 0;
		__syncthreads();
		acc += y;
		sh[t] = acc;
		__syncthreads();
	}
	if (total)
		*total = sh[NT - 1];
	return acc - x;
}

/* hist in place; the grand total to *tot */
struct RxHistIo {
	typedef uint32_t T;
	uint32_t *h, *tot;
	__device__ T load(uint32_t i) const { return h[i]; }
	__device__ void store(uint32_t i, T v) const { h[i] = v; }
	__device__ void store_total(T v) const { *tot = v; }
};

/* pad(fast_bytes) of the connections -> conn_off[0, nconn], the total last */
struct RxConnIo {
	typedef unsigned long long T;
	const uint4 *conn, *out_conn;
	unsigned long long *conn_off;
	uint32_t nconn, amask;
	__device__ T load(uint32_t c) const
	{
		/* rcv_nxt: word 5 of gcl_tcp_conn, word 4 of gcl_tcp_conn_out */
		return gcl_tcprx_pad(out_conn[3 * (size_t)c + 1].x - conn[3 * (size_t)c + 1].y, amask);
	}
	__device__ void store(uint32_t c, T v) const { conn_off[c] = v; }
	__device__ void store_total(T v) const { conn_off[nconn] = v; }
};

template <typename Io>
__global__ void __launch_bounds__(kRxThreads) rx_scan_sum_kernel(Io io, uint32_t total, typename Io::T *csum)
{
	typedef typename Io::T T;
	const uint32_t i0 = blockIdx.x * kRxChunk + threadIdx.x * 8;
	T s = 0, tot;

	for (uint32_t j = 0; j < 8; j++)
		s += i0 + j < total ? io.load(i0 + j) : 0;
	(void)rx_block_scan<T, kRxThreads>(s, &tot);
	if (threadIdx.x == 0)
		csum[blockIdx.x] = tot;
}

/* one block: csum[0, nchunks) -> its exclusive scan, and the grand total */
template <typename Io>
__global__ void __launch_bounds__(kRxTopThreads) rx_scan_top_kernel(Io io, typename Io::T *csum, uint32_t nchunks)
{
	typedef typename Io::T T;
	const uint32_t per = (nchunks + kRxTopThreads - 1) / kRxTopThreads;
	const uint32_t i0 = threadIdx.x * per;
	T s = 0;

	for (uint32_t j = 0; j < per; j++)
		s += i0 + j < nchunks ? csum[i0 + j] : 0;
	T acc = rx_block_scan<T, kRxTopThreads>(s, nullptr);
	for (uint32_t j = 0; j < per; j++) {
		if (i0 + j < nchunks) {
			const T x = csum[i0 + j];
			csum[i0 + j] = acc;
			acc += x;
		}
	}
	if (threadIdx.x == kRxTopThreads - 1)
		io.store_total(acc);
}

template <typename Io>
__global__ void __launch_bounds__(kRxThreads) rx_scan_apply_kernel(Io io, uint32_t total, const typename Io::T *csum)
{
	typedef typename Io::T T;
	const uint32_t i0 = blockIdx.x * kRxChunk + threadIdx.x * 8;
	T x[8], s = 0;

	for (uint32_t j = 0; j < 8; j++) {
		x[j] = i0 + j < total ? io.load(i0 + j) : 0;
		s += x[j];
	}
	T acc = csum[blockIdx.x] + rx_block_scan<T, kRxThreads>(s, nullptr);
	for (uint32_t j = 0; j < 8; j++) {
		if (i0 + j < total) {
			io.store(i0 + j, acc);
			acc += x[j];
		}
	}
}

/* ---- parse ---- */

/* frame dwords 3..12 out of the window's sixteen, the frame starting 4 L bytes in */
template <int L>
__device__ __forceinline__ void rx_pick(const uint4 (&w)[4], uint32_t d[10])
{
	const uint32_t W[16] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w,
	                        w[2].x, w[2].y, w[2].z, w[2].w, w[3].x, w[3].y, w[3].z, w[3].w};
#pragma unroll
	for (int i = 0; i < 10; i++)
		d[i] = W[3 + i + L];
}

__global__ void __launch_bounds__(kRxThreads) rx_parse_kernel(RxParams k)
{
	const uint32_t fbase = (uint32_t)(uintptr_t)k.frames;
	uint32_t cnt[3] = {0, 0, 0}; /* DROP, NOCONN, NA: wave-uniform */

	for (uint64_t j0 = (uint64_t)blockIdx.x * kRxThreads; j0 < k.m; j0 += (uint64_t)gridDim.x * kRxThreads) {
		const uint64_t j = j0 + threadIdx.x;
		uint32_t verdict = GCL_TCPRX_FAST; /* here: takes part, or no entry */
		if (j < k.m) {
			const uint64_t i = k.order ? k.order[j] : j;
			uint32_t ck = GCL_TCPRX_NONE;
			struct gcl_tcprx_seg s = {0, 0, 0, 0, 0};
			if (i < k.n) {
				const uint32_t st = k.l4_status ? k.l4_status[i] : 0;
				const uint32_t sk = k.sock[i];
				const uint64_t off = k.offs ? k.offs[i] : i * k.stride;
				const uint64_t o = off < k.frames_len ? off : k.frames_len;
				const uint64_t avail = k.frames_len - o;
				const uint64_t L = k.pkt_len[i] < avail ? k.pkt_len[i] : avail;
				const uint32_t lead = (fbase + (uint32_t)o) & 15;
				const bool al = (lead & 3) == 0 && o >= lead && k.frames_len >= 64 &&
				                o - lead <= k.frames_len - 64;
				uint32_t d[10];
				if (al) {
					/* window dword x is frame dword x - lead / 4; wanted are 3..12 */
					const uint4 *w = (const uint4 *)(k.frames + (o - lead));
					uint4 c[4];
					c[0] = make_uint4(0, 0, 0, 0);
					if (lead == 0)
						c[0] = w[0];
					c[1] = w[1];
					c[2] = w[2];
					c[3] = w[3];
					if (lead == 0)
						rx_pick<0>(c, d);
					else if (lead == 4)
						rx_pick<1>(c, d);
					else if (lead == 8)
						rx_pick<2>(c, d);
					else
						rx_pick<3>(c, d);
				} else {
					const uint8_t *f = k.frames + o;
					for (uint32_t x = 0; x < 10; x++) {
						uint32_t v = 0;
						for (uint32_t y = 0; y < 4; y++) {
							const uint32_t at = 12 + 4 * x + y;
							v |= (at < avail ? (uint32_t)f[at] : 0u) << (8 * y);
						}
						d[x] = v;
					}
				}
				const struct gcl_pay_desc r = gcl_pay_rule(d, o, L, k.l4_status != nullptr, st, 1, sk);
				if (r.kind == GCL_PAY_TCP) {
					ck = sk;
					s = gcl_tcprx_parse(d, r.len);
				}
			}
			if (ck == GCL_TCPRX_NONE) {
				verdict = GCL_TCPRX_NA;
			} else if (ck >= k.nconn) {
				verdict = GCL_TCPRX_NOCONN;
			} else {
				const uint32_t mss = k.conn[3 * (size_t)ck + 1].w & 0xFFFFu; /* rcv_mss */
				if (s.len > mss)
					verdict = GCL_TCPRX_DROP;
			}
			if (verdict != GCL_TCPRX_FAST) {
				k.verdict[j] = (uint8_t)verdict;
				k.sflags[j] = 0;
				k.after[j] = 0;
				k.copy_len[j] = 0;
				k.dst_off[j] = 0;
				ck = GCL_TCPRX_NONE;
			} else {
				k.rec[j] = make_uint4(s.seq, s.ack, s.win | s.flags << 16, s.len);
			}
			k.cookie[j] = ck;
		}
		cnt[0] += (uint32_t)__popcll(__ballot(verdict == GCL_TCPRX_DROP));
		cnt[1] += (uint32_t)__popcll(__ballot(verdict == GCL_TCPRX_NOCONN));
		cnt[2] += (uint32_t)__popcll(__ballot(verdict == GCL_TCPRX_NA));
	}
	if (k.counts && (threadIdx.x & 63) == 0) {
		if (cnt[0])
			atomicAdd(k.counts + GCL_TCPRXC_DROP, (unsigned long long)cnt[0]);
		if (cnt[1])
			atomicAdd(k.counts + GCL_TCPRXC_NOCONN, (unsigned long long)cnt[1]);
		if (cnt[2])
			atomicAdd(k.counts + GCL_TCPRXC_NA, (unsigned long long)cnt[2]);
	}
}

/* ---- group ---- */

struct RxPass {
	const uint32_t *src; /* NULL: the list itself, entries that do not take part skipped */
	uint32_t *dst;
	uint32_t shift, nb, kbits;
};

/* the lanes of this wave that are @valid and hold this lane's @key */
__device__ __forceinline__ uint64_t rx_match(uint32_t key, bool valid, uint32_t kbits)
{
	uint64_t m = __ballot(valid);

	for (uint32_t b = 0; b < kbits; b++) {
		const bool bit = (key >> b) & 1u;
		const uint64_t bal = __ballot(bit);
		m &= bit ? bal : ~bal;
	}
	return m;
}

/* source position p of a pass: the list position it names and its digit */
__device__ __forceinline__ bool rx_key(const RxParams &k, const RxPass &ps, uint64_t p, uint64_t end,
                                       uint32_t *j, uint32_t *key)
{
	bool valid = p < end;
	uint32_t at = 0, ck = GCL_TCPRX_NONE;

	if (valid) {
		at = ps.src ? ps.src[p] : (uint32_t)p;
		valid = at < k.m;
	}
	if (valid) {
		ck = k.cookie[at];
		valid = ck < k.nconn;
	}
	const uint32_t dg = valid ? (ck >> ps.shift) & (kRxDigits - 1) : 0;
	*j = at;
	*key = dg < ps.nb ? dg : ps.nb - 1;
	return valid;
}

__device__ __forceinline__ uint64_t rx_limit(const RxParams &k, const RxPass &ps)
{
	const uint64_t t = ps.src ? *k.tot : k.m;
	return t < k.m ? t : k.m;
}

__global__ void __launch_bounds__(kRxThreads) rx_count_kernel(RxParams k, RxPass ps)
{
	__shared__ uint32_t lds[kRxWaves][kRxDigits];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kRxWaves + wave;

	if (r >= k.ranges)
		return; /* waves share nothing: no barrier below */
	uint32_t *cnt = lds[wave];
	for (uint32_t b = lane; b < ps.nb; b += 64)
		cnt[b] = 0;
	const uint64_t limit = rx_limit(k, ps);
	const uint64_t start = (uint64_t)r * k.range_len;
	const uint64_t end = start + k.range_len < limit ? start + k.range_len : limit;
	for (uint64_t base = start; base < end; base += 64) {
		uint32_t j, key;
		const bool valid = rx_key(k, ps, base + lane, end, &j, &key);
		const uint64_t mt = rx_match(key, valid, ps.kbits);
		/* one add per distinct key of the step, by its lowest lane */
		if (valid && !(mt & ((1ull << lane) - 1)))
			atomicAdd(&cnt[key], (uint32_t)__popcll(mt));
	}
	asm volatile("" ::: "memory");
	/* every entry of this range's column is written: no zeroing of the workspace */
	for (uint32_t b = lane; b < ps.nb; b += 64)
		k.hist[(size_t)b * k.ranges + r] = cnt[b];
}

__global__ void __launch_bounds__(kRxThreads) rx_scatter_kernel(RxParams k, RxPass ps)
{
	__shared__ uint32_t lds[kRxWaves][kRxDigits];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kRxWaves + wave;

	if (r >= k.ranges)
		return;
	/* read and moved on by different lanes from step to step: LDS serves one
	 * wave's accesses in issue order, and volatile keeps the compiler to it */
	volatile uint32_t *cnt = lds[wave];
	const uint64_t limit = rx_limit(k, ps);
	const uint64_t start = (uint64_t)r * k.range_len;
	const uint64_t end = start + k.range_len < limit ? start + k.range_len : limit;

	if (start >= end)
		return;
	for (uint32_t b = lane; b < ps.nb; b += 64)
		cnt[b] = k.hist[(size_t)b * k.ranges + r];
	for (uint64_t base = start; base < end; base += 64) {
		uint32_t j, key;
		const bool valid = rx_key(k, ps, base + lane, end, &j, &key);
		const uint64_t mt = rx_match(key, valid, ps.kbits);
		const uint32_t rank = (uint32_t)__popcll(mt & ((1ull << lane) - 1));
		const uint32_t at = cnt[key]; /* key < nb <= kRxDigits, whatever the bytes */
		if (valid) {
			const uint32_t pos = at + rank;
			if (pos < k.m)
				ps.dst[pos] = j;
			if (rank == 0)
				cnt[key] = at + (uint32_t)__popcll(mt);
		}
		asm volatile("" ::: "memory");
	}
}

/* ---- runs ---- */

__global__ void __launch_bounds__(kRxThreads) rx_runs_kernel(RxParams k, const uint32_t *sorted)
{
	const uint64_t t = *k.tot < k.m ? *k.tot : k.m;

	for (uint64_t p = (uint64_t)blockIdx.x * kRxThreads + threadIdx.x; p < t;
	     p += (uint64_t)gridDim.x * kRxThreads) {
		const uint32_t j = sorted[p], jp = p ? sorted[p - 1] : 0, jn = p + 1 < t ? sorted[p + 1] : 0;
		const uint32_t c = j < k.m ? k.cookie[j] : GCL_TCPRX_NONE;
		const uint32_t cp = p && jp < k.m ? k.cookie[jp] : GCL_TCPRX_NONE;
		const uint32_t cn = p + 1 < t && jn < k.m ? k.cookie[jn] : GCL_TCPRX_NONE;
		if (c < k.nconn) {
			if (c != cp)
				k.run[c].x = (uint32_t)p;
			if (c != cn)
				k.run[c].y = (uint32_t)p + 1;
		}
	}
}

/* ---- walk ---- */

__device__ __forceinline__ uint32_t rx_lane(uint32_t v, uint32_t l)
{
	return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}

/* the connection this wave walks: wave-uniform */
__device__ __forceinline__ uint32_t rx_wave_conn()
{
	return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * kRxWaves + (threadIdx.x >> 6)));
}

__device__ __forceinline__ struct gcl_tcp_conn rx_conn_load(const RxParams &k, uint32_t c)
{
	const uint4 a = k.conn[3 * (size_t)c], b = k.conn[3 * (size_t)c + 1], d = k.conn[3 * (size_t)c + 2];
	struct gcl_tcp_conn cn;

	cn.snd_una = a.x; cn.snd_nxt = a.y; cn.snd_wnd = a.z; cn.snd_wl1 = a.w;
	cn.snd_wl2 = b.x; cn.rcv_nxt = b.y; cn.rcv_wnd = b.z;
	cn.rcv_mss = (uint16_t)b.w; cn.snd_wscale = (uint8_t)(b.w >> 16); cn.flags = (uint8_t)(b.w >> 24);
	cn.acks_delayed_cnt = (uint8_t)d.x;
	return cn;
}

/* connection c's run of sorted positions [*rs, *re): both at most m whatever the workspace holds */
__device__ __forceinline__ void rx_run_bounds(const RxParams &k, uint32_t c, uint64_t *rs, uint64_t *re)
{
	const uint2 rn = k.run[c];

	*re = rn.y < k.m ? rn.y : k.m;
	*rs = rn.x < *re ? rn.x : *re;
}

/* up to 64 entries of a run from @base on, entry i in lane i: its list position (below m) and its record */
struct RxChunk {
	uint32_t nv, j;
	bool valid;
	uint4 rec;
};

__device__ __forceinline__ RxChunk rx_gather(const RxParams &k, const uint32_t *sorted, uint64_t base, uint64_t re,
                                             uint32_t lane)
{
	RxChunk ch;

	ch.nv = re - base < 64 ? (uint32_t)(re - base) : 64;
	ch.valid = lane < ch.nv;
	ch.j = ch.valid ? sorted[base + lane] : 0;
	if (ch.j >= k.m)
		ch.j = (uint32_t)(k.m - 1);
	ch.rec = ch.valid ? k.rec[ch.j] : make_uint4(0, 0, 0, 0);
	return ch;
}

/* struct gcl_tcp_conn_out of connection c; one lane calls it */
__device__ __forceinline__ void rx_conn_store(const RxParams &k, uint32_t c, const struct gcl_tcprx_live &l,
                                              uint32_t nfast, uint32_t nslow, uint32_t nacks, uint32_t first_slow)
{
	k.out_conn[3 * (size_t)c] = make_uint4(l.snd_una, l.snd_wnd, l.snd_wl1, l.snd_wl2);
	k.out_conn[3 * (size_t)c + 1] = make_uint4(l.rcv_nxt, l.rcv_wnd, nfast, nslow);
	k.out_conn[3 * (size_t)c + 2] = make_uint4(nacks, first_slow, (l.cnt & 0xFFu) | (l.flags & 0xFFu) << 8, 0);
}

__global__ void __launch_bounds__(kRxThreads) rx_walk_kernel(RxParams k, const uint32_t *sorted)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t c = rx_wave_conn();

	if (c >= k.nconn)
		return;
	const struct gcl_tcp_conn cn = rx_conn_load(k, c);
	struct gcl_tcprx_live l = gcl_tcprx_live_of(&cn);
	uint64_t rs, re;
	rx_run_bounds(k, c, &rs, &re);
	uint32_t nfast = 0, nslow = 0, nacks = 0, wakes = 0, first_slow = GCL_TCPRX_NONE;

	for (uint64_t base = rs; base < re; base += 64) { /* uniform */
		const RxChunk ch = rx_gather(k, sorted, base, re, lane);
		const uint32_t seq = ch.rec.x, ack = ch.rec.y, win = ch.rec.z & 0xFFFFu, flags = ch.rec.z >> 16, len = ch.rec.w;
		const bool stopped = (l.flags & GCL_TCPO_STOPPED) != 0;

		/* the sum of len over the lanes below: the chain's rcv_nxt and rcv_wnd at this lane */
		uint32_t incl = len;
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t u = (uint32_t)__shfl_up((int)incl, d);
			if (lane >= (uint32_t)d)
				incl += u;
		}
		const uint32_t excl = incl - len;
		const bool bad = !ch.valid || gcl_tcprx_slow_fixed(flags, len, ack, cn.snd_nxt, cn.flags) ||
		                 gcl_tcprx_slow_rcv(seq, len, l.rcv_nxt + excl, l.rcv_wnd - excl);
		const uint64_t badmask = __ballot(bad);
		uint32_t F = stopped ? 0 : badmask ? (uint32_t)__builtin_ctzll(badmask) : 64;

		uint32_t sf_mine = 0, after_mine = 0;
		for (uint32_t x = 0; x < F; x++) { /* uniform: the words that are carried serially */
			if (gcl_tcprx_snd_full(l.snd_una, l.snd_wnd, cn.snd_nxt)) {
				F = x;
				break;
			}
			uint32_t sf = gcl_tcprx_ack_step(&l, rx_lane(seq, x), rx_lane(ack, x),
			                                 rx_lane(win, x) << (cn.snd_wscale & 31));
			sf |= gcl_tcprx_rx_step(&l, rx_lane(len, x), rx_lane(flags, x));
			if (lane == x) {
				sf_mine = sf;
				after_mine = l.rcv_nxt;
			}
			nacks += (sf & GCL_TCPRX_SF_ACK_NOW) != 0;
			wakes += (sf & GCL_TCPRX_SF_WAKE) != 0;
		}
		nfast += F;
		nslow += ch.nv - F;
		if (F < ch.nv) {
			if (!stopped)
				first_slow = rx_lane(ch.j, F);
			l.flags |= GCL_TCPO_STOPPED;
		}
		if (ch.valid) {
			const bool fast = lane < F;
			k.verdict[ch.j] = (uint8_t)(fast ? GCL_TCPRX_FAST : GCL_TCPRX_SLOW);
			k.sflags[ch.j] = (uint8_t)sf_mine;
			k.after[ch.j] = after_mine;
			k.copy_len[ch.j] = (uint16_t)(fast ? len : 0);
			k.dst_off[ch.j] = fast ? (uint32_t)(seq - cn.rcv_nxt) : 0; /* layout adds conn_off[c] */
		}
	}
	if (lane == 0) {
		rx_conn_store(k, c, l, nfast, nslow, nacks, first_slow);
		k.wakes[c] = wakes;
	}
}

/* ---- layout ---- */

/*
 * The entries that have bytes to copy get their connection's offset.  Which
 * those are is the call's: gcl_tcp_rx keys on the verdict FAST, the three
 * later calls (@kByCopyLen) on copy_len != 0.  A FAST segment of length 0
 * tells them apart, so the key is no run-time choice.
 */
template <bool kByCopyLen>
__global__ void __launch_bounds__(kRxThreads) rx_fix_kernel(RxParams k)
{
	for (uint64_t j = (uint64_t)blockIdx.x * kRxThreads + threadIdx.x; j < k.m;
	     j += (uint64_t)gridDim.x * kRxThreads) {
		const uint32_t c = k.cookie[j];
		if (c < k.nconn && (kByCopyLen ? k.copy_len[j] != 0 : k.verdict[j] == GCL_TCPRX_FAST))
			k.dst_off[j] += k.conn_off[c];
	}
}

/* ---- gcl_tcp_rx_full: its walk, its layout fix and its counters ---- */

struct RxfParams {
	RxParams k;
	const uint8_t *rep_acks; /* [nconn] or NULL */
	uint4 *out_ext;          /* struct gcl_tcp_conn_ext as one 16-B word */
	uint4 *xcnt;             /* the workspace, [nconn]: TXWAKE, FASTRTX and rep_acks++ segments */
};

__device__ __forceinline__ uint32_t rx_pop(bool b)
{
	return (uint32_t)__popcll(__ballot(b));
}

/* the live words a serial walk carries for connection c */
__device__ __forceinline__ struct gcl_tcprxf_live rxf_live_of(const RxfParams &p, const struct gcl_tcp_conn &cn,
                                                              uint32_t c)
{
	struct gcl_tcprxf_live x;

	x.l = gcl_tcprx_live_of(&cn);
	x.rep_acks = p.rep_acks ? p.rep_acks[c] : 0;
	x.fast_rtx_ack = 0;
	x.xflags = 0;
	return x;
}

/* the segment of lane @at of a chunk: wave-uniform */
__device__ __forceinline__ struct gcl_tcprx_seg rx_seg_at(const uint4 &rec, uint32_t at)
{
	const uint32_t z = rx_lane(rec.z, at);
	const struct gcl_tcprx_seg s = {rx_lane(rec.x, at), rx_lane(rec.y, at), z & 0xFFFFu, rx_lane(rec.w, at), z >> 16};

	return s;
}

/* what a serial walk counts per connection; wave-uniform */
struct RxfTally {
	uint32_t nfast, nslow, first_slow;
	uint32_t nacks, wakes, nrule2, ndropped, ntxw, nfrtx, ndup;
};

/*
 * The end of a chunk of which the first H segments went through: the counts,
 * the stop, and the sflags' tallies as ballots (lanes at and past H hold 0).
 */
__device__ __forceinline__ void rxf_chunk_end(RxfTally &t, struct gcl_tcprx_live &l, const RxChunk &ch, uint32_t H,
                                              bool stopped, uint32_t sf_mine)
{
	t.nfast += H;
	t.nslow += ch.nv - H;
	if (H < ch.nv) {
		if (!stopped)
			t.first_slow = rx_lane(ch.j, H);
		l.flags |= GCL_TCPO_STOPPED;
	}
	if (H) {
		t.nacks += rx_pop(sf_mine & GCL_TCPRX_SF_ACK_NOW);
		t.wakes += rx_pop(sf_mine & GCL_TCPRX_SF_WAKE);
		t.nrule2 += rx_pop(sf_mine & GCL_TCPRX_SF_RULE2);
		t.ndropped += rx_pop(sf_mine & GCL_TCPRX_SF_DROPPED);
		t.ntxw += rx_pop(sf_mine & GCL_TCPRX_SF_TXWAKE);
		t.nfrtx += rx_pop(sf_mine & GCL_TCPRX_SF_FASTRTX);
		t.ndup += rx_pop(sf_mine & GCL_TCPRXF_EV_DUPACK);
	}
}

/* connection c's out_conn, out_ext, xcnt (its fourth word is the queue walk's OOO count) and WAKE count; one
 * lane calls it */
__device__ __forceinline__ void rxf_conn_store(const RxfParams &p, uint32_t c, const struct gcl_tcprxf_live &x,
                                               const RxfTally &t, uint32_t nooo)
{
	rx_conn_store(p.k, c, x.l, t.nfast, t.nslow, t.nacks, t.first_slow);
	p.out_ext[c] = make_uint4(t.nrule2, t.ndropped, x.fast_rtx_ack, (x.rep_acks & 0xFFu) | (x.xflags & 0xFFu) << 8);
	p.xcnt[c] = make_uint4(t.ntxw, t.nfrtx, t.ndup, nooo);
	p.k.wakes[c] = t.wakes;
}

/*
 * One wave per connection, as rx_walk_kernel.  An unaccepted segment does not
 * move rcv_nxt, so the stop is no prefix sum: the wave walks the chunk's
 * records serially, wave-uniform, each read out of its lane, through
 * gcl_tcprxf_one; a lane keeps what its own record got, and the counters are
 * ballots over the chunk afterwards.
 */
__global__ void __launch_bounds__(kRxThreads) rxf_walk_kernel(RxfParams p, const uint32_t *sorted)
{
	const RxParams &k = p.k;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t c = rx_wave_conn();

	if (c >= k.nconn)
		return;
	const struct gcl_tcp_conn cn = rx_conn_load(k, c);
	struct gcl_tcprxf_live x = rxf_live_of(p, cn, c);
	uint64_t rs, re;
	rx_run_bounds(k, c, &rs, &re);
	RxfTally t = {0, 0, GCL_TCPRX_NONE, 0, 0, 0, 0, 0, 0, 0};

	for (uint64_t base = rs; base < re; base += 64) { /* uniform */
		const RxChunk ch = rx_gather(k, sorted, base, re, lane);
		const bool stopped = (x.l.flags & GCL_TCPO_STOPPED) != 0;
		uint32_t H = 0, sf_mine = 0, after_mine = 0, copy_mine = 0;

		if (!stopped) {
			H = ch.nv;
			for (uint32_t at = 0; at < ch.nv; at++) { /* uniform */
				const struct gcl_tcprx_seg s = rx_seg_at(ch.rec, at);
				uint32_t sf, cp;
				if (gcl_tcprxf_one(&cn, &x, &s, &sf, &cp) != GCL_TCPRX_FAST) {
					H = at;
					break;
				}
				if (lane == at) {
					sf_mine = sf;
					after_mine = x.l.rcv_nxt;
					copy_mine = cp;
				}
			}
		}
		rxf_chunk_end(t, x.l, ch, H, stopped, sf_mine);
		if (ch.valid) {
			k.verdict[ch.j] = (uint8_t)(lane < H ? GCL_TCPRX_FAST : GCL_TCPRX_SLOW);
			k.sflags[ch.j] = (uint8_t)sf_mine;
			k.after[ch.j] = after_mine;
			k.copy_len[ch.j] = (uint16_t)copy_mine;
			k.dst_off[ch.j] = copy_mine ? (uint32_t)(ch.rec.x - cn.rcv_nxt) : 0; /* layout adds conn_off[c] */
		}
	}
	if (lane == 0)
		rxf_conn_store(p, c, x, t, 0);
}

/* ---- gcl_tcp_rx_ooo: its walk with the queue in the wave, the output queues and its counters ---- */

struct RxoParams {
	RxfParams f;
	const uint32_t *q_off;  /* [nconn + 1] or NULL */
	const uint4 *q;         /* struct gcl_tcp_ooo_ent as one 16-B word */
	uint32_t nq, q_out_cap;
	uint8_t *oflags;
	uint16_t *skip;
	uint8_t *qin_state;
	uint16_t *qin_skip, *qin_len;
	unsigned long long *qin_dst_off;
	uint32_t *qout_off;
	uint4 *qout;
	unsigned long long *totals;
	/* the workspace, behind gcl_tcp_rx_full's */
	uint4 *ocnt;            /* [nconn]: QUEUED, DRAINED, FREED, HEADCLIP (OOO is xcnt's fourth word) */
	uint4 *qmeta;           /* [nconn]: the final queue's length | staged << 8 | taken << 9, HELD, and the 64-bit
	                           mask of the final positions that hold a list entry */
	uint32_t *qsum;         /* [scan blocks over nconn] */
	uint4 *stage;           /* [nq + m]: the final queues of the connections that have a run: the entries
	                           carried over from q in [0, nq), this call's list entries in [nq, nq + m) */
};

/* the final queue lengths -> qout_off[0, nconn], the total also to totals[0] */
struct RxQoutIo {
	typedef uint32_t T;
	const uint4 *qmeta;
	uint32_t *qout_off;
	unsigned long long *totals;
	uint32_t nconn;
	__device__ T load(uint32_t c) const { return qmeta[c].x & 0xFFu; }
	__device__ void store(uint32_t c, T v) const { qout_off[c] = v; }
	__device__ void store_total(T v) const
	{
		qout_off[nconn] = v;
		totals[0] = v;
	}
};

/* connection c's input queue q[*qs, *qe): both below nq whatever q_off holds */
__device__ __forceinline__ void rxo_range(const RxoParams &p, uint32_t c, uint32_t *qs, uint32_t *qe)
{
	*qs = *qe = 0;
	if (p.q_off) {
		const uint32_t a = p.q_off[c], b = p.q_off[(size_t)c + 1];
		*qs = a < p.nq ? a : p.nq;
		*qe = b < p.nq ? b : p.nq;
		if (*qe < *qs)
			*qe = *qs;
	}
}

/* what gcl_tcp_rx_states adds to gcl_tcp_rx_ooo's walk; every other launch is gcl_tcp_rx_ooo's */
struct RxsParams {
	RxoParams o;
	const uint8_t *state;   /* [nconn] or NULL */
	uint8_t *ev;            /* [m] */
	uint32_t *rst_seq;      /* [m] */
	uint8_t *state_after;   /* [m] */
	uint8_t *state_out;     /* [nconn] */
};

__device__ __forceinline__ const RxoParams &rxo_base(const RxoParams &p) { return p; }
__device__ __forceinline__ const RxoParams &rxo_base(const RxsParams &p) { return p.o; }

/* a live queue entry, entry i in lane i: @fl is flags | src << 16, @idx the index into q or the list */
struct RxoEnt {
	uint32_t seq, end, fl, idx;
};

/* tcp_in.c:124-135 over the wave: the two tests as ballots, the entry nearest the tail their highest bit */
__device__ __forceinline__ uint32_t rxo_find(const RxoEnt &e, uint32_t qn, uint32_t lane, uint32_t seq, uint32_t end)
{
	const uint32_t t = lane < qn ? gcl_tcprxo_pos_test(seq, end, e.seq, e.end) : 0;
	const uint64_t ends = __ballot((t & GCL_TCPRXO_POS_END) != 0), seqs = __ballot((t & GCL_TCPRXO_POS_SEQ) != 0);

	return gcl_tcprxo_pos(ends, seqs);
}

/* the insert: the lanes at and above @pos move up by one (the caller has seen to qn < 64), lane @pos takes @n */
__device__ __forceinline__ void rxo_insert(RxoEnt &e, uint32_t lane, uint32_t pos, const RxoEnt &n)
{
	const RxoEnt u = {(uint32_t)__shfl_up((int)e.seq, 1), (uint32_t)__shfl_up((int)e.end, 1),
	                  (uint32_t)__shfl_up((int)e.fl, 1), (uint32_t)__shfl_up((int)e.idx, 1)};

	if (lane > pos)
		e = u;
	if (lane == pos)
		e = n;
}

/* the pop of the head: every lane takes the entry above it */
__device__ __forceinline__ void rxo_pop(RxoEnt &e)
{
	e.seq = (uint32_t)__shfl_down((int)e.seq, 1);
	e.end = (uint32_t)__shfl_down((int)e.end, 1);
	e.fl = (uint32_t)__shfl_down((int)e.fl, 1);
	e.idx = (uint32_t)__shfl_down((int)e.idx, 1);
}

/* what an entry that leaves the queue gets; one lane calls it, and nothing else stores these words */
__device__ __forceinline__ void rxo_fate(const RxoParams &p, uint32_t fl, uint32_t idx, uint32_t t, uint32_t head,
                                         uint32_t ln, uint32_t rel)
{
	const RxParams &k = p.f.k;

	if (fl >> 16) {
		k.copy_len[idx] = (uint16_t)ln;
		k.dst_off[idx] = ln ? rel : 0; /* layout adds conn_off[c] */
		p.oflags[idx] = (uint8_t)(GCL_OOOF_OOO | GCL_OOOF_QUEUED | (head ? GCL_OOOF_HEADCLIP : 0) |
		                          (t == GCL_TCPRXO_APPEND ? GCL_OOOF_LATE_DRAINED : GCL_OOOF_LATE_FREED));
		p.skip[idx] = (uint16_t)head;
	} else {
		p.qin_state[idx] = (uint8_t)(t == GCL_TCPRXO_APPEND ? GCL_OOOQ_DRAINED : GCL_OOOQ_FREED);
		p.qin_skip[idx] = gcl_tcprxo_u16(head);
		p.qin_len[idx] = gcl_tcprxo_u16(ln);
		p.qin_dst_off[idx] = ln ? rel : 0;
	}
}

/* a segment's locals that outlive the text step: the rule's own struct, and its gcl_tcprxo_mid part */
__device__ __forceinline__ struct gcl_tcprxo_mid &rxo_mid(struct gcl_tcprxo_mid &mid) { return mid; }
__device__ __forceinline__ struct gcl_tcprxo_mid &rxo_mid(struct gcl_tcprxs_mid &mid) { return mid.o; }

/*
 * The queue walk of gcl_tcp_rx_ooo (P = RxoParams, the rule of gcl_tcprxo.h)
 * and of gcl_tcp_rx_states (P = RxsParams, the rule of gcl_tcprxs.h, @S below).
 *
 * One wave per connection, serial and wave-uniform over each chunk as
 * rxf_walk_kernel, with the connection's out-of-order queue in the wave's
 * registers: entry i in lane i, @qn entries.  The insert position is two
 * ballots, an insert or a pop a one-lane shift, the drain reads lane 0.
 * Wave-uniform throughout: qn, st, dead, H, the counters and the live words.
 *
 * What differs between the two calls, all of it under `if constexpr (S)`:
 *   taking      _ooo takes a connection whose flags gcl_tcprxo_state_ok accepts
 *               and whose input queue fits; a ballot un-takes one whose input
 *               queue holds a FIN entry, and a taken one gets ELIGIBLE into
 *               cn.flags.  _states takes by gcl_tcprxs_state_ok of the live
 *               state @st (gcl_tcprxs_state_of, made uniform), FIN entries
 *               included, and leaves cn.flags alone.
 *   full queue  whether a segment's insert would be the 65th: _ooo asks
 *               gcl_tcprxo_reaches_ooo; _states runs gcl_tcprxs_head on copies
 *               of the live words and the state, so that a stop leaves them
 *               untouched, then gcl_tcprxo_in_order.  A known cost: while a
 *               queue holds 64 entries every segment runs that head twice.
 *   head        gcl_tcprxo_head may say STOP; gcl_tcprxs_head carries @st and
 *               never does, but after a FAIL or a PUT (@dead) the next
 *               segment stops.
 *   text        the end is seq + len, for _states seq + mid.slen (the FIN's
 *               octet); the in-order wake is each rule's own; _states' append
 *               takes the FIN bit, in order the segment's and in the drain the
 *               popped entry's (its flags word at lane 0), notes it in
 *               mid.fin, and gcl_tcprxs_fin follows gcl_tcprxo_text_tail.
 *   segment     _states only: dead, the four event counters, and ev, rst_seq
 *               and state_after of the entry.
 *   the end     _states only: state_out[c], and the four counters added to
 *               counts by lane 0: atomics that only add.
 *
 * Store order.  copy_len, dst_off, oflags and skip of a list entry that was
 * QUEUED are stored exactly once, when its fate is known: by rxo_fate when it
 * is popped (in this chunk or a later one) or at the end of the walk when it
 * is HELD; the chunk's own store skips such an entry.  The same holds for the
 * qin_* words of an input entry.  ev, rst_seq and state_after of an entry are
 * final when the entry has been processed and only the chunk's own store
 * writes them.  So no two stores of this kernel hit one address and no fence
 * is needed.
 */
template <typename P>
__global__ void __launch_bounds__(kRxThreads) rxq_walk_kernel(P ps, const uint32_t *sorted)
{
	constexpr bool S = std::is_same<P, RxsParams>::value;
	typedef typename std::conditional<S, struct gcl_tcprxs_mid, struct gcl_tcprxo_mid>::type Mid;
	const RxoParams &p = rxo_base(ps);
	const RxParams &k = p.f.k;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t c = rx_wave_conn();

	if (c >= k.nconn)
		return;
	/* rx_conn_load's unpack, in place: through the helper the _states instantiation, which spills
	 * SGPRs to VGPR lanes as it is, comes out with 36 B of scratch per lane that it never touches */
	struct gcl_tcp_conn cn;
	{
		const uint4 a = k.conn[3 * (size_t)c], b = k.conn[3 * (size_t)c + 1], d = k.conn[3 * (size_t)c + 2];
		cn.snd_una = a.x; cn.snd_nxt = a.y; cn.snd_wnd = a.z; cn.snd_wl1 = a.w;
		cn.snd_wl2 = b.x; cn.rcv_nxt = b.y; cn.rcv_wnd = b.z;
		cn.rcv_mss = (uint16_t)b.w; cn.snd_wscale = (uint8_t)(b.w >> 16); cn.flags = (uint8_t)(b.w >> 24);
		cn.acks_delayed_cnt = (uint8_t)d.x;
	}
	struct gcl_tcprxf_live x = rxf_live_of(p.f, cn, c);
	uint32_t st = 0;
	if constexpr (S)
		st = (uint32_t)__builtin_amdgcn_readfirstlane((int)gcl_tcprxs_state_of(ps.state, c, cn.flags));
	const uint32_t rcv0 = cn.rcv_nxt;
	uint32_t qs, qe;
	rxo_range(p, c, &qs, &qe);
	const uint32_t nin = qe - qs;
	bool taken = (S ? gcl_tcprxs_state_ok(st) : gcl_tcprxo_state_ok(cn.flags)) && nin <= GCL_TCPOOO_CAP;
	RxoEnt e = {0, 0, 0, 0};
	if (taken && lane < nin) {
		const uint4 w = p.q[qs + lane];
		e.seq = w.x;
		e.end = w.y;
		e.fl = w.w & 0xFFFFu;
		e.idx = qs + lane;
	}
	if constexpr (!S) {
		if (__ballot(taken && lane < nin && (e.fl & GCL_TCPRX_FIN)))
			taken = false;
		if (taken)
			cn.flags |= GCL_TCPC_ELIGIBLE;
	}
	uint32_t qn = taken ? nin : 0;
	if (!taken && nin)
		x.xflags |= GCL_TCPX_QSKIP;

	uint64_t rs, re;
	rx_run_bounds(k, c, &rs, &re);
	RxfTally t = {0, 0, GCL_TCPRX_NONE, 0, 0, 0, 0, 0, 0, 0};
	uint32_t nooo = 0, nqueued = 0, ndrained = 0, nfreed = 0, nhead = 0;
	uint32_t nrst = 0, nfail = 0, nfin = 0, nstate = 0;
	bool dead = false; /* _states: a FAIL or a PUT went by: the next segment stops */

	for (uint64_t base = rs; base < re; base += 64) { /* uniform */
		const RxChunk ch = rx_gather(k, sorted, base, re, lane);
		const bool stopped = (x.l.flags & GCL_TCPO_STOPPED) != 0;
		uint32_t H = 0, sf_mine = 0, after_mine = 0, copy_mine = 0, head_mine = 0, of_mine = 0, rel_mine = 0;
		uint32_t ev_mine = 0, rseq_mine = 0, st_mine = 0;

		if (!stopped && taken) {
			H = ch.nv;
			for (uint32_t at = 0; at < ch.nv; at++) { /* uniform */
				const struct gcl_tcprx_seg s = rx_seg_at(ch.rec, at);
				const uint32_t jj = rx_lane(ch.j, at);
				const uint32_t rel = x.l.rcv_nxt - rcv0; /* where an in-order piece lands */
				Mid mid;
				uint32_t sf = 0, len = 0, head = 0, of = 0;
				bool stop = S && dead;

				if constexpr (S) {
					mid.ev = 0;
					mid.rst_seq = 0;
					if (!stop && qn == GCL_TCPOOO_CAP) { /* asked on copies: nothing moves */
						struct gcl_tcprxf_live xt = x;
						uint32_t stt = st, lt;

						if (gcl_tcprxs_head(&cn, &xt, &stt, &s, qn, &mid, &lt) == GCL_TCPRXO_TEXT &&
						    !gcl_tcprxo_in_order(&xt.l, s.seq))
							stop = rxo_find(e, qn, lane, s.seq, s.seq + mid.slen) != GCL_TCPRXO_REJECT;
					}
				} else {
					if (qn == GCL_TCPOOO_CAP && gcl_tcprxo_reaches_ooo(&cn, &x.l, &s))
						stop = rxo_find(e, qn, lane, s.seq, s.seq + s.len) != GCL_TCPRXO_REJECT;
				}
				if (!stop) {
					uint32_t t0;

					if constexpr (S)
						t0 = gcl_tcprxs_head(&cn, &x, &st, &s, qn, &mid, &len);
					else
						t0 = gcl_tcprxo_head(&cn, &x, &s, qn, &mid, &len);
					if (!S && t0 == GCL_TCPRXO_STOP) {
						stop = true;
					} else if (t0 == GCL_TCPRXO_FASTED) {
						sf = rxo_mid(mid).sf;
					} else {
						if (t0 == GCL_TCPRXO_TEXT) {
							uint32_t end = s.seq + s.len;
							int used = 1, wake = 0;

							if constexpr (S)
								end = s.seq + mid.slen;
							if (gcl_tcprxo_in_order(&x.l, s.seq)) {
								if constexpr (S) {
									wake = gcl_tcprxs_in_order_wake(&x.l, s.flags);
									if (wake && (s.flags & GCL_TCPRX_FIN))
										mid.fin = 1;
									gcl_tcprxs_append(&x.l, s.seq, end, (s.flags & GCL_TCPRX_FIN) != 0, &head, &len);
								} else {
									wake = gcl_tcprxo_in_order_wake(&x.l, s.flags);
									gcl_tcprxo_append(&x.l, s.seq, end, &head, &len);
								}
								if (head) {
									of |= GCL_OOOF_HEADCLIP;
									nhead++;
								}
							} else {
								const uint32_t pos = rxo_find(e, qn, lane, s.seq, end);

								of |= GCL_OOOF_OOO;
								nooo++;
								if (pos == GCL_TCPRXO_REJECT) {
									used = 0;
								} else {
									const RxoEnt n = {s.seq, end, s.flags | 1u << 16, jj};

									rxo_insert(e, lane, pos, n);
									qn++;
									of |= GCL_OOOF_QUEUED;
									nqueued++;
								}
							}
							while (used && qn) { /* uniform: the drain reads lane 0 */
								const uint32_t hs = rx_lane(e.seq, 0), he = rx_lane(e.end, 0);
								const uint32_t hf = rx_lane(e.fl, 0), hi = rx_lane(e.idx, 0);
								const uint32_t dt = gcl_tcprxo_drain_test(hs, he, x.l.rcv_nxt);
								const uint32_t r = x.l.rcv_nxt - rcv0;
								uint32_t h = 0, ln = 0;

								if (dt == GCL_TCPRXO_BREAK)
									break;
								if (dt == GCL_TCPRXO_APPEND) {
									wake = 1;
									if constexpr (S) {
										if (hf & GCL_TCPRX_FIN)
											mid.fin = 1;
										gcl_tcprxs_append(&x.l, hs, he, (hf & GCL_TCPRX_FIN) != 0, &h, &ln);
									} else {
										gcl_tcprxo_append(&x.l, hs, he, &h, &ln);
									}
									nhead += h != 0;
									ndrained++;
								} else {
									nfreed++;
								}
								if (lane == 0)
									rxo_fate(p, hf, hi, dt, h, ln, r);
								rxo_pop(e);
								qn--;
							}
							gcl_tcprxo_text_tail(&x.l, &rxo_mid(mid), used, wake, qn);
							if constexpr (S)
								gcl_tcprxs_fin(&x, &st, &mid);
						}
						sf = gcl_tcprxo_done(&x.l, &rxo_mid(mid));
					}
				}
				if (stop) {
					H = at;
					break;
				}
				if constexpr (S) {
					dead = gcl_tcprxs_ends(mid.ev);
					nrst += (mid.ev & (GCL_TCPS_RST | GCL_TCPS_RST_ACK)) != 0;
					nfail += (mid.ev & GCL_TCPS_FAIL) != 0;
					nfin += (mid.ev & GCL_TCPS_FIN) != 0;
					nstate += (mid.ev & GCL_TCPS_STATE) != 0;
				}
				if (lane == at) {
					sf_mine = sf;
					after_mine = x.l.rcv_nxt;
					copy_mine = len;
					head_mine = head;
					of_mine = of;
					rel_mine = rel;
					if constexpr (S) {
						ev_mine = mid.ev;
						rseq_mine = mid.rst_seq;
						st_mine = st;
					}
				}
			}
		}
		rxf_chunk_end(t, x.l, ch, H, stopped, sf_mine);
		if (ch.valid) {
			k.verdict[ch.j] = (uint8_t)(lane < H ? GCL_TCPRX_FAST : GCL_TCPRX_SLOW);
			k.sflags[ch.j] = (uint8_t)sf_mine;
			k.after[ch.j] = after_mine;
			if constexpr (S) {
				ps.ev[ch.j] = (uint8_t)ev_mine;
				ps.rst_seq[ch.j] = rseq_mine;
				ps.state_after[ch.j] = (uint8_t)st_mine;
			}
			if (!(of_mine & GCL_OOOF_QUEUED)) { /* a queued entry gets these with its fate */
				k.copy_len[ch.j] = (uint16_t)copy_mine;
				k.dst_off[ch.j] = copy_mine ? rel_mine : 0; /* layout adds conn_off[c] */
				p.oflags[ch.j] = (uint8_t)of_mine;
				p.skip[ch.j] = (uint16_t)head_mine;
			}
		}
	}
	/* the queue as it stands: HELD and KEPT, and the entries staged for rxo_qout_kernel */
	const bool staged = rs < re;
	const bool mine = lane < qn, held = mine && (e.fl >> 16) != 0;
	const uint64_t heldmask = __ballot(held);
	/* a carried entry is staged inside its connection's own input range, a list entry inside its
	 * connection's own run: disjoint between connections whatever order q_off puts the ranges in */
	const uint32_t rank_l = (uint32_t)__popcll(heldmask & ((1ull << lane) - 1)), rank_q = lane - rank_l;
	if (mine) {
		uint32_t ref = e.idx;
		if (held) {
			k.copy_len[e.idx] = 0;
			k.dst_off[e.idx] = 0;
			p.oflags[e.idx] = GCL_OOOF_OOO | GCL_OOOF_QUEUED | GCL_OOOF_HELD;
			p.skip[e.idx] = 0;
		} else {
			p.qin_state[e.idx] = GCL_OOOQ_KEPT;
			ref = p.q[e.idx].z;
		}
		if (staged) /* rank_q < qe - qs and rank_l < re - rs: below nq, and below nq + m */
			p.stage[held ? (size_t)p.nq + rs + rank_l : (size_t)qs + rank_q] = make_uint4(e.seq, e.end, ref, e.fl);
	}
	const uint32_t nheld = (uint32_t)__popcll(heldmask);
	if (lane == 0) {
		rxf_conn_store(p.f, c, x, t, nooo);
		p.ocnt[c] = make_uint4(nqueued, ndrained, nfreed, nhead);
		p.qmeta[c] = make_uint4(qn | (uint32_t)staged << 8 | (uint32_t)taken << 9, nheld, (uint32_t)heldmask,
		                        (uint32_t)(heldmask >> 32));
		if constexpr (S) {
			ps.state_out[c] = (uint8_t)st;
			if (k.counts) {
				if (nrst)
					atomicAdd(k.counts + GCL_TCPRXSC_RSTS, (unsigned long long)nrst);
				if (nfail)
					atomicAdd(k.counts + GCL_TCPRXSC_FAILS, (unsigned long long)nfail);
				if (nfin)
					atomicAdd(k.counts + GCL_TCPRXSC_FINS, (unsigned long long)nfin);
				if (nstate)
					atomicAdd(k.counts + GCL_TCPRXSC_STATE_CHANGES, (unsigned long long)nstate);
			}
		}
	}
}

/*
 * One wave per connection, after the scans: lane i writes entry i of the final
 * queue to qout (from the stage, or straight from q for a connection that had
 * no segment), and the drained input entries get their connection's offset.
 */
__global__ void __launch_bounds__(kRxThreads) rxo_qout_kernel(RxoParams p)
{
	const RxParams &k = p.f.k;
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t c = blockIdx.x * kRxWaves + (threadIdx.x >> 6);

	if (c >= k.nconn)
		return;
	const uint4 meta = p.qmeta[c];
	const uint32_t len = (meta.x & 0xFFu) < GCL_TCPOOO_CAP ? meta.x & 0xFFu : GCL_TCPOOO_CAP;
	const uint64_t heldmask = (uint64_t)meta.w << 32 | meta.z;
	const bool held = (heldmask >> lane & 1) != 0;
	const uint32_t rank_l = (uint32_t)__popcll(heldmask & ((1ull << lane) - 1)), rank_q = lane - rank_l;
	uint64_t rs, re;
	rx_run_bounds(k, c, &rs, &re);
	uint32_t qs, qe;
	rxo_range(p, c, &qs, &qe);

	if (lane < len) {
		const uint64_t at = (uint64_t)p.qout_off[c] + lane;
		uint4 w = make_uint4(0, 0, 0, 0);
		if (meta.x >> 8 & 1) { /* staged: the bounds hold again whatever the workspace holds */
			if (held ? rs + rank_l < re : qs + rank_q < qe)
				w = p.stage[held ? (size_t)p.nq + rs + rank_l : (size_t)qs + rank_q];
		} else if (qs + lane < qe) {
			w = p.q[qs + lane];
			w.w &= 0xFFFFu;
		}
		if (at < p.q_out_cap)
			p.qout[at] = w;
	}
	if ((meta.x >> 9 & 1) && lane < qe - qs) {
		const uint32_t i = qs + lane;
		if (p.qin_state[i] == GCL_OOOQ_DRAINED && p.qin_len[i])
			p.qin_dst_off[i] += k.conn_off[c];
	}
}

/* ---- the counters the walk decides, summed over the connections ---- */

__device__ __forceinline__ const RxParams &rx_base(const RxParams &k) { return k; }
__device__ __forceinline__ const RxParams &rx_base(const RxfParams &p) { return p.k; }
__device__ __forceinline__ const RxParams &rx_base(const RxoParams &p) { return p.f.k; }

/* connection c's share of a call's counters, in the order of rx_counts_kernel's slot table: gcl_tcp_rx's 5 */
__device__ __forceinline__ void rx_counts_of(const RxParams &k, uint32_t c, unsigned long long *v)
{
	const uint4 o1 = k.out_conn[3 * (size_t)c + 1], o2 = k.out_conn[3 * (size_t)c + 2];

	v[0] += o1.z;
	v[1] += o1.w;
	v[2] += (uint32_t)(o1.x - k.conn[3 * (size_t)c + 1].y);
	v[3] += o2.x;
	v[4] += k.wakes[c];
}

/* gcl_tcp_rx_full's 10: those 5 and its own */
__device__ __forceinline__ void rx_counts_of(const RxfParams &p, uint32_t c, unsigned long long *v)
{
	const uint4 e = p.out_ext[c], xc = p.xcnt[c];

	rx_counts_of(p.k, c, v);
	v[5] += e.x;
	v[6] += xc.x;
	v[7] += xc.y;
	v[8] += xc.z;
	v[9] += e.y;
}

/* gcl_tcp_rx_ooo's and gcl_tcp_rx_states' 16: those 10 and the queue's */
__device__ __forceinline__ void rx_counts_of(const RxoParams &p, uint32_t c, unsigned long long *v)
{
	const uint4 oc = p.ocnt[c];

	rx_counts_of(p.f, c, v);
	v[10] += p.f.xcnt[c].w;
	v[11] += oc.x;
	v[12] += oc.y;
	v[13] += oc.z;
	v[14] += oc.w;
	v[15] += p.qmeta[c].y;
}

/* N counters: a lane's sum over its connections, the wave's by shuffles, the block's in LDS, one add per
 * counter per block */
template <int N, typename P>
__global__ void __launch_bounds__(kRxThreads) rx_counts_kernel(P p)
{
	const RxParams &k = rx_base(p);
	__shared__ unsigned long long blk[N];
	unsigned long long v[N] = {};

	if (threadIdx.x < N)
		blk[threadIdx.x] = 0;
	__syncthreads();
	for (uint32_t c = blockIdx.x * kRxThreads + threadIdx.x; c < k.nconn; c += gridDim.x * kRxThreads)
		rx_counts_of(p, c, v);
#pragma unroll
	for (int x = 0; x < N; x++) {
		for (int d = 32; d; d >>= 1) {
			const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v[x], d);
			const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v[x] >> 32), d);
			v[x] += (unsigned long long)hi << 32 | lo;
		}
		if ((threadIdx.x & 63) == 0 && v[x])
			atomicAdd(&blk[x], v[x]);
	}
	__syncthreads();
	if (threadIdx.x < N && blk[threadIdx.x]) {
		const uint32_t slot[16] = {GCL_TCPRXC_FAST, GCL_TCPRXC_SLOW, GCL_TCPRXC_BYTES, GCL_TCPRXC_ACKS,
		                           GCL_TCPRXC_WAKES, GCL_TCPRXFC_RULE2, GCL_TCPRXFC_TXWAKES, GCL_TCPRXFC_FASTRTX,
		                           GCL_TCPRXFC_DUPACKS, GCL_TCPRXFC_DROPPED, GCL_TCPRXOC_OOO, GCL_TCPRXOC_QUEUED,
		                           GCL_TCPRXOC_DRAINED, GCL_TCPRXOC_FREED, GCL_TCPRXOC_HEADCLIP, GCL_TCPRXOC_HELD};
		atomicAdd(k.counts + slot[threadIdx.x], blk[threadIdx.x]);
	}
}

/* ---- the workspace ---- */

struct RxGeom {
	uint32_t passes, nb[2], kbits[2];
	uint32_t ranges; /* as sized: in->blocks or the cap */
	size_t rec, cookie, idx[2], hist, csum, lsum, tot, run, wakes, bytes;
};

static size_t rx_up16(size_t x)
{
	return (x + 15) & ~(size_t)15;
}

static uint32_t rx_bits(uint32_t nb)
{
	return nb > 1 ? 32 - (uint32_t)__builtin_clz(nb - 1) : 0;
}

static int rx_geometry(uint64_t m, uint32_t nconn, uint32_t blocks, RxGeom *g)
{
	if (m > (1ull << 31) || nconn > GCL_TCPRX_MAX_CONN || blocks > GCL_TCPRX_MAX_BLOCKS)
		return -EINVAL;
	g->passes = nconn > kRxDigits ? 2 : 1;
	g->nb[0] = nconn > kRxDigits ? kRxDigits : nconn ? nconn : 1;
	g->nb[1] = g->passes == 2 ? ((nconn - 1) >> kRxDigitBits) + 1 : 0;
	g->kbits[0] = rx_bits(g->nb[0]);
	g->kbits[1] = rx_bits(g->nb[1]);
	/* the library's choice never exceeds one range per 256 entries, nor the cap */
	const uint64_t tiles = (m + kRxThreads - 1) / kRxThreads;
	g->ranges = blocks ? blocks : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, GCL_TCPRX_MAX_BLOCKS));
	const size_t entries = (size_t)std::max(g->nb[0], g->nb[1]) * g->ranges;
	size_t at = 0;
	g->rec = at;
	at += 16 * (size_t)m;
	g->cookie = at;
	at += rx_up16(4 * (size_t)m);
	g->idx[0] = at;
	at += rx_up16(4 * (size_t)m);
	g->idx[1] = at;
	at += g->passes == 2 ? rx_up16(4 * (size_t)m) : 0;
	g->hist = at;
	at += 4 * entries;
	g->csum = at;
	at += rx_up16(4 * ((entries + kRxChunk - 1) / kRxChunk));
	g->lsum = at;
	at += rx_up16(8 * (((size_t)nconn + kRxChunk - 1) / kRxChunk));
	g->tot = at;
	at += 16;
	g->run = at;
	at += rx_up16(8 * (size_t)nconn);
	g->wakes = at;
	at += rx_up16(4 * (size_t)nconn);
	g->bytes = at;
	return 0;
}

static bool rx_misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tcp_rx_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, size_t *bytes)
{
	RxGeom g;

	if (!bytes || rx_geometry(m, nconn, blocks, &g))
		return -EINVAL;
	*bytes = g.bytes;
	return 0;
}

/* what gcl_tcp_rx_full adds to a call; NULL: gcl_tcp_rx */
struct RxFull {
	const uint8_t *rep_acks;
	struct gcl_tcp_conn_ext *out_ext;
};

/* what gcl_tcp_rx_ooo adds to a gcl_tcp_rx_full call; NULL: not that call */
struct RxOoo {
	const struct gcl_tcprxo_in *in;
	const struct gcl_tcprxo_out *out;
};

/* what gcl_tcp_rx_states adds to a gcl_tcp_rx_ooo call; NULL: not that call */
struct RxStates {
	const uint8_t *state;
	const struct gcl_tcprxs_out *out;
};

/* the bytes gcl_tcp_rx_ooo keeps behind gcl_tcp_rx_full's workspace: ocnt, qmeta, qsum, stage */
static size_t rxo_extra(uint64_t m, uint32_t nconn, uint32_t nq)
{
	return 32 * (size_t)nconn + rx_up16(4 * (((size_t)nconn + kRxChunk - 1) / kRxChunk)) + 16 * ((size_t)nq + m);
}

/* the three launches of the exclusive scan of io.load(0 .. total) */
template <typename Io>
static void rx_scan(const Io &io, uint32_t total, typename Io::T *csum, hipStream_t s)
{
	const uint32_t nchunks = (total + kRxChunk - 1) / kRxChunk;

	hipLaunchKernelGGL(rx_scan_sum_kernel<Io>, dim3(nchunks), dim3(kRxThreads), 0, s, io, total, csum);
	hipLaunchKernelGGL(rx_scan_top_kernel<Io>, dim3(1), dim3(kRxTopThreads), 0, s, io, csum, nchunks);
	hipLaunchKernelGGL(rx_scan_apply_kernel<Io>, dim3(nchunks), dim3(kRxThreads), 0, s, io, total, csum);
}

/*
 * The driver of the four calls.  @full, @ooo and @sts nest: each call passes
 * what it adds to the one before it and NULL for the rest.  Validation, the
 * parameter blocks, the geometry, parse, group, runs and the three scans are
 * the same code for all four; a call chooses its walk, its fix-up key, whether
 * the queues are written out, and how many counters are summed.
 */
static int rx_run(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_tcprx_in *in,
                  const struct gcl_tcprx_out *out, const RxFull *full, const RxOoo *ooo, const RxStates *sts,
                  uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	RxGeom g;

	if (sts && (!full || !ooo || !ooo->in))
		return -EINVAL;
	if (!c || !b || !in || !out || in->size != sizeof(*in) || !gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || rx_geometry(in->m, in->nconn, in->blocks, &g) || !in->sock ||
	    !out->conn_off)
		return -EINVAL;
	if (in->nconn && (!in->conn || !out->out_conn || (full && !full->out_ext)))
		return -EINVAL;
	if (full && rx_misaligned(full->out_ext, 16))
		return -EINVAL;
	if (in->m && (!out->verdict || !out->sflags || !out->rcv_nxt_after || !out->copy_len || !out->dst_off))
		return -EINVAL;
	if (rx_misaligned(in->order, 4) || rx_misaligned(in->sock, 4) || rx_misaligned(in->conn, 16) ||
	    rx_misaligned(out->rcv_nxt_after, 4) || rx_misaligned(out->copy_len, 2) ||
	    rx_misaligned(out->dst_off, 8) || rx_misaligned(out->out_conn, 16) ||
	    rx_misaligned(out->conn_off, 8) || rx_misaligned(counts, 8))
		return -EINVAL;
	if (ooo) {
		const struct gcl_tcprxo_in *oi = ooo->in;
		const struct gcl_tcprxo_out *oo = ooo->out;

		if (!oo || oi->nq > (1u << 31) || !oo->qout_off || !oo->totals || (in->m && (!oo->oflags || !oo->skip)) ||
		    (oi->nq && (!oi->q || !oo->qin_state || !oo->qin_skip || !oo->qin_len || !oo->qin_dst_off)) ||
		    (oi->q_out_cap && !oo->qout))
			return -EINVAL;
		if (rx_misaligned(oi->q_off, 4) || rx_misaligned(oi->q, 16) || rx_misaligned(oo->skip, 2) ||
		    rx_misaligned(oo->qin_skip, 2) || rx_misaligned(oo->qin_len, 2) || rx_misaligned(oo->qin_dst_off, 8) ||
		    rx_misaligned(oo->qout_off, 4) || rx_misaligned(oo->qout, 16) || rx_misaligned(oo->totals, 8))
			return -EINVAL;
	}
	if (sts) {
		const struct gcl_tcprxs_out *so = sts->out;

		if (!so || (in->m && (!so->ev || !so->rst_seq || !so->state_after)) ||
		    (in->nconn && !so->state_out) || rx_misaligned(so->rst_seq, 4))
			return -EINVAL;
	}
	/* gcl_tcp_rx_full keeps xcnt behind gcl_tcp_rx's workspace, gcl_tcp_rx_ooo its own behind that */
	const size_t xbytes = (full ? 16 * (size_t)in->nconn : 0) + (ooo ? rxo_extra(in->m, in->nconn, ooo->in->nq) : 0);
	if (!workspace || rx_misaligned(workspace, 16) || workspace_bytes < g.bytes + xbytes)
		return -EINVAL;
	if (in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	              (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	              !b->pkt_len || rx_misaligned(b->pkt_len, 2)))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	uint8_t *ws = (uint8_t *)workspace;
	RxParams k;
	k.frames = b->frames;
	k.frames_len = b->frames_len;
	k.stride = b->stride;
	k.offs = b->offs;
	k.pkt_len = b->pkt_len;
	k.n = b->n;
	k.order = in->order;
	k.sock = in->sock;
	k.l4_status = in->l4_status;
	k.conn = (const uint4 *)in->conn;
	k.verdict = out->verdict;
	k.sflags = out->sflags;
	k.after = out->rcv_nxt_after;
	k.copy_len = out->copy_len;
	k.dst_off = out->dst_off;
	k.out_conn = (uint4 *)out->out_conn;
	k.conn_off = (unsigned long long *)out->conn_off;
	k.counts = (unsigned long long *)counts;
	k.rec = (uint4 *)(ws + g.rec);
	k.cookie = (uint32_t *)(ws + g.cookie);
	k.idx[0] = (uint32_t *)(ws + g.idx[0]);
	k.idx[1] = (uint32_t *)(ws + g.idx[1]);
	k.hist = (uint32_t *)(ws + g.hist);
	k.csum = (uint32_t *)(ws + g.csum);
	k.lsum = (unsigned long long *)(ws + g.lsum);
	k.tot = (uint32_t *)(ws + g.tot);
	k.run = (uint2 *)(ws + g.run);
	k.wakes = (uint32_t *)(ws + g.wakes);
	k.m = in->m;
	k.nconn = in->nconn;
	k.amask = in->align ? in->align - 1 : 0;

	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);
	const uint64_t tiles = (in->m + kRxThreads - 1) / kRxThreads;
	const unsigned egrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)cus * 8));
	k.ranges = in->blocks ? in->blocks :
	           (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::min<uint32_t>(cus * kRxBlocksPerCu,
	                                                                                      GCL_TCPRX_MAX_BLOCKS)));
	k.range_len = (uint32_t)(((in->m + k.ranges - 1) / k.ranges + 63) / 64 * 64);
	if (k.range_len == 0)
		k.range_len = 64;

	if (ooo) { /* what no walk may reach: entries that are NA, NOCONN or DROP, queue entries of no taken connection */
		const struct gcl_tcprxo_out *oo = ooo->out;
		const size_t nq = ooo->in->nq;

		if ((in->m && (hipMemsetAsync(oo->oflags, 0, in->m, s) != hipSuccess ||
		               hipMemsetAsync(oo->skip, 0, 2 * (size_t)in->m, s) != hipSuccess)) ||
		    (nq && (hipMemsetAsync(oo->qin_state, GCL_OOOQ_UNTOUCHED, nq, s) != hipSuccess ||
		            hipMemsetAsync(oo->qin_skip, 0, 2 * nq, s) != hipSuccess ||
		            hipMemsetAsync(oo->qin_len, 0, 2 * nq, s) != hipSuccess ||
		            hipMemsetAsync(oo->qin_dst_off, 0, 8 * nq, s) != hipSuccess)))
			return -EIO;
		if (in->nconn == 0 && (hipMemsetAsync(oo->qout_off, 0, 4, s) != hipSuccess ||
		                       hipMemsetAsync(oo->totals, 0, 8, s) != hipSuccess))
			return -EIO;
	}
	if (sts && in->m) { /* NA, NOCONN and DROP entries, and with nconn == 0 every entry */
		const struct gcl_tcprxs_out *so = sts->out;

		if (hipMemsetAsync(so->ev, 0, in->m, s) != hipSuccess ||
		    hipMemsetAsync(so->rst_seq, 0, 4 * (size_t)in->m, s) != hipSuccess ||
		    hipMemsetAsync(so->state_after, 0, in->m, s) != hipSuccess)
			return -EIO;
	}
	if (in->nconn == 0) { /* every TCP segment is NOCONN: nothing to group, walk or lay out */
		if (in->m)
			hipLaunchKernelGGL(rx_parse_kernel, dim3(egrid), dim3(kRxThreads), 0, s, k);
		if (hipMemsetAsync(out->conn_off, 0, sizeof(uint64_t), s) != hipSuccess)
			return -EIO;
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	if (hipMemsetAsync(k.run, 0, 8 * (size_t)in->nconn, s) != hipSuccess)
		return -EIO;
	const uint32_t *sorted = k.idx[g.passes - 1];
	if (in->m) {
		hipLaunchKernelGGL(rx_parse_kernel, dim3(egrid), dim3(kRxThreads), 0, s, k);
		for (uint32_t p = 0; p < g.passes; p++) {
			const RxPass ps = {p ? k.idx[0] : nullptr, k.idx[p], p * kRxDigitBits, g.nb[p], g.kbits[p]};
			const dim3 grid((k.ranges + kRxWaves - 1) / kRxWaves);
			hipLaunchKernelGGL(rx_count_kernel, grid, dim3(kRxThreads), 0, s, k, ps);
			rx_scan(RxHistIo{k.hist, k.tot}, ps.nb * k.ranges, k.csum, s);
			hipLaunchKernelGGL(rx_scatter_kernel, grid, dim3(kRxThreads), 0, s, k, ps);
		}
		hipLaunchKernelGGL(rx_runs_kernel, dim3(egrid), dim3(kRxThreads), 0, s, k, sorted);
	}
	RxfParams kf = {k, nullptr, nullptr, nullptr};
	RxoParams ko = {};
	const dim3 wgrid((in->nconn + kRxWaves - 1) / kRxWaves);
	if (full) {
		kf.rep_acks = full->rep_acks;
		kf.out_ext = (uint4 *)full->out_ext;
		kf.xcnt = (uint4 *)(ws + g.bytes);
	}
	if (ooo) {
		const struct gcl_tcprxo_in *oi = ooo->in;
		const struct gcl_tcprxo_out *oo = ooo->out;
		uint8_t *at = ws + g.bytes + 16 * (size_t)in->nconn;

		ko.f = kf;
		ko.q_off = oi->q_off;
		ko.q = (const uint4 *)oi->q;
		ko.nq = oi->nq;
		ko.q_out_cap = oi->q_out_cap;
		ko.oflags = oo->oflags;
		ko.skip = oo->skip;
		ko.qin_state = oo->qin_state;
		ko.qin_skip = oo->qin_skip;
		ko.qin_len = oo->qin_len;
		ko.qin_dst_off = (unsigned long long *)oo->qin_dst_off;
		ko.qout_off = oo->qout_off;
		ko.qout = (uint4 *)oo->qout;
		ko.totals = (unsigned long long *)oo->totals;
		ko.ocnt = (uint4 *)at;
		at += 16 * (size_t)in->nconn;
		ko.qmeta = (uint4 *)at;
		at += 16 * (size_t)in->nconn;
		ko.qsum = (uint32_t *)at;
		at += rx_up16(4 * (((size_t)in->nconn + kRxChunk - 1) / kRxChunk));
		ko.stage = (uint4 *)at;
		if (sts) {
			const RxsParams ks = {ko, sts->state, sts->out->ev, sts->out->rst_seq, sts->out->state_after,
			                      sts->out->state_out};
			hipLaunchKernelGGL(rxq_walk_kernel<RxsParams>, wgrid, dim3(kRxThreads), 0, s, ks, sorted);
		} else {
			hipLaunchKernelGGL(rxq_walk_kernel<RxoParams>, wgrid, dim3(kRxThreads), 0, s, ko, sorted);
		}
		rx_scan(RxQoutIo{ko.qmeta, ko.qout_off, ko.totals, in->nconn}, in->nconn, ko.qsum, s);
	} else if (full) {
		hipLaunchKernelGGL(rxf_walk_kernel, wgrid, dim3(kRxThreads), 0, s, kf, sorted);
	} else {
		hipLaunchKernelGGL(rx_walk_kernel, wgrid, dim3(kRxThreads), 0, s, k, sorted);
	}
	rx_scan(RxConnIo{k.conn, k.out_conn, k.conn_off, in->nconn, k.amask}, in->nconn, k.lsum, s);
	if (in->m && full)
		hipLaunchKernelGGL(rx_fix_kernel<true>, dim3(egrid), dim3(kRxThreads), 0, s, k);
	else if (in->m)
		hipLaunchKernelGGL(rx_fix_kernel<false>, dim3(egrid), dim3(kRxThreads), 0, s, k);
	if (ooo)
		hipLaunchKernelGGL(rxo_qout_kernel, wgrid, dim3(kRxThreads), 0, s, ko);
	if (counts) {
		const dim3 cgrid(std::min<uint32_t>((in->nconn + kRxThreads - 1) / kRxThreads, cus * 2));
		if (ooo)
			hipLaunchKernelGGL(rx_counts_kernel<16>, cgrid, dim3(kRxThreads), 0, s, ko);
		else if (full)
			hipLaunchKernelGGL(rx_counts_kernel<10>, cgrid, dim3(kRxThreads), 0, s, kf);
		else
			hipLaunchKernelGGL(rx_counts_kernel<5>, cgrid, dim3(kRxThreads), 0, s, k);
	}
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

extern "C" int gcl_tcp_rx(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_tcprx_in *in,
                          const struct gcl_tcprx_out *out, uint64_t *counts, void *workspace,
                          size_t workspace_bytes, void *hip_stream)
{
	return rx_run(c, b, in, out, nullptr, nullptr, nullptr, counts, workspace, workspace_bytes, hip_stream);
}

extern "C" int gcl_tcp_rx_full_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, size_t *bytes)
{
	RxGeom g;

	if (!bytes || rx_geometry(m, nconn, blocks, &g))
		return -EINVAL;
	*bytes = g.bytes + 16 * (size_t)nconn;
	return 0;
}

extern "C" int gcl_tcp_rx_full(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_tcprxf_in *in,
                               const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                               uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	if (!in || in->size != sizeof(*in))
		return -EINVAL;
	const struct gcl_tcprx_in rin = {sizeof(rin), in->align, in->order, in->m, in->sock, in->l4_status,
	                                 in->conn, in->nconn, in->blocks};
	const RxFull full = {in->rep_acks, out_ext};

	return rx_run(c, b, &rin, out, &full, nullptr, nullptr, counts, workspace, workspace_bytes, hip_stream);
}

extern "C" int gcl_tcp_rx_ooo_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, uint32_t nq, size_t *bytes)
{
	RxGeom g;

	if (!bytes || nq > (1u << 31) || rx_geometry(m, nconn, blocks, &g))
		return -EINVAL;
	*bytes = g.bytes + 16 * (size_t)nconn + rxo_extra(m, nconn, nq);
	return 0;
}

extern "C" int gcl_tcp_rx_ooo(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_tcprxo_in *in,
                              const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                              const struct gcl_tcprxo_out *ooo, uint64_t *counts, void *workspace,
                              size_t workspace_bytes, void *hip_stream)
{
	if (!in || in->size != sizeof(*in))
		return -EINVAL;
	const struct gcl_tcprx_in rin = {sizeof(rin), in->align, in->order, in->m, in->sock, in->l4_status,
	                                 in->conn, in->nconn, in->blocks};
	const RxFull full = {in->rep_acks, out_ext};
	const RxOoo o = {in, ooo};

	return rx_run(c, b, &rin, out, &full, &o, nullptr, counts, workspace, workspace_bytes, hip_stream);
}

extern "C" int gcl_tcp_rx_states_workspace(uint64_t m, uint32_t nconn, uint32_t blocks, uint32_t nq, size_t *bytes)
{
	return gcl_tcp_rx_ooo_workspace(m, nconn, blocks, nq, bytes);
}

extern "C" int gcl_tcp_rx_states(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_tcprxs_in *in,
                                 const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                                 const struct gcl_tcprxo_out *ooo, const struct gcl_tcprxs_out *st,
                                 uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	if (!in || in->size != sizeof(*in) || !st)
		return -EINVAL;
	const struct gcl_tcprx_in rin = {sizeof(rin), in->align, in->order, in->m, in->sock, in->l4_status,
	                                 in->conn, in->nconn, in->blocks};
	const struct gcl_tcprxo_in oin = {sizeof(oin), in->align, in->order, in->m, in->sock, in->l4_status,
	                                  in->conn, in->nconn, in->blocks, in->rep_acks, in->q_off, in->q, in->nq,
	                                  in->q_out_cap};
	const RxFull full = {in->rep_acks, out_ext};
	const RxOoo o = {&oin, ooo};
	const RxStates ss = {in->state, st};

	return rx_run(c, b, &rin, out, &full, &o, &ss, counts, workspace, workspace_bytes, hip_stream);
}
