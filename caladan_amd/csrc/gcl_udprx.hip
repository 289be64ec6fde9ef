/*
 * gcl_udprx.hip - udp_conn_recv and udp_par_recv for one runtime's list of
 * packets (gcl_udp_rx, gclassify.h; runtime/net/udp.c:79-107, :811-840): every
 * socket's datagrams, in arrival order, through the rule of gcl_udprx.h, and
 * the layout that puts the datagrams a socket took in one piece.
 *
 * udp_conn_recv carries one count from datagram to datagram, so whether
 * datagram j is queued depends only on how many datagrams of its socket came
 * before it.  After a stable sort by socket that number is a position minus a
 * run start, and every launch below is one lane per entry or per socket: none
 * walks a socket's run, so no launch's time grows with the longest run.
 *
 * Launches on the stream, ordered by the stream alone: no block waits for
 * another, there is no look-back, flag or cooperative launch, and the only
 * atomics are counter additions whose order changes nothing.
 *
 *   parse    one lane per list entry: order[j], the per-packet arrays, the
 *            frame's bytes [12, 48) with gcl_payload.hip's loads (the 16-B
 *            chunks of an aligned 64-B window, else byte by byte), then
 *            gcl_pay_rule and gcl_udprx_class.  An entry that is NA or NOSOCK
 *            gets its final outputs here and the key GCL_UDPRX_NONE in the
 *            workspace; a datagram gets its socket index as key and one 8-B
 *            record (rip, rport | len << 16).
 *   group    the stable LSD counting sort of the list positions of the
 *            datagrams by socket index, 11 bits a pass: one pass for
 *            nsock <= 2048, two up to 2^20, in gcl_plan.hip's form: count (a
 *            wave per contiguous range, its counters in LDS), three scan
 *            launches over hist[digit][range], and scatter (a wave re-reads
 *            its range in order, a lane's rank among the equal keys of its 64
 *            entries is a ballot population count, the wave's leader lanes
 *            move its counters on).  No atomic hands out a position.  The
 *            last pass also stores the sorted keys.
 *   bounds   one lane per socket s <= nsock: the first sorted position whose
 *            key is >= s, by binary search over the sorted keys (at most 32
 *            steps whatever the list holds).  start[s] .. start[s + 1] is the
 *            socket's run, empty sockets included, so no array is cleared
 *            and no run start is scattered.
 *   decide   one lane per sorted position p: k = p - start[key], the closed
 *            form gcl_udprx_closed, one dword (verdict, sflags, len) to the
 *            workspace, and the sum of the pair (taken, pad(len)) over each
 *            2048-position chunk.
 *   top      one block: the exclusive scan of the chunk sums, the totals.
 *   emit     one lane per sorted position again: the exclusive scan of the
 *            pair inside the chunk (ballot counts for taken, a wave shuffle
 *            scan for the bytes, the four waves through LDS, a carry from
 *            tile to tile) on top of the chunk's base.  Sorted order is
 *            socket order, so the scanned pair IS the entry's rec_idx and
 *            dst_off.  It writes the per-entry outputs, the record as one
 *            16-B store, the scanned pair for the socket pass, and the
 *            counters (ballot counts per wave, one add per counter per block).
 *   socks    one lane per socket s <= nsock: rec_off[s] and sock_off[s] are
 *            the scanned pair at start[s] (the totals when no run starts at
 *            or behind s), out_sock[s] is gcl_udprx_after of the run length.
 *
 * Bounds.  A list index is used only below m, a packet index only below n, a
 * socket index only below nsock (parse leaves no other in the workspace, and
 * every later use clamps again); sorted positions are used only below
 * min(*tot, m); a record index only below m.  The frame is read as in
 * gcl_payload.hip: an aligned window only when it lies inside
 * frames[0, frames_len), else every byte's index is tested.  No inline
 * assembly beyond compiler barriers.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_pay.h"
#include "gcl_udprx.h"

namespace gclk {

constexpr uint32_t kUxThreads = 256;
constexpr uint32_t kUxWaves = kUxThreads / 64;
constexpr uint32_t kUxDigitBits = 11;
constexpr uint32_t kUxDigits = 1u << kUxDigitBits; /* counters of one wave */
constexpr uint32_t kUxChunk = 2048;                /* entries per scan block */
constexpr uint32_t kUxTiles = kUxChunk / kUxThreads;
constexpr uint32_t kUxTopThreads = 1024;
constexpr uint32_t kUxBlocksPerCu = 4;
static_assert(sizeof(struct gcl_udp_sock) == 16 && sizeof(struct gcl_udp_sock_out) == 16 &&
              sizeof(struct gcl_udp_rec) == 16, "records as 16-B words");

struct UxParams {
	const uint8_t *frames;
	uint64_t frames_len;
	uint64_t stride;
	const uint64_t *offs;
	const uint16_t *pkt_len;
	uint64_t n;
	const uint32_t *order;
	const uint32_t *sock;
	const uint8_t *l4_status;
	const uint4 *usock;       /* struct gcl_udp_sock as one 16-B word */
	uint8_t *verdict, *sflags;
	uint16_t *copy_len;
	uint64_t *dst_off;
	uint32_t *rec_idx;
	uint4 *rec;
	uint4 *out_sock;
	uint32_t *rec_off;
	unsigned long long *sock_off;
	unsigned long long *counts;
	/* the workspace */
	uint2 *info;              /* [m]: rip, rport | len << 16 of a datagram */
	uint32_t *key;            /* [m]: socket index, or GCL_UDPRX_NONE */
	uint32_t *idx[2];         /* [m] each: the sorted list positions of pass 0 and 1 */
	uint32_t *skey;           /* [m]: the key at every sorted position */
	uint32_t *dv;             /* [m]: verdict | sflags << 8 | len << 16 at every sorted position */
	uint32_t *sc_cnt;         /* [m]: the taken datagrams before a sorted position */
	unsigned long long *sc_off; /* [m]: their padded bytes */
	uint32_t *hist;           /* [digits][ranges] */
	uint32_t *csum;           /* [scan blocks of hist] */
	unsigned long long *pcnt, *poff; /* [chunks] each: the pair's chunk sums, then bases */
	uint32_t *tot;            /* the number of datagrams */
	unsigned long long *ptot; /* [2]: the totals of the pair */
	uint32_t *start;          /* [nsock + 1] */
	uint64_t m;               /* <= 2^31 */
	uint32_t nsock, sock_base;
	uint32_t ranges, range_len; /* range_len: a multiple of 64 */
	uint32_t amask;
};

/* the datagrams of the list: sorted positions are used below this */
__device__ __forceinline__ uint64_t ux_total(const UxParams &k)
{
	const uint64_t t = *k.tot;

	return t < k.m ? t : k.m;
}

/* ---- the exclusive scan of hist[0, total), kUxChunk entries per block ---- */

template <typename T, int NT>
__device__ __forceinline__ T ux_block_scan(T x, T *total)
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

__global__ void __launch_bounds__(kUxThreads) ux_hist_sum_kernel(UxParams k, uint32_t total)
{
	const uint32_t i0 = blockIdx.x * kUxChunk + threadIdx.x * 8;
	uint32_t s = 0, tot;

	for (uint32_t j = 0; j < 8; j++)
		s += i0 + j < total ? k.hist[i0 + j] : 0;
	(void)ux_block_scan<uint32_t, kUxThreads>(s, &tot);
	if (threadIdx.x == 0)
		k.csum[blockIdx.x] = tot;
}

/* one block: csum[0, nchunks) -> its exclusive scan; the grand total to *tot */
__global__ void __launch_bounds__(kUxTopThreads) ux_hist_top_kernel(UxParams k, uint32_t nchunks)
{
	const uint32_t per = (nchunks + kUxTopThreads - 1) / kUxTopThreads;
	const uint32_t i0 = threadIdx.x * per;
	uint32_t s = 0;

	for (uint32_t j = 0; j < per; j++)
		s += i0 + j < nchunks ? k.csum[i0 + j] : 0;
	uint32_t acc = ux_block_scan<uint32_t, kUxTopThreads>(s, nullptr);
	for (uint32_t j = 0; j < per; j++) {
		if (i0 + j < nchunks) {
			const uint32_t x = k.csum[i0 + j];
			k.csum[i0 + j] = acc;
			acc += x;
		}
	}
	if (threadIdx.x == kUxTopThreads - 1)
		*k.tot = acc;
}

__global__ void __launch_bounds__(kUxThreads) ux_hist_apply_kernel(UxParams k, uint32_t total)
{
	const uint32_t i0 = blockIdx.x * kUxChunk + threadIdx.x * 8;
	uint32_t x[8], s = 0;

	for (uint32_t j = 0; j < 8; j++) {
		x[j] = i0 + j < total ? k.hist[i0 + j] : 0;
		s += x[j];
	}
	uint32_t acc = k.csum[blockIdx.x] + ux_block_scan<uint32_t, kUxThreads>(s, nullptr);
	for (uint32_t j = 0; j < 8; j++) {
		if (i0 + j < total) {
			k.hist[i0 + j] = acc;
			acc += x[j];
		}
	}
}

/* ---- parse ---- */

/* frame dwords 3..11 out of the window's sixteen, the frame starting 4 L bytes in */
template <int L>
__device__ __forceinline__ void ux_pick(const uint4 (&w)[4], uint32_t d[9])
{
	const uint32_t W[16] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w,
	                        w[2].x, w[2].y, w[2].z, w[2].w, w[3].x, w[3].y, w[3].z, w[3].w};
#pragma unroll
	for (int i = 0; i < 9; i++)
		d[i] = W[3 + i + L];
}

__global__ void __launch_bounds__(kUxThreads) ux_parse_kernel(UxParams k)
{
	const uint32_t fbase = (uint32_t)(uintptr_t)k.frames;
	uint32_t cnt[2] = {0, 0}; /* NOSOCK, NA: wave-uniform */

	for (uint64_t j0 = (uint64_t)blockIdx.x * kUxThreads; j0 < k.m; j0 += (uint64_t)gridDim.x * kUxThreads) {
		const uint64_t j = j0 + threadIdx.x;
		uint32_t verdict = GCL_UDPRX_QUEUED; /* here: a datagram, or no entry */
		if (j < k.m) {
			const uint64_t i = k.order ? k.order[j] : j;
			uint32_t s = GCL_UDPRX_NONE;
			struct gcl_pay_desc r = {0, 0, GCL_PAY_OOR, {0, 0, 0, 0}};

			verdict = GCL_UDPRX_NA;
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
				uint32_t d[9];
				if (al) {
					/* window dword x is frame dword x - lead / 4; wanted are 3..11 */
					const uint4 *w = (const uint4 *)(k.frames + (o - lead));
					uint4 c[4];
					c[0] = c[3] = make_uint4(0, 0, 0, 0);
					if (lead == 0)
						c[0] = w[0];
					c[1] = w[1];
					c[2] = w[2];
					if (lead != 0)
						c[3] = w[3];
					if (lead == 0)
						ux_pick<0>(c, d);
					else if (lead == 4)
						ux_pick<1>(c, d);
					else if (lead == 8)
						ux_pick<2>(c, d);
					else
						ux_pick<3>(c, d);
				} else {
					const uint8_t *f = k.frames + o;
					for (uint32_t x = 0; x < 9; x++) {
						uint32_t v = 0;
						for (uint32_t y = 0; y < 4; y++) {
							const uint32_t at = 12 + 4 * x + y;
							v |= (at < avail ? (uint32_t)f[at] : 0u) << (8 * y);
						}
						d[x] = v;
					}
				}
				r = gcl_pay_rule(d, o, L, k.l4_status != nullptr, st, 1, sk);
				verdict = gcl_udprx_class(&r, sk, k.sock_base, k.nsock, &s);
			}
			if (verdict != GCL_UDPRX_QUEUED) {
				k.verdict[j] = (uint8_t)verdict;
				k.sflags[j] = 0;
				k.copy_len[j] = 0;
				k.dst_off[j] = 0;
				k.rec_idx[j] = GCL_UDPRX_NONE;
				s = GCL_UDPRX_NONE;
			} else {
				k.info[j] = make_uint2(r.meta[0], gcl_udprx_rport(&r) | r.len << 16);
			}
			k.key[j] = s;
		}
		cnt[0] += (uint32_t)__popcll(__ballot(verdict == GCL_UDPRX_NOSOCK));
		cnt[1] += (uint32_t)__popcll(__ballot(verdict == GCL_UDPRX_NA));
	}
	if (k.counts && (threadIdx.x & 63) == 0) {
		if (cnt[0])
			atomicAdd(k.counts + GCL_UDPRX_NOSOCK, (unsigned long long)cnt[0]);
		if (cnt[1])
			atomicAdd(k.counts + GCL_UDPRX_NA, (unsigned long long)cnt[1]);
	}
}

/* ---- group ---- */

struct UxPass {
	const uint32_t *src; /* NULL: the list itself, entries that are no datagrams skipped */
	uint32_t *dst;
	uint32_t *skey;      /* the last pass: where the sorted keys go */
	uint32_t shift, nb, kbits;
};

/* the lanes of this wave that are @valid and hold this lane's @key */
__device__ __forceinline__ uint64_t ux_match(uint32_t key, bool valid, uint32_t kbits)
{
	uint64_t m = __ballot(valid);

	for (uint32_t b = 0; b < kbits; b++) {
		const bool bit = (key >> b) & 1u;
		const uint64_t bal = __ballot(bit);
		m &= bit ? bal : ~bal;
	}
	return m;
}

/* source position p of a pass: the list position it names, its socket and its digit */
__device__ __forceinline__ bool ux_key(const UxParams &k, const UxPass &ps, uint64_t p, uint64_t end, uint32_t *j,
                                       uint32_t *sk, uint32_t *key)
{
	bool valid = p < end;
	uint32_t at = 0, s = GCL_UDPRX_NONE;

	if (valid) {
		at = ps.src ? ps.src[p] : (uint32_t)p;
		valid = at < k.m;
	}
	if (valid) {
		s = k.key[at];
		valid = s < k.nsock;
	}
	const uint32_t dg = valid ? (s >> ps.shift) & (kUxDigits - 1) : 0;
	*j = at;
	*sk = s;
	*key = dg < ps.nb ? dg : ps.nb - 1;
	return valid;
}

__device__ __forceinline__ uint64_t ux_limit(const UxParams &k, const UxPass &ps)
{
	return ps.src ? ux_total(k) : k.m;
}

__global__ void __launch_bounds__(kUxThreads) ux_count_kernel(UxParams k, UxPass ps)
{
	__shared__ uint32_t lds[kUxWaves][kUxDigits];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kUxWaves + wave;

	if (r >= k.ranges)
		return; /* waves share nothing: no barrier below */
	uint32_t *cnt = lds[wave];
	for (uint32_t b = lane; b < ps.nb; b += 64)
		cnt[b] = 0;
	const uint64_t limit = ux_limit(k, ps);
	const uint64_t start = (uint64_t)r * k.range_len;
	const uint64_t end = start + k.range_len < limit ? start + k.range_len : limit;
	for (uint64_t base = start; base < end; base += 64) {
		uint32_t j, sk, key;
		const bool valid = ux_key(k, ps, base + lane, end, &j, &sk, &key);
		const uint64_t mt = ux_match(key, valid, ps.kbits);
		/* one add per distinct key of the step, by its lowest lane */
		if (valid && !(mt & ((1ull << lane) - 1)))
			atomicAdd(&cnt[key], (uint32_t)__popcll(mt));
	}
	asm volatile("" ::: "memory");
	/* every entry of this range's column is written: no zeroing of the workspace */
	for (uint32_t b = lane; b < ps.nb; b += 64)
		k.hist[(size_t)b * k.ranges + r] = cnt[b];
}

__global__ void __launch_bounds__(kUxThreads) ux_scatter_kernel(UxParams k, UxPass ps)
{
	__shared__ uint32_t lds[kUxWaves][kUxDigits];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * kUxWaves + wave;

	if (r >= k.ranges)
		return;
	/* read and moved on by different lanes from step to step: LDS serves one
	 * wave's accesses in issue order, and volatile keeps the compiler to it */
	volatile uint32_t *cnt = lds[wave];
	const uint64_t limit = ux_limit(k, ps);
	const uint64_t start = (uint64_t)r * k.range_len;
	const uint64_t end = start + k.range_len < limit ? start + k.range_len : limit;

	if (start >= end)
		return;
	for (uint32_t b = lane; b < ps.nb; b += 64)
		cnt[b] = k.hist[(size_t)b * k.ranges + r];
	for (uint64_t base = start; base < end; base += 64) {
		uint32_t j, sk, key;
		const bool valid = ux_key(k, ps, base + lane, end, &j, &sk, &key);
		const uint64_t mt = ux_match(key, valid, ps.kbits);
		const uint32_t rank = (uint32_t)__popcll(mt & ((1ull << lane) - 1));
		const uint32_t at = cnt[key]; /* key < nb <= kUxDigits, whatever the bytes */
		if (valid) {
			const uint32_t pos = at + rank;
			if (pos < k.m) {
				ps.dst[pos] = j;
				if (ps.skey)
					ps.skey[pos] = sk;
			}
			if (rank == 0)
				cnt[key] = at + (uint32_t)__popcll(mt);
		}
		asm volatile("" ::: "memory");
	}
}

/* ---- bounds ---- */

__global__ void __launch_bounds__(kUxThreads) ux_bounds_kernel(UxParams k)
{
	const uint32_t s = blockIdx.x * kUxThreads + threadIdx.x;

	if (s > k.nsock)
		return;
	const uint64_t t = ux_total(k);
	uint64_t lo = 0, hi = t; /* the first position in [0, t] whose key is >= s */

	while (lo < hi) { /* at most 32 rounds: t <= 2^31 */
		const uint64_t mid = lo + (hi - lo) / 2;
		if (k.skey[mid] < s)
			lo = mid + 1;
		else
			hi = mid;
	}
	k.start[s] = (uint32_t)lo;
}

/* ---- decide, top, emit ---- */

/* sorted position p < the total: its list position (below m), its socket (below nsock) and its rank in the run */
__device__ __forceinline__ void ux_at(const UxParams &k, const uint32_t *sorted, uint64_t p, uint32_t *j, uint32_t *s,
                                      uint32_t *rank)
{
	uint32_t jj = sorted[p], ss = k.skey[p];

	if (jj >= k.m)
		jj = (uint32_t)(k.m - 1);
	if (ss >= k.nsock)
		ss = k.nsock - 1;
	const uint32_t st = k.start[ss];
	*j = jj;
	*s = ss;
	*rank = p >= st ? (uint32_t)(p - st) : 0;
}

/* @v summed over the wave, in every lane; all lanes active */
__device__ __forceinline__ uint64_t ux_wave_sum(uint64_t v)
{
	for (int x = 32; x; x >>= 1) {
		const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, x);
		const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), x);
		v += (uint64_t)hi << 32 | lo;
	}
	return v;
}

__global__ void __launch_bounds__(kUxThreads) ux_decide_kernel(UxParams k, const uint32_t *sorted)
{
	__shared__ unsigned long long blk[2];
	const uint64_t t = ux_total(k);
	const uint64_t p0 = (uint64_t)blockIdx.x * kUxChunk;
	uint64_t cnt = 0, bytes = 0; /* this lane's positions */

	if (threadIdx.x < 2)
		blk[threadIdx.x] = 0;
	__syncthreads();
	for (uint32_t x = 0; x < kUxTiles; x++) {
		const uint64_t p = p0 + x * kUxThreads + threadIdx.x;
		if (p < t) {
			uint32_t j, s, rank, sf;
			ux_at(k, sorted, p, &j, &s, &rank);
			const uint4 u = k.usock[s];
			const uint32_t len = k.info[j].y >> 16;
			const uint32_t v = gcl_udprx_closed((int32_t)u.x, (int32_t)u.y, u.z & 0xFFu, rank, &sf);

			k.dv[p] = v | sf << 8 | len << 16;
			if (gcl_udprx_taken(v)) {
				cnt++;
				bytes += gcl_pay_pad(len, k.amask);
			}
		}
	}
	cnt = ux_wave_sum(cnt);
	bytes = ux_wave_sum(bytes);
	if ((threadIdx.x & 63) == 0) {
		atomicAdd(&blk[0], (unsigned long long)cnt);
		atomicAdd(&blk[1], (unsigned long long)bytes);
	}
	__syncthreads();
	if (threadIdx.x == 0) { /* every chunk stores its words, an empty one 0 */
		k.pcnt[blockIdx.x] = blk[0];
		k.poff[blockIdx.x] = blk[1];
	}
}

/* one block: pcnt and poff [0, nchunks) -> their exclusive scans; the totals */
__global__ void __launch_bounds__(kUxTopThreads) ux_top_kernel(UxParams k, uint32_t nchunks)
{
	const uint32_t per = (nchunks + kUxTopThreads - 1) / kUxTopThreads;
	const uint32_t i0 = threadIdx.x * per;

	for (uint32_t a = 0; a < 2; a++) { /* uniform */
		unsigned long long *v = a ? k.poff : k.pcnt, s = 0;

		for (uint32_t j = 0; j < per; j++)
			s += i0 + j < nchunks ? v[i0 + j] : 0;
		unsigned long long acc = ux_block_scan<unsigned long long, kUxTopThreads>(s, nullptr);
		for (uint32_t j = 0; j < per; j++) {
			if (i0 + j < nchunks) {
				const unsigned long long x = v[i0 + j];
				v[i0 + j] = acc;
				acc += x;
			}
		}
		if (threadIdx.x == kUxTopThreads - 1)
			k.ptot[a] = acc;
		__syncthreads(); /* the scan's LDS is used again */
	}
}

__global__ void __launch_bounds__(kUxThreads) ux_emit_kernel(UxParams k, const uint32_t *sorted)
{
	__shared__ uint32_t wt[2][2][kUxWaves];
	__shared__ unsigned long long blk[GCL_UDPRXC_NR];
	const uint64_t t = ux_total(k);
	const uint64_t p0 = (uint64_t)blockIdx.x * kUxChunk;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t below = (1ull << lane) - 1;
	uint64_t ccarry = k.pcnt[blockIdx.x], bcarry = k.poff[blockIdx.x]; /* the chunk's base, then the tiles before */
	uint32_t cnt[4] = {0, 0, 0, 0}, pollins = 0;                     /* wave-uniform */
	uint64_t bytes = 0;                                              /* this lane's positions */
	uint32_t par = 0;

	if (threadIdx.x < GCL_UDPRXC_NR)
		blk[threadIdx.x] = 0;
	for (uint32_t x = 0; x < kUxTiles; x++, par ^= 1) { /* uniform: every lane reaches the barrier */
		const uint64_t p = p0 + x * kUxThreads + threadIdx.x;
		const uint32_t d = p < t ? k.dv[p] : GCL_UDPRX_NA;
		const uint32_t v = d & 0xFFu, sf = (d >> 8) & 0xFFu, len = d >> 16;
		const bool taken = p < t && gcl_udprx_taken(v);
		const uint32_t own = taken ? gcl_pay_pad(len, k.amask) : 0;
		const uint64_t tm = __ballot(taken);
		uint32_t incl = own; /* a tile's padded bytes stay below 2^25 */

		for (int s = 1; s < 64; s <<= 1) {
			const uint32_t up = (uint32_t)__shfl_up((int)incl, s);
			if (lane >= (uint32_t)s)
				incl += up;
		}
		if (lane == 63) {
			wt[par][0][wave] = (uint32_t)__popcll(tm);
			wt[par][1][wave] = incl;
		}
		__syncthreads();
		uint64_t c = ccarry + (uint32_t)__popcll(tm & below), b = bcarry + (incl - own);
#pragma unroll
		for (uint32_t w = 0; w < kUxWaves; w++) {
			if (w < wave) {
				c += wt[par][0][w];
				b += wt[par][1][w];
			}
			ccarry += wt[par][0][w];
			bcarry += wt[par][1][w];
		}
#pragma unroll
		for (uint32_t y = 0; y < 4; y++)
			cnt[y] += (uint32_t)__popcll(__ballot(p < t && v == y));
		pollins += (uint32_t)__popcll(__ballot(p < t && (sf & GCL_UDPRX_SF_POLLIN)));
		if (p >= t)
			continue; /* the loop's own barrier is behind every lane of this tile */
		uint32_t j = sorted[p];
		if (j >= k.m)
			j = (uint32_t)(k.m - 1);
		k.sc_cnt[p] = (uint32_t)c;
		k.sc_off[p] = b;
		k.verdict[j] = (uint8_t)v;
		k.sflags[j] = (uint8_t)sf;
		k.copy_len[j] = (uint16_t)(taken ? len : 0);
		k.dst_off[j] = taken ? b : 0;
		k.rec_idx[j] = taken ? (uint32_t)c : GCL_UDPRX_NONE;
		if (taken) {
			const uint2 f = k.info[j];

			bytes += len;
			if (c < k.m) /* c < the datagrams <= m */
				k.rec[c] = make_uint4((uint32_t)b, (uint32_t)(b >> 32), f.x, f.y);
		}
	}
	if (!k.counts)
		return;
	__syncthreads(); /* blk was cleared; with no tile no barrier came before */
	bytes = ux_wave_sum(bytes);
	if (lane == 0) {
#pragma unroll
		for (uint32_t y = 0; y < 4; y++)
			atomicAdd(&blk[y], (unsigned long long)cnt[y]);
		atomicAdd(&blk[GCL_UDPRXC_BYTES], (unsigned long long)bytes);
		atomicAdd(&blk[GCL_UDPRXC_POLLINS], (unsigned long long)pollins);
	}
	__syncthreads();
	if (threadIdx.x < GCL_UDPRXC_NR && blk[threadIdx.x])
		atomicAdd(k.counts + threadIdx.x, blk[threadIdx.x]);
}

/* ---- socks ---- */

__global__ void __launch_bounds__(kUxThreads) ux_socks_kernel(UxParams k)
{
	const uint32_t s = blockIdx.x * kUxThreads + threadIdx.x;

	if (s > k.nsock)
		return;
	const uint64_t t = k.m ? ux_total(k) : 0; /* m == 0: nothing ran before this launch */
	uint64_t a = 0, e = 0;
	unsigned long long c = 0, b = 0;

	if (t) {
		a = k.start[s] < t ? k.start[s] : t;
		e = s < k.nsock ? k.start[s + 1] : t;
		e = e < a ? a : e < t ? e : t;
		if (a < t) {
			c = k.sc_cnt[a];
			b = k.sc_off[a];
		} else {
			c = k.ptot[0];
			b = k.ptot[1];
		}
	}
	k.rec_off[s] = (uint32_t)c;
	k.sock_off[s] = b;
	if (s < k.nsock) {
		const uint4 u = k.usock[s];
		uint32_t o[4];

		gcl_udprx_after((int32_t)u.x, (int32_t)u.y, u.z & 0xFFu, (uint32_t)(e - a), o);
		k.out_sock[s] = make_uint4(o[0], o[1], o[2], o[3]);
	}
}

/* ---- the workspace ---- */

struct UxGeom {
	uint32_t passes, nb[2], kbits[2];
	uint32_t ranges; /* as sized: in->blocks or the cap */
	size_t info, key, idx[2], skey, dv, sc_cnt, sc_off, hist, csum, pcnt, poff, tot, ptot, start, bytes;
};

static size_t ux_up16(size_t x)
{
	return (x + 15) & ~(size_t)15;
}

static uint32_t ux_bits(uint32_t nb)
{
	return nb > 1 ? 32 - (uint32_t)__builtin_clz(nb - 1) : 0;
}

static int ux_geometry(uint64_t m, uint32_t nsock, uint32_t blocks, UxGeom *g)
{
	if (m > (1ull << 31) || nsock > GCL_SOCK_MAX_ENTRIES || blocks > GCL_UDPRX_MAX_BLOCKS)
		return -EINVAL;
	g->passes = nsock > kUxDigits ? 2 : 1;
	g->nb[0] = nsock > kUxDigits ? kUxDigits : nsock ? nsock : 1;
	g->nb[1] = g->passes == 2 ? ((nsock - 1) >> kUxDigitBits) + 1 : 0;
	g->kbits[0] = ux_bits(g->nb[0]);
	g->kbits[1] = ux_bits(g->nb[1]);
	/* the library's choice never exceeds one range per 256 entries, nor the cap */
	const uint64_t tiles = (m + kUxThreads - 1) / kUxThreads;
	g->ranges = blocks ? blocks : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, GCL_UDPRX_MAX_BLOCKS));
	const size_t entries = (size_t)std::max(g->nb[0], g->nb[1]) * g->ranges;
	const size_t chunks = ((size_t)m + kUxChunk - 1) / kUxChunk;
	size_t at = 0;
	g->info = at;
	at += ux_up16(8 * (size_t)m);
	g->sc_off = at;
	at += ux_up16(8 * (size_t)m);
	g->key = at;
	at += ux_up16(4 * (size_t)m);
	g->idx[0] = at;
	at += ux_up16(4 * (size_t)m);
	g->idx[1] = at;
	at += g->passes == 2 ? ux_up16(4 * (size_t)m) : 0;
	g->skey = at;
	at += ux_up16(4 * (size_t)m);
	g->dv = at;
	at += ux_up16(4 * (size_t)m);
	g->sc_cnt = at;
	at += ux_up16(4 * (size_t)m);
	g->hist = at;
	at += ux_up16(4 * entries);
	g->csum = at;
	at += ux_up16(4 * ((entries + kUxChunk - 1) / kUxChunk));
	g->pcnt = at;
	at += ux_up16(8 * chunks);
	g->poff = at;
	at += ux_up16(8 * chunks);
	g->tot = at;
	at += 16;
	g->ptot = at;
	at += 16;
	g->start = at;
	at += ux_up16(4 * ((size_t)nsock + 1));
	g->bytes = at;
	return 0;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_udp_rx_workspace(uint64_t m, uint32_t nsock, uint32_t blocks, size_t *bytes)
{
	UxGeom g;

	if (!bytes || ux_geometry(m, nsock, blocks, &g))
		return -EINVAL;
	*bytes = g.bytes;
	return 0;
}

extern "C" int gcl_udp_rx(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_udprx_in *in,
                          const struct gcl_udprx_out *out, uint64_t *counts, void *workspace,
                          size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	UxGeom g;

	if (!c || gcl_udprx_refused(b, in, out, counts) || ux_geometry(in->m, in->nsock, in->blocks, &g))
		return -EINVAL;
	if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < g.bytes)
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	uint8_t *ws = (uint8_t *)workspace;
	UxParams k;
	k.frames = b->frames;
	k.frames_len = b->frames_len;
	k.stride = b->stride;
	k.offs = b->offs;
	k.pkt_len = b->pkt_len;
	k.n = b->n;
	k.order = in->order;
	k.sock = in->sock;
	k.l4_status = in->l4_status;
	k.usock = (const uint4 *)in->usock;
	k.verdict = out->verdict;
	k.sflags = out->sflags;
	k.copy_len = out->copy_len;
	k.dst_off = out->dst_off;
	k.rec_idx = out->rec_idx;
	k.rec = (uint4 *)out->rec;
	k.out_sock = (uint4 *)out->out_sock;
	k.rec_off = out->rec_off;
	k.sock_off = (unsigned long long *)out->sock_off;
	k.counts = (unsigned long long *)counts;
	k.info = (uint2 *)(ws + g.info);
	k.key = (uint32_t *)(ws + g.key);
	k.idx[0] = (uint32_t *)(ws + g.idx[0]);
	k.idx[1] = (uint32_t *)(ws + g.idx[1]);
	k.skey = (uint32_t *)(ws + g.skey);
	k.dv = (uint32_t *)(ws + g.dv);
	k.sc_cnt = (uint32_t *)(ws + g.sc_cnt);
	k.sc_off = (unsigned long long *)(ws + g.sc_off);
	k.hist = (uint32_t *)(ws + g.hist);
	k.csum = (uint32_t *)(ws + g.csum);
	k.pcnt = (unsigned long long *)(ws + g.pcnt);
	k.poff = (unsigned long long *)(ws + g.poff);
	k.tot = (uint32_t *)(ws + g.tot);
	k.ptot = (unsigned long long *)(ws + g.ptot);
	k.start = (uint32_t *)(ws + g.start);
	k.m = in->m;
	k.nsock = in->nsock;
	k.sock_base = in->sock_base;
	k.amask = in->align ? in->align - 1 : 0;

	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);
	const uint64_t tiles = (in->m + kUxThreads - 1) / kUxThreads;
	const unsigned egrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)cus * 8));
	const dim3 sgrid(in->nsock / kUxThreads + 1); /* nsock + 1 lanes */
	k.ranges = in->blocks ? in->blocks :
	           (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::min<uint32_t>(cus * kUxBlocksPerCu,
	                                                                                      GCL_UDPRX_MAX_BLOCKS)));
	k.range_len = (uint32_t)(((in->m + k.ranges - 1) / k.ranges + 63) / 64 * 64);
	if (k.range_len == 0)
		k.range_len = 64;

	if (in->m == 0) { /* every socket gets its input back; the offsets are 0 */
		hipLaunchKernelGGL(ux_socks_kernel, sgrid, dim3(kUxThreads), 0, s, k);
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	hipLaunchKernelGGL(ux_parse_kernel, dim3(egrid), dim3(kUxThreads), 0, s, k);
	if (in->nsock == 0) { /* every datagram is NOSOCK: nothing to group or lay out */
		if (hipMemsetAsync(out->rec_off, 0, sizeof(uint32_t), s) != hipSuccess ||
		    hipMemsetAsync(out->sock_off, 0, sizeof(uint64_t), s) != hipSuccess)
			return -EIO;
		return hipGetLastError() == hipSuccess ? 0 : -EIO;
	}
	const uint32_t *sorted = k.idx[g.passes - 1];
	for (uint32_t p = 0; p < g.passes; p++) {
		const UxPass ps = {p ? k.idx[0] : nullptr, k.idx[p], p + 1 == g.passes ? k.skey : nullptr, p * kUxDigitBits,
		                   g.nb[p], g.kbits[p]};
		const dim3 grid((k.ranges + kUxWaves - 1) / kUxWaves);
		const uint32_t total = ps.nb * k.ranges, nchunks = (total + kUxChunk - 1) / kUxChunk;

		hipLaunchKernelGGL(ux_count_kernel, grid, dim3(kUxThreads), 0, s, k, ps);
		hipLaunchKernelGGL(ux_hist_sum_kernel, dim3(nchunks), dim3(kUxThreads), 0, s, k, total);
		hipLaunchKernelGGL(ux_hist_top_kernel, dim3(1), dim3(kUxTopThreads), 0, s, k, nchunks);
		hipLaunchKernelGGL(ux_hist_apply_kernel, dim3(nchunks), dim3(kUxThreads), 0, s, k, total);
		hipLaunchKernelGGL(ux_scatter_kernel, grid, dim3(kUxThreads), 0, s, k, ps);
	}
	/* the positions the last three launches cover: the datagrams are at most m */
	const uint32_t pchunks = (uint32_t)((in->m + kUxChunk - 1) / kUxChunk);

	hipLaunchKernelGGL(ux_bounds_kernel, sgrid, dim3(kUxThreads), 0, s, k);
	hipLaunchKernelGGL(ux_decide_kernel, dim3(pchunks), dim3(kUxThreads), 0, s, k, sorted);
	hipLaunchKernelGGL(ux_top_kernel, dim3(1), dim3(kUxTopThreads), 0, s, k, pchunks);
	hipLaunchKernelGGL(ux_emit_kernel, dim3(pchunks), dim3(kUxThreads), 0, s, k, sorted);
	hipLaunchKernelGGL(ux_socks_kernel, sgrid, dim3(kUxThreads), 0, s, k);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
