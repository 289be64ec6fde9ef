/*
 * gcl_tcpread.hip - tcp_read and tcp_readv for a batch of connections
 * (gcl_tcp_read, gclassify.h): tcp_wait_rx, tcp_read_wait, tcp_read_wait_peek
 * and the copies of copy_mbufs_to_buf / copy_into_iov (runtime/net/tcp.c:
 * 850-934, :963-988, :1013-1038, :1133-1185) for every connection of one
 * runtime at one instant, with the window-update ACKs of tcp_tx_ack.  The
 * parts of the rule that are not a walk are those of gcl_tcpread.h, the same
 * inline code the host twin runs; the walks are replaced by their closed
 * form over prefix sums, so that no launch walks a queue: one connection may
 * own every entry.
 *
 * Seven launches on the stream; no block waits for another and no atomic hands
 * out a position.  Every sweep is cut into `blocks` contiguous ranges of whole
 * 256-element tiles.
 *
 *   scan sum    grid (blocks, 1 or 2): y = 0 the queue entries, y = 1 the
 *               vectors.  Block r sums its range of (bytes u64, FIN entries,
 *               zero-length FIN entries).
 *   scan top    one block per array: the range sums -> their exclusive prefix
 *               sums, in place.
 *   scan apply  block r walks its range tile by tile with a carry and writes
 *               the exclusive prefix sums P[e] (bytes), FZ[e] (the two
 *               counts) for e in [0, nent], Q[v] for v in [0, nvec].  The
 *               scan is global and unsegmented: A_i of connection c is
 *               P[qoff[c] + i] - P[qoff[c]].
 *   decide      one lane per connection: binary searches over its slice of P
 *               and FZ give z, npop, pull, ret, ne and nv; the FIN counts
 *               give RX_CLOSED.  It writes out_conn[c] with the items it wants
 *               in nitems, ne and nv to the workspace, and the range's sums of
 *               (items, ACKs, positive ret).
 *   top         one block: the exclusive prefix sums of the range sums, both
 *               totals.
 *   place       one lane per connection again: its first item and its ACK's
 *               position from the range's base and a block scan per tile;
 *               first_item, nitems, the NOSPACE flags, its ACK, the counts.
 *   items       one lane per item k < totals[1], tiles dealt round robin: the
 *               connection by binary search over first_item (monotone and
 *               written by place, so no input bends it), then entry i and
 *               vector j by a merge-path search over the two slices.
 *
 * Bounds.  A connection index is used only below nconn; an entry index only
 * inside a range gcl_rd_range found inside [0, nent], P and FZ up to nent; a
 * vector index likewise with nvec and Q; an item index only below item_cap, a
 * segment index only below seg_cap; a range-sum word only below blocks.  The
 * items launch checks ne, nv and the item's number against the ranges it
 * reads again before it uses them.  No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_tcpread.h"
#include "gcl_tcptmr.h"

namespace gclk {

constexpr uint32_t kRdThreads = 256;
constexpr uint32_t kRdWaves = kRdThreads / 64;
constexpr uint32_t kRdBlocksPerCu = 4;
constexpr uint32_t kRdTopPer = GCL_RD_MAX_BLOCKS / kRdThreads;
static_assert(kRdTopPer * kRdThreads == GCL_RD_MAX_BLOCKS, "the top kernels are one block");
static_assert(sizeof(struct gcl_tcp_rd) == 32 && sizeof(struct gcl_rdq_ent) == 16 && sizeof(struct gcl_rd_iov) == 16 &&
              sizeof(struct gcl_rd_conn_out) == 32 && sizeof(struct gcl_tcp_conn) == 48 &&
              sizeof(struct gcl_tcp_addr) == 16 && sizeof(struct gcl_txh_desc) == 32, "records as 16-B words");

/* what the scans add up: a 64-bit sum and two counts */
struct RdTri {
	uint64_t a;
	uint32_t b, c;
};

struct RdParams {
	struct gcl_rd_out out;
	const uint32_t *qoff, *voff;
	const uint4 *ent, *iov;  /* struct gcl_rdq_ent, gcl_rd_iov as 16-B words */
	const uint4 *rd;         /* struct gcl_tcp_rd as two 16-B words */
	const uint4 *conn;       /* struct gcl_tcp_conn as three */
	const uint4 *addr;
	unsigned long long *counts;
	/* workspace */
	uint64_t *P;             /* [nent + 1]: the bytes of the entries before */
	uint2 *FZ;               /* [nent + 1]: the FIN and the zero-length FIN entries before */
	uint64_t *Q;             /* [nvec + 1] */
	uint4 *ssum;             /* [2][blocks]: a range's sums, then the sums before it */
	uint4 *bsum;             /* [blocks]: items (64 bits), ACKs */
	uint64_t *rsum;          /* [blocks]: positive ret */
	uint32_t *wne, *wnv, *wfirst; /* [nconn] */
	uint64_t nent, nvec, item_cap, seg_cap, frame_base;
	uint64_t per_e, per_v, per_c; /* elements per range, multiples of kRdThreads */
	uint32_t nconn, frame_stride, blocks;
};

__device__ __forceinline__ RdTri rd_add(const RdTri &x, const RdTri &y)
{
	return RdTri{x.a + y.a, x.b + y.b, x.c + y.c};
}

__device__ __forceinline__ RdTri rd_tri(const uint4 &v)
{
	return RdTri{(uint64_t)v.y << 32 | v.x, v.z, v.w};
}

__device__ __forceinline__ uint4 rd_word(const RdTri &t)
{
	return make_uint4((uint32_t)t.a, (uint32_t)(t.a >> 32), t.b, t.c);
}

/*
 * The exclusive prefix sums of @v over the block's lanes, and the block's sum
 * in *@total.  Every lane of the block calls it.
 */
__device__ __forceinline__ RdTri rd_block_scan(const RdTri &v, RdTri *total)
{
	__shared__ RdTri ws[kRdWaves];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	RdTri inc = v;

#pragma unroll
	for (uint32_t s = 1; s < 64; s <<= 1) {
		RdTri t;
		t.a = (uint64_t)__shfl_up((uint32_t)(inc.a >> 32), s) << 32 | __shfl_up((uint32_t)inc.a, s);
		t.b = __shfl_up(inc.b, s);
		t.c = __shfl_up(inc.c, s);
		if (lane >= s)
			inc = rd_add(inc, t);
	}
	__syncthreads(); /* the reads of the call before */
	if (lane == 63)
		ws[wave] = inc;
	__syncthreads();
	RdTri base = {0, 0, 0}, tot = {0, 0, 0};
#pragma unroll
	for (uint32_t w = 0; w < kRdWaves; w++) {
		const RdTri t = ws[w];
		if (w < wave)
			base = rd_add(base, t);
		tot = rd_add(tot, t);
	}
	*total = tot;
	return RdTri{base.a + inc.a - v.a, base.b + inc.b - v.b, base.c + inc.c - v.c};
}

__device__ __forceinline__ uint64_t rd_wave_sum(uint64_t v)
{
#pragma unroll
	for (int s = 32; s; s >>= 1)
		v += (uint64_t)__shfl_xor((uint32_t)(v >> 32), s) << 32 | __shfl_xor((uint32_t)v, s);
	return v;
}

/* element @e of the entries (@which 0) or the vectors as the scans count it */
__device__ __forceinline__ RdTri rd_elem(const RdParams &p, uint32_t which, uint64_t e)
{
	if (which) {
		const uint4 v = p.iov[e];
		return RdTri{v.z, 0, 0};
	}
	const uint4 v = p.ent[e];
	const uint32_t len = v.z & 0xFFFFu, fin = (v.z >> 16) & GCL_RDQE_FIN;
	return RdTri{len, fin ? 1u : 0u, fin && len == 0 ? 1u : 0u};
}

__global__ void __launch_bounds__(kRdThreads) rd_scan_sum_kernel(RdParams p)
{
	const uint32_t which = blockIdx.y;
	const uint64_t total = which ? p.nvec : p.nent, per = which ? p.per_v : p.per_e;
	const uint64_t lo = std::min<uint64_t>((uint64_t)blockIdx.x * per, total), hi = std::min<uint64_t>(lo + per, total);
	RdTri acc = {0, 0, 0}, tot;

	for (uint64_t e = lo + threadIdx.x; e < hi; e += kRdThreads)
		acc = rd_add(acc, rd_elem(p, which, e));
	rd_block_scan(acc, &tot);
	if (threadIdx.x == 0)
		p.ssum[which * p.blocks + blockIdx.x] = rd_word(tot);
}

/* @sum[0, blocks) -> its exclusive prefix sums in place; returns the sum of all.  One block. */
__device__ __forceinline__ RdTri rd_top_scan(uint4 *sum, uint32_t blocks)
{
	const uint32_t t = threadIdx.x;
	RdTri v[kRdTopPer], mine = {0, 0, 0}, tot;

#pragma unroll
	for (uint32_t x = 0; x < kRdTopPer; x++) {
		const uint32_t r = t * kRdTopPer + x;
		v[x] = r < blocks ? rd_tri(sum[r]) : RdTri{0, 0, 0};
		mine = rd_add(mine, v[x]);
	}
	RdTri base = rd_block_scan(mine, &tot);
#pragma unroll
	for (uint32_t x = 0; x < kRdTopPer; x++) {
		const uint32_t r = t * kRdTopPer + x;
		if (r < blocks)
			sum[r] = rd_word(base);
		base = rd_add(base, v[x]);
	}
	return tot;
}

__global__ void __launch_bounds__(kRdThreads) rd_scan_top_kernel(RdParams p)
{
	rd_top_scan(p.ssum + blockIdx.x * p.blocks, p.blocks);
}

__global__ void __launch_bounds__(kRdThreads) rd_scan_apply_kernel(RdParams p)
{
	const uint32_t which = blockIdx.y;
	const uint64_t total = which ? p.nvec : p.nent, per = which ? p.per_v : p.per_e;
	const uint64_t lo = std::min<uint64_t>((uint64_t)blockIdx.x * per, total), hi = std::min<uint64_t>(lo + per, total);
	RdTri carry = rd_tri(p.ssum[which * p.blocks + blockIdx.x]);

	for (uint64_t j0 = lo; j0 < hi; j0 += kRdThreads) { /* uniform: every lane reaches the barriers */
		const uint64_t e = j0 + threadIdx.x;
		const bool in = e < hi;
		RdTri tot;
		const RdTri ex = rd_block_scan(in ? rd_elem(p, which, e) : RdTri{0, 0, 0}, &tot);

		if (in) {
			if (which) {
				p.Q[e] = carry.a + ex.a;
			} else {
				p.P[e] = carry.a + ex.a;
				p.FZ[e] = make_uint2(carry.b + ex.b, carry.c + ex.c);
			}
		}
		carry = rd_add(carry, tot);
	}
	/* the element behind the last: the range that ends the array, or block 0 of an empty one */
	if (threadIdx.x == 0 && hi == total && (lo < hi || (total == 0 && blockIdx.x == 0))) {
		if (which) {
			p.Q[total] = carry.a;
		} else {
			p.P[total] = carry.a;
			p.FZ[total] = make_uint2(carry.b, carry.c);
		}
	}
}

/* the smallest i in [lo, hi] with S[base + i] - S[base] >= want; hi is taken to hold it */
__device__ __forceinline__ uint32_t rd_lower(const uint64_t *S, uint64_t base, uint32_t lo, uint32_t hi, uint64_t want)
{
	const uint64_t s0 = S[base];

	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (S[base + mid] - s0 >= want)
			hi = mid;
		else
			lo = mid + 1;
	}
	return lo;
}

/* a connection's two ranges and its read's length */
struct RdConn {
	uint64_t L;
	uint32_t e0, n, v0, m, bad;
};

__device__ __forceinline__ RdConn rd_ranges(const RdParams &p, uint32_t c, uint32_t rd_len)
{
	RdConn t;

	t.bad = 0;
	t.v0 = 0;
	t.m = 1;
	t.L = rd_len;
	t.n = gcl_rd_range(p.qoff[c], p.qoff[c + 1], p.nent, &t.e0, &t.bad);
	if (p.voff) {
		t.m = gcl_rd_range(p.voff[c], p.voff[c + 1], p.nvec, &t.v0, &t.bad);
		t.L = p.Q[(uint64_t)t.v0 + t.m] - p.Q[t.v0];
	}
	return t;
}

__global__ void __launch_bounds__(kRdThreads) rd_decide_kernel(RdParams p)
{
	const uint64_t lo = std::min<uint64_t>((uint64_t)blockIdx.x * p.per_c, p.nconn);
	const uint64_t hi = std::min<uint64_t>(lo + p.per_c, p.nconn);
	RdTri acc = {0, 0, 0}, tot, rtot;
	uint64_t retsum = 0;

	for (uint64_t c64 = lo + threadIdx.x; c64 < hi; c64 += kRdThreads) {
		const uint32_t c = (uint32_t)c64;
		const uint4 r0 = p.rd[2 * (size_t)c], r1 = p.rd[2 * (size_t)c + 1], c1 = p.conn[3 * (size_t)c + 1];
		const uint32_t rdflags = r1.w & 0xFFu, rcv_nxt = c1.y, rcv_wnd = c1.z;
		const RdConn t = rd_ranges(p, c, r0.z);
		const uint64_t e0 = t.e0;
		struct gcl_rd_res r;
		uint32_t w[8];

		if (gcl_rd_wait(rdflags, t.n, (int32_t)r1.z, t.bad, rcv_wnd, &r)) {
			const uint64_t p0 = p.P[e0], An = p.P[e0 + t.n] - p0;

			if (rdflags & GCL_RD_PEEK) {
				gcl_rd_peek_done(&r, An < t.L ? An : t.L);
			} else {
				const uint2 f0 = p.FZ[e0];
				uint32_t z = t.n, npop, pull = 0;
				uint64_t readlen;

				if (p.FZ[e0 + t.n].y != f0.y) { /* the first zero-length FIN entry */
					uint32_t a = 1, b = t.n;
					while (a < b) {
						const uint32_t mid = a + (b - a) / 2;
						if (p.FZ[e0 + mid].y != f0.y)
							b = mid;
						else
							a = mid + 1;
					}
					z = a - 1;
				}
				const uint64_t Az = p.P[e0 + z] - p0;
				if (Az >= t.L) {
					const uint32_t i = rd_lower(p.P, e0, 0, z, t.L);
					npop = i;
					readlen = t.L;
					if (p.P[e0 + i] - p0 > t.L) { /* i >= 1: A_0 = 0 */
						npop = i - 1;
						pull = (uint32_t)(t.L - (p.P[e0 + npop] - p0));
					}
				} else {
					npop = z;
					readlen = Az;
				}
				/* the entries the walk looked at as the top of the queue */
				const uint32_t exam = npop + ((t.L > 0 && npop < t.n && (pull || Az < t.L)) ? 1u : 0u);
				gcl_rd_read_done(&r, readlen, npop, pull, p.FZ[e0 + exam].x != f0.x, t.n, rcv_nxt, r0.w, r1.x,
				                 r1.y);
			}
			if (r.ret > 0) {
				r.ne = rd_lower(p.P, e0, 1, t.n, (uint64_t)r.ret);
				r.nv = p.voff ? rd_lower(p.Q, t.v0, 1, t.m, (uint64_t)r.ret) : 1;
				r.nitems = (uint64_t)r.ne + r.nv - 1;
				retsum += (uint64_t)r.ret;
			}
		}
		gcl_rd_conn_words(&r, 0, (uint32_t)r.nitems, r.flags, w);
		uint4 *o = (uint4 *)&p.out.out_conn[c];
		o[0] = make_uint4(w[0], w[1], w[2], w[3]);
		o[1] = make_uint4(w[4], w[5], w[6], w[7]);
		p.wne[c] = r.ne;
		p.wnv[c] = r.nv;
		acc.a += r.nitems;
		acc.b += (r.flags & GCL_RDO_ACK) ? 1u : 0u;
	}
	rd_block_scan(acc, &tot);
	rd_block_scan(RdTri{retsum, 0, 0}, &rtot);
	if (threadIdx.x == 0) {
		p.bsum[blockIdx.x] = rd_word(tot);
		p.rsum[blockIdx.x] = rtot.a;
	}
}

__global__ void __launch_bounds__(kRdThreads) rd_top_kernel(RdParams p)
{
	RdTri mine = {0, 0, 0}, rtot;

	for (uint32_t r = threadIdx.x; r < p.blocks; r += kRdThreads)
		mine.a += p.rsum[r];
	rd_block_scan(mine, &rtot);
	const RdTri tot = rd_top_scan(p.bsum, p.blocks);
	if (threadIdx.x == 0) {
		p.out.totals[0] = tot.a;
		p.out.totals[1] = tot.a < p.item_cap ? tot.a : p.item_cap;
		p.out.totals[2] = 0; /* the items launch adds the bytes */
		p.out.totals[3] = rtot.a;
		p.out.seg.totals[0] = tot.b;
		p.out.seg.totals[1] = tot.b < p.seg_cap ? tot.b : p.seg_cap;
	}
}

/* the lanes' counters -> counts */
__device__ __forceinline__ void rd_flush(const RdParams &p, uint64_t cnt[GCL_RDC_NR])
{
	if (!p.counts)
		return;
#pragma unroll
	for (uint32_t x = 0; x < GCL_RDC_NR; x++) {
		const uint64_t s = rd_wave_sum(cnt[x]);
		if ((threadIdx.x & 63) == 0 && s)
			atomicAdd(p.counts + x, (unsigned long long)s);
	}
}

__global__ void __launch_bounds__(kRdThreads) rd_place_kernel(RdParams p)
{
	const uint64_t lo = std::min<uint64_t>((uint64_t)blockIdx.x * p.per_c, p.nconn);
	const uint64_t hi = std::min<uint64_t>(lo + p.per_c, p.nconn);
	RdTri carry = rd_tri(p.bsum[blockIdx.x]);
	uint64_t cnt[GCL_RDC_NR] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

	for (uint64_t j0 = lo; j0 < hi; j0 += kRdThreads) { /* uniform: every lane reaches the barriers */
		const uint64_t c64 = j0 + threadIdx.x;
		const bool live = c64 < hi;
		const uint32_t c = (uint32_t)c64;
		uint4 w0 = make_uint4(0, 0, 0, 0), w1 = w0;
		RdTri tot;

		if (live) {
			w0 = ((const uint4 *)&p.out.out_conn[c])[0];
			w1 = ((const uint4 *)&p.out.out_conn[c])[1];
		}
		const uint32_t want = w1.z, status = w1.w & 0xFFu;
		uint32_t flags = (w1.w >> 8) & 0xFFu;
		const bool ack = (flags & GCL_RDO_ACK) != 0;
		const RdTri ex = rd_block_scan(RdTri{want, ack ? 1u : 0u, 0}, &tot);

		if (live) {
			const uint64_t at = carry.a + ex.a, k = (uint64_t)carry.b + ex.b;
			const uint64_t first = at < p.item_cap ? at : p.item_cap;
			const uint64_t room = p.item_cap - first;
			const uint32_t written = want < room ? want : (uint32_t)room;

			if (written < want)
				flags |= GCL_RDO_ITEM_NOSPACE;
			if (ack) {
				if (k < p.seg_cap) {
					const uint4 c0 = p.conn[3 * (size_t)c], c1 = p.conn[3 * (size_t)c + 1], ad = p.addr[c];
					const uint32_t a[4] = {ad.x, ad.y, ad.z, ad.w};
					uint32_t d[8];

					gcl_ctl_desc(a, c0.y, c1.y, w1.x, d); /* snd_nxt, rcv_nxt, rcv_wnd after the read */
					((uint4 *)&p.out.seg.desc[k])[0] = make_uint4(d[0], d[1], d[2], d[3]);
					((uint4 *)&p.out.seg.desc[k])[1] = make_uint4(d[4], d[5], d[6], d[7]);
					p.out.seg.frame_off[k] = p.frame_base + k * p.frame_stride;
					p.out.seg.seg_conn[k] = c;
					p.out.seg.seg_kind[k] = GCL_CTL_ACK;
					p.out.seg.seg_src[k] = c;
					cnt[GCL_RDC_ACKS]++;
				} else {
					flags |= GCL_RDO_SEG_NOSPACE;
				}
			}
			((uint4 *)&p.out.out_conn[c])[1] = make_uint4(w1.x, (uint32_t)first, written, status | flags << 8);
			p.wfirst[c] = (uint32_t)first;
			cnt[GCL_RDC_DONE] += status == GCL_RDS_DONE;
			cnt[GCL_RDC_AGAIN] += status == GCL_RDS_AGAIN;
			cnt[GCL_RDC_BLOCK] += status == GCL_RDS_BLOCK;
			cnt[GCL_RDC_CLOSED] += status == GCL_RDS_CLOSED;
			cnt[GCL_RDC_PEEKS] += status == GCL_RDS_DONE && (p.rd[2 * (size_t)c + 1].w & GCL_RD_PEEK);
			cnt[GCL_RDC_POPPED] += w0.z;
			cnt[GCL_RDC_PARTIAL] += (flags & GCL_RDO_PARTIAL) ? 1 : 0;
			cnt[GCL_RDC_RX_CLOSED] += (flags & GCL_RDO_RX_CLOSED) ? 1 : 0;
			cnt[GCL_RDC_ITEMS] += written;
			cnt[GCL_RDC_NOSPACE] += (flags & (GCL_RDO_SEG_NOSPACE | GCL_RDO_ITEM_NOSPACE)) ? 1 : 0;
		}
		carry = rd_add(carry, tot);
	}
	rd_flush(p, cnt);
}

__global__ void __launch_bounds__(kRdThreads) rd_items_kernel(RdParams p)
{
	const uint64_t total = p.out.totals[1]; /* min(wanted, item_cap), from the top launch */
	uint64_t bytes = 0;

	for (uint64_t k = (uint64_t)blockIdx.x * kRdThreads + threadIdx.x; k < total; k += (uint64_t)gridDim.x * kRdThreads) {
		/* the last connection whose first item is not past k: wfirst[0] == 0 */
		uint32_t a = 0, b = p.nconn - 1;
		while (a < b) {
			const uint32_t mid = a + (b - a + 1) / 2;
			if (p.wfirst[mid] <= k)
				a = mid;
			else
				b = mid - 1;
		}
		const uint32_t c = a, ne = p.wne[c], nv = p.wnv[c];
		const uint64_t t64 = k - p.wfirst[c];
		const uint4 r0 = p.rd[2 * (size_t)c], o0 = ((const uint4 *)&p.out.out_conn[c])[0];
		const uint64_t ret = (uint64_t)o0.y << 32 | o0.x;
		const RdConn q = rd_ranges(p, c, r0.z);

		/* what decide made of the same ranges; checked, not trusted */
		if (q.bad || ne == 0 || nv == 0 || ne > q.n || nv > q.m || t64 >= (uint64_t)ne + nv - 1)
			continue;
		const uint32_t t = (uint32_t)t64;
		const uint64_t e0 = q.e0, v0 = q.v0, p0 = p.P[e0], q0 = p.voff ? p.Q[v0] : 0;
		/* merge path: i entry cuts and j = t - i vector cuts lie before item t; at a tie the entry cut first */
		uint32_t lo = t > nv - 1 ? t - (nv - 1) : 0, hi = t < ne - 1 ? t : ne - 1;
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (p.P[e0 + mid + 1] - p0 <= p.Q[v0 + (t - mid)] - q0) /* reached only with voff: nv > 1 */
				lo = mid + 1;
			else
				hi = mid;
		}
		const uint32_t i = lo, j = t - lo;
		const uint64_t ea = p.P[e0 + i] - p0, vb = j ? p.Q[v0 + j] - q0 : 0;
		const uint64_t ee = i < ne - 1 ? p.P[e0 + i + 1] - p0 : ret;
		const uint64_t ve = j < nv - 1 ? p.Q[v0 + j + 1] - q0 : ret;
		const uint64_t from = ea > vb ? ea : vb, to = ee < ve ? ee : ve;
		const uint4 ev = p.ent[e0 + i];
		uint64_t voff = (uint64_t)r0.y << 32 | r0.x;

		if (p.voff) {
			const uint4 vv = p.iov[v0 + j];
			voff = (uint64_t)vv.y << 32 | vv.x;
		}
		gcl_rd_item_store(&p.out, k, c, (uint32_t)(e0 + i), (uint64_t)ev.y << 32 | ev.x, ea, voff, vb, from, to);
		bytes += (to - from) & 0xFFFFu;
	}
	bytes = rd_wave_sum(bytes);
	if ((threadIdx.x & 63) == 0 && bytes) {
		atomicAdd((unsigned long long *)p.out.totals + 2, (unsigned long long)bytes);
		if (p.counts)
			atomicAdd(p.counts + GCL_RDC_BYTES, (unsigned long long)bytes);
	}
}

static bool rd_misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

static size_t rd_r16(size_t b)
{
	return (b + 15) & ~(size_t)15;
}

/* the workspace's parts, in order; returns its size */
static size_t rd_carve(RdParams *p, char *base, uint32_t nconn, uint64_t nent, uint64_t nvec, uint32_t blocks)
{
	const size_t nb = blocks ? blocks : GCL_RD_MAX_BLOCKS;
	size_t at = 0;

	if (p) p->P = (uint64_t *)(base + at);
	at += rd_r16(8 * (size_t)(nent + 1));
	if (p) p->FZ = (uint2 *)(base + at);
	at += rd_r16(8 * (size_t)(nent + 1));
	if (p) p->Q = (uint64_t *)(base + at);
	at += rd_r16(8 * (size_t)(nvec + 1));
	if (p) p->ssum = (uint4 *)(base + at);
	at += 2 * 16 * nb;
	if (p) p->bsum = (uint4 *)(base + at);
	at += 16 * nb;
	if (p) p->rsum = (uint64_t *)(base + at);
	at += rd_r16(8 * nb);
	if (p) p->wne = (uint32_t *)(base + at);
	at += rd_r16(4 * (size_t)nconn);
	if (p) p->wnv = (uint32_t *)(base + at);
	at += rd_r16(4 * (size_t)nconn);
	if (p) p->wfirst = (uint32_t *)(base + at);
	at += rd_r16(4 * (size_t)nconn);
	return at;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tcp_read_workspace(uint32_t nconn, uint64_t nent, uint64_t nvec, uint32_t blocks, size_t *bytes)
{
	if (!bytes || nconn > GCL_RD_MAX_CONN || nent > (1ull << 31) || nvec > (1ull << 31) || blocks > GCL_RD_MAX_BLOCKS)
		return -EINVAL;
	*bytes = rd_carve(nullptr, nullptr, nconn, nent, nvec, blocks);
	return 0;
}

extern "C" int gcl_tcp_read(struct gcl_ctx *c, const struct gcl_rd_in *in, const struct gcl_rd_out *out,
                            uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !in || !out || in->size != sizeof(*in) || in->nconn > GCL_RD_MAX_CONN ||
	    in->blocks > GCL_RD_MAX_BLOCKS || in->nent > (1ull << 31) || in->item_cap > (1ull << 31) ||
	    in->seg_cap > (1ull << 31) || in->frame_stride < GCL_CTL_MIN_STRIDE || !out->totals || !out->seg.totals)
		return -EINVAL;
	const uint64_t nvec = in->voff ? in->nvec : 0;
	if (nvec > (1ull << 31))
		return -EINVAL;
	if (in->nconn && (!in->qoff || !in->rd || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if ((in->nent && !in->ent) || (nvec && !in->iov))
		return -EINVAL;
	if (in->nconn && in->item_cap && (!out->src_off || !out->len || !out->dst_off || !out->item_conn || !out->item_ent))
		return -EINVAL;
	if (in->nconn && in->seg_cap && (!out->seg.desc || !out->seg.frame_off || !out->seg.seg_conn ||
	                                 !out->seg.seg_kind || !out->seg.seg_src))
		return -EINVAL;
	if (rd_misaligned(in->qoff, 4) || rd_misaligned(in->voff, 4) || rd_misaligned(in->ent, 16) ||
	    rd_misaligned(in->iov, 16) || rd_misaligned(in->rd, 16) || rd_misaligned(in->conn, 16) ||
	    rd_misaligned(in->addr, 16) || rd_misaligned(out->out_conn, 16) || rd_misaligned(out->src_off, 8) ||
	    rd_misaligned(out->len, 2) || rd_misaligned(out->dst_off, 8) || rd_misaligned(out->item_conn, 4) ||
	    rd_misaligned(out->item_ent, 4) || rd_misaligned(out->totals, 8) || rd_misaligned(out->seg.desc, 16) ||
	    rd_misaligned(out->seg.frame_off, 8) || rd_misaligned(out->seg.seg_conn, 4) ||
	    rd_misaligned(out->seg.seg_src, 4) || rd_misaligned(out->seg.totals, 8) || rd_misaligned(counts, 8))
		return -EINVAL;
	if (!workspace || rd_misaligned(workspace, 16) ||
	    workspace_bytes < rd_carve(nullptr, nullptr, in->nconn, in->nent, nvec, in->blocks))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->nconn == 0)
		return hipMemsetAsync(out->totals, 0, 4 * sizeof(uint64_t), s) == hipSuccess &&
		       hipMemsetAsync(out->seg.totals, 0, 2 * sizeof(uint64_t), s) == hipSuccess ? 0 : -EIO;

	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);
	const uint64_t tiles_e = (in->nent + kRdThreads - 1) / kRdThreads, tiles_v = (nvec + kRdThreads - 1) / kRdThreads;
	const uint64_t tiles_c = ((uint64_t)in->nconn + kRdThreads - 1) / kRdThreads;
	const uint64_t tiles = std::max<uint64_t>(std::max(tiles_e, tiles_v), tiles_c);
	RdParams p;

	p.out = *out;
	p.qoff = in->qoff;
	p.voff = in->voff;
	p.ent = (const uint4 *)in->ent;
	p.iov = (const uint4 *)in->iov;
	p.rd = (const uint4 *)in->rd;
	p.conn = (const uint4 *)in->conn;
	p.addr = (const uint4 *)in->addr;
	p.counts = (unsigned long long *)counts;
	p.nent = in->nent;
	p.nvec = nvec;
	p.item_cap = in->item_cap;
	p.seg_cap = in->seg_cap;
	p.frame_base = in->frame_base;
	p.nconn = in->nconn;
	p.frame_stride = in->frame_stride;
	p.blocks = in->blocks ? in->blocks :
	           (uint32_t)std::min<uint64_t>(tiles, std::min<uint32_t>(cus * kRdBlocksPerCu, GCL_RD_MAX_BLOCKS));
	/* whole tiles per range */
	p.per_e = std::max<uint64_t>(1, (tiles_e + p.blocks - 1) / p.blocks) * kRdThreads;
	p.per_v = std::max<uint64_t>(1, (tiles_v + p.blocks - 1) / p.blocks) * kRdThreads;
	p.per_c = std::max<uint64_t>(1, (tiles_c + p.blocks - 1) / p.blocks) * kRdThreads;
	rd_carve(&p, (char *)workspace, in->nconn, in->nent, nvec, in->blocks);

	const dim3 sgrid(p.blocks, in->voff ? 2 : 1);
	hipLaunchKernelGGL(rd_scan_sum_kernel, sgrid, dim3(kRdThreads), 0, s, p);
	hipLaunchKernelGGL(rd_scan_top_kernel, dim3(sgrid.y), dim3(kRdThreads), 0, s, p);
	hipLaunchKernelGGL(rd_scan_apply_kernel, sgrid, dim3(kRdThreads), 0, s, p);
	hipLaunchKernelGGL(rd_decide_kernel, dim3(p.blocks), dim3(kRdThreads), 0, s, p);
	hipLaunchKernelGGL(rd_top_kernel, dim3(1), dim3(kRdThreads), 0, s, p);
	hipLaunchKernelGGL(rd_place_kernel, dim3(p.blocks), dim3(kRdThreads), 0, s, p);
	hipLaunchKernelGGL(rd_items_kernel, dim3(p.blocks), dim3(kRdThreads), 0, s, p);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
