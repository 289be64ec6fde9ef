/*
 * gcl_tcpwrite.hip - tcp_write and tcp_writev for a batch of connections
 * (gcl_tcp_write, gclassify.h): tcp_write_wait, tcp_write3 / tcp_writev2,
 * tcp_write_finish (runtime/net/tcp.c:1259-1422) and tcp_tx_send
 * (tcp_out.c:313-386) for every connection of one runtime at one instant.
 * The rule is gcl_tcpwrite.h, the same inline code the host twin runs; where
 * the twin runs tcp_tx_send's passes one after the other, the kernels use its
 * closed forms, so that nothing that grows with the bytes runs serially: one
 * connection may own every segment.
 *
 * Six launches on the stream; no block waits for another and no atomic hands
 * out a position.  The connections are cut into `blocks` contiguous ranges of
 * whole 256-connection tiles.
 *
 *   count   block r sums the vectors its range's vector writes name.
 *   vtop    one block: the range sums -> their exclusive prefix sums.
 *   plan    one lane per connection: its place in the walk's table from the
 *           range's base and a block scan per tile; the wait; then the walk
 *           over its vectors, at most GCL_WR_MAX_IOV steps of gcl_wr_step, the
 *           state before each vector written to the table W.  It writes
 *           out_conn[c] with the segments and items it wants, the slots, the
 *           short and pushed segments and the held slot to the workspace, and
 *           the range's sums of (segments, items, slots).
 *   top     one block: the exclusive prefix sums of those, totals[0] and [2].
 *   place   one lane per connection: S_c, I_c and K_c from the range's base
 *           and a block scan per tile, DONE or NOSPACE, the rest of out_conn,
 *           the counts, and the sums of the DONE connections into totals.
 *   emit    one lane per sent segment k < totals[1], then one per item k <
 *           totals[3]: the connection by binary search over first_seg
 *           (first_item), monotone and written by place, the vector by binary
 *           search over the connection's rows of W, the pass by subtraction.
 *
 * Bounds.  A connection index is used only below nconn; a vector index only
 * inside a range gcl_wr_range found inside [0, nvec] and no longer than
 * GCL_WR_MAX_IOV; a row of W only below nvec (a connection whose rows would
 * end past it is REFUSED); a segment index only below seg_cap, an item index
 * only below item_cap (a connection is DONE only when all of its fit); a
 * range-sum word only below blocks.  The emit launch checks what it reads back
 * from the workspace against the ranges and the rule again before it uses it.
 * No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_tcpwrite.h"

namespace gclk {

constexpr uint32_t kWrThreads = 256;
constexpr uint32_t kWrWaves = kWrThreads / 64;
constexpr uint32_t kWrBlocksPerCu = 4;
constexpr uint32_t kWrTopPer = GCL_WR_MAX_BLOCKS / kWrThreads;
static_assert(kWrTopPer * kWrThreads == GCL_WR_MAX_BLOCKS, "the top kernels are one block");
static_assert(sizeof(struct gcl_tcp_wr) == 48 && sizeof(struct gcl_wr_conn_out) == 48 &&
              sizeof(struct gcl_rd_iov) == 16 && sizeof(struct gcl_tcp_conn) == 48 &&
              sizeof(struct gcl_tcp_addr) == 16 && sizeof(struct gcl_txh_desc) == 32 &&
              sizeof(struct gcl_txq_ent) == 16 && sizeof(struct gcl_txq_cold) == 16, "records as 16-B words");

/* what the scans add up */
struct WrTri {
	uint64_t a, b, c;
};

struct WrParams {
	struct gcl_wr_out out;
	const uint32_t *voff;
	const uint4 *iov;        /* struct gcl_rd_iov as a 16-B word */
	const uint4 *wr;         /* struct gcl_tcp_wr as three */
	const uint4 *conn;       /* struct gcl_tcp_conn as three */
	const uint4 *addr;
	unsigned long long *counts;
	/* workspace */
	uint4 *W;                /* [2 * nvec]: the walk before a vector: (S, h, segs, items), (slots, hslot) */
	WrTri *vsum;             /* [blocks]: a range's named vectors, then those before it */
	WrTri *bsum;             /* [blocks]: segments, items, slots */
	uint4 *winfo;            /* [nconn]: slots, shorts, pushes, hslot */
	uint32_t *wbase, *wfseg, *wfitem; /* [nconn] */
	uint64_t *wslot0;        /* [nconn] */
	uint64_t nvec, seg_cap, item_cap, frame_base, slot_cap, now, per_c;
	uint32_t nconn, frame_stride, blocks;
};

__device__ __forceinline__ WrTri wr_add(const WrTri &x, const WrTri &y)
{
	return WrTri{x.a + y.a, x.b + y.b, x.c + y.c};
}

__device__ __forceinline__ uint64_t wr_shfl_up(uint64_t v, uint32_t s)
{
	return (uint64_t)__shfl_up((uint32_t)(v >> 32), s) << 32 | __shfl_up((uint32_t)v, s);
}

__device__ __forceinline__ uint64_t wr_wave_sum(uint64_t v)
{
#pragma unroll
	for (int s = 32; s; s >>= 1)
		v += (uint64_t)__shfl_xor((uint32_t)(v >> 32), s) << 32 | __shfl_xor((uint32_t)v, s);
	return v;
}

/*
 * The exclusive prefix sums of @v over the block's lanes, and the block's sum
 * in *@total.  Every lane of the block calls it.
 */
__device__ __forceinline__ WrTri wr_block_scan(const WrTri &v, WrTri *total)
{
	__shared__ WrTri ws[kWrWaves];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	WrTri inc = v;

#pragma unroll
	for (uint32_t s = 1; s < 64; s <<= 1) {
		const WrTri t = {wr_shfl_up(inc.a, s), wr_shfl_up(inc.b, s), wr_shfl_up(inc.c, s)};
		if (lane >= s)
			inc = wr_add(inc, t);
	}
	__syncthreads(); /* the reads of the call before */
	if (lane == 63)
		ws[wave] = inc;
	__syncthreads();
	WrTri base = {0, 0, 0}, tot = {0, 0, 0};
#pragma unroll
	for (uint32_t w = 0; w < kWrWaves; w++) {
		const WrTri t = ws[w];
		if (w < wave)
			base = wr_add(base, t);
		tot = wr_add(tot, t);
	}
	*total = tot;
	return WrTri{base.a + inc.a - v.a, base.b + inc.b - v.b, base.c + inc.c - v.c};
}

/* @sum[0, blocks) -> its exclusive prefix sums in place; returns the sum of all.  One block. */
__device__ __forceinline__ WrTri wr_top_scan(WrTri *sum, uint32_t blocks)
{
	const uint32_t t = threadIdx.x;
	WrTri v[kWrTopPer], mine = {0, 0, 0}, tot;

#pragma unroll
	for (uint32_t x = 0; x < kWrTopPer; x++) {
		const uint32_t r = t * kWrTopPer + x;
		v[x] = r < blocks ? sum[r] : WrTri{0, 0, 0};
		mine = wr_add(mine, v[x]);
	}
	WrTri base = wr_block_scan(mine, &tot);
#pragma unroll
	for (uint32_t x = 0; x < kWrTopPer; x++) {
		const uint32_t r = t * kWrTopPer + x;
		if (r < blocks)
			sum[r] = base;
		base = wr_add(base, v[x]);
	}
	return tot;
}

/* the twelve dwords of wr[c] */
__device__ __forceinline__ void wr_load(const WrParams &p, uint32_t c, uint32_t w[12])
{
	const uint4 a = p.wr[3 * (size_t)c], b = p.wr[3 * (size_t)c + 1], d = p.wr[3 * (size_t)c + 2];

	w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
	w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
	w[8] = d.x; w[9] = d.y; w[10] = d.z; w[11] = d.w;
}

__device__ __forceinline__ void wr_store_conn(const WrParams &p, uint32_t c, const uint32_t w[12])
{
	uint4 *o = (uint4 *)&p.out.out_conn[c];

	o[0] = make_uint4(w[0], w[1], w[2], w[3]);
	o[1] = make_uint4(w[4], w[5], w[6], w[7]);
	o[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

__global__ void __launch_bounds__(kWrThreads) wr_count_kernel(WrParams p)
{
	const uint64_t lo = std::min<uint64_t>((uint64_t)blockIdx.x * p.per_c, p.nconn);
	const uint64_t hi = std::min<uint64_t>(lo + p.per_c, p.nconn);
	WrTri acc = {0, 0, 0}, tot;

	for (uint64_t c64 = lo + threadIdx.x; c64 < hi; c64 += kWrThreads) {
		uint32_t w[12];
		wr_load(p, (uint32_t)c64, w);
		acc.a += gcl_wr_named(w, p.voff, (uint32_t)c64, p.nvec);
	}
	wr_block_scan(acc, &tot);
	if (threadIdx.x == 0)
		p.vsum[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kWrThreads) wr_vtop_kernel(WrParams p)
{
	wr_top_scan(p.vsum, p.blocks);
}

__global__ void __launch_bounds__(kWrThreads) wr_plan_kernel(WrParams p)
{
	const uint64_t lo = std::min<uint64_t>((uint64_t)blockIdx.x * p.per_c, p.nconn);
	const uint64_t hi = std::min<uint64_t>(lo + p.per_c, p.nconn);
	uint64_t vcarry = p.vsum[blockIdx.x].a;
	WrTri acc = {0, 0, 0}, tot;

	for (uint64_t j0 = lo; j0 < hi; j0 += kWrThreads) { /* uniform: every lane reaches the barriers */
		const uint64_t c64 = j0 + threadIdx.x;
		const bool live = c64 < hi;
		const uint32_t c = (uint32_t)c64;
		uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
		WrTri vtot;

		if (live)
			wr_load(p, c, w);
		const uint32_t named = live ? gcl_wr_named(w, p.voff, c, p.nvec) : 0;
		const WrTri vex = wr_block_scan(WrTri{named, 0, 0}, &vtot);

		if (live) {
			const uint4 c0 = p.conn[3 * (size_t)c];
			const uint32_t snd_una = c0.x, snd_nxt = c0.y, snd_wnd = c0.z;
			const uint32_t fl = gcl_wr_flags(w), mss = gcl_wr_mss(w);
			const uint64_t vbase = vcarry + vex.a, pend_off = (uint64_t)w[5] << 32 | w[4];
			uint32_t v0 = 0, m = 0, bad = 0, o[12];
			struct gcl_wr_res r;
			struct gcl_wr_walk s;

			if (fl & GCL_WR_VEC) {
				m = gcl_wr_range(p.voff, c, p.nvec, &v0, &bad);
				if (vbase + m > p.nvec) /* its rows of W */
					bad = 1;
			}
			gcl_wr_walk_init(&s, w[6]);
			if (gcl_wr_wait(w, bad, snd_una, snd_wnd, snd_nxt, p.frame_stride, &r)) {
				if (fl & GCL_WR_VEC) {
					for (uint32_t i = 0; i < m; i++) {
						const uint4 v = p.iov[(uint64_t)v0 + i];
						p.W[2 * (vbase + i)] = make_uint4(s.S, s.h, s.segs, s.items);
						p.W[2 * (vbase + i) + 1] = make_uint4(s.slots, s.hslot, 0, 0);
						gcl_wr_step(&s, mss, r.winlen, v.z, i == m - 1, 0);
					}
				} else {
					gcl_wr_step(&s, mss, r.winlen, w[2], 1, 1);
				}
				acc.a += s.segs;
				acc.b += s.items;
				acc.c += s.slots;
			}
			gcl_wr_conn_words(r.status == GCL_WRS_DONE ? (int64_t)s.S : r.ret, snd_nxt + s.S, 0, s.segs, 0, s.items,
			                  s.h, pend_off, r.status, r.flags, o);
			wr_store_conn(p, c, o);
			p.winfo[c] = make_uint4(s.slots, s.shorts, s.pushes, s.hslot);
			p.wbase[c] = (uint32_t)(vbase < p.nvec ? vbase : p.nvec);
		}
		vcarry += vtot.a;
	}
	wr_block_scan(acc, &tot);
	if (threadIdx.x == 0)
		p.bsum[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kWrThreads) wr_top_kernel(WrParams p)
{
	const WrTri tot = wr_top_scan(p.bsum, p.blocks);

	if (threadIdx.x == 0) {
		p.out.totals[0] = tot.a;
		p.out.totals[1] = 0; /* place adds the DONE connections' */
		p.out.totals[2] = tot.b;
		p.out.totals[3] = 0;
		p.out.totals[4] = 0;
		p.out.totals[5] = 0;
	}
}

__global__ void __launch_bounds__(kWrThreads) wr_place_kernel(WrParams p)
{
	const uint64_t lo = std::min<uint64_t>((uint64_t)blockIdx.x * p.per_c, p.nconn);
	const uint64_t hi = std::min<uint64_t>(lo + p.per_c, p.nconn);
	WrTri carry = p.bsum[blockIdx.x];
	uint64_t cnt[GCL_WRC_NR] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, slots = 0;

	for (uint64_t j0 = lo; j0 < hi; j0 += kWrThreads) { /* uniform: every lane reaches the barriers */
		const uint64_t c64 = j0 + threadIdx.x;
		const bool live = c64 < hi;
		const uint32_t c = (uint32_t)c64;
		uint4 o0 = make_uint4(0, 0, 0, 0), o1 = o0, o2 = o0, inf = o0;
		WrTri tot;

		if (live) {
			const uint4 *o = (const uint4 *)&p.out.out_conn[c];
			o0 = o[0];
			o1 = o[1];
			o2 = o[2];
			inf = p.winfo[c];
		}
		uint32_t status = o2.z & 0xFFu, flags = (o2.z >> 8) & 0xFFu;
		const bool go = status == GCL_WRS_DONE;
		const uint32_t nseg = go ? o1.x : 0, nitems = go ? o1.z : 0, nslots = go ? inf.x : 0;
		const WrTri ex = wr_block_scan(WrTri{nseg, nitems, nslots}, &tot);

		if (live) {
			const uint64_t S = carry.a + ex.a, I = carry.b + ex.b, K = carry.c + ex.c;
			const uint32_t fseg = (uint32_t)(S < p.seg_cap ? S : p.seg_cap);
			const uint32_t fitem = (uint32_t)(I < p.item_cap ? I : p.item_cap);
			uint32_t w[12], ow[12];

			if (go) {
				const uint4 c0 = p.conn[3 * (size_t)c], c1 = p.conn[3 * (size_t)c + 1];
				wr_load(p, c, w);
				const uint64_t pend_off = (uint64_t)w[5] << 32 | w[4];

				if (gcl_wr_fits(S, nseg, p.seg_cap, I, nitems, p.item_cap, K, nslots, p.slot_cap)) {
					const int64_t ret = (int64_t)((uint64_t)o0.y << 32 | o0.x);
					flags = gcl_wr_finish_flags(flags, nseg, c1.y, w[3], c0.x, c0.z, o0.z);
					gcl_wr_conn_words(ret, o0.z, fseg, nseg, fitem, nitems, o1.w,
					                  o1.w ? gcl_wr_frame(inf.w, K, pend_off, p.frame_base, p.frame_stride) : 0,
					                  status, flags, ow);
					cnt[GCL_WRC_SEGS] += nseg;
					cnt[GCL_WRC_PUSH] += inf.z;
					cnt[GCL_WRC_HELD] += o1.w ? 1 : 0;
					cnt[GCL_WRC_SHORT] += inf.y;
					cnt[GCL_WRC_ITEMS] += nitems;
					cnt[GCL_WRC_BYTES] += (uint64_t)ret;
					slots += nslots;
				} else {
					status = GCL_WRS_NOSPACE;
					gcl_wr_conn_words(-GCL_WR_ENOBUFS, c0.y, fseg, 0, fitem, 0, w[6], pend_off, status, 0, ow);
				}
				wr_store_conn(p, c, ow);
			} else {
				uint4 *o = (uint4 *)&p.out.out_conn[c];
				o[0] = make_uint4(o0.x, o0.y, o0.z, fseg);
				o[1] = make_uint4(0, fitem, 0, o1.w);
			}
			p.wfseg[c] = fseg;
			p.wfitem[c] = fitem;
			p.wslot0[c] = K;
#pragma unroll
			for (uint32_t x = 0; x <= GCL_WRS_NOSPACE; x++)
				cnt[x] += status == x;
		}
		carry = wr_add(carry, tot);
	}
	/* the lanes' sums -> totals and counts */
	const uint64_t t1 = wr_wave_sum(cnt[GCL_WRC_SEGS]), t3 = wr_wave_sum(cnt[GCL_WRC_ITEMS]);
	const uint64_t t4 = wr_wave_sum(slots), t5 = wr_wave_sum(cnt[GCL_WRC_BYTES]);
	if ((threadIdx.x & 63) == 0) {
		unsigned long long *t = (unsigned long long *)p.out.totals;
		if (t1) atomicAdd(t + 1, (unsigned long long)t1);
		if (t3) atomicAdd(t + 3, (unsigned long long)t3);
		if (t4) atomicAdd(t + 4, (unsigned long long)t4);
		if (t5) atomicAdd(t + 5, (unsigned long long)t5);
	}
	if (p.counts) {
#pragma unroll
		for (uint32_t x = 0; x < GCL_WRC_NR; x++) {
			const uint64_t s = wr_wave_sum(cnt[x]);
			if ((threadIdx.x & 63) == 0 && s)
				atomicAdd(p.counts + x, (unsigned long long)s);
		}
	}
}

/* the last connection whose @first is not past @k: first[0] == 0 */
__device__ __forceinline__ uint32_t wr_owner(const uint32_t *first, uint32_t nconn, uint64_t k)
{
	uint32_t a = 0, b = nconn - 1;

	while (a < b) {
		const uint32_t mid = a + (b - a + 1) / 2;
		if (first[mid] <= k)
			a = mid;
		else
			b = mid - 1;
	}
	return a;
}

/* the pass that owns local segment (@item 0) or item (@item 1) @t of connection @c; false: none */
struct WrHit {
	struct gcl_wr_pass ps;
	uint64_t src;        /* the vector's off */
	uint32_t local_seg;  /* the pass's segment among the connection's */
};

__device__ __forceinline__ bool wr_find(const WrParams &p, uint32_t c, const uint32_t w[12], uint32_t winlen,
                                        uint32_t t, int item, WrHit *hit)
{
	const uint32_t fl = gcl_wr_flags(w), mss = gcl_wr_mss(w);
	struct gcl_wr_walk s;
	uint32_t len, X, push, last = 1;

	gcl_wr_walk_init(&s, w[6]);
	hit->src = (uint64_t)w[1] << 32 | w[0];
	len = w[2];
	if (fl & GCL_WR_VEC) {
		uint32_t v0, bad = 0;
		const uint32_t m = gcl_wr_range(p.voff, c, p.nvec, &v0, &bad);
		const uint64_t vbase = p.wbase[c];

		if (bad || m == 0 || vbase + m > p.nvec)
			return false;
		/* the last vector whose count before is not past t */
		uint32_t a = 0, b = m - 1;
		while (a < b) {
			const uint32_t mid = a + (b - a + 1) / 2;
			const uint4 r0 = p.W[2 * (vbase + mid)];
			if ((item ? r0.w : r0.z) <= t)
				a = mid;
			else
				b = mid - 1;
		}
		const uint4 r0 = p.W[2 * (vbase + a)], r1 = p.W[2 * (vbase + a) + 1], v = p.iov[(uint64_t)v0 + a];
		s.S = r0.x;
		s.h = r0.y;
		s.segs = r0.z;
		s.items = r0.w;
		s.slots = r1.x;
		s.hslot = r1.y;
		hit->src = (uint64_t)v.y << 32 | v.x;
		len = v.z;
		last = a == m - 1;
		if (s.h > mss || s.S > winlen)
			return false;
	}
	if (!gcl_wr_vec_send(len, winlen - s.S, last, !(fl & GCL_WR_VEC), &X, &push))
		return false;
	const struct gcl_wr_send r = gcl_wr_send_rule(mss, s.h, X, push);
	const uint32_t before = item ? s.items : s.segs;
	if (t < before || t - before >= (item ? r.passes : r.sent))
		return false;
	hit->ps = gcl_wr_pass_at(&s, mss, X, push, t - before);
	hit->local_seg = s.segs + (t - before);
	return true;
}

__global__ void __launch_bounds__(kWrThreads) wr_emit_kernel(WrParams p)
{
	const uint64_t nseg = std::min<uint64_t>(p.out.totals[1], p.seg_cap);
	const uint64_t nitem = std::min<uint64_t>(p.out.totals[3], p.item_cap);
	const uint64_t step = (uint64_t)gridDim.x * kWrThreads, k0 = (uint64_t)blockIdx.x * kWrThreads + threadIdx.x;

	for (uint64_t k = k0; k < nseg + nitem; k += step) {
		const int item = k >= nseg;
		const uint64_t kk = item ? k - nseg : k;
		const uint32_t c = wr_owner(item ? p.wfitem : p.wfseg, p.nconn, kk);
		const uint4 *oc = (const uint4 *)&p.out.out_conn[c];
		const uint4 o0 = oc[0], o1 = oc[1], o2 = oc[2];
		const uint32_t first = item ? o1.y : o0.w, n = item ? o1.z : o1.x;
		uint32_t w[12];
		WrHit hit;

		if ((o2.z & 0xFFu) != GCL_WRS_DONE || kk < first || kk - first >= n)
			continue;
		const uint4 c0 = p.conn[3 * (size_t)c], c1 = p.conn[3 * (size_t)c + 1];
		wr_load(p, c, w);
		if (!wr_find(p, c, w, c0.x + c0.z - c0.y, (uint32_t)(kk - first), item, &hit))
			continue;
		const uint64_t frame = gcl_wr_frame(hit.ps.slot, p.wslot0[c], (uint64_t)w[5] << 32 | w[4], p.frame_base,
		                                    p.frame_stride);
		if (item) {
			p.out.src_off[kk] = hit.src + hit.ps.off;
			p.out.len[kk] = (uint16_t)hit.ps.take;
			p.out.dst_off[kk] = frame + GCL_WR_HDR + hit.ps.fill0;
			p.out.item_conn[kk] = c;
			p.out.item_seg[kk] = hit.local_seg < o1.x ? o0.w + hit.local_seg : GCL_WR_SEG_HELD;
		} else {
			const uint4 ad = p.addr[c];
			const uint32_t a[4] = {ad.x, ad.y, ad.z, ad.w};
			uint32_t d[16];

			gcl_wr_seg_words(a, (w[8] >> 16) & 0xFFu, hit.ps.tcp_flags, c0.y + hit.ps.seq, c1.y, c1.z,
			                 hit.ps.fill0 + hit.ps.take, frame, p.now, d);
			((uint4 *)&p.out.desc[kk])[0] = make_uint4(d[0], d[1], d[2], d[3]);
			((uint4 *)&p.out.desc[kk])[1] = make_uint4(d[4], d[5], d[6], d[7]);
			*(uint4 *)&p.out.txq_ent[kk] = make_uint4(d[8], d[9], d[10], d[11]);
			*(uint4 *)&p.out.txq_cold[kk] = make_uint4(d[12], d[13], d[14], d[15]);
			p.out.frame_off[kk] = frame;
			p.out.seg_conn[kk] = c;
		}
	}
}

static bool wr_misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

static size_t wr_r16(size_t b)
{
	return (b + 15) & ~(size_t)15;
}

/* the workspace's parts, in order; returns its size */
static size_t wr_carve(WrParams *p, char *base, uint32_t nconn, uint64_t nvec, uint32_t blocks)
{
	const size_t nb = blocks ? blocks : GCL_WR_MAX_BLOCKS;
	size_t at = 0;

	if (p) p->W = (uint4 *)(base + at);
	at += 32 * (size_t)nvec;
	if (p) p->winfo = (uint4 *)(base + at);
	at += 16 * (size_t)nconn;
	if (p) p->vsum = (WrTri *)(base + at);
	at += wr_r16(sizeof(WrTri) * nb);
	if (p) p->bsum = (WrTri *)(base + at);
	at += wr_r16(sizeof(WrTri) * nb);
	if (p) p->wslot0 = (uint64_t *)(base + at);
	at += wr_r16(8 * (size_t)nconn);
	if (p) p->wbase = (uint32_t *)(base + at);
	at += wr_r16(4 * (size_t)nconn);
	if (p) p->wfseg = (uint32_t *)(base + at);
	at += wr_r16(4 * (size_t)nconn);
	if (p) p->wfitem = (uint32_t *)(base + at);
	at += wr_r16(4 * (size_t)nconn);
	return at;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tcp_write_workspace(uint32_t nconn, uint64_t nvec, uint32_t blocks, size_t *bytes)
{
	if (!bytes || nconn > GCL_WR_MAX_CONN || nvec > (1ull << 31) || blocks > GCL_WR_MAX_BLOCKS)
		return -EINVAL;
	*bytes = wr_carve(nullptr, nullptr, nconn, nvec, blocks);
	return 0;
}

extern "C" int gcl_tcp_write(struct gcl_ctx *c, const struct gcl_wr_in *in, const struct gcl_wr_out *out,
                             uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !in || !out || in->size != sizeof(*in) || in->nconn > GCL_WR_MAX_CONN ||
	    in->blocks > GCL_WR_MAX_BLOCKS || in->seg_cap > (1ull << 31) || in->item_cap > (1ull << 31) ||
	    in->frame_stride < GCL_WR_HDR || in->frame_stride > GCL_WR_MAX_STRIDE || !out->totals)
		return -EINVAL;
	const uint64_t nvec = in->voff ? in->nvec : 0;
	if (nvec > (1ull << 31))
		return -EINVAL;
	if (in->nconn && (!in->wr || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if (nvec && !in->iov)
		return -EINVAL;
	if (in->nconn && in->seg_cap && (!out->desc || !out->frame_off || !out->seg_conn || !out->txq_ent || !out->txq_cold))
		return -EINVAL;
	if (in->nconn && in->item_cap && (!out->src_off || !out->len || !out->dst_off || !out->item_conn || !out->item_seg))
		return -EINVAL;
	if (wr_misaligned(in->voff, 4) || wr_misaligned(in->iov, 16) || wr_misaligned(in->wr, 16) ||
	    wr_misaligned(in->conn, 16) || wr_misaligned(in->addr, 16) || wr_misaligned(out->out_conn, 16) ||
	    wr_misaligned(out->desc, 16) || wr_misaligned(out->frame_off, 8) || wr_misaligned(out->seg_conn, 4) ||
	    wr_misaligned(out->txq_ent, 16) || wr_misaligned(out->txq_cold, 16) || wr_misaligned(out->src_off, 8) ||
	    wr_misaligned(out->len, 2) || wr_misaligned(out->dst_off, 8) || wr_misaligned(out->item_conn, 4) ||
	    wr_misaligned(out->item_seg, 4) || wr_misaligned(out->totals, 8) || wr_misaligned(counts, 8))
		return -EINVAL;
	if (!workspace || wr_misaligned(workspace, 16) ||
	    workspace_bytes < wr_carve(nullptr, nullptr, in->nconn, nvec, in->blocks))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->nconn == 0)
		return hipMemsetAsync(out->totals, 0, 6 * sizeof(uint64_t), s) == hipSuccess ? 0 : -EIO;

	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);
	const uint64_t tiles_c = ((uint64_t)in->nconn + kWrThreads - 1) / kWrThreads;
	WrParams p;

	p.out = *out;
	p.voff = in->voff;
	p.iov = (const uint4 *)in->iov;
	p.wr = (const uint4 *)in->wr;
	p.conn = (const uint4 *)in->conn;
	p.addr = (const uint4 *)in->addr;
	p.counts = (unsigned long long *)counts;
	p.nvec = nvec;
	p.seg_cap = in->seg_cap;
	p.item_cap = in->item_cap;
	p.frame_base = in->frame_base;
	p.slot_cap = gcl_wr_slot_cap(in->frames_len, in->frame_base, in->frame_stride);
	p.now = in->now;
	p.nconn = in->nconn;
	p.frame_stride = in->frame_stride;
	p.blocks = in->blocks ? in->blocks :
	           (uint32_t)std::min<uint64_t>(tiles_c, std::min<uint32_t>(cus * kWrBlocksPerCu, GCL_WR_MAX_BLOCKS));
	p.per_c = std::max<uint64_t>(1, (tiles_c + p.blocks - 1) / p.blocks) * kWrThreads; /* whole tiles per range */
	wr_carve(&p, (char *)workspace, in->nconn, nvec, in->blocks);

	/* the emission is dealt over all CUs however few the connections are */
	const uint32_t eblocks = in->blocks ? in->blocks : std::min<uint32_t>(cus * kWrBlocksPerCu, GCL_WR_MAX_BLOCKS);

	hipLaunchKernelGGL(wr_count_kernel, dim3(p.blocks), dim3(kWrThreads), 0, s, p);
	hipLaunchKernelGGL(wr_vtop_kernel, dim3(1), dim3(kWrThreads), 0, s, p);
	hipLaunchKernelGGL(wr_plan_kernel, dim3(p.blocks), dim3(kWrThreads), 0, s, p);
	hipLaunchKernelGGL(wr_top_kernel, dim3(1), dim3(kWrThreads), 0, s, p);
	hipLaunchKernelGGL(wr_place_kernel, dim3(p.blocks), dim3(kWrThreads), 0, s, p);
	hipLaunchKernelGGL(wr_emit_kernel, dim3(eblocks), dim3(kWrThreads), 0, s, p);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
