/*
 * gcl_tcpshut.hip - tcp_shutdown, tcp_close and tcp_abort for a batch of
 * connections (gcl_tcp_shut, gclassify.h): runtime/net/tcp.c:1555-1633 with
 * tcp_conn_shutdown_tx, tcp_conn_shutdown_rx and tcp_conn_fail, and the FIN of
 * tcp_tx_ctl and the RST of tcp_tx_raw_rst (runtime/net/tcp_out.c) as
 * gcl_txh_desc records in connection order.  The rule is gcl_tcpshut.h's, the
 * same inline code the host twin runs.
 *
 * The call is an ordered compaction, as gcl_tcp_tick is: connection c asks for
 * 0 or 1 segment, and its segment lies at the count of the askers before it.
 * Three launches on the stream, and no block ever waits for another: no
 * look-back, no flag, no cooperative launch; no atomic hands out a position.
 * The connections are cut into `blocks` contiguous ranges of whole 256-lane
 * tiles (the library's choice, or in->blocks).
 *
 *   decide   block r walks range r, one lane per connection: the 16-B request,
 *            the 64-B timer record as four 16-B loads and the first 16-B word
 *            of the PCB words (snd_nxt), the rule, out_conn as three 16-B
 *            stores as if its segment had room, and one byte of the workspace:
 *            what it wants and what the counters need of it should it get it.
 *            The wave's askers are the population count of a ballot; the
 *            range's sum goes to workspace word r, and every block stores it.
 *   top      one block turns the range sums into their exclusive prefix sums
 *            in place and writes totals.
 *   emit     block r walks range r again tile by tile, reading the byte.  An
 *            asker's position is the range's base + the tiles before + the
 *            waves before (LDS, two buffers in turn: one barrier per tile) +
 *            the population count of the ballot below its lane.  Below the cap
 *            it writes its segment: desc as two 16-B stores, txq_ent and
 *            txq_cold as one each, frame_off, seg_conn, seg_kind, seg_src, and
 *            first_seg of its out_conn.  At or past the cap it runs
 *            gcl_shut_nospace on its inputs and writes its out_conn again.
 *            A connection that asks for nothing reads one byte here.
 *
 * Bounds.  A connection index is used only below nconn, a segment index only
 * below min(seg_cap, the frames that fit), a workspace word only below blocks,
 * a workspace byte only below nconn.  Nothing is written outside the first
 * seg_cap entries of the per-segment arrays, out_conn[0, nconn), totals,
 * counts and the workspace.  No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_tcpshut.h"

namespace gclk {

constexpr uint32_t kShutThreads = 256;
constexpr uint32_t kShutWaves = kShutThreads / 64;
constexpr uint32_t kShutBlocksPerCu = 4;
constexpr uint32_t kShutTopPer = GCL_SHUT_MAX_BLOCKS / kShutThreads;
static_assert(kShutTopPer * kShutThreads == GCL_SHUT_MAX_BLOCKS, "the top kernel is one block");
static_assert(sizeof(struct gcl_tcp_shut) == 16 && sizeof(struct gcl_shut_conn_out) == 48 &&
              sizeof(struct gcl_tcp_tmr) == 64 && sizeof(struct gcl_tcp_conn) == 48 &&
              sizeof(struct gcl_tcp_addr) == 16 && sizeof(struct gcl_txq_ent) == 16 &&
              sizeof(struct gcl_txq_cold) == 16 && sizeof(struct gcl_txh_desc) == 32, "records as 16-B words");

/* the workspace byte of a connection: bits 0-1 GCL_SHUT_WANT_*, then what the counters need */
constexpr uint32_t kShutWFail = 0x04, kShutWWarn = 0x08, kShutWPutShift = 4;

struct ShutParams {
	const uint4 *shut, *tmr, *conn, *addr;
	uint4 *out_conn;
	uint4 *desc;
	uint64_t *frame_off;
	uint32_t *seg_conn;
	uint8_t *seg_kind;
	uint32_t *seg_src;
	uint4 *txq_ent, *txq_cold;
	unsigned long long *totals, *counts;
	uint32_t *bsum;            /* workspace: [blocks], a range's askers, then the askers before it */
	uint8_t *want;             /* workspace: [nconn] */
	uint64_t now, per;         /* per: connections per range, a multiple of kShutThreads */
	uint64_t cap, frame_base;  /* cap: gcl_shut_cap, <= seg_cap */
	uint32_t nconn, frame_stride, blocks;
};

/* connection c < nconn as the rule reads it */
__device__ __forceinline__ void shut_load(const ShutParams &p, uint64_t c, struct gcl_shut_one *t)
{
	const uint4 s = p.shut[c];
	const uint4 a = p.tmr[4 * c], b = p.tmr[4 * c + 1], d = p.tmr[4 * c + 2], e = p.tmr[4 * c + 3];
	const uint4 c0 = p.conn[3 * c]; /* snd_una, snd_nxt, snd_wnd, snd_wl1 */
	const uint32_t m[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w, e.x, e.y, e.z, e.w};
	const uint32_t sw[4] = {s.x, s.y, s.z, s.w};

	gcl_shut_load(m, sw, c0.y, t);
}

__device__ __forceinline__ void shut_store_conn(const ShutParams &p, uint64_t c, const struct gcl_shut_res &r,
                                                uint32_t first_seg, uint32_t nseg)
{
	uint32_t o[12];

	gcl_shut_conn_words(&r, first_seg, nseg, o);
	p.out_conn[3 * c] = make_uint4(o[0], o[1], o[2], o[3]);
	p.out_conn[3 * c + 1] = make_uint4(o[4], o[5], o[6], o[7]);
	p.out_conn[3 * c + 2] = make_uint4(o[8], o[9], o[10], o[11]);
}

/* wave-uniform sums of the lanes' values into counts; @on: the lane counts at all */
__device__ __forceinline__ void shut_count(uint32_t *cnt, bool on, uint32_t status, bool fail, bool warn,
                                           uint32_t nput, uint32_t want, bool written)
{
#pragma unroll
	for (uint32_t x = 0; x < GCL_SHUTS_NR; x++)
		cnt[x] += (uint32_t)__popcll(__ballot(on && status == x));
	cnt[GCL_SHUTC_FIN] += (uint32_t)__popcll(__ballot(on && written && want == GCL_SHUT_WANT_FIN));
	cnt[GCL_SHUTC_RST] += (uint32_t)__popcll(__ballot(on && written && want == GCL_SHUT_WANT_RST));
	cnt[GCL_SHUTC_FAIL] += (uint32_t)__popcll(__ballot(on && fail));
	cnt[GCL_SHUTC_PUT] += (uint32_t)__popcll(__ballot(on && (nput & 1u))) +
	                      2u * (uint32_t)__popcll(__ballot(on && (nput & 2u)));
	cnt[GCL_SHUTC_WARN] += (uint32_t)__popcll(__ballot(on && warn));
}

__device__ __forceinline__ void shut_count_flush(const ShutParams &p, const uint32_t *cnt)
{
	if ((threadIdx.x & 63) == 0) {
#pragma unroll
		for (uint32_t x = 0; x < GCL_SHUTC_NR; x++)
			if (cnt[x])
				atomicAdd(p.counts + x, (unsigned long long)cnt[x]);
	}
}

__global__ void __launch_bounds__(kShutThreads) shut_decide_kernel(ShutParams p)
{
	__shared__ uint32_t ws[kShutWaves];
	const uint64_t lo = (uint64_t)blockIdx.x * p.per;
	const uint64_t hi = lo + p.per < p.nconn ? lo + p.per : p.nconn; /* lo >= nconn: an empty range */
	uint32_t segs = 0, cnt[GCL_SHUTC_NR] = {0};                      /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kShutThreads) { /* uniform: every lane reaches the ballots */
		const uint64_t c = j0 + threadIdx.x;
		struct gcl_shut_res r;
		r.want = GCL_SHUT_WANT_NONE;
		r.status = GCL_SHUTS_NONE;
		r.err = 0;
		r.flags = 0;
		r.nput = 0;
		if (c < hi) {
			struct gcl_shut_one t;

			shut_load(p, c, &t);
			gcl_shut_rule(&t, p.now, &r);
			shut_store_conn(p, c, r, 0, r.want != GCL_SHUT_WANT_NONE);
			p.want[c] = (uint8_t)(r.want | (r.err ? kShutWFail : 0u) | ((r.flags & GCL_SHO_WARN) ? kShutWWarn : 0u) |
			                      r.nput << kShutWPutShift);
		}
		segs += (uint32_t)__popcll(__ballot(r.want != GCL_SHUT_WANT_NONE));
		if (p.counts) /* the askers are counted by emit, which knows whether they had room */
			shut_count(cnt, c < hi && r.want == GCL_SHUT_WANT_NONE, r.status, r.err != 0,
			           (r.flags & GCL_SHO_WARN) != 0, r.nput, 0, false);
	}
	if (p.counts)
		shut_count_flush(p, cnt);
	if ((threadIdx.x & 63) == 0)
		ws[threadIdx.x >> 6] = segs;
	__syncthreads();
	if (threadIdx.x == 0)
		p.bsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

/* bsum[0, blocks) -> its exclusive prefix sums; totals; one block.  A call's askers are <= 2^20. */
__global__ void __launch_bounds__(kShutThreads) shut_top_kernel(ShutParams p)
{
	__shared__ uint32_t sc[2][kShutThreads];
	const uint32_t t = threadIdx.x;
	uint32_t v[kShutTopPer], sum = 0;

#pragma unroll
	for (uint32_t x = 0; x < kShutTopPer; x++) {
		const uint32_t r = t * kShutTopPer + x;
		v[x] = r < p.blocks ? p.bsum[r] : 0;
		sum += v[x];
	}
	/* inclusive scan of the lanes' sums, ping-pong: one barrier per step */
	uint32_t cur = 0;
	sc[0][t] = sum;
	__syncthreads();
	for (uint32_t step = 1; step < kShutThreads; step <<= 1) {
		const uint32_t a = t >= step ? sc[cur][t - step] + sc[cur][t] : sc[cur][t];
		sc[cur ^ 1][t] = a;
		cur ^= 1;
		__syncthreads();
	}
	uint32_t base = t ? sc[cur][t - 1] : 0;
#pragma unroll
	for (uint32_t x = 0; x < kShutTopPer; x++) {
		const uint32_t r = t * kShutTopPer + x;
		if (r < p.blocks)
			p.bsum[r] = base;
		base += v[x];
	}
	if (t == kShutThreads - 1) {
		const unsigned long long wanted = base;
		p.totals[0] = wanted;
		p.totals[1] = wanted < p.cap ? wanted : p.cap;
	}
}

__global__ void __launch_bounds__(kShutThreads) shut_emit_kernel(ShutParams p)
{
	__shared__ uint32_t wt[2][kShutWaves];
	const uint64_t lo = (uint64_t)blockIdx.x * p.per;
	const uint64_t hi = lo + p.per < p.nconn ? lo + p.per : p.nconn;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t below = (1ull << lane) - 1;
	uint64_t carry = lo < hi ? p.bsum[blockIdx.x] : 0; /* the range's base, then the tiles before */
	uint32_t par = 0, cnt[GCL_SHUTC_NR] = {0};         /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kShutThreads, par ^= 1) { /* uniform: every lane active */
		const uint64_t c = j0 + threadIdx.x;
		const uint32_t w = c < hi ? p.want[c] : 0;
		const uint32_t want = w & 3u;
		const uint64_t m0 = __ballot(want != GCL_SHUT_WANT_NONE);

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

		const bool fits = at < p.cap;
		if (want != GCL_SHUT_WANT_NONE) { /* c < hi <= nconn */
			if (fits) {                   /* at < cap <= seg_cap */
				const uint4 c0 = p.conn[3 * c], c1 = p.conn[3 * c + 1], ad = p.addr[c];
				const uint32_t a[4] = {ad.x, ad.y, ad.z, ad.w};
				const uint64_t off = p.frame_base + at * p.frame_stride;
				uint32_t d[16];

				/* snd_nxt: word 1; rcv_nxt, rcv_wnd: words 5, 6 */
				gcl_shut_seg_words(a, want, c0.y, c1.y, c1.z, off, p.now, d);
				p.desc[2 * at] = make_uint4(d[0], d[1], d[2], d[3]);
				p.desc[2 * at + 1] = make_uint4(d[4], d[5], d[6], d[7]);
				p.txq_ent[at] = make_uint4(d[8], d[9], d[10], d[11]);
				p.txq_cold[at] = make_uint4(d[12], d[13], d[14], d[15]);
				p.frame_off[at] = off;
				p.seg_conn[at] = (uint32_t)c;
				p.seg_kind[at] = (uint8_t)(want == GCL_SHUT_WANT_FIN ? GCL_CTL_FIN : GCL_CTL_RST);
				p.seg_src[at] = (uint32_t)c;
				((uint32_t *)p.out_conn)[12 * c + 7] = (uint32_t)at; /* first_seg: this lane's alone */
			} else {
				struct gcl_shut_one t;
				struct gcl_shut_res r;

				shut_load(p, c, &t);
				gcl_shut_nospace(&t, &r);
				shut_store_conn(p, c, r, 0, 0);
			}
		}
		if (p.counts) {
			const bool on = want != GCL_SHUT_WANT_NONE;
			shut_count(cnt, on, fits ? GCL_SHUTS_DONE : GCL_SHUTS_NOSPACE, fits && (w & kShutWFail),
			           fits && (w & kShutWWarn), fits ? (w >> kShutWPutShift) & 3u : 0u, want, fits);
		}
	}
	if (p.counts)
		shut_count_flush(p, cnt);
}

static bool shut_misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

static size_t shut_ws_sums(uint32_t blocks)
{
	return ((size_t)4 * (blocks ? blocks : GCL_SHUT_MAX_BLOCKS) + 15) & ~(size_t)15;
}

static size_t shut_workspace(uint32_t nconn, uint32_t blocks)
{
	return shut_ws_sums(blocks) + (((size_t)nconn + 15) & ~(size_t)15);
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tcp_shut_workspace(uint32_t nconn, uint32_t blocks, size_t *bytes)
{
	if (!bytes || nconn > GCL_SHUT_MAX_CONN || blocks > GCL_SHUT_MAX_BLOCKS)
		return -EINVAL;
	*bytes = shut_workspace(nconn, blocks);
	return 0;
}

extern "C" int gcl_tcp_shut(struct gcl_ctx *c, const struct gcl_shut_in *in, const struct gcl_shut_out *out,
                            uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !in || !out || in->size != sizeof(*in) || in->nconn > GCL_SHUT_MAX_CONN ||
	    in->blocks > GCL_SHUT_MAX_BLOCKS || in->seg_cap > (1ull << 31) || in->frame_stride < GCL_CTL_MIN_STRIDE ||
	    !out->seg.totals)
		return -EINVAL;
	if (in->nconn && (!in->shut || !in->tmr || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if (in->nconn && in->seg_cap &&
	    (!out->seg.desc || !out->seg.frame_off || !out->seg.seg_conn || !out->seg.seg_kind || !out->seg.seg_src ||
	     !out->txq_ent || !out->txq_cold))
		return -EINVAL;
	if (shut_misaligned(in->shut, 16) || shut_misaligned(in->tmr, 16) || shut_misaligned(in->conn, 16) ||
	    shut_misaligned(in->addr, 16) || shut_misaligned(out->out_conn, 16) || shut_misaligned(out->seg.desc, 16) ||
	    shut_misaligned(out->seg.frame_off, 8) || shut_misaligned(out->seg.seg_conn, 4) ||
	    shut_misaligned(out->seg.seg_src, 4) || shut_misaligned(out->txq_ent, 16) ||
	    shut_misaligned(out->txq_cold, 16) || shut_misaligned(out->seg.totals, 8) || shut_misaligned(counts, 8))
		return -EINVAL;
	if (!workspace || shut_misaligned(workspace, 16) || workspace_bytes < shut_workspace(in->nconn, in->blocks))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->nconn == 0)
		return hipMemsetAsync(out->seg.totals, 0, 2 * sizeof(uint64_t), s) == hipSuccess ? 0 : -EIO;

	const uint64_t tiles = ((uint64_t)in->nconn + kShutThreads - 1) / kShutThreads;
	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);
	ShutParams p;

	p.shut = (const uint4 *)in->shut;
	p.tmr = (const uint4 *)in->tmr;
	p.conn = (const uint4 *)in->conn;
	p.addr = (const uint4 *)in->addr;
	p.out_conn = (uint4 *)out->out_conn;
	p.desc = (uint4 *)out->seg.desc;
	p.frame_off = out->seg.frame_off;
	p.seg_conn = out->seg.seg_conn;
	p.seg_kind = out->seg.seg_kind;
	p.seg_src = out->seg.seg_src;
	p.txq_ent = (uint4 *)out->txq_ent;
	p.txq_cold = (uint4 *)out->txq_cold;
	p.totals = (unsigned long long *)out->seg.totals;
	p.counts = (unsigned long long *)counts;
	p.bsum = (uint32_t *)workspace;
	p.want = (uint8_t *)workspace + shut_ws_sums(in->blocks);
	p.now = in->now;
	p.blocks = in->blocks ? in->blocks :
	           (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::min<uint32_t>(cus * kShutBlocksPerCu,
	                                                                                      GCL_SHUT_MAX_BLOCKS)));
	/* whole tiles per range, so that every range starts at a multiple of 256 */
	p.per = std::max<uint64_t>(1, (tiles + p.blocks - 1) / p.blocks) * kShutThreads;
	p.cap = gcl_shut_cap(in->seg_cap, in->frames_len, in->frame_base, in->frame_stride);
	p.frame_base = in->frame_base;
	p.nconn = in->nconn;
	p.frame_stride = in->frame_stride;

	hipLaunchKernelGGL(shut_decide_kernel, dim3(p.blocks), dim3(kShutThreads), 0, s, p);
	hipLaunchKernelGGL(shut_top_kernel, dim3(1), dim3(kShutThreads), 0, s, p);
	hipLaunchKernelGGL(shut_emit_kernel, dim3(p.blocks), dim3(kShutThreads), 0, s, p);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
