/*
 * gcl_seg.hip - cut a batch of socket writes into tx segments (gcl_tx_seg,
 * gclassify.h): tcp_write3's window clamp, the segmenter loop of tcp_tx_send
 * and udp_write_to's size check (runtime/net/tcp.c:1362-1380, tcp_out.c:
 * 313-386, udp.c:590-591) for m writes at once, and the scan that lays the
 * segments out.  The rule is gcl_seg_rule / gcl_seg_emit of gcl_seg.h, the
 * same inline code the host twin runs.
 *
 * One write becomes 1 to 2^32 - 1 segments, so the work is cut by OUTPUT: the
 * three per-write launches only count and scan, and the expansion has one
 * lane per segment, never a lane looping over a write's segments.
 *
 * Four launches on the stream, and no block ever waits for another: no
 * look-back, no flag, no cooperative launch; the stream orders the launches.
 * The writes are cut into `blocks` contiguous ranges of whole 256-write tiles
 * (the library's choice, or in->blocks), as gcl_l4_payload cuts its list.
 *
 *   count    block r walks range r, one lane per write: three 16-B loads of
 *            the write, the rule, then the provisional per-write outputs
 *            (status with GCL_SEG_ST_TCP for a TCP write, sent = L,
 *            snd_nxt_out = snd_nxt + L, nseg) and the write's layout bytes to
 *            the workspace.  The range's triple (segments, layout bytes,
 *            writes not refused) goes to workspace range r; every block
 *            stores it, an empty range zeros.
 *   top      one block turns the range triples into their exclusive prefix
 *            sums in place and writes the totals of a batch in which
 *            everything fits.
 *   writes   block r scans range r tile by tile (shuffles inside a wave, the
 *            four waves' totals through LDS, two buffers in turn: one barrier
 *            per tile) and so knows S_i, B_i and the rank among the writes not
 *            refused.  It decides OK or NOSPACE, finishes the per-write
 *            outputs, and for an OK write stores B_i over its layout bytes
 *            and (S_i, i) at its rank in the compacted list: the OK writes are
 *            a prefix of the writes not refused, so the rank needs no second
 *            scan.  The first NOSPACE write, if any, is the one lane of the
 *            grid whose own sums still fit; it stores the totals.  Counters:
 *            ballot popcounts and per-lane sums reduced once per block, one
 *            add per counter per block.
 *   expand   one lane per segment g < *total_segs, a block a contiguous run
 *            of 256-segment tiles.  The block finds the write of its first
 *            segment with one uniform binary search over the compacted S;
 *            the compacted list holds only writes with segments, so a tile of
 *            256 segments spans at most 256 of its entries however many
 *            refused writes lie between them: the block loads that window
 *            (257 S values, 256 indices) into LDS, a lane finds its write in
 *            eight LDS steps, and lane 255's answer is the next tile's start.
 *            A lane loads its write (neighbours share it: one line), emits
 *            and stores desc (two 16-B stores), frame_off, src_off, len,
 *            dst_off and send_idx, all coalesced in g.
 *
 * Bounds.  A write index is used only below m (the compacted index is clamped
 * to m - 1 besides), a compacted rank only below the number of OK writes
 * (clamped to m), a segment index only below min(*total_segs, seg_cap); the
 * window reads LDS at t + step <= 255 and t + 1 <= 256.  Nothing is read
 * outside send[0, m) and the workspace, nothing written outside the first
 * *total_segs <= seg_cap entries of the per-segment arrays, the m-element
 * per-write arrays, the totals, counts and the workspace.  No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_seg.h"

namespace gclk {

constexpr uint32_t kSegThreads = 256;
/* ranges per CU for the per-write launches, tile runs per CU for the expansion */
constexpr uint32_t kSegBlocksPerCu = 4;
constexpr uint32_t kSegExpandPerCu = 8;
constexpr uint32_t kSegTopPer = GCL_SEG_MAX_BLOCKS / kSegThreads;
static_assert(kSegTopPer * kSegThreads == GCL_SEG_MAX_BLOCKS, "the top kernel is one block");

/* segments, layout bytes (saturating) and writes not refused */
struct SegTri {
	unsigned long long s, b, e;
};
struct SegRange {
	SegTri t;
	unsigned long long pad;
};
static_assert(sizeof(SegRange) == 32, "workspace layout");

struct SegParams {
	const uint4 *send;
	uint8_t *status;
	uint32_t *sent, *snd_nxt_out, *seg_first, *nseg;
	uint4 *desc;
	uint64_t *frame_off, *src_off;
	uint16_t *len;
	uint64_t *dst_off;
	uint32_t *send_idx;
	unsigned long long *total_segs, *total_bytes;
	unsigned long long *counts;
	SegRange *ranges;          /* workspace: [blocks] */
	unsigned long long *nok;   /* workspace: the number of OK writes */
	unsigned long long *wb;    /* workspace: u64[m], layout bytes, then B_i of the OK writes */
	uint32_t *cfirst, *cidx;   /* workspace: u32[m] each, S_i and i of the OK writes, compacted */
	uint64_t m, per;           /* per: writes per range, a multiple of kSegThreads */
	uint64_t seg_cap, byte_cap;
	uint64_t first_byte;       /* frame_base + lead */
	uint32_t stride, lead, udp_max, blocks;
};

__device__ __forceinline__ SegTri seg_add(const SegTri &a, const SegTri &b)
{
	return SegTri{a.s + b.s, gcl_seg_sat(a.b, b.b), a.e + b.e};
}

__device__ __forceinline__ unsigned long long seg_shfl_up(unsigned long long v, int d)
{
	const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d);
	const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d);
	return (unsigned long long)hi << 32 | lo;
}

__device__ __forceinline__ unsigned long long seg_shfl_xor(unsigned long long v, int x)
{
	const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, x);
	const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), x);
	return (unsigned long long)hi << 32 | lo;
}

/* @v summed over the wave, in every lane; all lanes active */
__device__ __forceinline__ SegTri seg_wave_sum(SegTri v)
{
	for (int x = 32; x; x >>= 1)
		v = seg_add(v, SegTri{seg_shfl_xor(v.s, x), seg_shfl_xor(v.b, x), seg_shfl_xor(v.e, x)});
	return v;
}

__device__ __forceinline__ void seg_load(const SegParams &k, uint64_t i, uint32_t s[12])
{
	const uint4 a = k.send[3 * i], b = k.send[3 * i + 1], c = k.send[3 * i + 2];
	s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
	s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
	s[8] = c.x; s[9] = c.y; s[10] = c.z; s[11] = c.w;
}

__global__ void __launch_bounds__(kSegThreads) seg_count_kernel(SegParams k)
{
	__shared__ SegTri wt[kSegThreads / 64];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m; /* lo >= m: an empty range */
	SegTri sum = {0, 0, 0};                                   /* this lane's writes */

	for (uint64_t i = lo + threadIdx.x; i < hi; i += kSegThreads) {
		uint32_t s[12];
		seg_load(k, i, s);
		const struct gcl_seg_plan p = gcl_seg_rule(s, k.udp_max, k.stride, k.lead);
		const bool nonref = p.status == GCL_SEG_OK;
		k.status[i] = (uint8_t)(nonref ? GCL_SEG_OK | (p.tcp ? GCL_SEG_ST_TCP : 0) : GCL_SEG_REFUSED);
		k.sent[i] = p.L;
		k.snd_nxt_out[i] = s[4] + p.L;
		k.nseg[i] = p.nseg;
		k.wb[i] = p.wbytes;
		sum = seg_add(sum, SegTri{p.nseg, p.wbytes, nonref ? 1ull : 0ull});
	}
	sum = seg_wave_sum(sum);
	if ((threadIdx.x & 63) == 0)
		wt[threadIdx.x >> 6] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		SegRange r = {seg_add(seg_add(wt[0], wt[1]), seg_add(wt[2], wt[3])), 0};
		k.ranges[blockIdx.x] = r;
	}
}

/* ranges[0, blocks) -> their exclusive prefix sums; the totals when everything fits; one block */
__global__ void __launch_bounds__(kSegThreads) seg_top_kernel(SegParams k)
{
	__shared__ SegTri sc[2][kSegThreads];
	const uint32_t t = threadIdx.x;
	SegTri v[kSegTopPer], sum = {0, 0, 0};

#pragma unroll
	for (uint32_t x = 0; x < kSegTopPer; x++) {
		const uint32_t r = t * kSegTopPer + x;
		v[x] = r < k.blocks ? k.ranges[r].t : SegTri{0, 0, 0};
		sum = seg_add(sum, v[x]);
	}
	/* inclusive scan of the lanes' sums, ping-pong: one barrier per step */
	uint32_t cur = 0;
	sc[0][t] = sum;
	__syncthreads();
	for (uint32_t step = 1; step < kSegThreads; step <<= 1) {
		const SegTri a = t >= step ? seg_add(sc[cur][t - step], sc[cur][t]) : sc[cur][t];
		sc[cur ^ 1][t] = a;
		cur ^= 1;
		__syncthreads();
	}
	SegTri base = t ? sc[cur][t - 1] : SegTri{0, 0, 0};
#pragma unroll
	for (uint32_t x = 0; x < kSegTopPer; x++) {
		const uint32_t r = t * kSegTopPer + x;
		if (r < k.blocks)
			k.ranges[r].t = base;
		base = seg_add(base, v[x]);
	}
	if (t == kSegThreads - 1) {
		/* when a write does not fit, the first such write stores these instead (seg_writes_kernel) */
		const bool fits = base.s <= k.seg_cap && base.b <= k.byte_cap;
		*k.total_segs = fits ? base.s : 0;
		*k.total_bytes = fits ? base.b : 0;
		*k.nok = fits ? base.e : 0;
	}
}

__global__ void __launch_bounds__(kSegThreads) seg_writes_kernel(SegParams k)
{
	__shared__ SegTri wt[2][kSegThreads / 64];
	__shared__ unsigned long long blk[GCL_SEGC_NR];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	SegTri carry = lo < hi ? k.ranges[blockIdx.x].t : SegTri{0, 0, 0}; /* the range's base, then the tiles before */
	uint32_t cnt[3] = {0, 0, 0}, push = 0;                              /* wave-uniform */
	unsigned long long segs = 0, bytes = 0;                             /* this lane's OK writes */
	uint32_t par = 0;

	for (uint64_t j0 = lo; j0 < hi; j0 += kSegThreads, par ^= 1) { /* uniform: every lane active */
		const uint64_t i = j0 + threadIdx.x;
		const bool in = i < hi;
		const uint32_t st = in ? k.status[i] : GCL_SEG_REFUSED;
		const uint32_t n = in ? k.nseg[i] : 0, L = in ? k.sent[i] : 0;
		const unsigned long long w = in ? k.wb[i] : 0;
		const bool nonref = st != GCL_SEG_REFUSED;

		SegTri v = {n, w, nonref ? 1ull : 0ull};
		for (int d = 1; d < 64; d <<= 1) {
			const SegTri u = {seg_shfl_up(v.s, d), seg_shfl_up(v.b, d), seg_shfl_up(v.e, d)};
			if (lane >= (uint32_t)d)
				v = seg_add(u, v);
		}
		if (lane == 63)
			wt[par][wave] = v;
		/* exclusive inside the wave */
		SegTri ex = {seg_shfl_up(v.s, 1), seg_shfl_up(v.b, 1), seg_shfl_up(v.e, 1)};
		if (lane == 0)
			ex = SegTri{0, 0, 0};
		__syncthreads();
		const SegTri w0 = wt[par][0], w1 = wt[par][1], w2 = wt[par][2], w3 = wt[par][3];
		SegTri at = carry;
		if (wave > 0)
			at = seg_add(at, w0);
		if (wave > 1)
			at = seg_add(at, w1);
		if (wave > 2)
			at = seg_add(at, w2);
		at = seg_add(at, ex);
		carry = seg_add(seg_add(carry, seg_add(w0, w1)), seg_add(w2, w3));

		/* S + n < 2^63 and at.b, w <= 2^62: neither test can wrap */
		const bool fits = nonref && at.s + n <= k.seg_cap && gcl_seg_sat(at.b, w) <= k.byte_cap;
		const uint32_t status = !in ? 3u : !nonref ? GCL_SEG_REFUSED : fits ? GCL_SEG_OK : GCL_SEG_NOSPACE;
		if (in) {
			k.status[i] = (uint8_t)status;
			k.seg_first[i] = (uint32_t)(at.s < k.seg_cap ? at.s : k.seg_cap);
			if (fits) {
				k.wb[i] = at.b;
				k.cfirst[at.e] = (uint32_t)at.s; /* at.e <= i: every write before is counted at most once */
				k.cidx[at.e] = (uint32_t)i;
				segs += n;
				bytes += L;
			} else if (nonref) {
				k.sent[i] = 0;
				k.snd_nxt_out[i] = k.snd_nxt_out[i] - L;
				k.nseg[i] = 0;
				if (at.s <= k.seg_cap && at.b <= k.byte_cap) { /* the first write that does not fit */
					*k.total_segs = at.s;
					*k.total_bytes = at.b;
					*k.nok = at.e;
				}
			}
		}
#pragma unroll
		for (uint32_t x = 0; x < 3; x++)
			cnt[x] += (uint32_t)__popcll(__ballot(status == x));
		push += (uint32_t)__popcll(__ballot(fits && (st & GCL_SEG_ST_TCP)));
	}

	if (!k.counts)
		return;
	if (threadIdx.x < GCL_SEGC_NR)
		blk[threadIdx.x] = 0;
	__syncthreads();
	for (int x = 32; x; x >>= 1) {
		segs += seg_shfl_xor(segs, x);
		bytes += seg_shfl_xor(bytes, x);
	}
	if (lane == 0) {
		atomicAdd(&blk[GCL_SEGC_OK], (unsigned long long)cnt[GCL_SEG_OK]);
		atomicAdd(&blk[GCL_SEGC_REFUSED], (unsigned long long)cnt[GCL_SEG_REFUSED]);
		atomicAdd(&blk[GCL_SEGC_NOSPACE], (unsigned long long)cnt[GCL_SEG_NOSPACE]);
		atomicAdd(&blk[GCL_SEGC_SEGS], segs);
		atomicAdd(&blk[GCL_SEGC_BYTES], bytes);
		atomicAdd(&blk[GCL_SEGC_PUSH], (unsigned long long)push);
	}
	__syncthreads();
	if (threadIdx.x <= GCL_SEGC_PUSH && blk[threadIdx.x])
		atomicAdd(k.counts + threadIdx.x, blk[threadIdx.x]);
}

__global__ void __launch_bounds__(kSegThreads) seg_expand_kernel(SegParams k)
{
	__shared__ uint32_t wf[kSegThreads + 1], wi[kSegThreads];
	__shared__ unsigned long long next_e;
	const unsigned long long ts = *k.total_segs, no = *k.nok;
	const uint64_t total = ts < k.seg_cap ? ts : k.seg_cap; /* <= 2^31 */
	const uint64_t ne = no < k.m ? no : k.m;
	if (total == 0 || ne == 0)
		return;
	const uint64_t tiles = (total + kSegThreads - 1) / kSegThreads;
	const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x;
	const uint64_t t0 = blockIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
	if (t0 >= t1)
		return;

	/* the last e with cfirst[e] <= the block's first segment: cfirst[0] is 0.  Uniform. */
	uint64_t e0 = 0;
	{
		const uint32_t g0 = (uint32_t)(t0 * kSegThreads);
		uint64_t end = ne;
		while (end - e0 > 1) {
			const uint64_t mid = e0 + (end - e0) / 2;
			if (k.cfirst[mid] <= g0)
				e0 = mid;
			else
				end = mid;
		}
	}

	for (uint64_t tile = t0; tile < t1; tile++) { /* uniform */
		const uint32_t g = (uint32_t)(tile * kSegThreads) + threadIdx.x; /* < 2^31 + 256 */
		const uint64_t e = e0 + threadIdx.x;
		wf[threadIdx.x] = e < ne ? k.cfirst[e] : UINT32_MAX;
		wi[threadIdx.x] = e < ne ? k.cidx[e] : 0;
		if (threadIdx.x == 0)
			wf[kSegThreads] = e0 + kSegThreads < ne ? k.cfirst[e0 + kSegThreads] : UINT32_MAX;
		__syncthreads();
		/* the last t with wf[t] <= g: wf[0] <= the tile's first segment */
		uint32_t t = 0;
#pragma unroll
		for (uint32_t step = kSegThreads / 2; step; step >>= 1)
			if (wf[t + step] <= g)
				t += step;
		if (g < total) {
			const uint64_t i = wi[t] < k.m ? wi[t] : k.m - 1;
			uint32_t s[12];
			seg_load(k, i, s);
			const struct gcl_seg_one r = gcl_seg_emit(s, g - wf[t], k.first_byte + k.wb[i], k.stride);
			k.desc[2 * (uint64_t)g] = make_uint4(r.d[0], r.d[1], r.d[2], r.d[3]);
			k.desc[2 * (uint64_t)g + 1] = make_uint4(r.d[4], r.d[5], r.d[6], r.d[7]);
			k.frame_off[g] = r.frame_off;
			k.src_off[g] = r.src_off;
			k.len[g] = (uint16_t)r.paylen;
			k.dst_off[g] = r.dst_off;
			if (k.send_idx)
				k.send_idx[g] = (uint32_t)i;
		}
		if (threadIdx.x == kSegThreads - 1) /* the next tile starts in this lane's write or the one after */
			next_e = e0 + t + (wf[t + 1] <= g + 1 ? 1 : 0);
		__syncthreads();
		e0 = next_e;
	}
}

static bool seg_misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tx_seg_workspace(uint64_t m, uint32_t blocks, size_t *bytes)
{
	if (!bytes || m > (1ull << 31) || blocks > GCL_SEG_MAX_BLOCKS)
		return -EINVAL;
	*bytes = sizeof(SegRange) * (size_t)(blocks ? blocks : GCL_SEG_MAX_BLOCKS) + 16 + 16 * (size_t)m;
	return 0;
}

extern "C" int gcl_tx_seg(struct gcl_ctx *c, const struct gcl_seg_in *in, const struct gcl_seg_out *out,
                          uint64_t *counts, void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	size_t need;

	if (!c || !in || !out || in->size != sizeof(*in) || in->seg_cap > (1ull << 31) ||
	    in->stride > GCL_SEG_MAX_STRIDE || in->lead > GCL_SEG_MAX_LEAD || in->udp_max > GCL_SEG_MAX_UDP ||
	    !out->total_segs || !out->total_bytes || gcl_tx_seg_workspace(in->m, in->blocks, &need))
		return -EINVAL;
	if (in->m && (!in->send || !out->status || !out->sent || !out->snd_nxt_out || !out->seg_first ||
	              !out->nseg))
		return -EINVAL;
	if (in->m && in->seg_cap && (!out->desc || !out->frame_off || !out->src_off || !out->len ||
	                             !out->dst_off))
		return -EINVAL;
	if (seg_misaligned(in->send, 16) || seg_misaligned(out->sent, 4) || seg_misaligned(out->snd_nxt_out, 4) ||
	    seg_misaligned(out->seg_first, 4) || seg_misaligned(out->nseg, 4) || seg_misaligned(out->desc, 16) ||
	    seg_misaligned(out->frame_off, 8) || seg_misaligned(out->src_off, 8) || seg_misaligned(out->len, 2) ||
	    seg_misaligned(out->dst_off, 8) || seg_misaligned(out->send_idx, 4) ||
	    seg_misaligned(out->total_segs, 8) || seg_misaligned(out->total_bytes, 8) || seg_misaligned(counts, 8))
		return -EINVAL;
	if (!workspace || seg_misaligned(workspace, 16) || workspace_bytes < need)
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->m == 0) {
		HipErr he;
		he(hipMemsetAsync(out->total_segs, 0, sizeof(uint64_t), s));
		he(hipMemsetAsync(out->total_bytes, 0, sizeof(uint64_t), s));
		return he.bad() ? -EIO : 0;
	}

	SegParams k;
	const uint64_t tiles = (in->m + kSegThreads - 1) / kSegThreads;
	k.blocks = in->blocks ? in->blocks :
	           (uint32_t)std::min<uint64_t>(tiles, std::min<uint32_t>((uint32_t)c->num_cus * kSegBlocksPerCu,
	                                                                   GCL_SEG_MAX_BLOCKS));
	/* whole tiles per range, so that every range starts at a multiple of 256 */
	k.per = (tiles + k.blocks - 1) / k.blocks * kSegThreads;
	uint8_t *ws = (uint8_t *)workspace;
	const size_t nranges = in->blocks ? in->blocks : GCL_SEG_MAX_BLOCKS;
	k.ranges = (SegRange *)ws;
	k.nok = (unsigned long long *)(ws + sizeof(SegRange) * nranges);
	k.wb = k.nok + 2;
	k.cfirst = (uint32_t *)(k.wb + in->m);
	k.cidx = k.cfirst + in->m;
	k.send = (const uint4 *)in->send;
	k.status = out->status;
	k.sent = out->sent;
	k.snd_nxt_out = out->snd_nxt_out;
	k.seg_first = out->seg_first;
	k.nseg = out->nseg;
	k.desc = (uint4 *)out->desc;
	k.frame_off = out->frame_off;
	k.src_off = out->src_off;
	k.len = out->len;
	k.dst_off = out->dst_off;
	k.send_idx = out->send_idx;
	k.total_segs = (unsigned long long *)out->total_segs;
	k.total_bytes = (unsigned long long *)out->total_bytes;
	k.counts = (unsigned long long *)counts;
	k.m = in->m;
	k.seg_cap = in->seg_cap;
	k.byte_cap = gcl_seg_byte_cap(in->frames_len, in->frame_base, in->stride, in->lead);
	k.first_byte = in->frame_base + in->lead;
	k.stride = in->stride;
	k.lead = in->lead;
	k.udp_max = in->udp_max;

	hipLaunchKernelGGL(seg_count_kernel, dim3(k.blocks), dim3(kSegThreads), 0, s, k);
	hipLaunchKernelGGL(seg_top_kernel, dim3(1), dim3(kSegThreads), 0, s, k);
	hipLaunchKernelGGL(seg_writes_kernel, dim3(k.blocks), dim3(kSegThreads), 0, s, k);
	if (in->seg_cap) {
		const uint64_t want = (in->seg_cap + kSegThreads - 1) / kSegThreads;
		const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)c->num_cus * kSegExpandPerCu);
		hipLaunchKernelGGL(seg_expand_kernel, dim3(grid), dim3(kSegThreads), 0, s, k);
	}
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
