/*
 * gcl_payload.hip - payload descriptors and the packed receive layout of a
 * list of packets (gcl_l4_payload, gclassify.h): what udp_conn_recv and
 * tcp_rx_conn find out about a datagram before udp_read_from / tcp_read copy
 * it (runtime/net/udp.c:79-107, :373-379, runtime/net/tcp_in.c:182-218), for
 * every entry of a delivery list at once, and the exclusive scan that lays
 * the kept payloads out back to back.  The rule for one entry is gcl_pay_rule
 * of gcl_pay.h, the same inline code the host twin runs.
 *
 * Three launches on the stream (four with seg_off), and no block ever waits
 * for another: there is no look-back, no flag and no cooperative launch, so a
 * stuck block is impossible by construction; the stream orders the launches.
 * The list is cut into `blocks` contiguous ranges of whole 256-entry tiles
 * (the library's choice: kPayBlocksPerCu blocks per CU, at most
 * GCL_PAY_MAX_BLOCKS and no more than there are tiles; or in->blocks).
 *
 *   describe  block r walks range r tile by tile, one lane per entry.  A lane
 *             loads order[j], then pkt_len, the offset, sock and l4_status of
 *             its packet, then the frame's bytes [12, 48): for a 4-B-aligned
 *             frame whose 16-B-aligned 64-B window (starting up to 12 B before
 *             the frame, as gcl_sock.hip's) lies inside frames[0, frames_len),
 *             the three 16-B chunks of the window that hold them; any other
 *             frame byte by byte, every byte at or past frames_len as 0.  It
 *             writes src_off, len, kind and meta (one 16-B store), coalesced
 *             in j.  The kind counters are ballot popcounts kept per wave;
 *             BYTES and the range's padded length are per-lane u64 sums
 *             reduced over the wave once; a wave adds all eight to 64 bytes
 *             of LDS, seven lanes add the counters to @counts (one add per
 *             counter per block) and one stores the range's padded length to
 *             workspace[r].  Every block stores its word, an empty range 0:
 *             the workspace need not be zeroed.
 *   top       one block turns workspace[0, blocks) into its exclusive prefix
 *             sums in place (four words per lane, then a 256-wide scan in
 *             LDS) and writes *total.
 *   offsets   block r re-reads len[] of range r and scans it tile by tile:
 *             row_shr DPP moves inside a 16-lane row, three lane reads across
 *             the rows, the four waves' totals through LDS (two buffers in
 *             turn: one barrier per tile).  A tile's sums stay in 32 bits
 *             (256 entries of at most 65 536 padded bytes: 2^24); the carry
 *             over the tiles and the range's base from the workspace are
 *             64-bit.  It writes dst_off.
 *   segments  seg_bytes[s] = seg_off[s] < m ? dst_off[seg_off[s]] : *total,
 *             a launch of its own because it reads other blocks' dst_off.
 *
 * Bounds.  A list index is used only below m, a packet index only below n
 * (order[j] >= n is GCL_PAY_OOR and reads nothing), seg_off[s] only below m.
 * With o the offset clamped to frames_len, an aligned window is loaded only
 * when [w, w + 64) lies inside [0, frames_len); the bytewise form tests every
 * byte's index against frames_len - o.  The rule uses a byte only below
 * L = min(pkt_len, frames_len - o).  Nothing is read outside frames[0,
 * frames_len) and the given arrays, nothing written outside the m-element
 * outputs, seg_bytes[0, nseg], total, counts and workspace[0, blocks).
 * No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_pay.h"

namespace gclk {

constexpr uint32_t kPayThreads = 256;
/* the library's choice of ranges: blocks per CU (4 waves each).  The describe
 * kernel's three dependent loads (order, the per-packet arrays, the frame)
 * want many waves in flight; 4 x 256 CUs is also GCL_PAY_MAX_BLOCKS */
constexpr uint32_t kPayBlocksPerCu = 4;
/* workspace words one lane of the top kernel scans */
constexpr uint32_t kPayTopPer = GCL_PAY_MAX_BLOCKS / kPayThreads;
static_assert(kPayTopPer * kPayThreads == GCL_PAY_MAX_BLOCKS, "the top kernel is one block");

struct PayParams {
	const uint8_t *frames;
	uint64_t frames_len;
	uint64_t stride;
	const uint64_t *offs;
	const uint16_t *pkt_len;
	uint64_t n;
	const uint32_t *order;
	const uint32_t *sock;
	const uint8_t *l4_status;
	const uint32_t *seg_off;
	uint64_t *src_off;
	uint16_t *len;
	uint64_t *dst_off;
	uint8_t *kind;
	uint4 *meta;
	uint64_t *seg_bytes;
	uint64_t *total;
	unsigned long long *counts;
	unsigned long long *ws; /* u64[blocks]: range sums, then range bases */
	uint64_t m;             /* <= 2^31 */
	uint64_t per;           /* entries per range: a multiple of kPayThreads */
	uint32_t nseg;
	uint32_t blocks;
	uint32_t amask;         /* align - 1; 0: dense */
};

/* frame dwords 3..11 out of the window's sixteen, the frame starting 4 L bytes in */
template <int L>
__device__ __forceinline__ void pay_pick(const uint4 (&w)[4], uint32_t d[9])
{
	const uint32_t W[16] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w,
	                        w[2].x, w[2].y, w[2].z, w[2].w, w[3].x, w[3].y, w[3].z, w[3].w};
#pragma unroll
	for (int i = 0; i < 9; i++)
		d[i] = W[3 + i + L];
}

/* @v summed over the wave, in every lane; all lanes active */
__device__ __forceinline__ uint64_t pay_wave_sum(uint64_t v)
{
	for (int x = 32; x; x >>= 1) {
		const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, x);
		const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), x);
		v += (uint64_t)hi << 32 | lo;
	}
	return v;
}

__global__ void __launch_bounds__(kPayThreads) pay_describe_kernel(PayParams k)
{
	const uint32_t fbase = (uint32_t)(uintptr_t)k.frames;
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m; /* lo >= m: an empty range */
	uint32_t cnt[GCL_PAY_KINDS] = {0, 0, 0, 0, 0, 0};         /* wave-uniform */
	uint64_t bytes = 0, padded = 0;                           /* this lane's entries */

	for (uint64_t j0 = lo; j0 < hi; j0 += kPayThreads) { /* uniform */
		const uint64_t j = j0 + threadIdx.x;
		uint32_t kind = GCL_PAY_KINDS;
		if (j < hi) {
			const uint64_t i = k.order ? k.order[j] : j;
			struct gcl_pay_desc r = {0, 0, GCL_PAY_OOR, {0, 0, 0, 0}};
			if (i < k.n) {
				const uint32_t st = k.l4_status ? k.l4_status[i] : 0;
				const uint32_t sk = k.sock ? k.sock[i] : 0;
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
						pay_pick<0>(c, d);
					else if (lead == 4)
						pay_pick<1>(c, d);
					else if (lead == 8)
						pay_pick<2>(c, d);
					else
						pay_pick<3>(c, d);
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
				r = gcl_pay_rule(d, o, L, k.l4_status != nullptr, st, k.sock != nullptr, sk);
			}
			k.src_off[j] = r.src_off;
			k.len[j] = (uint16_t)r.len;
			k.kind[j] = (uint8_t)r.kind;
			if (k.meta)
				k.meta[j] = make_uint4(r.meta[0], r.meta[1], r.meta[2], r.meta[3]);
			kind = r.kind;
			bytes += r.len;
			padded += gcl_pay_pad(r.len, k.amask);
		}
#pragma unroll
		for (uint32_t x = 0; x < GCL_PAY_KINDS; x++)
			cnt[x] += (uint32_t)__popcll(__ballot(kind == x));
	}

	/* the block's eight sums: the six kinds by their counter, BYTES, the padded length */
	__shared__ unsigned long long blk[GCL_PAYC_NR];
	if (threadIdx.x < GCL_PAYC_NR)
		blk[threadIdx.x] = 0;
	__syncthreads();
	bytes = pay_wave_sum(bytes);
	padded = pay_wave_sum(padded);
	if ((threadIdx.x & 63) == 0) {
#pragma unroll
		for (uint32_t x = 0; x < GCL_PAY_KINDS; x++)
			atomicAdd(&blk[gcl_pay_counter(x)], (unsigned long long)cnt[x]);
		atomicAdd(&blk[GCL_PAYC_BYTES], (unsigned long long)bytes);
		atomicAdd(&blk[GCL_PAYC_NR - 1], (unsigned long long)padded);
	}
	__syncthreads();
	if (threadIdx.x <= GCL_PAYC_BYTES) {
		if (k.counts && blk[threadIdx.x])
			atomicAdd(k.counts + threadIdx.x, blk[threadIdx.x]);
	} else if (threadIdx.x == GCL_PAYC_NR - 1) {
		k.ws[blockIdx.x] = blk[GCL_PAYC_NR - 1];
	}
}

/* ws[0, blocks) -> its exclusive prefix sums, *total = the sum; one block */
__global__ void __launch_bounds__(kPayThreads) pay_top_kernel(PayParams k)
{
	__shared__ unsigned long long sc[2][kPayThreads];
	const uint32_t t = threadIdx.x;
	unsigned long long v[kPayTopPer], sum = 0;

#pragma unroll
	for (uint32_t x = 0; x < kPayTopPer; x++) {
		const uint32_t r = t * kPayTopPer + x;
		v[x] = r < k.blocks ? k.ws[r] : 0;
		sum += v[x];
	}
	/* inclusive scan of the lanes' sums, ping-pong: one barrier per step */
	uint32_t cur = 0;
	sc[0][t] = sum;
	__syncthreads();
	for (uint32_t step = 1; step < kPayThreads; step <<= 1) {
		const unsigned long long a = sc[cur][t] + (t >= step ? sc[cur][t - step] : 0);
		sc[cur ^ 1][t] = a;
		cur ^= 1;
		__syncthreads();
	}
	unsigned long long base = sc[cur][t] - sum;
#pragma unroll
	for (uint32_t x = 0; x < kPayTopPer; x++) {
		const uint32_t r = t * kPayTopPer + x;
		if (r < k.blocks)
			k.ws[r] = base;
		base += v[x];
	}
	if (t == kPayThreads - 1)
		*k.total = base;
}

/* row_shr:N inside a 16-lane row; a lane with no source gets 0 */
template <int N>
__device__ __forceinline__ uint32_t pay_row_shr(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + N, 0xF, 0xF, false);
}

__global__ void __launch_bounds__(kPayThreads) pay_offsets_kernel(PayParams k)
{
	__shared__ uint32_t wt[2][kPayThreads / 64];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	uint64_t carry = lo < hi ? k.ws[blockIdx.x] : 0; /* the range's base, then the tiles before */
	uint32_t par = 0;

	for (uint64_t j0 = lo; j0 < hi; j0 += kPayThreads, par ^= 1) { /* uniform: every lane active */
		const uint64_t j = j0 + threadIdx.x;
		const uint32_t own = j < hi ? gcl_pay_pad(k.len[j], k.amask) : 0;
		uint32_t v = own;
		v += pay_row_shr<1>(v);
		v += pay_row_shr<2>(v);
		v += pay_row_shr<4>(v);
		v += pay_row_shr<8>(v);
		const uint32_t t0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
		const uint32_t t1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
		const uint32_t t2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 47);
		const uint32_t t3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
		const uint32_t row = lane >> 4;
		v += row == 0 ? 0 : row == 1 ? t0 : row == 2 ? t0 + t1 : t0 + t1 + t2;
		if (lane == 0)
			wt[par][wave] = t0 + t1 + t2 + t3;
		__syncthreads();
		const uint32_t w0 = wt[par][0], w1 = wt[par][1], w2 = wt[par][2], w3 = wt[par][3];
		v += wave == 0 ? 0 : wave == 1 ? w0 : wave == 2 ? w0 + w1 : w0 + w1 + w2;
		if (j < hi)
			k.dst_off[j] = carry + (v - own);
		carry += (uint64_t)w0 + w1 + w2 + w3;
	}
}

__global__ void __launch_bounds__(kPayThreads) pay_segments_kernel(PayParams k)
{
	const uint64_t total = *k.total;
	for (uint64_t s = (uint64_t)blockIdx.x * kPayThreads + threadIdx.x; s <= k.nseg;
	     s += (uint64_t)gridDim.x * kPayThreads) {
		const uint32_t at = k.seg_off[s];
		k.seg_bytes[s] = at < k.m ? k.dst_off[at] : total;
	}
}

static bool misaligned(const void *p, uintptr_t a)
{
	return ((uintptr_t)p & (a - 1)) != 0;
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_l4_payload_workspace(uint64_t m, uint32_t blocks, size_t *bytes)
{
	if (!bytes || m > (1ull << 31) || blocks > GCL_PAY_MAX_BLOCKS)
		return -EINVAL;
	*bytes = (size_t)align16(8u * (blocks ? blocks : GCL_PAY_MAX_BLOCKS));
	return 0;
}

extern "C" int gcl_l4_payload(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_pay_in *in,
                              const struct gcl_pay_out *out, uint64_t *counts, void *workspace,
                              size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	size_t need;

	if (!c || !b || !in || !out || in->size != sizeof(*in) || !gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || gcl_l4_payload_workspace(in->m, in->blocks, &need))
		return -EINVAL;
	if (!out->src_off || !out->len || !out->dst_off || !out->kind || !out->total ||
	    !in->seg_off != !out->seg_bytes)
		return -EINVAL;
	if (misaligned(out->src_off, 8) || misaligned(out->len, 2) || misaligned(out->dst_off, 8) ||
	    misaligned(out->meta, 16) || misaligned(out->seg_bytes, 8) || misaligned(out->total, 8) ||
	    misaligned(in->order, 4) || misaligned(in->sock, 4) || misaligned(in->seg_off, 4) ||
	    misaligned(counts, 8))
		return -EINVAL;
	if (!workspace || misaligned(workspace, 16) || workspace_bytes < need)
		return -EINVAL;
	if (in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	              (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	              !b->pkt_len || misaligned(b->pkt_len, 2)))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	if (in->m == 0) {
		HipErr he;
		he(hipMemsetAsync(out->total, 0, sizeof(uint64_t), s));
		if (out->seg_bytes)
			he(hipMemsetAsync(out->seg_bytes, 0, ((size_t)in->nseg + 1) * sizeof(uint64_t), s));
		return he.bad() ? -EIO : 0;
	}

	PayParams k;
	k.frames = b->frames;
	k.frames_len = b->frames_len;
	k.stride = b->stride;
	k.offs = b->offs;
	k.pkt_len = b->pkt_len;
	k.n = b->n;
	k.order = in->order;
	k.sock = in->sock;
	k.l4_status = in->l4_status;
	k.seg_off = in->seg_off;
	k.src_off = out->src_off;
	k.len = out->len;
	k.dst_off = out->dst_off;
	k.kind = out->kind;
	k.meta = (uint4 *)out->meta;
	k.seg_bytes = out->seg_bytes;
	k.total = out->total;
	k.counts = (unsigned long long *)counts;
	k.ws = (unsigned long long *)workspace;
	k.m = in->m;
	k.nseg = in->nseg;
	k.amask = in->align ? in->align - 1 : 0;

	const uint64_t tiles = (in->m + kPayThreads - 1) / kPayThreads;
	k.blocks = in->blocks ? in->blocks :
	           (uint32_t)std::min<uint64_t>(tiles, std::min<uint32_t>((uint32_t)c->num_cus * kPayBlocksPerCu,
	                                                                   GCL_PAY_MAX_BLOCKS));
	/* whole tiles per range, so that every range starts at a multiple of 256 */
	k.per = (tiles + k.blocks - 1) / k.blocks * kPayThreads;

	hipLaunchKernelGGL(pay_describe_kernel, dim3(k.blocks), dim3(kPayThreads), 0, s, k);
	hipLaunchKernelGGL(pay_top_kernel, dim3(1), dim3(kPayThreads), 0, s, k);
	hipLaunchKernelGGL(pay_offsets_kernel, dim3(k.blocks), dim3(kPayThreads), 0, s, k);
	if (k.seg_off) {
		const uint64_t want = ((uint64_t)k.nseg + 1 + kPayThreads - 1) / kPayThreads;
		const unsigned grid = (unsigned)std::min<uint64_t>(want, (uint64_t)c->num_cus * kPayBlocksPerCu);
		hipLaunchKernelGGL(pay_segments_kernel, dim3(grid), dim3(kPayThreads), 0, s, k);
	}
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
