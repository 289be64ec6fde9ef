/*
 * gcl_copy.hip - the loopback frame copy of a batch (gcl_copy_batch,
 * gclassify.h): copy_batch of rx_loopback (iokernel/rx.c:264, iokernel/dma.c:
 * 167-191), n frames of any length at any byte alignment out of the tx region
 * into the rx pool, with pkt_len, ol_flags and hash beside them.
 *
 * One launch.  A group of G neighbouring lanes (4, 16 or 64, a template
 * parameter; the host picks it from len_hint, any G is correct for any length)
 * owns one packet, so a wave holds 64 / G packets and a block 256 / G.  Every
 * lane of the group reads the packet's len, src_off and dst_off (one address
 * per group: the loads coalesce) and judges the refusal for itself; the
 * group's first lane writes pkt_len, olflags and rss.
 *
 * The destination range [d, d + L) is cut at the 16-B boundaries of dst + d
 * into a head of up to 15 bytes, a body of whole aligned 16-B chunks and a
 * tail of up to 15 bytes.  Head and tail bytes are stored one byte per store,
 * dealt over the group's lanes.  Body chunk c belongs to lane c % G and leaves
 * as one aligned 16-B store; it is built from the one or two aligned 16-B
 * source loads that cover it, funnel-shifted by sh = (source address -
 * destination address) & 15, which is the same for every chunk of a packet
 * (sh == 0: one load).  A lane issues the loads of kCopyUnroll chunks, G
 * chunks apart, before it stores the first of them.  Loads and stores are
 * plain (the second load of a shifted chunk is the first load of the next
 * lane's chunk and is served by the CU's L1).
 *
 * Bounds.  A packet index is used only below n.  A packet is copied only when
 * d <= dst_len and L <= dst_len - d (no sum formed), and every store is made
 * at a byte index j of the packet with j < L, or at a chunk [j, j + 16) with
 * j + 16 <= L: nothing is written outside [d, d + L), and no wider word is
 * read-modify-written.  The source is addressed through avail = src_len -
 * src_off (0 when src_off >= src_len, and then no source address is formed):
 * a byte j is read only when j < avail; the aligned loads of a chunk are
 * issued only when the 16 or 32 bytes they read start at or after src and end
 * at or before src + src_len, and a chunk for which they do not (the region's
 * first and last bytes, a frame cut by src_len, an offset past it) is read
 * byte by byte under the j < avail test, bytes past it reading 0.
 *
 * The counters: COPIED and REFUSED are ballot popcounts kept per wave, BYTES a
 * per-lane sum reduced over the wave once; a wave adds them to 24 bytes of
 * LDS and three lanes of the block add those to @counts, one add per counter
 * per block.  The grid is capped at kCopyBlocksPerCu blocks per CU
 * (gcl_tune.blocks_per_cu overrides it for A/Bs) and loops.  No inline
 * assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_device.h"

namespace gclk {

constexpr uint32_t kCopyThreads = 256;
/* grid cap: blocks per CU.  The kernels take 76-78 VGPRs, 6 waves per SIMD, so
 * 6 blocks of 4 waves are resident on a CU; a seventh would wait for a slot
 * (tools/copy_bench.py times 4, 6 and 8) */
constexpr uint32_t kCopyBlocksPerCu = 6;
/* chunks a lane has in flight: loads of all of them, then their stores */
constexpr uint32_t kCopyUnroll = 4;

struct CopyParams {
	const uint8_t *src;
	uint64_t src_len;
	const uint64_t *src_off;
	const uint16_t *len;
	const uint8_t *tx_olflags;
	const uint32_t *hash;
	uint8_t *dst;
	uint64_t dst_len;
	const uint64_t *dst_off;
	uint64_t dst_stride;
	uint16_t *pkt_len;
	uint8_t *olflags;
	uint32_t *rss;
	unsigned long long *counts;
	uint64_t n;
	uint32_t dst_cap;
};

/* bytes [sh, sh + 16) of the 32 bytes @lo, @hi (sh in [0, 16)) */
__device__ __forceinline__ uint4 copy_funnel(const uint4 &lo, const uint4 &hi, uint32_t sh)
{
	const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
	const uint32_t d = sh >> 2, b = sh & 3;
	uint32_t r[4];
#pragma unroll
	for (int i = 0; i < 4; i++) {
		const uint32_t x = d == 0 ? w[i] : d == 1 ? w[i + 1] : d == 2 ? w[i + 2] : w[i + 3];
		const uint32_t y = d == 0 ? w[i + 1] : d == 1 ? w[i + 2] : d == 2 ? w[i + 3] : w[i + 4];
		r[i] = __builtin_amdgcn_alignbyte(y, x, b);
	}
	return make_uint4(r[0], r[1], r[2], r[3]);
}

/* One packet by its group: lane @sub of G copies its share of the L > 0 bytes
 * at source offset @so to destination offset @d (judged to fit). */
template <uint32_t G>
__device__ __forceinline__ void copy_frame(const CopyParams &k, uint64_t so, uint64_t d, uint32_t L,
                                           uint32_t sub)
{
	/* source bytes the frame has before src_len; no address past the region */
	const uint64_t avail = so < k.src_len ? k.src_len - so : 0;
	const uint8_t *s = k.src + (avail ? so : 0);
	uint8_t *t = k.dst + d;
	auto byte = [&](uint32_t j) -> uint32_t { return j < avail ? s[j] : 0u; };

	const uint32_t lead = (uint32_t)(0 - (uintptr_t)t) & 15;
	const uint32_t h = lead < L ? lead : L;      /* head bytes */
	const uint32_t nb = (L - h) >> 4;            /* body chunks */
	const uint32_t tail0 = h + 16 * nb;          /* the tail is [tail0, L) */
	const uint32_t edge = h + (L - tail0);

	for (uint32_t x = sub; x < edge; x += G) {
		const uint32_t j = x < h ? x : x - h + tail0;
		t[j] = (uint8_t)byte(j);
	}
	if (!nb)
		return;

	const uint32_t sh = ((uint32_t)(uintptr_t)s + h) & 15;
	const uint32_t span = sh ? 32 - sh : 16;     /* bytes the aligned loads read from byte j on */
	for (uint32_t c0 = sub; c0 < nb; c0 += kCopyUnroll * G) {
		uint4 lo[kCopyUnroll], hi[kCopyUnroll];
		bool fast[kCopyUnroll];
#pragma unroll
		for (uint32_t u = 0; u < kCopyUnroll; u++) {
			const uint32_t c = c0 + u * G, j = h + 16 * c;
			/* [so + j - sh, so + j + span) inside [0, src_len) */
			fast[u] = c < nb && (so >= sh || so + j >= sh) && (uint64_t)j + span <= avail;
			lo[u] = hi[u] = make_uint4(0, 0, 0, 0);
			if (fast[u]) {
				const uint8_t *a = s + j - sh;
				lo[u] = *(const uint4 *)a;
				if (sh)
					hi[u] = *(const uint4 *)(a + 16);
			}
		}
#pragma unroll
		for (uint32_t u = 0; u < kCopyUnroll; u++) {
			const uint32_t c = c0 + u * G, j = h + 16 * c;
			if (c >= nb)
				break;
			uint4 v;
			if (fast[u]) {
				v = copy_funnel(lo[u], hi[u], sh);
			} else { /* rare: the region's ends */
				uint32_t r[4];
				for (uint32_t i = 0; i < 4; i++)
					r[i] = byte(j + 4 * i) | byte(j + 4 * i + 1) << 8 | byte(j + 4 * i + 2) << 16 |
					       byte(j + 4 * i + 3) << 24;
				v = make_uint4(r[0], r[1], r[2], r[3]);
			}
			*(uint4 *)(t + j) = v;
		}
	}
}

template <uint32_t G>
__global__ void __launch_bounds__(kCopyThreads) copy_kernel(CopyParams k)
{
	constexpr uint32_t kPerBlock = kCopyThreads / G, kPerWave = 64 / G;
	const uint32_t lane = threadIdx.x & 63, sub = lane % G;
	const uint64_t step = (uint64_t)gridDim.x * kPerBlock;
	uint32_t n_copied = 0, n_refused = 0; /* wave-uniform */
	uint64_t bytes = 0;                   /* this lane's packets */

	/* the wave's first packet decides: every lane of a wave makes the same passes */
	for (uint64_t pw = (uint64_t)blockIdx.x * kPerBlock + (threadIdx.x >> 6) * kPerWave; pw < k.n;
	     pw += step) {
		const uint64_t p = pw + lane / G;
		const bool valid = p < k.n;
		uint32_t L = 0;
		uint64_t so = 0, d = 0;
		bool copied = false;
		if (valid) {
			L = k.len[p];
			so = k.src_off[p];
			d = k.dst_off ? k.dst_off[p] : p * k.dst_stride;
			copied = !((k.dst_cap && L > k.dst_cap) || (!k.dst_off && L > k.dst_stride) ||
			           d > k.dst_len || L > k.dst_len - d);
			if (sub == 0) {
				k.pkt_len[p] = (uint16_t)(copied ? L : 0);
				if (k.olflags) /* gcl_loopback_olflags: TXFLAG_LOCAL_HINT is bit 6 */
					k.olflags[p] = (uint8_t)(((k.tx_olflags ? k.tx_olflags[p] : 0) & 0x40 ? GCL_F_RSS_HASH : 0) |
					                         GCL_F_IP_CKSUM_GOOD);
				if (k.rss)
					k.rss[p] = k.hash ? k.hash[p] : 0;
				bytes += copied ? L : 0;
			}
		}
		n_copied += (uint32_t)__popcll(__ballot(valid && sub == 0 && copied));
		n_refused += (uint32_t)__popcll(__ballot(valid && sub == 0 && !copied));
		if (copied && L)
			copy_frame<G>(k, so, d, L, sub);
	}

	if (k.counts) { /* uniform */
		__shared__ unsigned long long blk[3];
		if (threadIdx.x < 3)
			blk[threadIdx.x] = 0;
		__syncthreads();
		uint32_t blo = (uint32_t)bytes, bhi = (uint32_t)(bytes >> 32);
		for (int o = 32; o; o >>= 1) {
			const uint64_t other = (uint64_t)(uint32_t)__shfl_xor((int)bhi, o) << 32 |
			                       (uint32_t)__shfl_xor((int)blo, o);
			bytes += other;
			blo = (uint32_t)bytes;
			bhi = (uint32_t)(bytes >> 32);
		}
		if (lane == 0) {
			atomicAdd(&blk[GCL_COPY_COPIED], (unsigned long long)n_copied);
			atomicAdd(&blk[GCL_COPY_REFUSED], (unsigned long long)n_refused);
			atomicAdd(&blk[GCL_COPY_BYTES], (unsigned long long)bytes);
		}
		__syncthreads();
		if (threadIdx.x < 3 && blk[threadIdx.x])
			atomicAdd(k.counts + threadIdx.x, blk[threadIdx.x]);
	}
}

template <uint32_t G>
static void copy_launch(const CopyParams &k, uint32_t blocks_cap, hipStream_t s)
{
	constexpr uint32_t per_block = kCopyThreads / G;
	const uint64_t need = (k.n + per_block - 1) / per_block;
	const unsigned grid = (unsigned)std::min<uint64_t>(blocks_cap, need);
	hipLaunchKernelGGL(copy_kernel<G>, dim3(grid), dim3(kCopyThreads), 0, s, k);
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_copy_batch(struct gcl_ctx *c, const struct gcl_copy_in *in,
                              const struct gcl_copy_out *out, uint64_t *counts, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	auto misaligned = [](const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };

	if (!c || !in || !out || in->size != sizeof(*in) ||
	    (in->group != 0 && in->group != 4 && in->group != 16 && in->group != 64))
		return -EINVAL;
	if (in->n == 0)
		return 0;
	if (!in->src || !in->src_off || !in->len || !out->dst || !out->pkt_len ||
	    in->src_len == UINT64_MAX || out->dst_len == UINT64_MAX || in->n > (1ull << 40) ||
	    (!out->dst_off && (out->dst_stride < 16 || (out->dst_stride & 15) || out->dst_stride > (1u << 20))))
		return -EINVAL;
	if (misaligned(in->src_off, 8) || misaligned(in->len, 2) || misaligned(in->hash, 4) ||
	    misaligned(out->dst_off, 8) || misaligned(out->pkt_len, 2) || misaligned(out->rss, 4) ||
	    misaligned(counts, 8))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	/* a registered host region is given by its host address, as
	 * gcl_classify_host takes it; device memory maps to itself */
	const void *src_d = mapped(in->src);

	CopyParams k;
	k.src = src_d ? (const uint8_t *)src_d : in->src;
	k.src_len = in->src_len;
	k.src_off = in->src_off;
	k.len = in->len;
	k.tx_olflags = in->tx_olflags;
	k.hash = in->hash;
	k.dst = out->dst;
	k.dst_len = out->dst_len;
	k.dst_off = out->dst_off;
	k.dst_stride = out->dst_stride;
	k.pkt_len = out->pkt_len;
	k.olflags = out->olflags;
	k.rss = out->rss;
	k.counts = (unsigned long long *)counts;
	k.n = in->n;
	k.dst_cap = in->dst_cap;

	/* lanes per packet: a 16-B chunk or two per lane for small frames, a few
	 * for MTU frames, a wave for jumbo frames; 16 when nothing is known */
	const uint32_t group = in->group ? in->group : in->len_hint == 0 ? 16 : in->len_hint <= 128 ? 4 :
	                       in->len_hint <= 2048 ? 16 : 64;
	const uint32_t per_cu = c->tune.blocks_per_cu != GCL_TUNE_AUTO ? (uint32_t)c->tune.blocks_per_cu :
	                                                                 kCopyBlocksPerCu;
	const uint32_t cap = (uint32_t)c->num_cus * per_cu;
	if (group == 4)
		copy_launch<4>(k, cap, s);
	else if (group == 16)
		copy_launch<16>(k, cap, s);
	else
		copy_launch<64>(k, cap, s);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
