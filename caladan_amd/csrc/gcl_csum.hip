/*
 * gcl_csum.hip - the IPv4 header checksum offload of a batch (gcl_rx_csum,
 * gclassify.h): for every packet whose ol_flags do not already say
 * IP_CKSUM_GOOD, the 20-byte check net_rx_one makes (chksum_internet over
 * frame bytes [14, 34), runtime/net/core.c:275-279), with the verdict written
 * into the checksum bits of a new ol_flags array.
 *
 * One launch.  A wave owns a tile of 64 consecutive packets and a quad of
 * four neighbouring lanes reads one packet: lane q of the quad loads the q-th
 * 16-B chunk of the 16-B-aligned window that starts up to 12 B before the
 * frame.  Frame bytes [12, 34) always lie in the window's first 48 bytes, so a
 * chunk is loaded only when it holds some of them -- except in dense 64-B
 * slots, where all four lanes load and a wave instruction reads 16 whole
 * slots, 1 KiB of consecutive lines.  In load u (of four, all issued before
 * any is used) quad g reads packet 16 u + g of the tile, so that the loads of
 * a fixed stride are coalesced; lane q of quad g is the OWNER of packet
 * 16 q + g: it loads that packet's offset and ol_flags (one coalesced load
 * each per tile), hands the quad the packet's source by quad broadcast, and
 * finishes its verdict.
 *
 * A lane adds the 16-bit halves of its masked dwords into a 32-bit partial:
 * ten words of at most 0xFFFF cannot carry out of it, so the end-around
 * carries are all still there when the owner folds the quad's total (two
 * quad_perm adds) to 16 bits.  Bit 24 of the partial carries "bytes 12-13 are
 * 0x0800" from the one lane that holds them.
 *
 * A frame that is not 4-B aligned, or whose window does not lie inside
 * frames[0, frames_len) (the region's first and last 64 B, a cut frame, an
 * offset at or past frames_len), is read byte by byte with every byte at or
 * past frames_len as 0, the quad's lanes taking the words in turn.  Bytes are
 * addressed from the frame's own start there, so the sum needs no byte swap
 * at an odd address.
 *
 * The tile's 64 flag bytes leave as 16 dwords from lanes 0-15 (four lane
 * permutes gather a lane's four consecutive packets from their owners) when
 * the tile is whole and its first output byte 4-B aligned; a ragged last tile
 * or an unaligned array is stored a byte per owner.  In place is safe: a
 * wave reads its tile's flags before it writes them and no other wave
 * touches them.  The counters are kept per wave in scalar registers (ballot
 * popcounts), summed per block in 12 bytes of LDS (the only LDS; the per-wave
 * adds measured 8-35 % of a launch) and added once per block, by one 4-lane
 * vector atomic.
 *
 * The grid is capped at kCsumBlocksPerCu blocks per CU and loops: block b
 * takes tiles 4 (b + pass * grid) + wave.  No inline assembly.
 *
 * Bounds: a packet index is used only below n; an aligned window is loaded
 * only when [w, w + 64) lies inside [0, frames_len); the bytewise form tests
 * every byte's index against frames_len - off.  Whatever frames, offs and
 * olflags hold, nothing is read outside frames[0, frames_len), offs[0, n) and
 * olflags[0, n) and nothing written outside olflags_out[0, n).
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_device.h"

namespace gclk {

constexpr uint32_t kCsumThreads = 256;
constexpr uint32_t kCsumTile = 64;       /* packets per wave per pass */
/* grid cap: blocks per CU.  The kernel takes 70 VGPRs, 7 waves per SIMD, so 7
 * blocks of 4 waves are resident on a CU; an eighth would wait for a slot and
 * run its passes after the others had finished */
constexpr uint32_t kCsumBlocksPerCu = 7;
/* how a packet is read */
constexpr uint32_t kCsumNone = 0, kCsumAligned = 1, kCsumBytewise = 2;
constexpr uint32_t kCsumIsIp = 1u << 24; /* partial: frame bytes 12-13 are 0x0800 */

struct CsumParams {
	const uint8_t *frames;
	uint64_t frames_len;
	uint64_t stride;
	const uint64_t *offs;
	const uint8_t *olflags;
	uint8_t *out;
	unsigned long long *counts;
	uint64_t n;
	uint32_t default_flags;
	uint32_t dense; /* 64-B slots back to back: every lane of a quad loads */
};

/* DPP move with no "old" operand (a quad_perm leaves no lane without a source) */
template <int CTRL>
__device__ __forceinline__ uint32_t csum_dpp(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}

/* lane U of the quad's value in every lane of the quad */
template <int U>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v)
{
	return csum_dpp<U * 0x55>(v); /* quad_perm [U, U, U, U] */
}

/* The partial of lane @q for an aligned packet: @v is chunk @q of the window
 * that starts @lead (0, 4, 8 or 12) bytes before the frame.  Window dword
 * 4 q + j is frame dword i = 4 q + j - lead / 4, frame bytes [4 i, 4 i + 4):
 * the header's words are the high halves of i = 3..7 and the low halves of
 * i = 4..8, and the low half of i = 3 is bytes 12-13. */
__device__ __forceinline__ uint32_t csum_partial(const uint4 &v, uint32_t q, uint32_t lead)
{
	const uint32_t d[4] = {v.x, v.y, v.z, v.w};
	const int i0 = (int)(4 * q) - (int)(lead >> 2);
	uint32_t s = 0;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int i = i0 + j;
		s += (i >= 4 && i <= 8 ? d[j] & 0xFFFFu : 0u) + (i >= 3 && i <= 7 ? d[j] >> 16 : 0u);
		s |= i == 3 && (d[j] & 0xFFFFu) == 0x0008u ? kCsumIsIp : 0u;
	}
	return s;
}

/* The partial of lane @q for a packet read byte by byte from offset @o
 * (<= frames_len): header words q, q + 4 and q + 8 of the ten, and bytes
 * 12-13 on lane 3, which has only two words. */
__device__ __forceinline__ uint32_t csum_partial_bytes(const CsumParams &k, uint64_t o, uint32_t q)
{
	const uint64_t avail = k.frames_len - o;
	const uint8_t *f = k.frames + o;
	auto byte = [&](uint32_t i) -> uint32_t { return i < avail ? f[i] : 0u; };
	uint32_t s = 0;
	for (uint32_t w = q; w < 10; w += 4)
		s += byte(14 + 2 * w) | byte(15 + 2 * w) << 8;
	if (q == 3 && (byte(12) | byte(13) << 8) == 0x0008u)
		s |= kCsumIsIp;
	return s;
}

__global__ void __launch_bounds__(kCsumThreads) csum_kernel(CsumParams k)
{
	const uint32_t lane = threadIdx.x & 63, q = lane & 3, g = lane >> 2;
	const uint64_t ntiles = (k.n + kCsumTile - 1) / kCsumTile;
	const uint64_t tstep = (uint64_t)gridDim.x * (kCsumThreads / 64);
	const uint32_t fbase = (uint32_t)(uintptr_t)k.frames;
	uint32_t n_good = 0, n_bad = 0, n_skip = 0; /* wave-uniform */

	for (uint64_t t = (uint64_t)blockIdx.x * (kCsumThreads / 64) + (threadIdx.x >> 6); t < ntiles;
	     t += tstep) {
		const uint64_t p0 = t * kCsumTile;
		/* the packet this lane owns: its source and its flags */
		const uint64_t p = p0 + 16 * q + g;
		const bool valid = p < k.n;
		uint64_t x = 0;
		uint32_t info = kCsumNone; /* how | lead << 8 */
		uint32_t fl = k.default_flags;
		if (valid) {
			const uint64_t raw = k.offs ? k.offs[p] : p * k.stride;
			const uint64_t o = raw < k.frames_len ? raw : k.frames_len;
			const uint32_t lead = (fbase + (uint32_t)o) & 15;
			const bool al = (lead & 3) == 0 && o >= lead && k.frames_len >= 64 &&
			                o - lead <= k.frames_len - 64;
			x = al ? o - lead : o;
			info = al ? kCsumAligned | lead << 8 : kCsumBytewise;
			if (k.olflags)
				fl = k.olflags[p];
		}
		const uint32_t xlo = (uint32_t)x, xhi = (uint32_t)(x >> 32);

		/* the four packets of this quad: sources, then every load, then the sums */
		uint64_t src[4];
		uint32_t inf[4];
		src[0] = (uint64_t)quad_bcast<0>(xhi) << 32 | quad_bcast<0>(xlo);
		src[1] = (uint64_t)quad_bcast<1>(xhi) << 32 | quad_bcast<1>(xlo);
		src[2] = (uint64_t)quad_bcast<2>(xhi) << 32 | quad_bcast<2>(xlo);
		src[3] = (uint64_t)quad_bcast<3>(xhi) << 32 | quad_bcast<3>(xlo);
		inf[0] = quad_bcast<0>(info);
		inf[1] = quad_bcast<1>(info);
		inf[2] = quad_bcast<2>(info);
		inf[3] = quad_bcast<3>(info);

		uint4 v[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			/* chunk q holds frame dwords 4 q - lead / 4 .. + 3: wanted are 3..8 */
			const int i0 = (int)(4 * q) - (int)(inf[u] >> 10);
			const bool want = k.dense || (i0 + 3 >= 3 && i0 <= 8);
			v[u] = make_uint4(0, 0, 0, 0);
			if ((inf[u] & 0xFF) == kCsumAligned && want)
				v[u] = gcl::load16_nt(k.frames + src[u] + 16 * q);
		}
		uint32_t part[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			part[u] = csum_partial(v[u], q, inf[u] >> 8);
			if ((inf[u] & 0xFF) == kCsumBytewise) /* rare */
				part[u] = csum_partial_bytes(k, src[u], q);
			part[u] += csum_dpp<0xB1>(part[u]); /* quad_perm [1, 0, 3, 2] */
			part[u] += csum_dpp<0x4E>(part[u]); /* quad_perm [2, 3, 0, 1] */
		}

		/* the owner's verdict */
		const uint32_t mine = q == 0 ? part[0] : q == 1 ? part[1] : q == 2 ? part[2] : part[3];
		uint32_t sum = mine & (kCsumIsIp - 1);
		sum = (sum & 0xFFFFu) + (sum >> 16);
		sum = (sum & 0xFFFFu) + (sum >> 16);
		const bool good = sum == 0xFFFFu;
		const bool skip = !(mine & kCsumIsIp) || (fl & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD;
		const uint32_t res = skip ? fl : (fl & ~(uint32_t)GCL_F_IP_CKSUM_MASK) |
		                                         (good ? GCL_F_IP_CKSUM_GOOD : GCL_F_IP_CKSUM_BAD);

		n_skip += (uint32_t)__popcll(__ballot(valid && skip));
		n_good += (uint32_t)__popcll(__ballot(valid && !skip && good));
		n_bad += (uint32_t)__popcll(__ballot(valid && !skip && !good));

		uint8_t *o = k.out + p0;
		if (p0 + kCsumTile <= k.n && ((uintptr_t)o & 3) == 0) {
			/* lane d < 16 stores packets 4 d .. 4 d + 3: packet 4 d + j is
			 * owned by lane q = d >> 2 of quad g = 4 (d & 3) + j */
			const uint32_t d = lane & 15, s0 = 16 * (d & 3) + (d >> 2);
			const uint32_t b0 = (uint32_t)__shfl((int)res, (int)s0);
			const uint32_t b1 = (uint32_t)__shfl((int)res, (int)s0 + 4);
			const uint32_t b2 = (uint32_t)__shfl((int)res, (int)s0 + 8);
			const uint32_t b3 = (uint32_t)__shfl((int)res, (int)s0 + 12);
			if (lane < 16)
				((uint32_t *)o)[lane] = (b0 & 0xFF) | (b1 & 0xFF) << 8 | (b2 & 0xFF) << 16 | b3 << 24;
		} else if (valid) {
			k.out[p] = (uint8_t)res;
		}
	}

	/* one add per block: a wave-level add of four u64 from each of the
	 * launch's 8 192 waves took 32-48 us of a 32 Mi-packet launch */
	if (k.counts) { /* uniform */
		__shared__ uint32_t blk[3];
		if (threadIdx.x < 3)
			blk[threadIdx.x] = 0;
		__syncthreads();
		if (lane == 0) {
			atomicAdd(&blk[0], n_good);
			atomicAdd(&blk[1], n_bad);
			atomicAdd(&blk[2], n_skip);
		}
		__syncthreads();
		if (threadIdx.x < GCL_CSUM_NR) {
			const uint32_t t = threadIdx.x;
			const uint32_t c = t == GCL_CSUM_CHECKED ? blk[0] + blk[1] : t == GCL_CSUM_GOOD ? blk[0] :
			                   t == GCL_CSUM_BAD ? blk[1] : blk[2];
			if (c)
				atomicAdd(k.counts + t, (unsigned long long)c);
		}
	}
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_rx_csum(struct gcl_ctx *c, const struct gcl_batch *b, uint8_t *olflags_out,
                           uint64_t *counts, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !b || !olflags_out)
		return -EINVAL;
	if (b->n == 0)
		return 0;
	if (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	    (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	CsumParams k;
	k.frames = b->frames;
	k.frames_len = b->frames_len;
	k.stride = b->stride;
	k.offs = b->offs;
	k.olflags = b->olflags;
	k.out = olflags_out;
	k.counts = (unsigned long long *)counts;
	k.n = b->n;
	k.default_flags = c->cfg.default_olflags;
	k.dense = !b->offs && b->stride == GCL_HDR_GRANULE;

	const uint64_t per_block = (uint64_t)kCsumTile * (kCsumThreads / 64);
	const uint64_t need = (b->n + per_block - 1) / per_block;
	const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->num_cus * kCsumBlocksPerCu, need);
	hipLaunchKernelGGL(csum_kernel, dim3(grid), dim3(kCsumThreads), 0, s, k);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
