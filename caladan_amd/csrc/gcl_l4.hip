/*
 * gcl_l4.hip - the TCP/UDP checksum offload of a batch (gcl_l4_csum,
 * gclassify.h): ipv4_udptcp_cksum and ipv4_cksum (inc/net/chksum.h) over n
 * frames of any length at any byte alignment, checked (GCL_L4_VERIFY) or
 * written into the frames (GCL_L4_FILL).  Every L4 byte is read once.
 *
 * One launch.  A group of G neighbouring lanes (4, 16 or 64, a template
 * parameter; the host picks it from len_hint, any G is correct for any
 * length) owns one packet, so a wave holds 64 / G packets and a block 256 / G.
 * Every lane of the group reads the packet's pkt_len, offset and tx_olflags
 * and the eight header bytes that decide eligibility (one address per group:
 * the loads coalesce) and judges the packet for itself.
 *
 * The summed range is frame bytes [14, 14 + tot) of an L4-eligible packet and
 * [14, 34) of one that is only IP-eligible.  It is cut at the 16-B boundaries
 * of the frame's address into aligned chunks; chunk c belongs to lane c % G
 * and arrives as one aligned 16-B load, and a lane issues the loads of
 * kL4Unroll chunks, G chunks apart, before it sums the first of them.  A
 * chunk that lies wholly in the L4 bytes is added dword by dword into a
 * 64-bit accumulator (65 501 bytes of 0xFF are 16 376 dwords of 0xFFFFFFFF: 46
 * bits at most, no carry is lost; it is brought down to its four 16-bit
 * quarters' sum once per packet).  The first chunks and the last are masked by
 * byte first: the bytes of [14, 34) go to the IP header's sum (16-bit halves
 * into 32 bits: a few words), the bytes of [26, 14 + tot) to the L4 sum.  The
 * addresses [26, 34) are thereby the pseudo-header's first four words, read
 * where they lie; {0, proto} and hton16(l4len) are added by the group's first
 * lane.  Words are the aligned 16-bit words of memory: at an odd frame address
 * every byte sits in the other half of its word, which multiplies the
 * one's-complement sum by 256, and the folded sum is byte-swapped once to
 * undo it.
 *
 * The two partial sums are added over the group in registers (quad_perm and
 * row_ror DPP inside a 16-lane row, lane permutes across rows; the loop is
 * wave-uniform, so every lane is active there).  The group's first lane folds
 * them, takes the checksum field out again where FILL says it counts as 0
 * (one's-complement subtraction of the two bytes it reads itself: the rest of
 * either sum is never all zero, byte 14 is 0x45 and proto is not 0, so the
 * folded value is the one a sum without the field gives), and writes the
 * status byte and, in FILL, the fields, a byte per store.  Both sums of a
 * packet are complete before either field is written, and neither feeds the
 * other: the IP field [24, 26) is outside the L4 sum's bytes, the L4 field
 * outside the header.
 *
 * Bounds.  A packet index is used only below n.  With o the offset clamped to
 * frames_len and L = min(pkt_len, frames_len - o), a header byte is read only
 * when L >= 34, the range is summed only when its end 14 + tot <= L, and a
 * byte is written only inside it.  An aligned chunk is loaded only when its 16
 * bytes lie inside frames[0, frames_len); bytes of it outside the range (a
 * neighbour's, which another group may be writing) are masked away.  A chunk
 * that does not lie inside (the region's first and last bytes) is read byte
 * by byte, only the bytes of the range.  Nothing is read outside frames[0,
 * frames_len) and the n-element arrays, no byte at or past o + L enters a
 * result, and nothing but status[0, n), counts and the checksum bytes of a
 * filled packet is written; no wider word is read-modify-written.
 *
 * The counters: the status and fill counts are ballot popcounts kept per wave,
 * BYTES a per-lane sum reduced over the wave once; a wave adds them to 56
 * bytes of LDS (the only LDS) and seven lanes of the block add those to
 * @counts, one add per counter per block.  The grid is capped at
 * kL4BlocksPerCu blocks per CU (gcl_tune.blocks_per_cu overrides it for A/Bs)
 * and loops.  No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_device.h"

namespace gclk {

constexpr uint32_t kL4Threads = 256;
/* grid cap: blocks per CU.  The kernels take 67-69 VGPRs, 7 waves per SIMD, so
 * 7 blocks of 4 waves are resident on a CU; an eighth would wait for a slot
 * (tools/l4_bench.py times 4, 6 and 8 beside it: 7 is the fastest at every
 * frame length) */
constexpr uint32_t kL4BlocksPerCu = 7;
/* chunks a lane has in flight: loads of all of them, then their sums */
constexpr uint32_t kL4Unroll = 4;

struct L4Params {
	uint8_t *frames;
	uint64_t frames_len;
	uint64_t stride;
	const uint64_t *offs;
	const uint16_t *pkt_len;
	const uint8_t *tx_olflags;
	uint8_t *status;
	unsigned long long *counts;
	uint64_t n;
	uint32_t mode;
};

/* DPP move with no "old" operand (every lane has a source: quad_perm, row_ror) */
template <int CTRL>
__device__ __forceinline__ uint32_t l4_dpp(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}

/* @v summed over the group of G lanes, in every lane of it; all lanes active */
template <uint32_t G>
__device__ __forceinline__ uint32_t l4_group_sum(uint32_t v)
{
	if (G == 64) {
		v += (uint32_t)__shfl_xor((int)v, 32);
		v += (uint32_t)__shfl_xor((int)v, 16);
	}
	if (G >= 16) {
		v += l4_dpp<0x128>(v); /* row_ror:8 */
		v += l4_dpp<0x124>(v); /* row_ror:4 */
	}
	v += l4_dpp<0x4E>(v); /* quad_perm [2, 3, 0, 1] */
	v += l4_dpp<0xB1>(v); /* quad_perm [1, 0, 3, 2] */
	return v;
}

/* the bytes of the dword at frame byte @r (may be negative) that lie in [lo, hi) */
__device__ __forceinline__ uint32_t l4_mask(int r, int lo, int hi)
{
	const int s = lo - r > 0 ? lo - r : 0, e = hi - r < 4 ? hi - r : 4;
	if (s >= e)
		return 0;
	return (e == 4 ? 0xFFFFFFFFu : (1u << (8 * e)) - 1) & ~((1u << (8 * s)) - 1);
}

__device__ __forceinline__ uint32_t l4_fold16(uint32_t s)
{
	s = (s & 0xFFFFu) + (s >> 16);
	s = (s & 0xFFFFu) + (s >> 16);
	return s;
}

__device__ __forceinline__ uint32_t l4_swap16(uint32_t s)
{
	return (s >> 8 | s << 8) & 0xFFFFu;
}

/* Lane @sub of G's share of one packet's range [14, hi) at @f = frames + o:
 * the bytes of [14, 34) into @ip (16-bit halves), those of [26, hi_l4) into
 * @l4 (dwords).  hi <= L, so every byte of the range is the packet's own. */
template <uint32_t G>
__device__ __forceinline__ void l4_sum_range(const L4Params &k, uint64_t o, int hi, int hi_l4, uint32_t sub,
                                             uint32_t &ip, uint64_t &l4)
{
	const uint8_t *f = k.frames + o;
	/* chunk c is frame bytes [14 - lead + 16 c, + 16), 16-B aligned in memory */
	const uint32_t lead = ((uint32_t)(uintptr_t)f + 14) & 15;
	const uint32_t nc = ((uint32_t)hi - 14 + lead + 15) >> 4;

	for (uint32_t c0 = sub; c0 < nc; c0 += kL4Unroll * G) {
		uint4 v[kL4Unroll];
		bool inb[kL4Unroll];
#pragma unroll
		for (uint32_t u = 0; u < kL4Unroll; u++) {
			const uint32_t c = c0 + u * G;
			const int r0 = 14 - (int)lead + 16 * (int)c;
			/* [o + r0, o + r0 + 16) inside [0, frames_len); frames_len >= 34 here */
			const uint64_t x = o + (uint64_t)(int64_t)r0;
			inb[u] = c < nc && (r0 >= 0 || o >= (uint64_t)-r0) && x <= k.frames_len - 16;
			v[u] = make_uint4(0, 0, 0, 0);
			if (inb[u])
				v[u] = *(const uint4 *)(f + r0);
		}
#pragma unroll
		for (uint32_t u = 0; u < kL4Unroll; u++) {
			const uint32_t c = c0 + u * G;
			const int r0 = 14 - (int)lead + 16 * (int)c;
			if (c >= nc)
				break;
			uint32_t d[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
			if (!inb[u]) { /* rare: the region's ends */
				for (int i = 0; i < 4; i++) {
					d[i] = 0;
					for (int b = 0; b < 4; b++) {
						const int r = r0 + 4 * i + b;
						if (r >= 14 && r < hi)
							d[i] |= (uint32_t)f[r] << (8 * b);
					}
				}
			}
			if (r0 >= 34 && r0 + 16 <= hi_l4) {
				l4 += (uint64_t)d[0] + d[1] + d[2] + d[3];
			} else {
#pragma unroll
				for (int i = 0; i < 4; i++) {
					const uint32_t a = d[i] & l4_mask(r0 + 4 * i, 14, 34);
					ip += (a & 0xFFFFu) + (a >> 16);
					l4 += d[i] & l4_mask(r0 + 4 * i, 26, hi_l4);
				}
			}
		}
	}
}

template <uint32_t G>
__global__ void __launch_bounds__(kL4Threads) l4_kernel(L4Params k)
{
	constexpr uint32_t kPerBlock = kL4Threads / G, kPerWave = 64 / G;
	const uint32_t lane = threadIdx.x & 63, sub = lane % G;
	const uint64_t step = (uint64_t)gridDim.x * kPerBlock;
	const bool fill = k.mode == GCL_L4_FILL;
	uint32_t n_st[4] = {0, 0, 0, 0}, n_fip = 0, n_fl4 = 0; /* wave-uniform */
	uint64_t bytes = 0;                                    /* this lane's packets */

	/* the wave's first packet decides: every lane of a wave makes the same passes */
	for (uint64_t pw = (uint64_t)blockIdx.x * kPerBlock + (threadIdx.x >> 6) * kPerWave; pw < k.n;
	     pw += step) {
		const uint64_t p = pw + lane / G;
		const bool valid = p < k.n;
		uint64_t o = 0;
		uint32_t fl = 0, proto = 0, tot = 0;
		bool ip_ok = false, l4_ok = false, none = false;
		if (valid) {
			const uint64_t raw = k.offs ? k.offs[p] : p * k.stride;
			o = raw < k.frames_len ? raw : k.frames_len;
			const uint64_t avail = k.frames_len - o;
			const uint64_t L = k.pkt_len[p] < avail ? k.pkt_len[p] : avail;
			const uint8_t *f = k.frames + o;
			fl = !fill ? 0 : k.tx_olflags ? k.tx_olflags[p] : 3;
			if (L >= 34) {
				ip_ok = f[12] == (GCL_ETHTYPE_IP >> 8) && f[13] == (GCL_ETHTYPE_IP & 0xFF) &&
				        f[14] == 0x45;
				const uint32_t frag = (uint32_t)f[20] << 8 | f[21];
				proto = f[23];
				tot = (uint32_t)f[16] << 8 | f[17];
				l4_ok = ip_ok && !(frag & 0x3FFF) && (proto == 6 || proto == 17) &&
				        tot >= 20u + (proto == 6 ? 20u : 8u) && 14ull + tot <= L;
				/* VERIFY: a UDP datagram sent without a checksum is not summed */
				none = !fill && l4_ok && proto == 17 && !f[40] && !f[41];
			}
		}
		const bool do_ip = ip_ok && (fl & 1);
		const bool do_l4 = l4_ok && (fill ? (fl & 2) != 0 : !none);

		uint32_t ip = 0;
		uint64_t acc = 0;
		if (do_ip || do_l4) {
			const int hi_l4 = do_l4 ? 14 + (int)tot : 26;
			l4_sum_range<G>(k, o, do_l4 ? hi_l4 : 34, hi_l4, sub, ip, acc);
		}
		uint32_t l4 = (uint32_t)(acc & 0xFFFF) + (uint32_t)(acc >> 16 & 0xFFFF) +
		              (uint32_t)(acc >> 32 & 0xFFFF) + (uint32_t)(acc >> 48);
		ip = l4_group_sum<G>(ip);
		l4 = l4_group_sum<G>(l4);

		/* the group's first lane: the verdict, the fields, the status byte */
		const bool head = valid && sub == 0;
		uint32_t st = GCL_L4_NA;
		if (head) {
			uint8_t *f = k.frames + o;
			const bool odd = (uintptr_t)f & 1;
			const uint32_t l4len = tot - 20;
			if (do_ip) {
				uint32_t s = l4_fold16(ip);
				s = odd ? l4_swap16(s) : s;
				s = l4_fold16(s + (~(f[24] | (uint32_t)f[25] << 8) & 0xFFFFu));
				const uint32_t v = ~s & 0xFFFFu;
				f[24] = (uint8_t)v;
				f[25] = (uint8_t)(v >> 8);
				st |= GCL_L4_FILLED_IP;
			}
			if (do_l4) {
				uint8_t *fld = f + (proto == 6 ? 50 : 40);
				uint32_t s = l4_fold16(l4);
				s = odd ? l4_swap16(s) : s;
				s += (proto << 8) + l4_swap16(l4len);
				if (fill)
					s += ~(fld[0] | (uint32_t)fld[1] << 8) & 0xFFFFu;
				s = l4_fold16(s);
				if (fill) {
					uint32_t v = ~s & 0xFFFFu;
					v = v ? v : 0xFFFFu;
					fld[0] = (uint8_t)v;
					fld[1] = (uint8_t)(v >> 8);
					st |= GCL_L4_FILLED_L4;
				} else {
					st = s == 0xFFFFu ? GCL_L4_GOOD : GCL_L4_BAD;
				}
				bytes += l4len;
			} else if (none) {
				st = GCL_L4_NONE;
			}
			k.status[p] = (uint8_t)st;
		}
		n_st[GCL_L4C_GOOD] += (uint32_t)__popcll(__ballot(head && (st & 0xF) == GCL_L4_GOOD));
		n_st[GCL_L4C_BAD] += (uint32_t)__popcll(__ballot(head && (st & 0xF) == GCL_L4_BAD));
		n_st[GCL_L4C_NONE] += (uint32_t)__popcll(__ballot(head && (st & 0xF) == GCL_L4_NONE));
		n_st[GCL_L4C_NA] += (uint32_t)__popcll(__ballot(head && (st & 0xF) == GCL_L4_NA));
		n_fip += (uint32_t)__popcll(__ballot(head && (st & GCL_L4_FILLED_IP)));
		n_fl4 += (uint32_t)__popcll(__ballot(head && (st & GCL_L4_FILLED_L4)));
	}

	if (k.counts) { /* uniform */
		__shared__ unsigned long long blk[GCL_L4C_BYTES + 1];
		if (threadIdx.x <= GCL_L4C_BYTES)
			blk[threadIdx.x] = 0;
		__syncthreads();
		uint32_t blo = (uint32_t)bytes, bhi = (uint32_t)(bytes >> 32);
		for (int x = 32; x; x >>= 1) {
			const uint64_t other = (uint64_t)(uint32_t)__shfl_xor((int)bhi, x) << 32 |
			                       (uint32_t)__shfl_xor((int)blo, x);
			bytes += other;
			blo = (uint32_t)bytes;
			bhi = (uint32_t)(bytes >> 32);
		}
		if (lane == 0) {
			atomicAdd(&blk[GCL_L4C_GOOD], (unsigned long long)n_st[GCL_L4C_GOOD]);
			atomicAdd(&blk[GCL_L4C_BAD], (unsigned long long)n_st[GCL_L4C_BAD]);
			atomicAdd(&blk[GCL_L4C_NONE], (unsigned long long)n_st[GCL_L4C_NONE]);
			atomicAdd(&blk[GCL_L4C_NA], (unsigned long long)n_st[GCL_L4C_NA]);
			atomicAdd(&blk[GCL_L4C_FILLED_IP], (unsigned long long)n_fip);
			atomicAdd(&blk[GCL_L4C_FILLED_L4], (unsigned long long)n_fl4);
			atomicAdd(&blk[GCL_L4C_BYTES], (unsigned long long)bytes);
		}
		__syncthreads();
		if (threadIdx.x <= GCL_L4C_BYTES && blk[threadIdx.x])
			atomicAdd(k.counts + threadIdx.x, blk[threadIdx.x]);
	}
}

template <uint32_t G>
static void l4_launch(const L4Params &k, uint32_t blocks_cap, hipStream_t s)
{
	constexpr uint32_t per_block = kL4Threads / G;
	const uint64_t need = (k.n + per_block - 1) / per_block;
	const unsigned grid = (unsigned)std::min<uint64_t>(blocks_cap, need);
	hipLaunchKernelGGL(l4_kernel<G>, dim3(grid), dim3(kL4Threads), 0, s, k);
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_l4_csum(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_l4_in *in,
                           uint8_t *status, uint64_t *counts, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !b || !in || !status || in->size != sizeof(*in) || in->mode > GCL_L4_FILL ||
	    (in->group != 0 && in->group != 4 && in->group != 16 && in->group != 64))
		return -EINVAL;
	if (b->n == 0)
		return 0;
	if (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	    (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	    !b->pkt_len || ((uintptr_t)b->pkt_len & 1))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	L4Params k;
	k.frames = (uint8_t *)b->frames; /* FILL writes: the caller owns the memory */
	k.frames_len = b->frames_len;
	k.stride = b->stride;
	k.offs = b->offs;
	k.pkt_len = b->pkt_len;
	k.tx_olflags = in->mode == GCL_L4_FILL ? in->tx_olflags : nullptr;
	k.status = status;
	k.counts = (unsigned long long *)counts;
	k.n = b->n;
	k.mode = in->mode;

	/* lanes per packet: a 16-B chunk or two per lane for small frames, a few
	 * for MTU frames, a wave for jumbo frames; 16 when nothing is known */
	const uint32_t group = in->group ? in->group : in->len_hint == 0 ? 16 : in->len_hint <= 128 ? 4 :
	                       in->len_hint <= 2048 ? 16 : 64;
	const uint32_t per_cu = c->tune.blocks_per_cu != GCL_TUNE_AUTO ? (uint32_t)c->tune.blocks_per_cu :
	                                                                 kL4BlocksPerCu;
	const uint32_t cap = (uint32_t)c->num_cus * per_cu;
	if (group == 4)
		l4_launch<4>(k, cap, s);
	else if (group == 16)
		l4_launch<16>(k, cap, s);
	else
		l4_launch<64>(k, cap, s);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
