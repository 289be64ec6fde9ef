/*
 * gcl_txhdr.hip - the transmit headers of a send batch (gcl_neigh_set,
 * gcl_tx_hdr, gclassify.h): for every segment of one runtime the UDP or TCP
 * header, the IPv4 header, the route and the ARP hit, the Ethernet header,
 * the loopback hint, the padding and the txpkt_xmit_cmd with its payload word
 * (runtime/net/udp.c:24-40, tcp_out.c:54-81, core.c:504-538, 581-626,
 * 686-737, arp.c:331-344).
 *
 * The neighbour table is built on the host (gcl_neigh.c) and copied to the
 * device when it has changed, on the stream of the next gcl_tx_hdr and before
 * its kernel.  In front of the table image the device copy carries the
 * 12 x 256-word Toeplitz LUT of cfg.rss_key, the one build_image makes for
 * GCL_HASH_TOEPLITZ contexts, so the hint of a local entry is toeplitz_lut of
 * gcl_kern.h on every context.  The rule for one entry is gcl_txh_rule of
 * gcl_txh.h, the same inline code the host twin runs.
 *
 * One launch, one lane per entry.  A lane loads its descriptor (two 16-B
 * loads) and its offset, probes the table (four 16-B slot loads, issued
 * together, for the entries that get that far) and holds the header as
 * fourteen dwords.  The stores: the frame starts at any byte, so the lane
 * rotates its dwords by the frame address's low two bits and stores every
 * 4-B-aligned dword that lies wholly inside a range it owns ([14, 42 or 54),
 * and [0, 14) for an OK entry) as one dword; the up to three bytes at each
 * end of a range go out one byte per store.  No store is wider than what it
 * writes and nothing is read back, so the option bytes, the payload and the
 * neighbouring frames, which other lanes are writing, are never touched.  The
 * padding of a short OK frame is stored bytewise.  Four-byte stores were
 * chosen over 16-B chunks shared by a lane group: a header is three or four
 * chunks at best and its ends are ragged in two places (byte 14 when the
 * Ethernet header is not written, byte 54 before TCP options).
 *
 * The counters: the four statuses and LOCAL are ballot popcounts kept per
 * wave, BYTES a per-lane sum reduced over the wave once; a wave adds them to
 * LDS and six lanes of the block add those to @counts, one add per counter
 * per block.  The grid is capped at kTxhBlocksPerCu blocks per CU
 * (gcl_tune.blocks_per_cu overrides it) and loops.  No inline assembly.
 *
 * Bounds: an entry index is used only below m; a frame is written only when
 * o <= frames_len and elen <= frames_len - o (no sum formed), and every store
 * is made at a frame byte below 54 <= len or below pkt_len = elen; every table
 * index is masked (gcl_neigh.h) and every LUT index is a byte.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/gcl_host.h"
#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_neigh.h"
#include "gcl_txh.h"

namespace gclk {

constexpr uint32_t kTxhThreads = 256;
/* grid cap: blocks per CU (4 waves each) */
constexpr uint32_t kTxhBlocksPerCu = 4;
constexpr uint32_t kTxhCounters = 6; /* GCL_TXHC_OK .. GCL_TXHC_BYTES */

struct TxhParams {
	const uint4 *desc;
	const uint64_t *frame_off;
	uint8_t *frames;
	uint64_t frames_len;
	uint64_t shm_base;
	uint64_t m;
	uint64_t *cmd, *payload;
	uint16_t *pkt_len;
	uint8_t *tx_olflags;
	uint32_t *hash;
	uint8_t *status;
	unsigned long long *counts;
	const uint32_t *toep;
	struct gcl_neigh_view view;
	struct gcl_txh_net net;
	uint32_t cap;
};

/* Frame bytes [r0, r1) of the header @w (dword k = frame bytes 4 k .. 4 k + 3,
 * r1 <= 56) to the frame at @f: aligned dwords inside the range whole, the
 * ragged ends bytewise. */
__device__ __forceinline__ void txh_store(uint8_t *f, const uint32_t (&w)[14], uint32_t r0, uint32_t r1)
{
	const uint32_t a = (uint32_t)(uintptr_t)f & 3; /* aligned dword q covers frame bytes 4 q - a .. */
#pragma unroll
	for (int q = 0; q < 15; q++) {
		const uint32_t prev = q > 0 ? w[q - 1] : 0, cur = q < 14 ? w[q] : 0, next = q < 13 ? w[q + 1] : 0;
		const uint32_t v = __builtin_amdgcn_alignbyte(a ? cur : next, a ? prev : cur, (4 - a) & 3);
		const int k = 4 * q - (int)a;
		if (k >= (int)r0 && k + 4 <= (int)r1) {
			*(uint32_t *)(f + k) = v;
		} else {
#pragma unroll
			for (int b = 0; b < 4; b++)
				if (k + b >= (int)r0 && k + b < (int)r1)
					f[k + b] = (uint8_t)(v >> (8 * b));
		}
	}
}

__global__ void __launch_bounds__(kTxhThreads) txh_kernel(TxhParams k)
{
	const uint32_t lane = threadIdx.x & 63;
	uint32_t cnt[5] = {0, 0, 0, 0, 0}; /* wave-uniform: the statuses, LOCAL */
	uint64_t bytes = 0;                /* this lane's OK entries */

	for (uint64_t p0 = (uint64_t)blockIdx.x * kTxhThreads; p0 < k.m; p0 += (uint64_t)gridDim.x * kTxhThreads) {
		const uint64_t p = p0 + threadIdx.x;
		uint32_t status = 4, local = 0;
		if (p < k.m) {
			const uint4 d0 = k.desc[2 * p], d1 = k.desc[2 * p + 1];
			const uint64_t o = k.frame_off[p];
			const uint32_t d[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
			const struct gcl_txh_res r = gcl_txh_rule(&k.view, &k.net, d, o, k.frames_len, k.cap);
			uint32_t hash = 0;

			if (r.status != GCL_TXH_REFUSED) {
				uint8_t *f = k.frames + o;
				txh_store(f, r.w, r.eth ? 0 : 14, r.l4end);
				for (uint32_t j = r.len; j < r.pkt_len; j++) /* OK only: pkt_len == len otherwise */
					f[j] = 0;
			}
			if (r.local)
				hash = toeplitz_lut(k.toep, k.net.addr, r.nh, r.lport, r.rport);
			k.cmd[p] = gcl_txh_cmd(&r);
			k.payload[p] = gcl_txh_payload(&r, k.shm_base, o, hash);
			k.pkt_len[p] = (uint16_t)r.pkt_len;
			k.tx_olflags[p] = (uint8_t)r.olflags;
			if (k.hash)
				k.hash[p] = hash;
			k.status[p] = (uint8_t)r.status;
			status = r.status;
			local = r.local;
			bytes += r.status == GCL_TXH_OK ? r.pkt_len : 0;
		}
#pragma unroll
		for (uint32_t j = 0; j < 4; j++)
			cnt[j] += (uint32_t)__popcll(__ballot(status == j));
		cnt[4] += (uint32_t)__popcll(__ballot(local != 0));
	}

	if (k.counts) { /* uniform */
		__shared__ unsigned long long blk[kTxhCounters];
		if (threadIdx.x < kTxhCounters)
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
#pragma unroll
			for (uint32_t j = 0; j < 5; j++)
				atomicAdd(&blk[j], (unsigned long long)cnt[j]);
			atomicAdd(&blk[GCL_TXHC_BYTES], (unsigned long long)bytes);
		}
		__syncthreads();
		if (threadIdx.x < kTxhCounters && blk[threadIdx.x])
			atomicAdd(k.counts + threadIdx.x, blk[threadIdx.x]);
	}
}

static int neigh_table(gcl_ctx *c)
{
	if (!c->neigh)
		c->neigh = gcl_neigh_tbl_new();
	return c->neigh ? 0 : -ENOMEM;
}

/* Bring the device copy up to date on @s and order this call after the copy,
 * as sock_upload does for the socket table: the one device image is
 * overwritten only after the calls that read it, those on @s by stream order,
 * those on other streams by waiting for them here (an upload may synchronise;
 * a call without one does not). */
static int neigh_upload(gcl_ctx *c, hipStream_t s)
{
	gcl_ctx::NeighDev &d = c->neighdev;
	struct gcl_neigh_tbl *t = c->neigh;
	HipErr he;

	if (!t->dirty && d.dimg) {
		if (s != d.up_stream)
			he(hipStreamWaitEvent(s, d.copied, 0));
	} else {
		const size_t bytes = kToepBytes + t->image_bytes;
		if (!d.copied)
			he(hipEventCreateWithFlags(&d.copied, hipEventDisableTiming));
		else
			he(hipEventSynchronize(d.copied)); /* the staging buffer is free */
		if (d.many) {
			he(hipDeviceSynchronize());
		} else {
			for (int i = 0; i < d.nusers; i++)
				if (d.users[i] != s)
					he(hipStreamSynchronize(d.users[i]));
		}
		if (he.bad())
			return -EIO;
		d.nusers = 0;
		d.many = false;
		if (bytes > d.cap) {
			if (d.dimg) {
				(void)hipStreamSynchronize(s);
				(void)hipFree(d.dimg);
				(void)hipHostFree(d.staging);
			}
			d.dimg = d.staging = nullptr;
			d.cap = 0;
			if (hipMalloc(&d.dimg, bytes) != hipSuccess ||
			    hipHostMalloc(&d.staging, bytes, hipHostMallocDefault) != hipSuccess) {
				(void)hipGetLastError();
				(void)hipFree(d.dimg);
				d.dimg = nullptr;
				return -ENOMEM;
			}
			d.cap = bytes;
			/* do_toeplitz's key, one word per tuple byte and value (as build_image) */
			uint32_t *lut = (uint32_t *)d.staging;
			for (int i = 0; i < 12; i++)
				for (int v = 0; v < 256; v++) {
					uint8_t in[12] = {0};
					in[i] = (uint8_t)v;
					lut[i * 256 + v] = gcl_toeplitz(c->cfg.rss_key, 40, in, 12);
				}
		}
		memcpy(d.staging + kToepBytes, t->image, t->image_bytes);
		he(hipMemcpyAsync(d.dimg, d.staging, bytes, hipMemcpyHostToDevice, s));
		he(hipEventRecord(d.copied, s));
		if (he.bad())
			return -EIO; /* dirty stays set: the next call uploads again */
		d.lg = t->log2_buckets;
		d.seed = t->seed;
		d.bits = t->img_bits;
		d.up_stream = s;
		t->dirty = 0;
	}
	if (he.bad())
		return -EIO;
	int i = 0;
	while (i < d.nusers && d.users[i] != s)
		i++;
	if (i == d.nusers) {
		if (d.nusers < kImgUsers)
			d.users[d.nusers++] = s;
		else
			d.many = true;
	}
	return 0;
}

void neigh_close(gcl_ctx *c)
{
	gcl_ctx::NeighDev &d = c->neighdev;
	(void)hipFree(d.dimg);
	(void)hipHostFree(d.staging);
	if (d.copied)
		(void)hipEventDestroy(d.copied);
	gcl_neigh_tbl_free(c->neigh);
	c->neigh = nullptr;
	memset(&d, 0, sizeof(d));
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_neigh_set(struct gcl_ctx *c, const struct gcl_neigh_entry *e, uint32_t n)
{
	if (!c || (n && !e))
		return -EINVAL;
	if (neigh_table(c))
		return -ENOMEM;
	return gcl_neigh_tbl_set(c->neigh, e, n);
}

extern "C" int gcl_tx_hdr(struct gcl_ctx *c, const struct gcl_txh_in *in, const struct gcl_txh_out *out,
                          uint64_t *counts, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	auto misaligned = [](const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; };

	if (!c || !in || !out || in->size != sizeof(*in) || in->m > (1ull << 31))
		return -EINVAL;
	if (in->m == 0)
		return 0;
	if (!in->desc || !in->frame_off || !in->frames || in->frames_len == UINT64_MAX || !out->cmd ||
	    !out->payload || !out->pkt_len || !out->tx_olflags || !out->status)
		return -EINVAL;
	if (misaligned(in->desc, 16) || misaligned(in->frame_off, 8) || misaligned(out->cmd, 8) ||
	    misaligned(out->payload, 8) || misaligned(out->pkt_len, 2) || misaligned(out->hash, 4) ||
	    misaligned(counts, 8))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	if (neigh_table(c))
		return -ENOMEM;
	const int ret = neigh_upload(c, s);
	if (ret)
		return ret;
	c->last_stream = s;

	TxhParams k;
	k.desc = (const uint4 *)in->desc;
	k.frame_off = in->frame_off;
	k.frames = in->frames;
	k.frames_len = in->frames_len;
	k.shm_base = in->shm_base;
	k.m = in->m;
	k.cmd = out->cmd;
	k.payload = out->payload;
	k.pkt_len = out->pkt_len;
	k.tx_olflags = out->tx_olflags;
	k.hash = out->hash;
	k.status = out->status;
	k.counts = (unsigned long long *)counts;
	k.toep = (const uint32_t *)c->neighdev.dimg;
	k.view = gcl_neigh_view_of(c->neighdev.lg, c->neighdev.seed, c->neighdev.bits,
	                           c->neighdev.dimg + kToepBytes);
	k.net = in->net;
	k.cap = in->cap;

	const uint64_t need = (in->m + kTxhThreads - 1) / kTxhThreads;
	const uint32_t per_cu = c->tune.blocks_per_cu != GCL_TUNE_AUTO ? (uint32_t)c->tune.blocks_per_cu :
	                                                                 kTxhBlocksPerCu;
	const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->num_cus * per_cu, need);
	hipLaunchKernelGGL(txh_kernel, dim3(grid), dim3(kTxhThreads), 0, s, k);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
