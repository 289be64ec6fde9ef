/*
 * gcl_sock.hip - the socket demux of a classified batch (gcl_sock_set,
 * gcl_sock_lookup, gclassify.h): trans_lookup (runtime/net/transport.c:
 * 341-397) for every packet the runtime would hand to net_rx_trans, against
 * the receiving runtime's entries in the context's socket table.
 *
 * The table is built on the host (gcl_sock.c) and copied to the device when
 * it has changed, on the stream of the next lookup and before its kernel.
 * The rule for one packet -- the verdict's runtime, the frame predicate, the
 * three keys, their probes and the choice among them -- is gcl_sock_rule of
 * gcl_sock.h, the same inline code the host lookup runs.
 *
 * One launch, one lane per packet.  A lane loads its verdict and its frame's
 * header: for a 4-B-aligned frame whose 16-B-aligned 64-B window (starting up
 * to 12 B before the frame, as gcl_csum.hip's) lies inside
 * frames[0, frames_len), the two or three 16-B chunks of the window that hold
 * frame bytes [12, 38); any other frame byte by byte, every byte at or past
 * frames_len as 0.  The three keys of a packet are known before any probe, so
 * the twelve 16-B key loads of its three probes are issued together and the
 * winner is chosen afterwards; its cookie is the one dependent load.  The
 * table lives in HBM; a small one stays in L2.
 *
 * The counters are kept per wave in scalar registers (ballot popcounts),
 * summed per block in LDS and added with one vector atomic per block.  The
 * grid is capped at kSockBlocksPerCu blocks per CU and loops: block b takes
 * packets 256 (b + pass * grid) + lane.  No inline assembly.
 *
 * Bounds: a packet index is used only below n; an aligned window is loaded
 * only when [w, w + 64) lies inside [0, frames_len); the bytewise form tests
 * every byte's index against frames_len - off; every table index is masked
 * (gcl_sock.h).  Whatever frames, offs, verdicts and the entries hold,
 * nothing is read outside frames[0, frames_len), offs[0, n), verdicts[0, n)
 * and the image, and nothing written outside sock[0, n).
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/gcl_host.h"
#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_sock.h"

namespace gclk {

constexpr uint32_t kSockThreads = 256;
/* grid cap: blocks per CU (4 waves each) */
constexpr uint32_t kSockBlocksPerCu = 4;
constexpr uint32_t kSockClasses = 6; /* GCL_SOCK_HIT5 .. GCL_SOCK_N_NA */

struct SockParams {
	const uint8_t *frames;
	uint64_t frames_len;
	uint64_t stride;
	const uint64_t *offs;
	const void *verdicts;
	uint32_t *sock;
	unsigned long long *counts;
	uint64_t n;
	struct gcl_sock_view view;
	uint32_t vbytes, thread_bits, max_rt;
};

/* frame dwords 3..9 out of the window's sixteen, the frame starting 4 L bytes in */
template <int L>
__device__ __forceinline__ void sock_pick(const uint4 (&w)[4], uint32_t d[7])
{
	const uint32_t W[16] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w,
	                        w[2].x, w[2].y, w[2].z, w[2].w, w[3].x, w[3].y, w[3].z, w[3].w};
#pragma unroll
	for (int i = 0; i < 7; i++)
		d[i] = W[3 + i + L];
}

__global__ void __launch_bounds__(kSockThreads) sock_kernel(SockParams k)
{
	const uint32_t fbase = (uint32_t)(uintptr_t)k.frames;
	uint32_t cnt[kSockClasses] = {0, 0, 0, 0, 0, 0}; /* wave-uniform */

	for (uint64_t p0 = (uint64_t)blockIdx.x * kSockThreads; p0 < k.n;
	     p0 += (uint64_t)gridDim.x * kSockThreads) {
		const uint64_t p = p0 + threadIdx.x;
		const bool valid = p < k.n;
		uint32_t klass = kSockClasses;
		if (valid) {
			uint64_t raw;
			if (k.vbytes == 8)
				raw = ((const uint64_t *)k.verdicts)[p];
			else if (k.vbytes == 4)
				raw = ((const uint32_t *)k.verdicts)[p];
			else if (k.vbytes == 2)
				raw = ((const uint16_t *)k.verdicts)[p];
			else
				raw = ((const uint8_t *)k.verdicts)[p];
			const uint64_t off = k.offs ? k.offs[p] : p * k.stride;
			const uint64_t o = off < k.frames_len ? off : k.frames_len;
			const uint32_t lead = (fbase + (uint32_t)o) & 15;
			const bool al = (lead & 3) == 0 && o >= lead && k.frames_len >= 64 &&
			                o - lead <= k.frames_len - 64;
			uint32_t d[7];
			if (al) {
				/* window dword j is frame dword j - lead / 4; wanted are 3..9 */
				const uint4 *w = (const uint4 *)(k.frames + (o - lead));
				uint4 c[4];
				c[0] = c[3] = make_uint4(0, 0, 0, 0);
				if (lead == 0)
					c[0] = w[0];
				c[1] = w[1];
				c[2] = w[2];
				if (lead == 12)
					c[3] = w[3];
				if (lead == 0)
					sock_pick<0>(c, d);
				else if (lead == 4)
					sock_pick<1>(c, d);
				else if (lead == 8)
					sock_pick<2>(c, d);
				else
					sock_pick<3>(c, d);
			} else {
				const uint64_t avail = k.frames_len - o;
				const uint8_t *f = k.frames + o;
				for (uint32_t j = 0; j < 7; j++) {
					uint32_t x = 0;
					for (uint32_t i = 0; i < 4; i++) {
						const uint32_t at = 12 + 4 * j + i;
						x |= (at < avail ? (uint32_t)f[at] : 0u) << (8 * i);
					}
					d[j] = x;
				}
			}
			const uint32_t u = gcl_sock_verdict_rt(raw, k.vbytes, k.thread_bits, k.max_rt);
			k.sock[p] = gcl_sock_rule(&k.view, u, d, &klass);
		}
#pragma unroll
		for (uint32_t j = 0; j < kSockClasses; j++)
			cnt[j] += (uint32_t)__popcll(__ballot(klass == j));
	}

	if (k.counts) { /* uniform */
		__shared__ uint32_t blk[kSockClasses];
		if (threadIdx.x < kSockClasses)
			blk[threadIdx.x] = 0;
		__syncthreads();
		if ((threadIdx.x & 63) == 0) {
#pragma unroll
			for (uint32_t j = 0; j < kSockClasses; j++)
				atomicAdd(&blk[j], cnt[j]);
		}
		__syncthreads();
		if (threadIdx.x < kSockClasses && blk[threadIdx.x])
			atomicAdd(k.counts + threadIdx.x, (unsigned long long)blk[threadIdx.x]);
	}
}

static int sock_table(gcl_ctx *c)
{
	if (!c->sock)
		c->sock = gcl_sock_tbl_new();
	return c->sock ? 0 : -ENOMEM;
}

/* Bring the device copy up to date on @s and order this lookup after the
 * copy.  The one device image is overwritten only after the lookups that
 * read it: those on @s by stream order, those on other streams by waiting
 * for them here (an upload may synchronise; a lookup without one does not). */
static int sock_upload(gcl_ctx *c, hipStream_t s)
{
	gcl_ctx::SockDev &d = c->sockdev;
	struct gcl_sock_tbl *t = c->sock;
	HipErr he;

	if (!t->dirty && d.dimg) {
		if (s != d.up_stream)
			he(hipStreamWaitEvent(s, d.copied, 0));
	} else {
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
		if (t->image_bytes > d.cap) {
			if (d.dimg) {
				(void)hipStreamSynchronize(s);
				(void)hipFree(d.dimg);
				(void)hipHostFree(d.staging);
			}
			d.dimg = d.staging = nullptr;
			d.cap = 0;
			if (hipMalloc(&d.dimg, t->image_bytes) != hipSuccess ||
			    hipHostMalloc(&d.staging, t->image_bytes, hipHostMallocDefault) != hipSuccess) {
				(void)hipGetLastError();
				(void)hipFree(d.dimg);
				d.dimg = nullptr;
				return -ENOMEM;
			}
			d.cap = t->image_bytes;
		}
		memcpy(d.staging, t->image, t->image_bytes);
		memcpy(d.hdr, t->image, sizeof(d.hdr));
		he(hipMemcpyAsync(d.dimg, d.staging, t->image_bytes, hipMemcpyHostToDevice, s));
		he(hipEventRecord(d.copied, s));
		if (he.bad())
			return -EIO; /* dirty stays set: the next call uploads again */
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

void sock_runtime_del(gcl_ctx *c, uint16_t uniqid)
{
	if (c->sock)
		(void)gcl_sock_tbl_del(c->sock, uniqid);
}

void sock_close(gcl_ctx *c)
{
	gcl_ctx::SockDev &d = c->sockdev;
	(void)hipFree(d.dimg);
	(void)hipHostFree(d.staging);
	if (d.copied)
		(void)hipEventDestroy(d.copied);
	gcl_sock_tbl_free(c->sock);
	c->sock = nullptr;
	memset(&d, 0, sizeof(d));
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_sock_set(struct gcl_ctx *c, uint16_t uniqid, const struct gcl_sock_entry *e, uint32_t n)
{
	if (!c || (n && !e))
		return -EINVAL;
	if (uniqid >= c->cfg.max_runtimes || !c->rt[uniqid].present)
		return -ENOENT;
	if (sock_table(c))
		return -ENOMEM;
	return gcl_sock_tbl_set(c->sock, uniqid, e, n);
}

extern "C" int gcl_sock_lookup(struct gcl_ctx *c, const struct gcl_batch *b, const void *verdicts,
                               uint32_t *sock, uint64_t *counts, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || !b || !verdicts || !sock)
		return -EINVAL;
	const uint32_t vb = verdict_bytes(c);
	if (((uintptr_t)verdicts & (vb - 1)) || ((uintptr_t)sock & 3))
		return -EINVAL;
	if (b->n == 0)
		return 0;
	if (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	    (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	if (sock_table(c))
		return -ENOMEM;
	const int ret = sock_upload(c, s);
	if (ret)
		return ret;
	c->last_stream = s;

	SockParams k;
	struct gcl_sock_img_hdr h;
	memcpy(&h, c->sockdev.hdr, sizeof(h));
	k.frames = b->frames;
	k.frames_len = b->frames_len;
	k.stride = b->stride;
	k.offs = b->offs;
	k.verdicts = verdicts;
	k.sock = sock;
	k.counts = (unsigned long long *)counts;
	k.n = b->n;
	k.view = gcl_sock_view_of(&h, c->sockdev.dimg);
	k.vbytes = vb;
	k.thread_bits = c->cfg.thread_bits;
	k.max_rt = c->cfg.max_runtimes;

	const uint64_t need = (b->n + kSockThreads - 1) / kSockThreads;
	const unsigned grid = (unsigned)std::min<uint64_t>((uint64_t)c->num_cus * kSockBlocksPerCu, need);
	hipLaunchKernelGGL(sock_kernel, dim3(grid), dim3(kSockThreads), 0, s, k);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
