/*
 * gcl_pack.hip - packed delivery records of an index list (gcl_plan_pack,
 * gclassify.h): for every entry i = order[j] of a plan's order, or of one
 * bucket's slice of it, the lrpc message of packet i ({cmd, payload}) and its
 * verdict widened to gcl_verdict4, written at position j.  The host post-pass
 * (gcl_host_deliver_packed, gcl_host.h) then reads three dense arrays in list
 * order instead of gathering from four per-packet arrays through the list.
 *
 * One launch, a gather: a lane owns the two consecutive positions 2t and
 * 2t + 1, so that its cmd and payload go out as one 16-B store each and its
 * two verdicts as one 8-B store.  It reads its two entries of order (8 B per
 * lane, coalesced), gathers verdict, pkt_len, olflags and offs of both
 * packets, and stores.  Inside one bucket the indices ascend, so neighbouring
 * lanes' gathers fall on the same or on adjacent lines; the outputs are
 * written fully coalesced.  An odd m leaves the last lane one position, which
 * it stores element by element.
 *
 * The gathers of a lane are independent and must all be in flight together:
 * the kernel is templated on which optional arrays are given (OPT), and an
 * entry that names no packet reads packet 0 and discards it, so that no
 * branch stands between two loads (a branch per optional array made the
 * compiler wait for each load before it issued the next).
 *
 * Bounds: an entry is used as an index only when i < n (else index 0, and a
 * batch of no packets reads nothing); positions are derived from the thread
 * index and checked against m.  Whatever order and verdicts hold, nothing is
 * read outside [0, n) of a per-packet array and nothing written outside
 * [0, m) of an output.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"

namespace gclk {

constexpr uint32_t kPackThreads = 256;
constexpr uint64_t kPackMaxM = 1ull << 31;
/* the record of an entry that names no packet of the batch */
constexpr uint32_t kPackNoVerdict =
	GCL_NO_RUNTIME | (uint32_t)GCL_NO_THREAD << 16 | (uint32_t)GCL_ACT_MASK << 24;
/* OPT: the optional per-packet arrays the caller gave */
constexpr int kPackLen = 1, kPackOlf = 2, kPackOffs = 4;

struct PackParams {
	const uint8_t *v;
	const uint32_t *order; /* 4-B aligned only */
	const uint16_t *pkt_len;
	const uint8_t *olflags;
	const uint64_t *offs;
	uint64_t *cmd, *payload;
	uint32_t *v4;
	uint64_t n, m, stride, shm_base;
	uint32_t thread_bits;
	uint32_t csum_def; /* csum_type of cfg.default_olflags */
};

struct PackRec {
	uint64_t cmd, payload;
	uint32_t v4; /* struct gcl_verdict4: uniqid | thread << 16 | action << 24 */
};

/* Verdict @i of @v in the context's width VB as the gcl_verdict4 word, from
 * the definitions of the four forms in gclassify.h. */
template <int VB>
__device__ __forceinline__ uint32_t pack_widen(const uint8_t *v, uint64_t i, uint32_t thread_bits)
{
	if (VB == 8) /* struct gcl_verdict: {hash, uniqid, thread, action} */
		return ((const uint32_t *)v)[2 * i + 1];
	if (VB == 4)
		return ((const uint32_t *)v)[i];

	const uint32_t tmask = (1u << thread_bits) - 1;
	uint32_t q, action;
	bool unicast;

	if (VB == 2) {
		const uint32_t x = ((const uint16_t *)v)[i];
		const uint32_t kind = x & GCL_V2_KIND;
		unicast = kind == GCL_V2_DELIVER || kind == GCL_V2_WAKE;
		q = x & GCL_V2_Q_MASK;
		action = unicast ? (kind == GCL_V2_WAKE ? GCL_ACT_WAKE : GCL_ACT_DELIVER)
		                 : (x & GCL_ACT_MASK);
	} else {
		const uint32_t x = v[i];
		unicast = !(x & GCL_V1_OTHER);
		q = x & GCL_V1_Q_MASK;
		action = unicast ? GCL_ACT_DELIVER : (x & GCL_ACT_MASK);
	}
	/* q = uniqid << thread_bits | slot; the fields are u16 and u8 */
	const uint32_t dest = unicast ? ((q >> thread_bits) & 0xFFFFu) | ((q & tmask) & 0xFFu) << 16
	                              : GCL_NO_RUNTIME | (uint32_t)GCL_NO_THREAD << 16;
	return dest | action << 24;
}

/* The record of entry @e; the batch has at least one packet. */
template <int VB, int OPT>
__device__ __forceinline__ PackRec pack_one(const PackParams &k, uint32_t e)
{
	const bool in = e < k.n;
	const uint32_t i = in ? e : 0;
	const uint64_t len = (OPT & kPackLen) ? k.pkt_len[i] : 0;
	const uint64_t csum = (OPT & kPackOlf) ?
		(k.olflags[i] & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD : k.csum_def;
	const uint64_t off = (OPT & kPackOffs) ? k.offs[i] : (uint64_t)i * k.stride;
	const uint32_t w = pack_widen<VB>(k.v, i, k.thread_bits);
	PackRec r;

	r.cmd = in ? len << 16 | csum << 48 : 0; /* RX_NET_RECV = 0 */
	r.payload = in ? k.shm_base + off : 0;
	r.v4 = in ? w : kPackNoVerdict;
	return r;
}

template <int VB, int OPT>
__global__ void __launch_bounds__(kPackThreads) pack_kernel(PackParams k)
{
	const uint64_t j = ((uint64_t)blockIdx.x * kPackThreads + threadIdx.x) * 2;

	if (j >= k.m)
		return;
	if (j + 1 < k.m) {
		uint32_t ea, eb;
		if (((uintptr_t)k.order & 7) == 0) { /* j is even */
			const uint2 o = *(const uint2 *)(k.order + j);
			ea = o.x;
			eb = o.y;
		} else { /* a slice of a plan's order starts at any entry */
			ea = k.order[j];
			eb = k.order[j + 1];
		}
		PackRec a, b;
		if (k.n) {
			a = pack_one<VB, OPT>(k, ea);
			b = pack_one<VB, OPT>(k, eb);
		} else {
			a.cmd = a.payload = 0;
			a.v4 = kPackNoVerdict;
			b = a;
		}
		/* the outputs are 16-B aligned */
		*(ulonglong2 *)(k.cmd + j) = make_ulonglong2(a.cmd, b.cmd);
		*(ulonglong2 *)(k.payload + j) = make_ulonglong2(a.payload, b.payload);
		*(uint2 *)(k.v4 + j) = make_uint2(a.v4, b.v4);
	} else { /* the last position of an odd m */
		PackRec a;
		if (k.n) {
			a = pack_one<VB, OPT>(k, k.order[j]);
		} else {
			a.cmd = a.payload = 0;
			a.v4 = kPackNoVerdict;
		}
		k.cmd[j] = a.cmd;
		k.payload[j] = a.payload;
		k.v4[j] = a.v4;
	}
}

template <int VB, int OPT>
static hipError_t pack_launch_opt(const PackParams &k, hipStream_t s)
{
	const uint64_t lanes = (k.m + 1) / 2; /* <= 2^30 */
	const dim3 grid((uint32_t)((lanes + kPackThreads - 1) / kPackThreads)), block(kPackThreads);

	hipLaunchKernelGGL((pack_kernel<VB, OPT>), grid, block, 0, s, k);
	return hipGetLastError();
}

template <int VB>
static hipError_t pack_launch(const PackParams &k, hipStream_t s)
{
	switch ((k.pkt_len ? kPackLen : 0) | (k.olflags ? kPackOlf : 0) | (k.offs ? kPackOffs : 0)) {
	case 0: return pack_launch_opt<VB, 0>(k, s);
	case 1: return pack_launch_opt<VB, 1>(k, s);
	case 2: return pack_launch_opt<VB, 2>(k, s);
	case 3: return pack_launch_opt<VB, 3>(k, s);
	case 4: return pack_launch_opt<VB, 4>(k, s);
	case 5: return pack_launch_opt<VB, 5>(k, s);
	case 6: return pack_launch_opt<VB, 6>(k, s);
	default: return pack_launch_opt<VB, 7>(k, s);
	}
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_plan_pack(struct gcl_ctx *c, const struct gcl_pack_in *in,
                             const struct gcl_pack_out *out, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	hipError_t e;

	if (!c || !in || in->size != sizeof(*in) || in->m > kPackMaxM)
		return -EINVAL;
	if (in->m == 0)
		return 0;
	const uint32_t vb = verdict_bytes(c);
	if (!in->verdicts || ((uintptr_t)in->verdicts & (vb - 1)) || !in->order ||
	    ((uintptr_t)in->order & 3) || ((uintptr_t)in->pkt_len & 1) || ((uintptr_t)in->offs & 7))
		return -EINVAL;
	if (!out || !out->cmd || !out->payload || !out->v4 || ((uintptr_t)out->cmd & 15) ||
	    ((uintptr_t)out->payload & 15) || ((uintptr_t)out->v4 & 15))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;

	PackParams k;
	k.v = (const uint8_t *)in->verdicts;
	k.order = in->order;
	k.pkt_len = in->pkt_len;
	k.olflags = in->olflags;
	k.offs = in->offs;
	k.cmd = out->cmd;
	k.payload = out->payload;
	k.v4 = (uint32_t *)out->v4;
	k.n = in->n;
	k.m = in->m;
	k.stride = in->stride;
	k.shm_base = in->shm_base;
	k.thread_bits = c->cfg.thread_bits;
	k.csum_def = (c->cfg.default_olflags & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD;
	switch (vb) {
	case 1: e = pack_launch<1>(k, s); break;
	case 2: e = pack_launch<2>(k, s); break;
	case 4: e = pack_launch<4>(k, s); break;
	default: e = pack_launch<8>(k, s); break;
	}
	return e == hipSuccess ? 0 : -EIO;
}
