/*
 * gcl_plan.hip - delivery plan of a classified batch: a stable partition of
 * the packet indices by destination runtime (or flow-table queue), so that
 * the host post-pass (gcl_host_deliver_idx, gcl_host.h) can be run per
 * runtime, on any core, with every ring seeing today's message sequence.
 *
 * A one-pass stable counting sort over up to 16385 buckets, as five launches
 * on the caller's stream (kernel boundaries order the phases; nothing is
 * handed between workgroups inside a launch):
 *
 *   plan_count_kernel    the batch is cut into contiguous RANGES, one per
 *                        wave; each wave counts its range's keys into
 *                        counters of its own in LDS and writes them to
 *                        hist[bucket][range]
 *   plan_sum_kernel      \
 *   plan_top_kernel       > exclusive scan of hist in bucket-major,
 *   plan_scan_kernel     /  range-minor order; its values at range 0 are
 *                           bucket_off
 *   plan_scatter_kernel  each wave re-reads its range in order and stores
 *                        the packet indices from its scanned counters on
 *
 * Stability: a range belongs to one wave, which walks it in steps of
 * 64 x (16 / verdict bytes) packets.  A step is loaded 16 B per lane,
 * transposed through LDS so that slice p holds packets base + 64 p + lane,
 * and the slices are taken in order: a packet's rank among the equal keys of
 * its slice is the population count of the lower lanes in the ballot mask of
 * its key (plan_match), and the slice's leader lane moves the wave's counter
 * on.  No atomics hand out positions.  Skew costs nothing: a slice whose 64
 * packets share one key makes one counter update.
 *
 * Garbage in the verdicts cannot index outside the counters (every key is
 * clamped to the host bucket) nor outside order[0, n) (every position is
 * checked against n: the verdicts are read twice, and a caller who changes
 * them in between gets a wrong list, not a stray write).
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"

namespace gclk {

constexpr uint32_t kPlanStage = 64 * 16;        /* one step of a wave, bytes */
constexpr uint32_t kPlanChunk = 2048;           /* hist entries per scan block */
constexpr uint32_t kPlanTopThreads = 1024;
constexpr uint64_t kPlanMaxN = 1ull << 31;
constexpr uint64_t kPlanAutoEntries = 4u << 20; /* ranges x nbuckets, the library's choice */
constexpr uint64_t kPlanMaxEntries = 16u << 20; /* ... with gcl_plan_cfg.blocks */

struct PlanParams {
	const uint8_t *v;   /* verdicts, 16-B aligned */
	uint32_t *hist;     /* [nbuckets][ranges] */
	uint32_t *order;
	uint32_t n;         /* <= 2^31 */
	uint32_t range_len; /* packets per range: a multiple of the step */
	uint32_t ranges;
	uint32_t nbuckets;  /* the last one is the host bucket */
	uint32_t shift;     /* queue index -> key (1-/2-B verdicts) */
	uint32_t kbits;     /* bits of the largest key */
	uint32_t lds_wave;  /* LDS bytes per wave: counters, then the stage */
};

/* The bucket of one verdict: @w is the u8 / u16 verdict, or the
 * {uniqid, thread, action} word of gcl_verdict4 / gcl_verdict. */
template <int VB>
__device__ __forceinline__ uint32_t plan_key(uint32_t w, uint32_t shift, uint32_t host)
{
	uint32_t key;
	bool unicast;

	if (VB >= 4) {
		unicast = ((w >> 24) & GCL_ACT_MASK) <= GCL_ACT_WAKE;
		key = w & 0xFFFFu;
	} else if (VB == 2) {
		unicast = !(w & 0x8000u); /* GCL_V2_DELIVER or GCL_V2_WAKE */
		key = (w & GCL_V2_Q_MASK) >> shift;
	} else {
		unicast = !(w & GCL_V1_OTHER);
		key = (w & GCL_V1_Q_MASK) >> shift;
	}
	return unicast && key < host ? key : host;
}

/* verdict @p of the 16 B a lane loaded */
template <int VB>
__device__ __forceinline__ uint32_t plan_elem(const uint4 &q, int p)
{
	const uint32_t w[4] = {q.x, q.y, q.z, q.w};

	if (VB == 8)
		return w[2 * p + 1];
	if (VB == 4)
		return w[p];
	if (VB == 2)
		return (w[p >> 1] >> (16 * (p & 1))) & 0xFFFFu;
	return (w[p >> 2] >> (8 * (p & 3))) & 0xFFu;
}

/* the lanes of this wave that are @valid and hold this lane's @key */
__device__ __forceinline__ uint64_t plan_match(uint32_t key, bool valid, uint32_t kbits)
{
	uint64_t m = __ballot(valid);

	for (uint32_t b = 0; b < kbits; b++) {
		const bool bit = (key >> b) & 1u;
		const uint64_t bal = __ballot(bit);
		m &= bit ? bal : ~bal;
	}
	return m;
}

/* One step's 16 B of this lane: verdicts [i0, i0 + 16 / VB), zeros past n. */
template <int VB>
__device__ __forceinline__ uint4 plan_load(const uint8_t *v, uint64_t i0, uint32_t n)
{
	constexpr int P = 16 / VB;
	uint4 q = make_uint4(0, 0, 0, 0);

	if (i0 + P <= n) {
		q = *(const uint4 *)(v + i0 * VB);
	} else if (i0 < n) { /* the batch's ragged end */
		uint32_t w[4] = {0, 0, 0, 0};
		const uint64_t nb = (uint64_t)n * VB;
		for (int j = 0; j < 16; j++) {
			const uint64_t a = i0 * VB + j;
			if (a < nb)
				w[j >> 2] |= (uint32_t)v[a] << (8 * (j & 3));
		}
		q = make_uint4(w[0], w[1], w[2], w[3]);
	}
	return q;
}

template <int VB>
__global__ void __launch_bounds__(256) plan_count_kernel(PlanParams k)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t plan_lds[];
	constexpr int P = 16 / VB;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * (blockDim.x >> 6) + wave;
	const uint32_t host = k.nbuckets - 1;

	if (r >= k.ranges)
		return; /* waves share nothing: no barrier below */
	uint32_t *cnt = (uint32_t *)(plan_lds + (size_t)wave * k.lds_wave);
	for (uint32_t b = lane; b < k.nbuckets; b += 64)
		cnt[b] = 0;
	const uint64_t start = (uint64_t)r * k.range_len;
	const uint64_t end = start + k.range_len < k.n ? start + k.range_len : k.n;
	for (uint64_t base = start; base < end; base += 64 * P) {
		const uint64_t i0 = base + (uint64_t)lane * P;
		const uint4 q = plan_load<VB>(k.v, i0, k.n);
#pragma unroll
		for (int p = 0; p < P; p++) {
			const bool valid = i0 + p < k.n;
			const uint32_t key = plan_key<VB>(plan_elem<VB>(q, p), k.shift, host);
			const uint64_t m = plan_match(key, valid, k.kbits);
			/* one add per distinct key of the slice, by its lowest lane */
			if (valid && !(m & ((1ull << lane) - 1)))
				atomicAdd(&cnt[key], (uint32_t)__popcll(m));
		}
	}
	asm volatile("" ::: "memory");
	/* every entry of this range's column is written: the caller's
	 * workspace needs no zeroing */
	for (uint32_t b = lane; b < k.nbuckets; b += 64)
		k.hist[(size_t)b * k.ranges + r] = cnt[b];
}

template <int VB>
__global__ void __launch_bounds__(256) plan_scatter_kernel(PlanParams k)
{
	extern __shared__ __attribute__((aligned(16))) uint8_t plan_lds[];
	constexpr int P = 16 / VB;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t r = blockIdx.x * (blockDim.x >> 6) + wave;
	const uint32_t host = k.nbuckets - 1;

	if (r >= k.ranges)
		return;
	/* the wave's counters are read and moved on by different lanes from
	 * slice to slice: LDS serves one wave's accesses in issue order, and
	 * volatile keeps the compiler to that order */
	volatile uint32_t *cnt = (volatile uint32_t *)(plan_lds + (size_t)wave * k.lds_wave);
	uint8_t *stage = plan_lds + (size_t)wave * k.lds_wave + (k.lds_wave - kPlanStage);
	const uint64_t start = (uint64_t)r * k.range_len;
	const uint64_t end = start + k.range_len < k.n ? start + k.range_len : k.n;

	if (start >= end)
		return;
	for (uint32_t b = lane; b < k.nbuckets; b += 64)
		cnt[b] = k.hist[(size_t)b * k.ranges + r];
	for (uint64_t base = start; base < end; base += 64 * P) {
		/* 16 B per lane in, one verdict per lane per slice out */
		*(uint4 *)(stage + lane * 16) = plan_load<VB>(k.v, base + (uint64_t)lane * P, k.n);
		asm volatile("" ::: "memory");
#pragma unroll
		for (int p = 0; p < P; p++) {
			const uint32_t e = (uint32_t)p * 64 + lane;
			const uint64_t i = base + e;
			const bool valid = i < k.n;
			uint32_t w;
			if (VB == 8)
				w = *(const volatile uint32_t *)(stage + e * 8 + 4);
			else if (VB == 4)
				w = *(const volatile uint32_t *)(stage + e * 4);
			else if (VB == 2)
				w = *(const volatile uint16_t *)(stage + e * 2);
			else
				w = *(const volatile uint8_t *)(stage + e);
			const uint32_t key = plan_key<VB>(w, k.shift, host);
			const uint64_t m = plan_match(key, valid, k.kbits);
			const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1));
			const uint32_t at = cnt[key]; /* key <= host < nbuckets, whatever the bytes */
			if (valid) {
				const uint32_t pos = at + rank;
				if (pos < k.n)
					k.order[pos] = (uint32_t)i;
				if (rank == 0)
					cnt[key] = at + (uint32_t)__popcll(m);
			}
		}
		asm volatile("" ::: "memory");
	}
}

/* ---- the exclusive scan of hist[0, total), kPlanChunk entries per block ---- */

/* exclusive scan of one value per thread over the block (NT a power of two);
 * @total, when given, receives the block's sum */
template <int NT>
__device__ __forceinline__ uint32_t plan_block_scan(uint32_t x, uint32_t *sh, uint32_t *total)
{
	const uint32_t t = threadIdx.x;
	uint32_t acc = x;

	sh[t] = acc;
	__syncthreads();
	for (uint32_t d = 1; d < NT; d <<= 1) {
		const uint32_t y = t >= d ? sh[t - d] : 0;
		__syncthreads();
		acc += y;
		sh[t] = acc;
		__syncthreads();
	}
	if (total)
		*total = sh[NT - 1];
	return acc - x;
}

__global__ void __launch_bounds__(256) plan_sum_kernel(const uint32_t *hist, uint32_t total,
                                                       uint32_t *csum)
{
	__shared__ uint32_t sh[256];
	const uint32_t i0 = blockIdx.x * kPlanChunk + threadIdx.x * 8;
	uint32_t s = 0, tot;

	for (uint32_t j = 0; j < 8; j++)
		s += i0 + j < total ? hist[i0 + j] : 0;
	(void)plan_block_scan<256>(s, sh, &tot);
	if (threadIdx.x == 0)
		csum[blockIdx.x] = tot;
}

/* one block: csum[0, nchunks) -> its exclusive scan; bucket_off's last entry */
__global__ void __launch_bounds__(kPlanTopThreads) plan_top_kernel(uint32_t *csum, uint32_t nchunks,
                                                                   uint32_t *bucket_off,
                                                                   uint32_t nbuckets, uint32_t n)
{
	__shared__ uint32_t sh[kPlanTopThreads];
	const uint32_t per = (nchunks + kPlanTopThreads - 1) / kPlanTopThreads;
	const uint32_t i0 = threadIdx.x * per;
	uint32_t s = 0;

	for (uint32_t j = 0; j < per; j++)
		s += i0 + j < nchunks ? csum[i0 + j] : 0;
	uint32_t acc = plan_block_scan<kPlanTopThreads>(s, sh, nullptr);
	for (uint32_t j = 0; j < per; j++) {
		if (i0 + j < nchunks) {
			const uint32_t x = csum[i0 + j];
			csum[i0 + j] = acc;
			acc += x;
		}
	}
	if (threadIdx.x == 0)
		bucket_off[nbuckets] = n;
}

__global__ void __launch_bounds__(256) plan_scan_kernel(uint32_t *hist, uint32_t total,
                                                        const uint32_t *csum, uint32_t ranges,
                                                        uint32_t *bucket_off)
{
	__shared__ uint32_t sh[256];
	const uint32_t i0 = blockIdx.x * kPlanChunk + threadIdx.x * 8;
	uint32_t x[8], s = 0;

	for (uint32_t j = 0; j < 8; j++) {
		x[j] = i0 + j < total ? hist[i0 + j] : 0;
		s += x[j];
	}
	uint32_t acc = csum[blockIdx.x] + plan_block_scan<256>(s, sh, nullptr);
	for (uint32_t j = 0; j < 8; j++) {
		const uint32_t i = i0 + j;
		if (i < total) {
			hist[i] = acc;
			if (i % ranges == 0) /* the first range's start is the bucket's */
				bucket_off[i / ranges] = acc;
			acc += x[j];
		}
	}
}

/* What a plan of @n verdicts of context @c takes. */
struct PlanGeom {
	uint32_t vb, nbuckets, shift, kbits;
	uint32_t ranges, range_len, wpb, lds_wave;
	uint32_t total, nchunks; /* hist entries, scan blocks */
	size_t hist_bytes, bytes;
};

static int plan_buckets(const gcl_ctx *c, uint32_t key, uint32_t *nbuckets)
{
	if (!c || key > GCL_PLAN_BY_QUEUE)
		return -EINVAL;
	if (key == GCL_PLAN_BY_QUEUE) {
		if (verdict_bytes(c) > 2)
			return -EINVAL;
		*nbuckets = (c->cfg.max_runtimes << c->cfg.thread_bits) + 1;
	} else {
		*nbuckets = c->cfg.max_runtimes + 1;
	}
	return 0;
}

static int plan_geometry(const gcl_ctx *c, const struct gcl_plan_cfg *cfg, uint64_t n, PlanGeom *g)
{
	if (!c || !cfg || cfg->size != sizeof(*cfg) || n > kPlanMaxN)
		return -EINVAL;
	if (plan_buckets(c, cfg->key, &g->nbuckets) != 0)
		return -EINVAL;
	g->vb = verdict_bytes(c);
	g->shift = cfg->key == GCL_PLAN_BY_RUNTIME && g->vb <= 2 ? c->cfg.thread_bits : 0;
	g->kbits = 32 - (uint32_t)__builtin_clz(g->nbuckets - 1 ? g->nbuckets - 1 : 1);
	g->lds_wave = align16(g->nbuckets * 4) + kPlanStage;
	g->wpb = 4 * g->lds_wave <= 80 * 1024 ? 4 : 1;

	const uint32_t step = 64 * (16 / g->vb);
	if (cfg->blocks) {
		if ((uint64_t)cfg->blocks * g->nbuckets > kPlanMaxEntries)
			return -EINVAL;
		g->ranges = cfg->blocks;
	} else {
		/* a wave per range, as many waves as the chip holds, ranges of at
		 * least four steps, and ranges x nbuckets bounded */
		uint32_t bpc = (160 * 1024) / (g->wpb * g->lds_wave);
		if (bpc > 8)
			bpc = 8;
		uint64_t cap = (uint64_t)(c->num_cus > 0 ? c->num_cus : 1) * bpc * g->wpb;
		const uint64_t fit = kPlanAutoEntries / g->nbuckets;
		if (cap > fit)
			cap = fit;
		uint64_t want = (n + 4 * step - 1) / (4 * step);
		if (want > cap)
			want = cap;
		g->ranges = want ? (uint32_t)want : 1;
	}
	uint64_t len = (n + g->ranges - 1) / g->ranges;
	len = (len + step - 1) / step * step;
	g->range_len = (uint32_t)(len ? len : step); /* <= 2^31 */
	g->total = g->ranges * g->nbuckets;
	g->nchunks = (g->total + kPlanChunk - 1) / kPlanChunk;
	g->hist_bytes = align16(g->total * 4);
	g->bytes = g->hist_bytes + align16(g->nchunks * 4);
	return 0;
}

template <int VB>
static hipError_t plan_launch(const PlanGeom &g, const PlanParams &k, uint32_t *csum,
                              uint32_t *bucket_off, hipStream_t s)
{
	const uint32_t lds = g.wpb * g.lds_wave;
	const dim3 grid((g.ranges + g.wpb - 1) / g.wpb), block(g.wpb * 64);

	if (lds > 64 * 1024) {
		static std::mutex mu;
		static bool raised;
		std::lock_guard<std::mutex> lk(mu);
		if (!raised) {
			hipError_t e = hipFuncSetAttribute((const void *)plan_count_kernel<VB>,
			                                   hipFuncAttributeMaxDynamicSharedMemorySize,
			                                   160 * 1024);
			if (e == hipSuccess)
				e = hipFuncSetAttribute((const void *)plan_scatter_kernel<VB>,
				                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
			if (e != hipSuccess)
				return e;
			raised = true;
		}
	}
	hipLaunchKernelGGL(plan_count_kernel<VB>, grid, block, lds, s, k);
	hipLaunchKernelGGL(plan_sum_kernel, dim3(g.nchunks), dim3(256), 0, s, k.hist, g.total, csum);
	hipLaunchKernelGGL(plan_top_kernel, dim3(1), dim3(kPlanTopThreads), 0, s, csum, g.nchunks,
	                   bucket_off, g.nbuckets, k.n);
	hipLaunchKernelGGL(plan_scan_kernel, dim3(g.nchunks), dim3(256), 0, s, k.hist, g.total, csum,
	                   g.ranges, bucket_off);
	hipLaunchKernelGGL(plan_scatter_kernel<VB>, grid, block, lds, s, k);
	return hipGetLastError();
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_plan_buckets(const struct gcl_ctx *c, uint32_t key, uint32_t *nbuckets)
{
	if (!nbuckets)
		return -EINVAL;
	return plan_buckets(c, key, nbuckets);
}

extern "C" int gcl_plan_workspace(const struct gcl_ctx *c, const struct gcl_plan_cfg *cfg, uint64_t n,
                                  size_t *bytes)
{
	PlanGeom g;

	if (!bytes)
		return -EINVAL;
	const int r = plan_geometry(c, cfg, n, &g);
	if (r == 0)
		*bytes = g.bytes;
	return r;
}

extern "C" int gcl_plan(struct gcl_ctx *c, const struct gcl_plan_cfg *cfg, const void *verdicts,
                        uint64_t n, const struct gcl_plan_out *out, void *workspace,
                        size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;
	PlanGeom g;
	hipError_t e;

	const int r = plan_geometry(c, cfg, n, &g);
	if (r != 0)
		return r;
	if (!out || !out->order || !out->bucket_off || ((uintptr_t)out->order & 3) ||
	    ((uintptr_t)out->bucket_off & 3))
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;
	if (n == 0)
		return hipMemsetAsync(out->bucket_off, 0, ((size_t)g.nbuckets + 1) * 4, s) == hipSuccess
		               ? 0 : -EIO;
	if (!verdicts || ((uintptr_t)verdicts & 15) || !workspace || ((uintptr_t)workspace & 15) ||
	    workspace_bytes < g.bytes)
		return -EINVAL;

	PlanParams k;
	k.v = (const uint8_t *)verdicts;
	k.hist = (uint32_t *)workspace;
	k.order = out->order;
	k.n = (uint32_t)n;
	k.range_len = g.range_len;
	k.ranges = g.ranges;
	k.nbuckets = g.nbuckets;
	k.shift = g.shift;
	k.kbits = g.kbits;
	k.lds_wave = g.lds_wave;
	uint32_t *csum = (uint32_t *)((uint8_t *)workspace + g.hist_bytes);
	switch (g.vb) {
	case 1: e = plan_launch<1>(g, k, csum, out->bucket_off, s); break;
	case 2: e = plan_launch<2>(g, k, csum, out->bucket_off, s); break;
	case 4: e = plan_launch<4>(g, k, csum, out->bucket_off, s); break;
	default: e = plan_launch<8>(g, k, csum, out->bucket_off, s); break;
	}
	return e == hipSuccess ? 0 : -EIO;
}
