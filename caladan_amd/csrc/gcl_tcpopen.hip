/*
 * gcl_tcpopen.hip - the passive open of a list of packets (gcl_tcp_rx_open,
 * gclassify.h): tcp_queue_recv -> tcp_rx_listener for a listener's packets
 * (runtime/net/tcp.c:488-522, runtime/net/tcp_in.c:614-694) and tcp_rx_closed
 * for those of no socket (tcp_in.c:696-723), with tcp_parse_options and the
 * option bytes of tcp_put_options.  The rule for one entry is that of
 * gcl_tcpopen.h, the same inline code the host twin runs.
 *
 * What packet j does depends on the packets before it in two ways: the running
 * backlog of its listener, and whether an earlier SYN of its tuple was
 * accepted.  Both are restated without any block waiting for another.  A
 * CANDIDATE is an entry that reaches line 5e with the backlog ignored; the
 * LEADER of a tuple is its first candidate.  Only a leader can be an ACCEPT:
 * the running backlog never grows, so a later candidate of the tuple is LATER
 * when the leader was accepted and FULL when it was not.  The leaders of a
 * listener are accepted in list order until the backlog runs out, so with
 * before(j) = the leaders of j's listener before j,
 *     leader j is accepted    <=>  not SHUTDOWN and before(j) < backlog
 *     running backlog at j is 0  <=>  before(j) >= backlog
 * and every listener-route entry needs before(j) and, for line 5a, its
 * leader's.
 *
 * The list is cut into `blocks` contiguous ranges of whole 256-entry tiles.
 * Launches on the stream (two memsets first: the tuple table to empty, the
 * count matrix to 0), ordered by the stream alone:
 *
 *   decide   one lane per entry: the frame's bytes [12, 56) as aligned dwords
 *            shifted into place (a dword that crosses frames_len byte by
 *            byte), gcl_open_head; a candidate fetches its 40 option bytes
 *            once and runs gcl_open_walk, fully unrolled.  Writes the 16-B
 *            tuple and a 16-B record (class, options, rst_seq / irs) to the
 *            workspace.
 *   insert   a launch of its own, so that every tuple is visible to every
 *            lane: a candidate probes the table of list indices from its
 *            tuple's hash; atomicCAS on an empty slot, and on a slot held by k
 *            (the value the CAS returns) the tuples are compared: equal,
 *            atomicMin(slot, j); not, the next slot.  A slot only ever holds
 *            indices of one tuple, so it ends as that tuple's leader whatever
 *            the order of arrival.
 *   count    a listener-route entry looks its tuple up and stores its leader;
 *            a leader adds 1 to matrix[range][listener] (a sum: no order).
 *   scan     one lane per listener turns its column into exclusive prefix
 *            sums over the ranges and writes backlog_out.
 *   rank     block r loads row r into per-listener LDS counters and walks its
 *            range tile by tile, the four waves of a tile in turn.  A wave
 *            takes its distinct listeners one at a time: a ballot of the lanes
 *            with that listener, a ballot of the leaders among them,
 *            before(j) = counter + the leaders in the lanes below.
 *   final    the verdict of every entry from its class, before(j) and its
 *            leader's; verdict, later_of, rst_seq; per range the segments and
 *            the records wanted, as ballot popcounts; the verdict counters.
 *   top      one block: the exclusive prefix sums of both, the totals.
 *   emit     positions as in gcl_tcp_rx_ctl's emit (range base + tiles before
 *            + waves before + lanes below); records as four 16-B stores,
 *            descriptors as two, the option bytes as byte stores.
 *
 * Bounds.  A list index is used only below m, a packet index only below n, a
 * listener only below nlisten (gcl_open_head admits no other), a table slot
 * only masked, a table value only when it is not the empty mark (it is then a
 * list index that was inserted), a record only below open_cap, a segment only
 * below min(seg_cap, the slots inside tx_frames_len), an option byte only
 * inside its segment's slot.  A frame dword is loaded whole only when all
 * four bytes lie below frames_len.  No inline assembly.
 */
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/gclassify.h"
#include "gcl_ctx.h"
#include "gcl_tcpopen.h"

namespace gclk {

constexpr uint32_t kOpenThreads = 256;
constexpr uint32_t kOpenWaves = kOpenThreads / 64;
constexpr uint32_t kOpenBlocksPerCu = 4;
constexpr uint32_t kOpenTopPer = GCL_OPEN_MAX_BLOCKS / kOpenThreads;
static_assert(kOpenTopPer * kOpenThreads == GCL_OPEN_MAX_BLOCKS, "the top kernel is one block");
static_assert(sizeof(struct gcl_tcp_open) == 64 && sizeof(struct gcl_tcp_listen) == 16, "records as 16-B words");

struct OpenParams {
	const uint8_t *frames;
	uint64_t frames_len, stride;
	const uint64_t *offs;
	const uint16_t *pkt_len;
	uint64_t n;
	const uint32_t *order, *sock;
	const uint8_t *l4_status;
	const uint4 *listen;
	const uint32_t *iss;
	uint8_t *verdict;
	uint32_t *later_of, *rst_seq;
	uint4 *open;
	uint32_t *backlog_out;
	unsigned long long *ototals;
	uint4 *desc;
	uint64_t *frame_off;
	uint32_t *seg_conn;
	uint8_t *seg_kind;
	uint32_t *seg_src;
	unsigned long long *stotals;
	unsigned long long *counts;
	uint8_t *tx_frames;
	/* workspace */
	uint4 *tup;      /* [m]: lip, rip, lport | rport << 16, listener */
	uint4 *inf;      /* [m]: class | opt_en << 8 | wscale << 16, rst_seq or irs, mss, leader */
	uint32_t *rank;  /* [m]: before(j) of a listener-route entry */
	uint32_t *table; /* [slots] */
	uint32_t *mat;   /* [blocks][nlisten] */
	uint32_t *bsum;  /* [2][blocks]: segments, records */
	uint64_t m, per, seg_lim, frame_base, open_cap;
	uint32_t listen_base, nlisten, frame_stride, blocks, slot_mask;
};

/* N little-endian dwords of frames from byte @at on (at >= 4), bytes at or past frames_len as 0 */
template <int N>
__device__ __forceinline__ void open_load(const uint8_t *frames, uint64_t frames_len, uint64_t at, uint32_t d[N])
{
	const uint32_t mis = (uint32_t)((uintptr_t)frames + at) & 3u, sh = 8 * mis;
	const uint64_t at0 = at - mis;
	uint32_t w[N + 1];

#pragma unroll
	for (int x = 0; x <= N; x++) {
		const uint64_t f = at0 + 4 * (uint64_t)x;
		uint32_t v = 0;
		if (f < frames_len && frames_len - f >= 4) {
			v = *(const uint32_t *)(frames + f);
		} else {
			for (uint32_t y = 0; y < 4; y++)
				if (f + y < frames_len)
					v |= (uint32_t)frames[f + y] << (8 * y);
		}
		w[x] = v;
	}
#pragma unroll
	for (int x = 0; x < N; x++)
		d[x] = sh ? w[x] >> sh | w[x + 1] << (32 - sh) : w[x];
}

__device__ __forceinline__ bool open_same(const uint4 &a, const uint4 &b)
{
	return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0;
}

__global__ void __launch_bounds__(kOpenThreads) open_decide_kernel(OpenParams k)
{
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;

	for (uint64_t j = lo + threadIdx.x; j < hi; j += kOpenThreads) {
		const uint64_t i = k.order ? k.order[j] : j;
		struct gcl_open_ent e = {GCL_OPEN_OOR, 0, 0, 0, 0, 0, 0};
		struct gcl_open_opts op = {0, 0, 0, 0};

		if (i < k.n) {
			const uint32_t st = k.l4_status ? k.l4_status[i] : 0;
			const uint32_t sk = k.sock[i];
			const uint64_t off = k.offs ? k.offs[i] : i * k.stride;
			const uint64_t o = off < k.frames_len ? off : k.frames_len;
			const uint64_t avail = k.frames_len - o;
			const uint64_t L = k.pkt_len[i] < avail ? k.pkt_len[i] : avail;
			uint32_t d[11];

			open_load<11>(k.frames, k.frames_len, o + 12, d);
			e = gcl_open_head(d, L, k.l4_status != nullptr, st, sk, k.listen_base, k.nlisten);
			if (e.cls == GCL_OPEN_ACCEPT) {
				uint32_t w[10];

				open_load<10>(k.frames, k.frames_len, o + 54, w);
				op = gcl_open_walk(w, e.optlen);
				if (op.bad)
					e.cls = GCL_OPEN_BADOPT;
			}
		}
		k.tup[j] = make_uint4(e.lip, e.rip, e.ports, e.listener);
		k.inf[j] = make_uint4(e.cls | op.opt_en << 8 | op.wscale << 16, e.val, op.mss, GCL_OPEN_NONE);
	}
}

__global__ void __launch_bounds__(kOpenThreads) open_insert_kernel(OpenParams k)
{
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;

	for (uint64_t j = lo + threadIdx.x; j < hi; j += kOpenThreads) {
		if ((k.inf[j].x & 0xFFu) != GCL_OPEN_ACCEPT)
			continue;
		const uint4 t = k.tup[j];
		uint32_t s = gcl_open_hash(t.x, t.y, t.z, t.w) & k.slot_mask;

		/* candidates <= m <= slots / 2: an empty slot or the tuple's own is met before the table is round */
		for (uint64_t probe = 0; probe <= k.slot_mask; probe++) {
			const uint32_t cur = atomicCAS(&k.table[s], GCL_OPEN_NONE, (uint32_t)j);
			if (cur == GCL_OPEN_NONE)
				break;
			if (open_same(k.tup[cur], t)) { /* cur was inserted: a list index below m */
				atomicMin(&k.table[s], (uint32_t)j);
				break;
			}
			s = (s + 1) & k.slot_mask;
		}
	}
}

__global__ void __launch_bounds__(kOpenThreads) open_count_kernel(OpenParams k)
{
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;

	for (uint64_t j = lo + threadIdx.x; j < hi; j += kOpenThreads) {
		if (!gcl_open_listener_route(k.inf[j].x & 0xFFu))
			continue;
		const uint4 t = k.tup[j];
		uint32_t s = gcl_open_hash(t.x, t.y, t.z, t.w) & k.slot_mask, leader = GCL_OPEN_NONE;

		for (uint64_t probe = 0; probe <= k.slot_mask; probe++) {
			const uint32_t cur = k.table[s];
			if (cur == GCL_OPEN_NONE)
				break;
			if (open_same(k.tup[cur], t)) {
				leader = cur;
				break;
			}
			s = (s + 1) & k.slot_mask;
		}
		((uint32_t *)&k.inf[j])[3] = leader;
		if (leader == (uint32_t)j)
			atomicAdd(&k.mat[(size_t)blockIdx.x * k.nlisten + t.w], 1u); /* t.w < nlisten: gcl_open_head */
	}
}

/* a column of the matrix -> its exclusive prefix sums over the ranges; backlog_out */
__global__ void __launch_bounds__(kOpenThreads) open_scan_kernel(OpenParams k)
{
	const uint32_t l = blockIdx.x * kOpenThreads + threadIdx.x;

	if (l >= k.nlisten)
		return;
	uint32_t run = 0;
	for (uint32_t r = 0; r < k.blocks; r++) {
		const uint32_t v = k.mat[(size_t)r * k.nlisten + l];
		k.mat[(size_t)r * k.nlisten + l] = run;
		run += v;
	}
	const uint4 L4 = k.listen[l];
	const uint32_t taken = (L4.z >> 24 & GCL_LISTEN_SHUTDOWN) ? 0 : run < L4.x ? run : L4.x;
	k.backlog_out[l] = L4.x - taken;
}

__global__ void __launch_bounds__(kOpenThreads) open_rank_kernel(OpenParams k)
{
	__shared__ uint32_t cnt[GCL_OPEN_MAX_LISTEN];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t below = (1ull << lane) - 1;

	for (uint32_t l = threadIdx.x; l < k.nlisten; l += kOpenThreads)
		cnt[l] = k.mat[(size_t)blockIdx.x * k.nlisten + l];
	__syncthreads();
	for (uint64_t j0 = lo; j0 < hi; j0 += kOpenThreads) { /* uniform: every lane reaches the barriers */
		const uint64_t j = j0 + threadIdx.x;
		bool lr = false, lead = false;
		uint32_t l = 0, rk = 0;

		if (j < hi) {
			const uint4 f = k.inf[j];
			lr = gcl_open_listener_route(f.x & 0xFFu);
			lead = f.w == (uint32_t)j;
			if (lr)
				l = k.tup[j].w;
		}
		for (uint32_t w = 0; w < kOpenWaves; w++) {
			if (wave == w) {
				uint64_t act = __ballot(lr);
				while (act) { /* wave-uniform: one round per distinct listener */
					const int first = __ffsll((unsigned long long)act) - 1;
					const uint32_t l0 = (uint32_t)__shfl((int)l, first);
					const bool same = lr && l == l0;
					const uint64_t sm = __ballot(same), lm = __ballot(same && lead);
					const uint32_t base = cnt[l0]; /* l0 < nlisten */
					if (same)
						rk = base + (uint32_t)__popcll(lm & below);
					if ((int)lane == first)
						cnt[l0] = base + (uint32_t)__popcll(lm);
					act &= ~sm;
				}
			}
			__syncthreads();
		}
		if (lr)
			k.rank[j] = rk;
	}
}

/* the verdict of entry j < m, from what decide, count and rank left */
__device__ __forceinline__ uint32_t open_verdict(const OpenParams &k, uint64_t j, const uint4 &f, uint32_t *later)
{
	const uint32_t cls = f.x & 0xFFu;

	*later = GCL_OPEN_NONE;
	if (!gcl_open_listener_route(cls))
		return cls;
	const uint4 L4 = k.listen[k.tup[j].w];
	const uint32_t lflags = L4.z >> 24;
	bool lat = false;

	if (f.w != GCL_OPEN_NONE && f.w < j) /* a leader is a listener-route entry: its rank was written */
		lat = !(lflags & GCL_LISTEN_SHUTDOWN) && k.rank[f.w] < L4.x;
	if (lat)
		*later = f.w;
	return gcl_open_final(cls, lat, lflags, L4.x, k.rank[j]);
}

__device__ __forceinline__ bool open_wants_seg(uint32_t v)
{
	return v == GCL_OPEN_ACCEPT || v == GCL_OPEN_RST || v == GCL_OPEN_CLOSED_RST || v == GCL_OPEN_CLOSED_RST_ACK;
}

__global__ void __launch_bounds__(kOpenThreads) open_final_kernel(OpenParams k)
{
	__shared__ uint32_t ws[2][kOpenWaves];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;
	uint32_t segs = 0, opens = 0, cnt[GCL_OPEN_NR_VERDICTS] = {0}; /* wave-uniform */

	for (uint64_t j0 = lo; j0 < hi; j0 += kOpenThreads) { /* uniform: every lane reaches the ballots */
		const uint64_t j = j0 + threadIdx.x;
		uint32_t v = GCL_OPEN_NR_VERDICTS;

		if (j < hi) {
			const uint4 f = k.inf[j];
			uint32_t later;

			v = open_verdict(k, j, f, &later);
			k.verdict[j] = (uint8_t)v;
			k.later_of[j] = later;
			k.rst_seq[j] = v == GCL_OPEN_RST || v == GCL_OPEN_CLOSED_RST || v == GCL_OPEN_CLOSED_RST_ACK ? f.y : 0;
		}
		segs += (uint32_t)__popcll(__ballot(v != GCL_OPEN_NR_VERDICTS && open_wants_seg(v)));
		opens += (uint32_t)__popcll(__ballot(v == GCL_OPEN_ACCEPT));
		if (k.counts) {
#pragma unroll
			for (uint32_t x = 0; x < GCL_OPEN_NR_VERDICTS; x++)
				cnt[x] += (uint32_t)__popcll(__ballot(v == x));
		}
	}
	if (k.counts && (threadIdx.x & 63) == 0) {
#pragma unroll
		for (uint32_t x = 0; x < GCL_OPEN_NR_VERDICTS; x++)
			if (cnt[x])
				atomicAdd(k.counts + x, (unsigned long long)cnt[x]);
	}
	if ((threadIdx.x & 63) == 0) {
		ws[0][threadIdx.x >> 6] = segs;
		ws[1][threadIdx.x >> 6] = opens;
	}
	__syncthreads();
	if (threadIdx.x < 2)
		k.bsum[threadIdx.x * k.blocks + blockIdx.x] = ws[threadIdx.x][0] + ws[threadIdx.x][1] + ws[threadIdx.x][2] +
		                                              ws[threadIdx.x][3];
}

/* bsum[a][0, blocks) -> its exclusive prefix sums, a = 0, 1; the totals; one block */
__global__ void __launch_bounds__(kOpenThreads) open_top_kernel(OpenParams k)
{
	__shared__ uint32_t sc[2][kOpenThreads];
	const uint32_t t = threadIdx.x;

	for (uint32_t a = 0; a < 2; a++) {
		uint32_t *bs = k.bsum + a * k.blocks;
		uint32_t v[kOpenTopPer], sum = 0;

#pragma unroll
		for (uint32_t x = 0; x < kOpenTopPer; x++) {
			const uint32_t r = t * kOpenTopPer + x;
			v[x] = r < k.blocks ? bs[r] : 0;
			sum += v[x];
		}
		uint32_t cur = 0;
		sc[0][t] = sum;
		__syncthreads();
		for (uint32_t step = 1; step < kOpenThreads; step <<= 1) {
			const uint32_t s = t >= step ? sc[cur][t - step] + sc[cur][t] : sc[cur][t];
			sc[cur ^ 1][t] = s;
			cur ^= 1;
			__syncthreads();
		}
		uint32_t base = t ? sc[cur][t - 1] : 0;
#pragma unroll
		for (uint32_t x = 0; x < kOpenTopPer; x++) {
			const uint32_t r = t * kOpenTopPer + x;
			if (r < k.blocks)
				bs[r] = base;
			base += v[x];
		}
		if (t == kOpenThreads - 1) {
			const unsigned long long wanted = base, cap = a == 0 ? k.seg_lim : k.open_cap;
			const unsigned long long written = wanted < cap ? wanted : cap;
			unsigned long long *tot = a == 0 ? k.stotals : k.ototals;

			tot[0] = wanted;
			tot[1] = written;
			if (k.counts) {
				if (a == 0 && written)
					atomicAdd(k.counts + GCL_OPENC_SEGS, written);
				if (wanted > written)
					atomicAdd(k.counts + (a == 0 ? GCL_OPENC_SEGSKIP : GCL_OPENC_NOSPACE), wanted - written);
			}
		}
		__syncthreads(); /* sc is reused */
	}
}

__global__ void __launch_bounds__(kOpenThreads) open_emit_kernel(OpenParams k)
{
	__shared__ uint32_t wt[2][2][kOpenWaves];
	const uint64_t lo = (uint64_t)blockIdx.x * k.per;
	const uint64_t hi = lo + k.per < k.m ? lo + k.per : k.m;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t below = (1ull << lane) - 1;
	uint64_t scarry = lo < hi ? k.bsum[blockIdx.x] : 0;            /* the range's base, then the tiles before */
	uint64_t ocarry = lo < hi ? k.bsum[k.blocks + blockIdx.x] : 0;
	uint32_t par = 0;

	for (uint64_t j0 = lo; j0 < hi; j0 += kOpenThreads, par ^= 1) { /* uniform: every lane active */
		const uint64_t j = j0 + threadIdx.x;
		const uint32_t v = j < hi ? k.verdict[j] : GCL_OPEN_NR_VERDICTS;
		const bool sg = j < hi && open_wants_seg(v), acc = v == GCL_OPEN_ACCEPT;
		const uint64_t m0 = __ballot(sg), m1 = __ballot(acc);

		if (lane == 0) {
			wt[par][0][wave] = (uint32_t)__popcll(m0);
			wt[par][1][wave] = (uint32_t)__popcll(m1);
		}
		__syncthreads();
		uint64_t at = scarry + (uint32_t)__popcll(m0 & below), oat = ocarry + (uint32_t)__popcll(m1 & below);
#pragma unroll
		for (uint32_t w = 0; w < kOpenWaves; w++) {
			if (w < wave) {
				at += wt[par][0][w];
				oat += wt[par][1][w];
			}
			scarry += wt[par][0][w];
			ocarry += wt[par][1][w];
		}

		if (!sg)
			continue; /* the loop's own barrier is behind every lane of this tile */
		const uint4 t = k.tup[j], f = k.inf[j];
		const uint64_t fo = k.frame_base + at * k.frame_stride;
		uint32_t d[8];

		if (acc) {
			const uint4 L4 = k.listen[t.w];
			const uint32_t l[4] = {L4.x, L4.y, L4.z, L4.w};
			const struct gcl_open_ent e = {v, t.w, t.x, t.y, t.z, f.y, 0};
			const struct gcl_open_opts op = {(f.x >> 8) & 0xFFu, f.z, (f.x >> 16) & 0xFFu, 0};
			uint32_t r[16];

			gcl_open_record(&e, &op, (uint32_t)j, k.iss[j], l, r);
			if (oat < k.open_cap) {
#pragma unroll
				for (int x = 0; x < 4; x++)
					k.open[4 * oat + x] = make_uint4(r[4 * x], r[4 * x + 1], r[4 * x + 2], r[4 * x + 3]);
			}
			if (at >= k.seg_lim)
				continue;
			gcl_open_synack_desc(r, d);
			k.seg_conn[at] = (uint32_t)oat;
			k.seg_kind[at] = GCL_CTL_SYNACK;
			/* at < seg_lim: [fo, fo + frame_stride) lies inside tx_frames_len, and frame_stride >= 62 */
			uint8_t ob[8];
			const uint32_t nb = gcl_open_optbytes(r, l, ob);
#pragma unroll
			for (uint32_t x = 0; x < 8; x++)
				if (x < nb)
					k.tx_frames[fo + 54 + x] = ob[x];
		} else {
			if (at >= k.seg_lim)
				continue;
			const uint32_t a[4] = {t.x, t.y, t.z, 0};
			const uint32_t kind = v == GCL_OPEN_CLOSED_RST_ACK ? GCL_CTL_RST_ACK : GCL_CTL_RST;

			gcl_ctl_rst_desc(a, kind, f.y, d);
			k.seg_conn[at] = GCL_OPEN_NONE;
			k.seg_kind[at] = (uint8_t)kind;
		}
		k.desc[2 * at] = make_uint4(d[0], d[1], d[2], d[3]);
		k.desc[2 * at + 1] = make_uint4(d[4], d[5], d[6], d[7]);
		k.frame_off[at] = fo;
		k.seg_src[at] = (uint32_t)j;
	}
}

struct OpenLayout {
	size_t tup, inf, rank, table, mat, bsum, total;
};

static size_t open_r16(size_t x)
{
	return (x + 15) & ~(size_t)15;
}

/* the ranges a call is cut into when in->blocks is 0 cannot be more than this */
static uint32_t open_blocks_bound(uint64_t m, uint32_t blocks)
{
	const uint64_t tiles = (m + kOpenThreads - 1) / kOpenThreads;

	return blocks ? blocks : (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, GCL_OPEN_MAX_BLOCKS));
}

static OpenLayout open_layout(uint64_t m, uint32_t nlisten, uint32_t blocks_bound, uint64_t slots)
{
	OpenLayout l;

	l.tup = 0;
	l.inf = l.tup + 16 * (size_t)m;
	l.rank = l.inf + 16 * (size_t)m;
	l.table = l.rank + open_r16(4 * (size_t)m);
	l.mat = l.table + open_r16(4 * (size_t)slots);
	l.bsum = l.mat + open_r16(4 * (size_t)blocks_bound * nlisten);
	l.total = l.bsum + open_r16(8 * (size_t)blocks_bound);
	return l;
}

static bool open_ws_refused(uint64_t m, uint32_t nlisten, uint32_t blocks, uint32_t hash_slots)
{
	return m > (1ull << 31) || nlisten > GCL_OPEN_MAX_LISTEN || blocks > GCL_OPEN_MAX_BLOCKS ||
	       (hash_slots && ((hash_slots & (hash_slots - 1)) || hash_slots < 2 * m));
}

} // namespace gclk

using namespace gclk;

extern "C" int gcl_tcp_rx_open_workspace(uint64_t m, uint32_t nlisten, uint32_t blocks, uint32_t hash_slots,
                                         size_t *bytes)
{
	if (!bytes || open_ws_refused(m, nlisten, blocks, hash_slots))
		return -EINVAL;
	*bytes = open_layout(m, nlisten, open_blocks_bound(m, blocks), hash_slots ? hash_slots : gcl_open_slots(m)).total;
	return 0;
}

extern "C" int gcl_tcp_rx_open(struct gcl_ctx *c, const struct gcl_batch *b, const struct gcl_tcpopen_in *in,
                               const struct gcl_tcpopen_out *out, const struct gcl_ctlseg_out *seg, uint64_t *counts,
                               void *workspace, size_t workspace_bytes, void *hip_stream)
{
	hipStream_t s = (hipStream_t)hip_stream;

	if (!c || gcl_open_refused(b, in, out, seg, counts))
		return -EINVAL;
	const uint64_t slots = in->hash_slots ? in->hash_slots : gcl_open_slots(in->m);
	const uint32_t bound = open_blocks_bound(in->m, in->blocks);
	const OpenLayout lay = open_layout(in->m, in->nlisten, bound, slots);

	if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < lay.total)
		return -EINVAL;
	if (hipSetDevice(c->device) != hipSuccess)
		return -EIO;
	c->last_stream = s;
	if (in->m == 0)
		return 0;

	const uint64_t tiles = (in->m + kOpenThreads - 1) / kOpenThreads;
	const uint32_t cus = (uint32_t)(c->num_cus > 0 ? c->num_cus : 1);
	uint8_t *ws = (uint8_t *)workspace;
	OpenParams k;

	k.frames = b->frames;
	k.frames_len = b->frames_len;
	k.stride = b->stride;
	k.offs = b->offs;
	k.pkt_len = b->pkt_len;
	k.n = b->n;
	k.order = in->order;
	k.sock = in->sock;
	k.l4_status = in->l4_status;
	k.listen = (const uint4 *)in->listen;
	k.iss = in->iss;
	k.verdict = out->verdict;
	k.later_of = out->later_of;
	k.rst_seq = out->rst_seq;
	k.open = (uint4 *)out->open;
	k.backlog_out = out->backlog_out;
	k.ototals = (unsigned long long *)out->totals;
	k.desc = (uint4 *)seg->desc;
	k.frame_off = seg->frame_off;
	k.seg_conn = seg->seg_conn;
	k.seg_kind = seg->seg_kind;
	k.seg_src = seg->seg_src;
	k.stotals = (unsigned long long *)seg->totals;
	k.counts = (unsigned long long *)counts;
	k.tx_frames = in->tx_frames;
	k.tup = (uint4 *)(ws + lay.tup);
	k.inf = (uint4 *)(ws + lay.inf);
	k.rank = (uint32_t *)(ws + lay.rank);
	k.table = (uint32_t *)(ws + lay.table);
	k.mat = (uint32_t *)(ws + lay.mat);
	k.bsum = (uint32_t *)(ws + lay.bsum);
	k.m = in->m;
	k.blocks = in->blocks ? in->blocks :
	           (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, std::min<uint32_t>(cus * kOpenBlocksPerCu,
	                                                                                      GCL_OPEN_MAX_BLOCKS)));
	/* whole tiles per range, so that every range starts at a multiple of 256 */
	k.per = std::max<uint64_t>(1, (tiles + k.blocks - 1) / k.blocks) * kOpenThreads;
	k.seg_lim = gcl_open_seg_lim(in->seg_cap, in->frame_base, in->frame_stride, in->tx_frames_len);
	k.frame_base = in->frame_base;
	k.open_cap = in->open_cap;
	k.listen_base = in->listen_base;
	k.nlisten = in->nlisten;
	k.frame_stride = in->frame_stride;
	k.slot_mask = (uint32_t)(slots - 1);

	if (hipMemsetAsync(k.table, 0xFF, 4 * (size_t)slots, s) != hipSuccess)
		return -EIO;
	if (in->nlisten && hipMemsetAsync(k.mat, 0, 4 * (size_t)k.blocks * in->nlisten, s) != hipSuccess)
		return -EIO;
	hipLaunchKernelGGL(open_decide_kernel, dim3(k.blocks), dim3(kOpenThreads), 0, s, k);
	hipLaunchKernelGGL(open_insert_kernel, dim3(k.blocks), dim3(kOpenThreads), 0, s, k);
	if (in->nlisten) {
		hipLaunchKernelGGL(open_count_kernel, dim3(k.blocks), dim3(kOpenThreads), 0, s, k);
		hipLaunchKernelGGL(open_scan_kernel, dim3((in->nlisten + kOpenThreads - 1) / kOpenThreads), dim3(kOpenThreads),
		                   0, s, k);
		hipLaunchKernelGGL(open_rank_kernel, dim3(k.blocks), dim3(kOpenThreads), 0, s, k);
	}
	hipLaunchKernelGGL(open_final_kernel, dim3(k.blocks), dim3(kOpenThreads), 0, s, k);
	hipLaunchKernelGGL(open_top_kernel, dim3(1), dim3(kOpenThreads), 0, s, k);
	hipLaunchKernelGGL(open_emit_kernel, dim3(k.blocks), dim3(kOpenThreads), 0, s, k);
	return hipGetLastError() == hipSuccess ? 0 : -EIO;
}
