/*
 * seg_fuzz.c - CPU fuzz driver for gcl_tx_seg_host, built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_seg; tests/test_seg_sanitize.py runs it).
 *
 *   seg_fuzz SEED ITERS   ITERS batches of up to 48 writes.  A write starts
 *                         plausible and gets hostile fields: any proto, any
 *                         mss (0 and 1 too), lengths and windows up to
 *                         2^32 - 1 (a write of billions of segments must be
 *                         NOSPACE, not a loop), snd_nxt and src_off near their
 *                         wrap.  seg_cap is 0..300; both layouts, any lead,
 *                         strides one byte around a frame, frame_base and
 *                         frames_len anywhere including UINT64_MAX.  Every
 *                         array is a heap block of its exact size: a segment
 *                         written at or past seg_cap is a sanitizer report.
 *
 * Checked besides the sanitizers: the three status counters are the census of
 * status[] and sum to m; *total_segs is the sum of nseg[], at most seg_cap and
 * equal to SEGS; BYTES is the sum of sent[]; the NOSPACE writes are a suffix
 * of the writes not refused; seg_first never decreases and is exact for the
 * OK writes; every segment of an OK write has the write's index, a paylen of
 * at most mss that sums to sent, and PSH exactly on the last; with frames_len
 * given every frame lies inside it; entries past *total_segs keep their fill.
 */
#include <errno.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"

#define MAXM 48

static uint64_t rng_state;

static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); abort(); } } while (0)

static void *block(size_t n, size_t w)
{
	void *p = NULL;
	/* exact size, 16-B aligned: the bytes behind it are poisoned */
	CHECK(posix_memalign(&p, 16, n * w ? n * w : 1) == 0, "no memory\n");
	memset(p, 0xA5, n * w ? n * w : 1);
	return p;
}

int main(int argc, char **argv)
{
	uint64_t seen[3] = {0};

	if (argc < 3) {
		fprintf(stderr, "usage: seg_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);

	for (uint64_t it = 0; it < iters; it++) {
		const uint64_t m = 1 + rnd() % MAXM;
		const uint64_t cap = rnd() % 5 == 0 ? rnd() % 4 : rnd() % 300;
		const bool use_idx = rnd() & 1, use_counts = rnd() % 4 != 0;
		struct gcl_seg_send *send = block(m, sizeof(*send));
		uint8_t *st = block(m, 1);
		uint32_t *sent = block(m, 4), *nxt = block(m, 4), *first = block(m, 4), *nseg = block(m, 4);
		struct gcl_txh_desc *desc = block(cap, sizeof(*desc));
		uint64_t *fo = block(cap, 8), *so = block(cap, 8), *dof = block(cap, 8);
		uint16_t *len = block(cap, 2);
		uint32_t *idx = use_idx ? block(cap, 4) : NULL;
		uint64_t tot[2] = {~0ull, ~0ull}, counts[GCL_SEGC_NR] = {0}, want[GCL_SEGC_NR] = {0};

		for (uint64_t i = 0; i < m; i++) {
			struct gcl_seg_send *w = &send[i];
			for (size_t b = 0; b < sizeof(*w); b++)
				((uint8_t *)w)[b] = (uint8_t)rnd();
			if (rnd() % 8)
				w->proto = rnd() % 3 ? 6 : 17;
			if (rnd() % 8)
				w->mss = rnd() % 4 ? 1 + rnd() % 1460 : rnd() % 3;
			if (rnd() % 6)
				w->len = rnd() % 4 ? rnd() % 4000 : rnd() % 3;
			if (rnd() % 4)
				w->winlen = rnd() & 1 ? w->len + rnd() % 3 - 1 : 1u << 20;
			if (rnd() % 8 == 0)
				w->src_off = UINT64_MAX - rnd() % 3000;
			if (rnd() % 8 == 0)
				w->snd_nxt = UINT32_MAX - (uint32_t)(rnd() % 3000);
		}
		struct gcl_seg_in in = { .size = sizeof(in), .send = send, .m = m, .seg_cap = cap,
		                         .udp_max = rnd() & 1 ? 1472 : (uint32_t)(rnd() % 65508),
		                         .lead = rnd() & 1 ? (uint32_t)(rnd() % 16) : (uint32_t)(rnd() % 65536) };
		switch (rnd() % 4) {
		case 0: in.stride = 0; break;
		case 1: in.stride = in.lead + 54 + 1460 + (uint32_t)(rnd() % 3) - 1; break;
		case 2: in.stride = 1 + (uint32_t)(rnd() % (1u << 20)); break;
		default: in.stride = 2048; break;
		}
		switch (rnd() % 4) {
		case 0: in.frame_base = rnd(); break;
		case 1: in.frame_base = UINT64_MAX - rnd() % 100000; break;
		default: in.frame_base = rnd() % 100000; break;
		}
		switch (rnd() % 4) {
		case 0: in.frames_len = 0; break;
		case 1: in.frames_len = rnd() & 1 ? UINT64_MAX : rnd(); break;
		default: in.frames_len = in.frame_base + rnd() % 400000 - (rnd() % 8 ? 0 : 1000); break;
		}
		struct gcl_seg_out out = { st, sent, nxt, first, nseg, desc, fo, so, len, dof, idx, &tot[0], &tot[1] };

		int ret = gcl_tx_seg_host(&in, &out, use_counts ? counts : NULL);
		CHECK(ret == 0, "tx_seg_host %d\n", ret);

		uint64_t g = 0, bytes = 0;
		bool full = false;
		uint32_t prev = 0;
		for (uint64_t i = 0; i < m; i++) {
			CHECK(st[i] <= GCL_SEG_NOSPACE, "status %u\n", st[i]);
			want[st[i]]++;
			seen[st[i]]++;
			CHECK(first[i] >= prev && first[i] <= cap, "seg_first\n");
			prev = first[i];
			if (st[i] == GCL_SEG_NOSPACE)
				full = true;
			if (st[i] != GCL_SEG_OK) {
				CHECK(!sent[i] && !nseg[i] && nxt[i] == send[i].snd_nxt, "a write that sent nothing\n");
				continue;
			}
			CHECK(!full, "an OK write behind a NOSPACE one\n");
			CHECK(first[i] == g && nseg[i] >= 1 && g + nseg[i] <= cap, "seg_first of an OK write\n");
			CHECK(nxt[i] == send[i].snd_nxt + sent[i], "snd_nxt_out\n");
			uint64_t sum = 0;
			for (uint32_t k = 0; k < nseg[i]; k++, g++) {
				const bool tcp = send[i].proto == 6, lastk = k + 1 == nseg[i];
				CHECK(desc[g].proto == send[i].proto && desc[g].paylen == len[g] && desc[g].pad == 0, "desc\n");
				CHECK(!tcp || (len[g] <= send[i].mss && desc[g].tcp_off == 5 &&
				               desc[g].tcp_flags == (lastk ? 0x18 : 0x10) &&
				               desc[g].seq == send[i].snd_nxt + (uint32_t)sum), "tcp segment\n");
				CHECK(so[g] == send[i].src_off + sum, "src_off\n");
				CHECK(dof[g] == fo[g] + 34 + (tcp ? 20 : 8), "dst_off\n");
				CHECK(!idx || idx[g] == i, "send_idx\n");
				if (in.frames_len)
					CHECK(fo[g] >= in.frame_base && fo[g] <= in.frames_len &&
					      34u + (tcp ? 20 : 8) + len[g] <= in.frames_len - fo[g], "frame outside the region\n");
				sum += len[g];
			}
			CHECK(sum == sent[i], "paylens do not sum to sent\n");
			bytes += sent[i];
			want[GCL_SEGC_PUSH] += send[i].proto == 6;
		}
		CHECK(tot[0] == g && g <= cap, "total_segs\n");
		want[GCL_SEGC_SEGS] = g;
		want[GCL_SEGC_BYTES] = bytes;
		for (uint64_t x = g; x < cap; x++)
			CHECK(len[x] == 0xA5A5 && fo[x] == 0xA5A5A5A5A5A5A5A5ull && (!idx || idx[x] == 0xA5A5A5A5u),
			      "an entry past total_segs was written\n");
		if (use_counts)
			CHECK(!memcmp(counts, want, sizeof(want)), "counts\n");
		in.size--;
		CHECK(gcl_tx_seg_host(&in, &out, NULL) == -EINVAL, "size\n");

		free(send); free(st); free(sent); free(nxt); free(first); free(nseg); free(desc); free(fo); free(so);
		free(dof); free(len); free(idx);
	}
	printf("seg ok %llu %llu %llu\n", (unsigned long long)seen[0], (unsigned long long)seen[1],
	       (unsigned long long)seen[2]);
	return 0;
}
