/*
 * copy_fuzz.c - CPU fuzz driver for gcl_copy_batch_host, built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_copy; tests/test_copy_sanitize.py runs it).
 *
 *   copy_fuzz SEED ITERS   ITERS batches of 1-48 packets: src and dst in heap
 *                          blocks of exactly src_len and dst_len bytes (0 to
 *                          400 each), the per-packet arrays in blocks of
 *                          exactly n elements, offsets and lengths random
 *                          with values near 0, src_len, dst_len, 2^63 and
 *                          UINT64_MAX, with offsets or with a stride, with
 *                          and without a cap and the optional arrays.  A read
 *                          or write outside a block is a sanitizer report.
 *                          The result is compared with the rule written out
 *                          byte by byte in packet order.
 *
 * Exit 0 when every batch came out as the rule says; a sanitizer report
 * aborts with non-zero.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"

static uint64_t rng_state;

static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

/* an offset into a region of @len bytes: inside, at its ends, or far away */
static uint64_t rnd_off(uint64_t len)
{
	const uint64_t r = rnd();
	switch (r & 7) {
	case 0: return len + (r >> 8) % 17 - 8;   /* near the end (wraps near 0) */
	case 1: return (r >> 8) % 17;
	case 2: return UINT64_MAX - (r >> 8) % 70;
	case 3: return (1ull << 63) + (r >> 8) % 3 - 1;
	default: return len ? (r >> 8) % len : 0;
	}
}

#define DIE(...) do { fprintf(stderr, __VA_ARGS__); abort(); } while (0)

int main(int argc, char **argv)
{
	uint64_t total[GCL_COPY_NR] = { 0 }, zero_tails = 0;

	if (argc < 3) {
		fprintf(stderr, "usage: copy_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);
	for (uint64_t it = 0; it < iters; it++) {
		const uint64_t r = rnd();
		const uint64_t n = 1 + (r >> 4) % 48;
		const uint64_t src_len = (r >> 12) % 401, dst_len = (r >> 24) % 401;
		const int use_off = r & 1, use_fl = r >> 1 & 1, use_hash = r >> 2 & 1, use_out = r >> 3 & 1;
		uint8_t *src = malloc(src_len), *dst = malloc(dst_len), *want = malloc(dst_len);
		uint64_t *src_off = malloc(n * 8), *dst_off = use_off ? malloc(n * 8) : NULL;
		uint16_t *len = malloc(n * 2), *pkt_len = malloc(n * 2);
		uint8_t *txf = use_fl ? malloc(n) : NULL, *olf = use_out ? malloc(n) : NULL;
		uint32_t *hash = use_hash ? malloc(n * 4) : NULL, *rss = use_out ? malloc(n * 4) : NULL;
		uint64_t counts[GCL_COPY_NR] = { 5, 6, 7, 8 }, wc[GCL_COPY_NR] = { 5, 6, 7, 8 };
		const uint64_t strides[4] = { 16, 32, 64, 1 << 20 };
		struct gcl_copy_in in = { .size = sizeof(in), .src = src, .src_len = src_len, .src_off = src_off,
			                  .len = len, .tx_olflags = txf, .hash = hash, .n = n,
			                  .dst_cap = (r >> 40 & 3) ? 0 : (uint32_t)((r >> 42) % 200) };
		struct gcl_copy_out out = { .dst = dst, .dst_len = dst_len, .dst_off = dst_off,
			                    .dst_stride = strides[r >> 50 & 3], .pkt_len = pkt_len,
			                    .olflags = olf, .rss = rss };

		if (!src || !dst || !want)
			DIE("malloc\n");
		for (uint64_t i = 0; i < src_len; i++)
			src[i] = (uint8_t)(rnd() | 1);
		memset(dst, 0x5A, dst_len);
		memset(want, 0x5A, dst_len);
		for (uint64_t i = 0; i < n; i++) {
			const uint64_t q = rnd();
			src_off[i] = rnd_off(src_len);
			if (dst_off)
				dst_off[i] = rnd_off(dst_len);
			len[i] = (q & 3) == 0 ? (uint16_t)(q >> 8) : (uint16_t)((q >> 8) % 80);
			if (txf)
				txf[i] = (uint8_t)(q >> 32);
			if (hash)
				hash[i] = (uint32_t)(q >> 24);
		}

		if (gcl_copy_batch_host(&in, &out, counts))
			DIE("iter %llu: refused the batch\n", (unsigned long long)it);

		for (uint64_t i = 0; i < n; i++) {
			const uint64_t L = len[i], d = dst_off ? dst_off[i] : i * out.dst_stride;
			int refused = (in.dst_cap && L > in.dst_cap) || (!dst_off && L > out.dst_stride) ||
			              d > dst_len || L > dst_len - d;
			if (!refused) {
				for (uint64_t j = 0; j < L; j++) {
					/* src_off + j < src_len without the sum */
					const int inside = src_off[i] < src_len && j < src_len - src_off[i];
					want[d + j] = inside ? src[src_off[i] + j] : 0;
					zero_tails += !inside;
				}
				wc[GCL_COPY_COPIED]++;
				wc[GCL_COPY_BYTES] += L;
			} else {
				wc[GCL_COPY_REFUSED]++;
			}
			if (pkt_len[i] != (refused ? 0 : L))
				DIE("iter %llu packet %llu: pkt_len %u\n", (unsigned long long)it,
				    (unsigned long long)i, pkt_len[i]);
			if (olf && olf[i] != gcl_loopback_olflags(txf ? txf[i] : 0))
				DIE("iter %llu packet %llu: olflags\n", (unsigned long long)it, (unsigned long long)i);
			if (rss && rss[i] != (hash ? hash[i] : 0))
				DIE("iter %llu packet %llu: rss\n", (unsigned long long)it, (unsigned long long)i);
		}
		if (dst_len && memcmp(dst, want, dst_len))
			DIE("iter %llu: destination differs\n", (unsigned long long)it);
		if (memcmp(counts, wc, sizeof(wc)))
			DIE("iter %llu: counts differ\n", (unsigned long long)it);
		for (int k = 0; k < 3; k++)
			total[k] += counts[k] - (uint64_t)(5 + k);
		free(src); free(dst); free(want); free(src_off); free(dst_off); free(len); free(pkt_len);
		free(txf); free(olf); free(hash); free(rss);
	}
	printf("copy ok %llu %llu %llu %llu\n", (unsigned long long)total[0], (unsigned long long)total[1],
	       (unsigned long long)total[2], (unsigned long long)zero_tails);
	return 0;
}
