/*
 * csum_fuzz.c - CPU fuzz driver for gcl_rx_csum_flags, built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_csum; tests/test_csum_sanitize.py runs it).
 *
 *   csum_fuzz SEED ITERS   ITERS rounds over every len in [0, 80]: a random
 *                          frame in a heap block of exactly len bytes (len 0:
 *                          a NULL frame), half of them IPv4 with the header
 *                          checksum made valid where the frame is long enough
 *                          to hold it, every value of the flags' low nibble.
 *                          A read at or past len is a sanitizer report.  The
 *                          result is compared with the rule written out over a
 *                          zero-padded copy.
 *
 * Exit 0 when every call returned what the rule says; a sanitizer report
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

/* big-endian 16-bit words of pad[14, 34), folded */
static uint32_t hdr_sum(const uint8_t *pad)
{
	uint32_t s = 0;
	for (int i = 14; i < 34; i += 2)
		s += (uint32_t)pad[i] << 8 | pad[i + 1];
	while (s >> 16)
		s = (s & 0xFFFF) + (s >> 16);
	return s;
}

int main(int argc, char **argv)
{
	uint64_t good = 0, bad = 0, kept = 0;

	if (argc < 3) {
		fprintf(stderr, "usage: csum_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);
	for (uint64_t it = 0; it < iters; it++) {
		for (size_t len = 0; len <= 80; len++) {
			uint8_t pad[96] = { 0 };
			uint8_t *frame = len ? malloc(len) : NULL; /* exactly len bytes */
			const uint64_t r = rnd();
			const uint8_t fl = (uint8_t)(r >> 8);

			for (size_t i = 0; i < len; i++)
				pad[i] = (uint8_t)rnd();
			if (r & 1) {
				pad[12] = 0x08;
				pad[13] = 0x00;
			}
			if (r & 2) { /* a valid checksum field, as far as the frame holds it */
				pad[24] = pad[25] = 0;
				const uint32_t c = ~hdr_sum(pad) & 0xFFFF;
				pad[24] = (uint8_t)(c >> 8);
				pad[25] = (uint8_t)c;
			}
			memset(pad + len, 0, sizeof(pad) - len);
			if (len)
				memcpy(frame, pad, len);

			uint8_t want = fl;
			if (pad[12] == 0x08 && pad[13] == 0x00 && (fl & GCL_F_IP_CKSUM_MASK) != GCL_F_IP_CKSUM_GOOD)
				want = (uint8_t)((fl & ~GCL_F_IP_CKSUM_MASK) |
				                 (hdr_sum(pad) == 0xFFFF ? GCL_F_IP_CKSUM_GOOD : GCL_F_IP_CKSUM_BAD));
			const uint8_t got = gcl_rx_csum_flags(frame, len, fl);
			if (got != want) {
				fprintf(stderr, "len %zu flags %#x: got %#x want %#x\n", len, fl, got, want);
				abort();
			}
			if (got == fl && want == fl && !(pad[12] == 0x08 && pad[13] == 0x00 &&
			                                 (fl & GCL_F_IP_CKSUM_MASK) != GCL_F_IP_CKSUM_GOOD))
				kept++;
			else if ((got & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD)
				good++;
			else
				bad++;
			free(frame);
		}
	}
	printf("csum ok %llu %llu %llu\n", (unsigned long long)good, (unsigned long long)bad,
	       (unsigned long long)kept);
	return 0;
}
