/*
 * l4_fuzz.c - CPU fuzz driver for gcl_l4_csum_host, built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_l4; tests/test_l4_sanitize.py runs it).
 *
 *   l4_fuzz SEED ITERS   ITERS batches of up to 48 packets over a heap region
 *                        of exactly frames_len bytes (1..4096; a read or write
 *                        at or past it is a sanitizer report).  Most packets
 *                        start as well-formed TCP or UDP frames, then get
 *                        hostile fields: a tot that lies about the length, a
 *                        pkt_len longer or shorter than the frame, an offset
 *                        near, at or far past frames_len (UINT64_MAX too), a
 *                        frame cut by frames_len, fragments, other protocols
 *                        and IHLs.  Each batch is run in VERIFY, then in FILL
 *                        with random tx_olflags, then in VERIFY again.
 *
 * Checked besides the sanitizers: VERIFY changes no frame byte; FILL changes
 * only checksum bytes of packets whose status says so, and nothing in a batch
 * whose tx_olflags are all 0; the counts are the status bytes' census; after
 * a FILL of everything, every packet it filled that no other packet overlaps
 * verifies GOOD.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"

#define MAXP 48

static uint64_t rng_state;

static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); abort(); } } while (0)

static void census(const uint8_t *st, uint64_t n, const uint64_t *cnt)
{
	uint64_t c[GCL_L4C_NR] = {0};

	for (uint64_t i = 0; i < n; i++) {
		const uint8_t v = st[i] & 0xF;
		c[v == GCL_L4_GOOD ? GCL_L4C_GOOD : v == GCL_L4_BAD ? GCL_L4C_BAD :
		  v == GCL_L4_NONE ? GCL_L4C_NONE : GCL_L4C_NA]++;
		c[GCL_L4C_FILLED_IP] += !!(st[i] & GCL_L4_FILLED_IP);
		c[GCL_L4C_FILLED_L4] += !!(st[i] & GCL_L4_FILLED_L4);
		CHECK(v <= GCL_L4_NONE && !(st[i] & ~0x3F), "status %#x\n", st[i]);
	}
	for (int k = 0; k < GCL_L4C_BYTES; k++)
		CHECK(c[k] == cnt[k], "count %d: %llu != %llu\n", k, (unsigned long long)cnt[k],
		      (unsigned long long)c[k]);
	CHECK(c[GCL_L4C_GOOD] + c[GCL_L4C_BAD] + c[GCL_L4C_NONE] + c[GCL_L4C_NA] == n, "census\n");
}

int main(int argc, char **argv)
{
	uint64_t good = 0, bad = 0, na = 0, filled = 0;

	if (argc < 3) {
		fprintf(stderr, "usage: l4_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);

	for (uint64_t it = 0; it < iters; it++) {
		const uint64_t flen = it % 7 == 0 ? 1 + rnd() % 80 : 1 + rnd() % 4096;
		const uint64_t n = 1 + rnd() % MAXP;
		const bool use_offs = rnd() & 1;
		const uint64_t stride = 16 * (1 + rnd() % 12);
		/* exactly sized heap blocks: every array and the region */
		uint8_t *frames = malloc(flen), *snap = malloc(flen);
		uint64_t *offs = malloc(n * sizeof(*offs));
		uint16_t *plen = malloc(n * sizeof(*plen));
		uint8_t *txf = malloc(n), *st = malloc(n), *st2 = malloc(n);
		uint64_t cnt[GCL_L4C_NR];

		for (uint64_t i = 0; i < flen; i++)
			frames[i] = (uint8_t)rnd();
		uint64_t cur = 0;
		for (uint64_t i = 0; i < n; i++) {
			const uint64_t r = rnd();
			const bool tcp = r & 1;
			const uint32_t l4len = (tcp ? 20 : 8) + (uint32_t)(rnd() % 120);
			uint32_t tot = 20 + l4len, flen_i = 34 + l4len + (uint32_t)(rnd() % 4);
			const uint64_t o = use_offs ? cur + rnd() % 5 : i * stride;
			uint8_t h[34] = {0};

			cur = o + flen_i;
			h[12] = 0x08;
			h[14] = 0x45;
			h[20] = r & 2 ? 0x40 : 0;
			h[23] = tcp ? 6 : 17;
			for (int k = 26; k < 34; k++)
				h[k] = (uint8_t)rnd();
			switch ((r >> 8) % 16) { /* half of them hostile */
			case 0: tot = (uint32_t)rnd() & 0xFFFF; break;
			case 1: tot += 1 + (uint32_t)rnd() % 4; break;
			case 2: h[14] = (uint8_t)rnd(); break;
			case 3: h[20] = (uint8_t)rnd(); h[21] = (uint8_t)rnd(); break;
			case 4: h[23] = (uint8_t)rnd(); break;
			case 5: h[12] = (uint8_t)rnd(); break;
			case 6: flen_i = (uint32_t)rnd() % 70; break;
			case 7: flen_i = 65535; break;
			default: break;
			}
			h[16] = (uint8_t)(tot >> 8);
			h[17] = (uint8_t)tot;
			offs[i] = o;
			plen[i] = (uint16_t)flen_i;
			/* the header goes where it fits; a frame near the end is cut by frames_len */
			for (int k = 0; k < 34; k++)
				if (o + k < flen && (k >= 12 && k != 24 && k != 25))
					frames[o + k] = h[k];
			if ((r >> 16) % 16 == 0)
				offs[i] = (r >> 20) % 4 == 0 ? UINT64_MAX : (r >> 20) % 4 == 1 ? flen :
				          (r >> 20) % 4 == 2 ? flen + rnd() % 64 : flen - rnd() % (flen < 40 ? flen : 40);
			txf[i] = (uint8_t)rnd();
		}
		struct gcl_batch b = { .frames = frames, .frames_len = flen, .stride = stride,
		                       .offs = use_offs ? offs : NULL, .pkt_len = plen, .n = n };
		struct gcl_l4_in in = { .size = sizeof(in), .mode = GCL_L4_VERIFY };

		/* VERIFY writes no frame byte */
		memcpy(snap, frames, flen);
		memset(cnt, 0, sizeof(cnt));
		CHECK(gcl_l4_csum_host(&b, &in, st, cnt) == 0, "verify failed\n");
		CHECK(!memcmp(snap, frames, flen), "VERIFY wrote a frame byte\n");
		census(st, n, cnt);
		for (uint64_t i = 0; i < n; i++) {
			CHECK(!(st[i] & 0xF0), "VERIFY set a fill bit\n");
			bad += st[i] == GCL_L4_BAD;
			na += st[i] == GCL_L4_NA;
		}

		/* FILL with random flags: only checksum bytes of packets that say so change */
		in.mode = GCL_L4_FILL;
		in.tx_olflags = txf;
		if (it % 5 == 0)
			memset(txf, 0xFC, n); /* neither bit: nothing may change */
		memset(cnt, 0, sizeof(cnt));
		CHECK(gcl_l4_csum_host(&b, &in, st, cnt) == 0, "fill failed\n");
		census(st, n, cnt);
		for (uint64_t i = 0; i < n; i++) {
			const uint64_t raw = use_offs ? offs[i] : i * stride, o = raw < flen ? raw : flen;
			CHECK(!(st[i] & 0xF), "FILL set a verdict\n");
			CHECK(!(st[i] & GCL_L4_FILLED_IP) || (txf[i] & 1), "IP filled unasked\n");
			CHECK(!(st[i] & GCL_L4_FILLED_L4) || (txf[i] & 2), "L4 filled unasked\n");
			if (st[i] & GCL_L4_FILLED_IP) /* forget the bytes that may differ */
				snap[o + 24] = frames[o + 24], snap[o + 25] = frames[o + 25];
			if (st[i] & GCL_L4_FILLED_L4) {
				const uint64_t fo = o + (frames[o + 23] == 6 ? 50 : 40);
				snap[fo] = frames[fo], snap[fo + 1] = frames[fo + 1];
			}
		}
		CHECK(!memcmp(snap, frames, flen), "FILL wrote outside its fields\n");

		/* FILL of everything, then VERIFY: a filled packet nobody overlaps is GOOD */
		in.tx_olflags = NULL;
		CHECK(gcl_l4_csum_host(&b, &in, st, NULL) == 0, "fill all failed\n");
		in.mode = GCL_L4_VERIFY;
		CHECK(gcl_l4_csum_host(&b, &in, st2, NULL) == 0, "verify 2 failed\n");
		for (uint64_t i = 0; i < n; i++) {
			if (!(st[i] & GCL_L4_FILLED_L4))
				continue;
			filled++;
			good += st2[i] == GCL_L4_GOOD;
			bool alone = true;
			const uint64_t oi = use_offs ? offs[i] : i * stride;
			for (uint64_t j = 0; j < n; j++) {
				const uint64_t oj = use_offs ? offs[j] : j * stride;
				if (j != i && (st[j] & 0xF0) && oj < oi + plen[i] && oi < oj + plen[j])
					alone = false;
			}
			CHECK(!alone || st2[i] == GCL_L4_GOOD, "filled packet %llu verifies %#x\n",
			      (unsigned long long)i, st2[i]);
		}

		/* the refusals read nothing */
		struct gcl_batch nb = b;
		nb.pkt_len = NULL;
		CHECK(gcl_l4_csum_host(&nb, &in, st, NULL) == -EINVAL, "NULL pkt_len accepted\n");
		in.mode = 2;
		CHECK(gcl_l4_csum_host(&b, &in, st, NULL) == -EINVAL, "mode 2 accepted\n");

		free(frames), free(snap), free(offs), free(plen), free(txf), free(st), free(st2);
	}
	printf("l4 ok %llu %llu %llu %llu\n", (unsigned long long)good, (unsigned long long)bad,
	       (unsigned long long)na, (unsigned long long)filled);
	return 0;
}
