/*
 * pay_fuzz.c - CPU fuzz driver for gcl_l4_payload_host, built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_pay; tests/test_pay_sanitize.py runs it).
 *
 *   pay_fuzz SEED ITERS   ITERS batches of up to 48 packets over a heap region
 *                         of exactly frames_len bytes (1..4096; a read at or
 *                         past it is a sanitizer report), described through a
 *                         list of up to 96 entries.  Most packets start as
 *                         well-formed TCP or UDP frames, then get hostile
 *                         fields: a tot that lies about the length, a TCP
 *                         data offset of any value, a pkt_len longer or
 *                         shorter than the frame, an offset near, at or far
 *                         past frames_len (UINT64_MAX too), a frame cut by
 *                         frames_len, fragments, other protocols and IHLs.
 *                         order[] holds duplicates and values >= n, seg_off[]
 *                         values past m, sock[] and l4_status[] any bytes.
 *                         Every array is a heap block of its exact size.
 *
 * Checked besides the sanitizers: the six kind counters are the census of
 * kind[] and sum to m, BYTES is the sum of len[]; dst_off is monotone, starts
 * at 0, is a multiple of align and steps by the padded len; total is its end;
 * a kept entry has src_off + len <= frames_len, src_off inside its packet and
 * a meta that names its protocol; an entry that is not kept is all zeros;
 * seg_bytes is dst_off or total; m == 0 writes only total and seg_bytes; the
 * refusals write nothing.
 */
#include <errno.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"

#define MAXP 48
#define MAXM 96

static uint64_t rng_state;

static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); abort(); } } while (0)

int main(int argc, char **argv)
{
	uint64_t kept = 0, na = 0, filtered = 0, oor = 0;

	if (argc < 3) {
		fprintf(stderr, "usage: pay_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);

	for (uint64_t it = 0; it < iters; it++) {
		const uint64_t flen = it % 7 == 0 ? 1 + rnd() % 80 : 1 + rnd() % 4096;
		const uint64_t n = 1 + rnd() % MAXP;
		const bool use_offs = rnd() & 1, use_order = it % 4 != 0;
		const bool use_sock = rnd() & 1, use_st = rnd() & 1, use_seg = rnd() & 1, use_meta = rnd() % 4 != 0;
		const uint64_t m = use_order ? 1 + rnd() % MAXM : n;
		const uint32_t nseg = (uint32_t)(rnd() % 9);
		const uint32_t align = it % 3 == 0 ? 0 : 1u << (rnd() % 9);
		const uint64_t stride = 16 * (1 + rnd() % 12);
		/* exactly sized heap blocks: every array and the region */
		uint8_t *frames = malloc(flen), *snap = malloc(flen);
		uint64_t *offs = malloc(n * sizeof(*offs));
		uint16_t *plen = malloc(n * sizeof(*plen));
		uint32_t *sock = malloc(n * sizeof(*sock)), *order = malloc(m * sizeof(*order));
		uint8_t *st = malloc(n);
		uint32_t *seg = malloc((nseg + 1) * sizeof(*seg));
		uint64_t *src = malloc(m * sizeof(*src)), *dst = malloc(m * sizeof(*dst));
		uint16_t *len = malloc(m * sizeof(*len));
		uint8_t *kind = malloc(m);
		struct gcl_pay_meta *meta = aligned_alloc(16, m * sizeof(*meta));
		uint64_t *segb = malloc((nseg + 1) * sizeof(*segb)), *total = malloc(sizeof(*total));
		uint64_t cnt[GCL_PAYC_NR];

		for (uint64_t i = 0; i < flen; i++)
			frames[i] = (uint8_t)rnd();
		uint64_t cur = 0;
		for (uint64_t i = 0; i < n; i++) {
			const uint64_t r = rnd();
			const bool tcp = r & 1;
			const uint32_t doff = 5 + (uint32_t)((r >> 4) % 4);
			const uint32_t l4len = (tcp ? 4 * doff : 8) + (uint32_t)(rnd() % 100);
			uint32_t tot = 20 + l4len, flen_i = 34 + l4len + (uint32_t)(rnd() % 4);
			const uint64_t o = use_offs ? cur + rnd() % 5 : i * stride;
			uint8_t h[48] = {0};

			cur = o + flen_i;
			h[12] = 0x08;
			h[14] = 0x45;
			h[20] = r & 2 ? 0x40 : 0;
			h[23] = tcp ? 6 : 17;
			h[46] = (uint8_t)(doff << 4 | (rnd() & 15));
			switch ((r >> 8) % 16) { /* half of them hostile */
			case 0: tot = (uint32_t)rnd() & 0xFFFF; break;
			case 1: tot += 1 + (uint32_t)rnd() % 4; break;
			case 2: h[14] = (uint8_t)rnd(); break;
			case 3: h[20] = (uint8_t)rnd(); h[21] = (uint8_t)rnd(); break;
			case 4: h[23] = (uint8_t)rnd(); break;
			case 5: h[12] = (uint8_t)rnd(); break;
			case 6: flen_i = (uint32_t)rnd() % 70; break;
			case 7: flen_i = 65535; break;
			case 8: h[46] = (uint8_t)rnd(); break;
			default: break;
			}
			h[16] = (uint8_t)(tot >> 8);
			h[17] = (uint8_t)tot;
			offs[i] = o;
			plen[i] = (uint16_t)flen_i;
			/* the header fields go where they fit; a frame near the end is cut by frames_len */
			static const int fld[] = {12, 13, 14, 16, 17, 20, 21, 23, 46};
			for (unsigned k = 0; k < sizeof(fld) / sizeof(fld[0]); k++)
				if (o + fld[k] < flen)
					frames[o + fld[k]] = h[fld[k]];
			if ((r >> 16) % 16 == 0)
				offs[i] = (r >> 20) % 4 == 0 ? UINT64_MAX : (r >> 20) % 4 == 1 ? flen :
				          (r >> 20) % 4 == 2 ? flen + rnd() % 64 : flen - rnd() % (flen < 40 ? flen : 40);
			sock[i] = rnd() % 3 == 0 ? (uint32_t)rnd() | 0xFFFFFFE0u : (uint32_t)rnd();
			st[i] = (uint8_t)rnd();
		}
		for (uint64_t j = 0; j < m; j++)
			order[j] = rnd() % 8 == 0 ? (uint32_t)rnd() : (uint32_t)(rnd() % (n + 2));
		for (uint32_t s = 0; s <= nseg; s++)
			seg[s] = rnd() % 4 == 0 ? (uint32_t)rnd() : (uint32_t)(rnd() % (m + 2));
		memset(src, 0xA7, m * sizeof(*src));
		memset(dst, 0xA7, m * sizeof(*dst));
		memset(len, 0xA7, m * sizeof(*len));
		memset(kind, 0xA7, m);
		memset(meta, 0xA7, m * sizeof(*meta));
		memset(segb, 0xA7, (nseg + 1) * sizeof(*segb));
		memset(total, 0xA7, sizeof(*total));
		memset(cnt, 0, sizeof(cnt));
		memcpy(snap, frames, flen);

		struct gcl_batch b = { .frames = frames, .frames_len = flen, .stride = stride,
		                       .offs = use_offs ? offs : NULL, .pkt_len = plen, .n = n };
		struct gcl_pay_in in = { .size = sizeof(in), .align = align, .order = use_order ? order : NULL,
		                         .m = m, .sock = use_sock ? sock : NULL, .l4_status = use_st ? st : NULL,
		                         .seg_off = use_seg ? seg : NULL, .nseg = nseg,
		                         .blocks = (uint32_t)(rnd() % (GCL_PAY_MAX_BLOCKS + 1)) };
		struct gcl_pay_out out = { .src_off = src, .len = len, .dst_off = dst, .kind = kind,
		                           .meta = use_meta ? meta : NULL, .seg_bytes = use_seg ? segb : NULL,
		                           .total = total };

		CHECK(gcl_l4_payload_host(&b, &in, &out, cnt) == 0, "call failed\n");
		CHECK(!memcmp(snap, frames, flen), "a frame byte was written\n");

		const uint32_t amask = align ? align - 1 : 0;
		uint64_t census[GCL_PAYC_NR] = {0}, at = 0;
		for (uint64_t j = 0; j < m; j++) {
			const uint64_t i = use_order ? order[j] : j;
			const struct gcl_pay_meta zero = {0};

			CHECK(kind[j] <= GCL_PAY_OOR, "kind %u\n", kind[j]);
			CHECK((kind[j] == GCL_PAY_OOR) == (i >= n), "entry %llu: kind %u for packet %llu of %llu\n",
			      (unsigned long long)j, kind[j], (unsigned long long)i, (unsigned long long)n);
			CHECK(dst[j] == at && !(at & amask), "dst_off[%llu]\n", (unsigned long long)j);
			at += ((uint64_t)len[j] + amask) & ~(uint64_t)amask;
			census[GCL_PAYC_BYTES] += len[j];
			if (kind[j] == GCL_PAY_UDP || kind[j] == GCL_PAY_TCP) {
				const uint64_t raw = use_offs ? offs[i] : i * stride, o = raw < flen ? raw : flen;
				const uint64_t L = plen[i] < flen - o ? plen[i] : flen - o;
				const uint32_t hl = kind[j] == GCL_PAY_TCP ? 4u * (frames[o + 46] >> 4) : 8;

				census[kind[j] == GCL_PAY_UDP ? GCL_PAYC_UDP : GCL_PAYC_TCP]++;
				CHECK(src[j] + len[j] <= flen, "payload past frames_len\n");
				CHECK(src[j] == o + 34 + hl && src[j] + len[j] <= o + L, "payload outside its packet\n");
				CHECK(hl >= 8 && 34 + hl + len[j] == 14u + (frames[o + 16] << 8 | frames[o + 17]),
				      "len does not match tot\n");
				CHECK(!use_st || (st[i] & 0xF) != GCL_L4_BAD, "a BAD packet was kept\n");
				CHECK(!use_sock || sock[i] <= GCL_SOCK_COOKIE_MAX, "a packet without a socket was kept\n");
				if (use_meta)
					CHECK(meta[j].proto == frames[o + 23] && meta[j].proto == (kind[j] == GCL_PAY_TCP ? 6 : 17) &&
					      meta[j].rport == (frames[o + 34] << 8 | frames[o + 35]) &&
					      (kind[j] == GCL_PAY_TCP ? meta[j].tcp_flags == frames[o + 47] :
					       !meta[j].tcp_flags && !meta[j].seq && !meta[j].ack), "meta\n");
				kept++;
			} else {
				census[kind[j] == GCL_PAY_NA ? GCL_PAYC_NA : kind[j] == GCL_PAY_NOSOCK ? GCL_PAYC_NOSOCK :
				       kind[j] == GCL_PAY_BADCSUM ? GCL_PAYC_BADCSUM : GCL_PAYC_OOR]++;
				CHECK(!len[j] && !src[j], "a dropped entry has a payload\n");
				CHECK(!use_meta || !memcmp(&meta[j], &zero, sizeof(zero)), "a dropped entry has a meta\n");
				CHECK(kind[j] != GCL_PAY_BADCSUM || use_st, "BADCSUM without l4_status\n");
				CHECK(kind[j] != GCL_PAY_NOSOCK || use_sock, "NOSOCK without sock\n");
				na += kind[j] == GCL_PAY_NA;
				oor += kind[j] == GCL_PAY_OOR;
				filtered += kind[j] == GCL_PAY_NOSOCK || kind[j] == GCL_PAY_BADCSUM;
			}
		}
		CHECK(*total == at, "total\n");
		uint64_t sum = 0;
		for (int k = 0; k < GCL_PAYC_NR; k++) {
			CHECK(cnt[k] == census[k], "count %d: %llu != %llu\n", k, (unsigned long long)cnt[k],
			      (unsigned long long)census[k]);
			sum += k < GCL_PAYC_BYTES ? cnt[k] : 0;
		}
		CHECK(sum == m, "the kind counters do not sum to m\n");
		if (use_seg)
			for (uint32_t s = 0; s <= nseg; s++)
				CHECK(segb[s] == (seg[s] < m ? dst[seg[s]] : at), "seg_bytes[%u]\n", s);

		/* m == 0 writes total and seg_bytes only; the refusals write nothing */
		if (use_order) {
			memset(total, 0xA7, sizeof(*total));
			memset(kind, 0xA7, m);
			in.m = 0;
			CHECK(gcl_l4_payload_host(&b, &in, &out, cnt) == 0 && *total == 0, "m == 0\n");
			for (uint32_t s = 0; use_seg && s <= nseg; s++)
				CHECK(segb[s] == 0, "m == 0: seg_bytes\n");
			for (uint64_t j = 0; j < m; j++)
				CHECK(kind[j] == 0xA7, "m == 0 wrote kind\n");
			in.m = m;
		}
		memset(total, 0xA7, sizeof(*total));
		struct gcl_batch nb = b;
		nb.pkt_len = NULL;
		CHECK(gcl_l4_payload_host(&nb, &in, &out, NULL) == -EINVAL, "NULL pkt_len accepted\n");
		in.align = 3;
		CHECK(gcl_l4_payload_host(&b, &in, &out, NULL) == -EINVAL, "align 3 accepted\n");
		in.align = align;
		in.blocks = GCL_PAY_MAX_BLOCKS + 1;
		CHECK(gcl_l4_payload_host(&b, &in, &out, NULL) == -EINVAL, "blocks past the cap accepted\n");
		uint64_t sentinel;
		memset(&sentinel, 0xA7, sizeof(sentinel));
		CHECK(*total == sentinel, "a refused call wrote total\n");

		free(frames), free(snap), free(offs), free(plen), free(sock), free(order), free(st), free(seg);
		free(src), free(dst), free(len), free(kind), free(meta), free(segb), free(total);
	}
	printf("pay ok %llu %llu %llu %llu\n", (unsigned long long)kept, (unsigned long long)na,
	       (unsigned long long)filtered, (unsigned long long)oor);
	return 0;
}
