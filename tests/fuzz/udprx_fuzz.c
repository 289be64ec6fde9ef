/*
 * udprx_fuzz.c - stand-alone ASan + UBSan driver of gcl_udp_rx_host
 * (csrc/gcl_host.c with the rule of csrc/gcl_udprx.h): random and half-sane
 * frames (UDP datagrams of every length, TCP, bad lengths, truncated frames,
 * frames cut by frames_len), random cookies, orders, socket words, caps, flags,
 * sock_base and align over heap arrays of their exact size, so that a read or
 * write past any of them traps.  It also checks what must hold whatever the
 * bytes: the records and offsets name each other, and the per-socket counts
 * add up.  Usage: udprx_fuzz SEED ROUNDS.  Prints "udprx ok" and the eight
 * counters.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"
#include "../../include/gclassify.h"

static uint64_t rs;

static uint64_t rnd(void)
{
	rs ^= rs << 13;
	rs ^= rs >> 7;
	rs ^= rs << 17;
	return rs;
}

static void *exact(size_t bytes)
{
	void *p = malloc(bytes ? bytes : 1);

	if (!p)
		abort();
	for (size_t i = 0; i < bytes; i++)
		((uint8_t *)p)[i] = (uint8_t)rnd();
	return p;
}

static void *exact16(size_t bytes)
{
	void *p = aligned_alloc(16, bytes ? (bytes + 15) & ~(size_t)15 : 16);

	if (!p)
		abort();
	for (size_t i = 0; i < bytes; i++)
		((uint8_t *)p)[i] = (uint8_t)rnd();
	return p;
}

/* a half-sane frame of at most @room bytes at @f; returns its length */
static uint32_t make_frame(uint8_t *f, uint32_t room)
{
	uint8_t h[14 + 20 + 8 + 64] = {0};
	const uint32_t pay = rnd() % 6 ? rnd() % 64 : 0;
	uint32_t tot = 28 + pay, len = 14 + tot;

	h[12] = 0x08;
	h[14] = 0x45;
	h[23] = rnd() % 10 ? 17 : 6;
	for (int x = 26; x < 38; x++)
		h[x] = (uint8_t)rnd();
	h[46] = 0x50;
	if (rnd() % 10 == 0)
		tot = 18 + rnd() % 90;
	h[16] = (uint8_t)(tot >> 8);
	h[17] = (uint8_t)tot;
	if (rnd() % 16 == 0)
		h[12 + rnd() % 12] ^= (uint8_t)(1u << (rnd() % 8)); /* ethertype, version, fragment, protocol ... */
	if (rnd() % 12 == 0)
		len = rnd() % (len + 1);
	if (len > room)
		len = room;
	memcpy(f, h, len);
	return len;
}

int main(int argc, char **argv)
{
	const uint64_t rounds = argc > 2 ? strtoull(argv[2], NULL, 0) : 1000;
	uint64_t counts[GCL_UDPRXC_NR] = {0};

	rs = (argc > 1 ? strtoull(argv[1], NULL, 0) : 1) * 0x9E3779B97F4A7C15ull + 1;
	for (uint64_t r = 0; r < rounds; r++) {
		const int sane = rnd() % 4 != 0;
		const uint32_t n = rnd() % 200, nsock = rnd() % 6 == 0 ? 0 : 1 + rnd() % 9;
		const uint32_t stride = 16 * (7 + rnd() % 4);
		const uint64_t flen = (uint64_t)n * stride - (n && !sane ? rnd() % stride : 0);
		const int with_order = rnd() & 1, with_st = rnd() & 1, with_offs = !sane && (rnd() & 1);
		const uint64_t m = with_order ? rnd() % 300 : n;
		const uint32_t base = rnd() % 4 ? 1000 : rnd() % 2 ? 0 : 0xFFFFFFE0u;
		static const uint32_t aligns[] = {0, 1, 2, 16, 64, 256};
		uint8_t *frames = exact(flen);
		uint16_t *plen = exact(2 * (size_t)n);
		uint64_t *offs = with_offs ? exact(8 * (size_t)n) : NULL;
		uint32_t *sock = exact(4 * (size_t)n), *order = with_order ? exact(4 * (size_t)m) : NULL;
		uint8_t *st = with_st ? exact(n) : NULL;
		struct gcl_udp_sock *us = exact16(16 * (size_t)nsock);
		uint8_t *verdict = exact(m), *sflags = exact(m);
		uint16_t *copy_len = exact(2 * (size_t)m);
		uint64_t *dst_off = exact(8 * (size_t)m), *sock_off = exact(8 * ((size_t)nsock + 1));
		uint32_t *rec_idx = exact(4 * (size_t)m), *rec_off = exact(4 * ((size_t)nsock + 1));
		struct gcl_udp_rec *rec = exact16(16 * (size_t)m);
		struct gcl_udp_sock_out *os = exact16(16 * (size_t)nsock);
		uint64_t before[GCL_UDPRXC_NR], taken = 0, dropped = 0;

		for (uint32_t i = 0; i < n; i++) {
			const uint64_t o = (uint64_t)i * stride;
			plen[i] = sane || rnd() % 4 ? 0 : (uint16_t)rnd();
			if (o < flen && (sane || rnd() % 4))
				plen[i] = (uint16_t)make_frame(frames + o, (uint32_t)(flen - o < stride ? flen - o : stride));
			if (!sane && rnd() % 8 == 0)
				plen[i] = (uint16_t)rnd();
			sock[i] = rnd() % 10 < 8 ? base + rnd() % (nsock + 1) : rnd() % 2 ? (uint32_t)rnd() :
			          GCL_SOCK_MULTI + rnd() % 3;
			if (offs)
				offs[i] = rnd() % 4 ? o + rnd() % 3 : rnd();
			if (st)
				st[i] = rnd() % 8 ? GCL_L4_GOOD : (uint8_t)rnd();
		}
		for (uint64_t j = 0; order && j < m; j++)
			order[j] = rnd() % 16 ? (uint32_t)(rnd() % (n + 1)) : (uint32_t)rnd();
		for (uint32_t s = 0; s < nsock; s++) {
			const int32_t ln = rnd() % 4 ? (int32_t)(rnd() % 5) - 1 : (int32_t)rnd();
			us[s].inq_len = ln;
			us[s].inq_cap = rnd() % 6 ? (int32_t)((int64_t)ln + (int64_t)(rnd() % 40) > INT32_MAX ? INT32_MAX :
			                                      (int64_t)ln + (int64_t)(rnd() % 40)) : (int32_t)rnd();
			us[s].flags = rnd() % 3 ? 0 : rnd() % 4 ? (uint8_t)(1u << (rnd() % 3)) : (uint8_t)rnd();
		}
		const struct gcl_batch b = {.frames = frames, .frames_len = flen, .stride = offs ? 0 : stride, .offs = offs,
		                            .pkt_len = plen, .n = n};
		const struct gcl_udprx_in in = {.size = sizeof(in), .align = aligns[rnd() % 6], .order = order, .m = m,
		                                .sock = sock, .l4_status = st, .usock = us, .nsock = nsock,
		                                .sock_base = base, .blocks = (uint32_t)(rnd() % 5)};
		const struct gcl_udprx_out out = {verdict, sflags, copy_len, dst_off, rec_idx, rec, os, rec_off, sock_off};

		memcpy(before, counts, sizeof(before));
		const int ret = gcl_udp_rx_host(&b, &in, &out, counts);

		if (ret) {
			printf("udprx refused round %llu: %d\n", (unsigned long long)r, ret);
			return 1;
		}
		/* a taken entry's record is its own, inside its socket's range, and repeats its offset and length */
		for (uint64_t j = 0; j < m; j++) {
			const int tk = verdict[j] == GCL_UDPRX_QUEUED || verdict[j] == GCL_UDPRX_SPAWN;

			if (tk != (rec_idx[j] != 0xFFFFFFFFu))
				abort();
			if (tk && (rec_idx[j] >= rec_off[nsock] || rec[rec_idx[j]].dst_off != dst_off[j] ||
			           rec[rec_idx[j]].len != copy_len[j] || dst_off[j] + copy_len[j] > sock_off[nsock]))
				abort();
			if (!tk && (copy_len[j] || dst_off[j]))
				abort();
		}
		for (uint32_t s = 0; s < nsock; s++) {
			if (rec_off[s + 1] - rec_off[s] != os[s].ntaken || sock_off[s + 1] < sock_off[s])
				abort();
			taken += os[s].ntaken;
			dropped += os[s].ndropped;
		}
		if (taken != counts[GCL_UDPRX_QUEUED] - before[GCL_UDPRX_QUEUED] + counts[GCL_UDPRX_SPAWN] -
		                     before[GCL_UDPRX_SPAWN] ||
		    dropped != counts[GCL_UDPRX_FULL] - before[GCL_UDPRX_FULL] + counts[GCL_UDPRX_CLOSED] -
		                       before[GCL_UDPRX_CLOSED] ||
		    rec_off[nsock] != taken)
			abort();
		free(frames); free(plen); free(offs); free(sock); free(order); free(st); free(us); free(verdict);
		free(sflags); free(copy_len); free(dst_off); free(sock_off); free(rec_idx); free(rec_off); free(rec); free(os);
	}
	printf("udprx ok");
	for (int k = 0; k < GCL_UDPRXC_NR; k++)
		printf(" %llu", (unsigned long long)counts[k]);
	printf("\n");
	return 0;
}
