/*
 * tcprxf_fuzz.c - stand-alone ASan + UBSan driver of gcl_tcp_rx_full_host
 * (csrc/gcl_host.c with the rule of csrc/gcl_tcprxf.h): garbage frames,
 * offsets, lengths, cookies, connection words, rep_acks, orders and blocks
 * over heap arrays of their exact size, so that a read or write past any of
 * them traps.  About half of the rounds carry well-formed streams of in-order
 * text, new and duplicate pure ACKs and an occasional fault, so that every
 * branch of the slow rule is reached.  Usage: tcprxf_fuzz SEED ROUNDS.  Prints
 * "tcprxf ok" and the thirteen counters.
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

static void put32(uint8_t *p, uint32_t v)
{
	p[0] = v >> 24;
	p[1] = v >> 16;
	p[2] = v >> 8;
	p[3] = v;
}

int main(int argc, char **argv)
{
	const uint64_t rounds = argc > 2 ? strtoull(argv[2], NULL, 0) : 1000;
	uint64_t counts[GCL_TCPRXFC_NR] = {0};

	rs = (argc > 1 ? strtoull(argv[1], NULL, 0) : 1) * 0x9E3779B97F4A7C15ull + 1;
	for (uint64_t r = 0; r < rounds; r++) {
		const int sane = rnd() & 1;
		const uint32_t n = rnd() % 200, nconn = sane ? 1 + rnd() % 8 : rnd() % 12;
		const uint32_t stride = 16 * (4 + rnd() % 100);
		const uint64_t flen = (uint64_t)n * stride - (n && !sane ? rnd() % stride : 0);
		const int with_order = rnd() & 1, with_st = rnd() & 1, with_offs = !sane && (rnd() & 1);
		const uint64_t m = with_order ? rnd() % 300 : n;
		uint8_t *frames = exact(flen);
		uint16_t *plen = exact(2 * (size_t)n);
		uint64_t *offs = with_offs ? exact(8 * (size_t)n) : NULL;
		uint32_t *sock = exact(4 * (size_t)n);
		uint8_t *st = with_st ? exact(n) : NULL;
		uint32_t *order = with_order ? exact(4 * (size_t)m) : NULL;
		struct gcl_tcp_conn *conn = aligned_alloc(16, 48 * (size_t)(nconn ? nconn : 1));
		struct gcl_tcp_conn_out *oc = aligned_alloc(16, 48 * (size_t)(nconn ? nconn : 1));
		struct gcl_tcp_conn_ext *ext = aligned_alloc(16, 16 * (size_t)(nconn ? nconn : 1));
		uint8_t *rep = rnd() & 3 ? exact(nconn) : NULL;
		uint8_t *verdict = exact(m), *sflags = exact(m);
		uint32_t *after = exact(4 * m);
		uint16_t *clen = exact(2 * m);
		uint64_t *doff = exact(8 * m), *coff = exact(8 * ((size_t)nconn + 1));

		if (!conn || !oc || !ext)
			abort();
		for (size_t i = 0; i < 48 * (size_t)(nconn ? nconn : 1); i++)
			((uint8_t *)conn)[i] = (uint8_t)rnd();
		for (uint32_t i = 0; i < n; i++) {
			if (with_offs && (rnd() & 3))
				offs[i] = rnd() % (flen + 64);
			if (rnd() & 7)
				sock[i] = (uint32_t)(rnd() % (nconn + 2));
			if (with_order && (rnd() & 7) && i < m)
				order[i] = (uint32_t)(rnd() % (n + 2));
		}
		if (sane) { /* in-order chains with an occasional fault */
			uint32_t nxt[8];
			for (uint32_t c = 0; c < nconn; c++) {
				memset(&conn[c], 0, sizeof(conn[c]));
				conn[c].snd_una = (uint32_t)rnd();
				conn[c].snd_nxt = conn[c].snd_una + 1000;
				conn[c].snd_wnd = rnd() & 3 ? 1u << 20 : 1000; /* 1000: the send window is full */
				conn[c].rcv_nxt = nxt[c] = rnd() & 1 ? 0xFFFFFF00u : (uint32_t)rnd();
				conn[c].snd_wl1 = nxt[c] - 1;
				conn[c].rcv_wnd = rnd() & 3 ? 1u << 20 : rnd() % 3000;
				conn[c].rcv_mss = 200;
				conn[c].snd_wscale = rnd() % 15;
				conn[c].flags = GCL_TCPC_ELIGIBLE | (rnd() & 6);
				conn[c].acks_delayed_cnt = rnd() & 1;
			}
			for (uint32_t i = 0; i < n; i++) {
				uint8_t *f = frames + (uint64_t)i * stride;
				const uint32_t c = rnd() % nconn, fault = rnd() % 24;
				const uint32_t len = fault == 0 ? 201 : fault == 1 || (rnd() & 1) ? 0 : 1 + rnd() % 200;
				const uint32_t tot = 40 + len;

				plen[i] = (uint16_t)(14 + tot);
				sock[i] = fault == 2 ? nconn : c;
				f[12] = 0x08; f[13] = 0x00; f[14] = 0x45;
				f[16] = tot >> 8; f[17] = tot;
				f[20] = 0x40; f[21] = 0;
				f[23] = fault == 3 ? 17 : 6;
				put32(f + 38, nxt[c] + (fault == 4));
				put32(f + 42, conn[c].snd_una + (fault == 5 ? 2000 : rnd() & 1 ? 0 : rnd() % 500));
				f[46] = 0x50;
				f[48] = rnd() & 1 ? 0 : 0xFF; /* a window of 0 is never taken over a larger one: duplicates */
				f[49] = 0;
				f[47] = 0x10 | (fault == 6 ? 0x01 : 0) | (rnd() & 8);
				if (st)
					st[i] = fault == 7 ? GCL_L4_BAD : GCL_L4_GOOD;
				if (fault > 7 || fault == 6 || fault == 5 || fault == 4)
					nxt[c] += fault > 7 && sock[i] == c ? len : 0;
			}
		}
		const struct gcl_batch b = {.frames = frames, .frames_len = flen, .stride = stride, .offs = offs,
		                            .pkt_len = plen, .n = n};
		const struct gcl_tcprxf_in in = {.size = sizeof(in), .align = 1u << (rnd() % 9) >> 1, .order = order,
		                                 .m = m, .sock = sock, .l4_status = st, .conn = conn, .nconn = nconn,
		                                 .blocks = rnd() % (GCL_TCPRX_MAX_BLOCKS + 1), .rep_acks = rep};
		const struct gcl_tcprx_out out = {verdict, sflags, after, clen, doff, oc, coff};
		uint64_t c[GCL_TCPRXFC_NR] = {0};
		const int rc = gcl_tcp_rx_full_host(&b, &in, &out, ext, c);

		if (rc != 0) {
			printf("tcprxf round %llu: %d\n", (unsigned long long)r, rc);
			return 1;
		}
		if (c[0] + c[1] + c[2] + c[3] + c[4] != m) {
			printf("tcprxf round %llu: the verdict counts do not sum to m\n", (unsigned long long)r);
			return 1;
		}
		for (uint64_t j = 0; j < m; j++)
			if ((clen[j] && verdict[j] != GCL_TCPRX_FAST) || ((sflags[j] & GCL_TCPRX_SF_DROPPED) && clen[j]) ||
			    (clen[j] && doff[j] + clen[j] > coff[nconn])) {
				printf("tcprxf round %llu: entry %llu lies outside the layout\n", (unsigned long long)r,
				       (unsigned long long)j);
				return 1;
			}
		for (int k = 0; k < GCL_TCPRXFC_NR; k++)
			counts[k] += c[k];
		free(frames); free(plen); free(offs); free(sock); free(st); free(order); free(conn); free(oc); free(ext); free(rep);
		free(verdict); free(sflags); free(after); free(clen); free(doff); free(coff);
	}
	printf("tcprxf ok");
	for (int k = 0; k < GCL_TCPRXFC_NR; k++)
		printf(" %llu", (unsigned long long)counts[k]);
	printf("\n");
	return 0;
}
