/*
 * tcpopen_fuzz.c - stand-alone ASan + UBSan driver of gcl_tcp_rx_open_host
 * (csrc/gcl_host.c with the rule and the option walk of csrc/gcl_tcpopen.h):
 * random and half-sane frames (SYNs with random option bytes, every flag, bad
 * lengths and offsets, truncated frames, frames cut by frames_len), random
 * cookies, orders, listeners, backlogs, open_cap, seg_cap, tx_frames_len and
 * hash_slots over heap arrays of their exact size, so that a read or write past
 * any of them traps.  Usage: tcpopen_fuzz SEED ROUNDS.  Prints "tcpopen ok",
 * the sixteen counters, ":" and the SYN|ACKs written with the WSCALE word and
 * with the MSS word.
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

/* a half-sane TCP frame of at most @room bytes at @f; returns its length */
static uint32_t make_frame(uint8_t *f, uint32_t room, uint32_t ntup)
{
	static const uint8_t flagset[] = {0x02, 0x02, 0x02, 0x02, 0x10, 0x04, 0x12, 0x00, 0x01, 0x14, 0x03};
	uint8_t h[14 + 20 + 60 + 16] = {0};
	const uint32_t optw = rnd() % 4 ? rnd() % 3 : rnd() % 11, pay = rnd() % 8 ? 0 : 1 + rnd() % 16;
	uint32_t off = 5 + optw, tot = 20 + 4 * off + pay, len;
	const uint32_t t = rnd() % ntup;

	h[12] = 0x08;
	h[14] = 0x45;
	h[23] = 6;
	h[26] = 10; h[29] = (uint8_t)(t >> 8);               /* saddr */
	h[30] = 10; h[33] = 1;                               /* daddr */
	h[34] = 0x80; h[35] = (uint8_t)t;                    /* sport */
	h[37] = 80;                                          /* dport */
	for (int x = 38; x < 46; x++)
		h[x] = (uint8_t)rnd();
	h[47] = rnd() % 6 ? flagset[rnd() % sizeof(flagset)] : (uint8_t)rnd();
	for (uint32_t x = 0; x < 4 * optw; x++) {            /* option bytes: mostly meaningful kinds and lengths */
		static const uint8_t ob[] = {0, 1, 1, 1, 2, 3, 4, 3, 3, 8, 10, 2, 0x05, 0xB4, 7, 15, 200, 1};
		h[54 + x] = rnd() % 8 ? ob[rnd() % sizeof(ob)] : (uint8_t)rnd();
	}
	if (rnd() % 3 == 0 && optw) {                        /* a well-formed pair of options */
		static const uint8_t good[8] = {2, 4, 0x02, 0x18, 1, 3, 3, 9};
		memcpy(h + 54, good, optw >= 2 ? 8 : 4);
	}
	if (rnd() % 10 == 0)
		off = rnd() % 16;
	if (rnd() % 10 == 0)
		tot = 18 + rnd() % 80;
	h[46] = (uint8_t)(off << 4);
	h[16] = (uint8_t)(tot >> 8);
	h[17] = (uint8_t)tot;
	if (rnd() % 16 == 0)
		h[12 + rnd() % 12] ^= (uint8_t)(1u << (rnd() % 8)); /* ethertype, version, fragment, protocol ... */
	len = 14 + 20 + 4 * (5 + optw) + pay;
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
	uint64_t counts[GCL_OPENC_NR] = {0}, words[2] = {0};

	rs = (argc > 1 ? strtoull(argv[1], NULL, 0) : 1) * 0x9E3779B97F4A7C15ull + 1;
	for (uint64_t r = 0; r < rounds; r++) {
		const int sane = rnd() % 4 != 0;
		const uint32_t n = rnd() % 200, nlisten = rnd() % 6 == 0 ? 0 : 1 + rnd() % 5;
		const uint32_t stride = 16 * (7 + rnd() % 4);
		const uint64_t flen = (uint64_t)n * stride - (n && !sane ? rnd() % stride : 0);
		const int with_order = rnd() & 1, with_st = rnd() & 1, with_offs = !sane && (rnd() & 1);
		const uint64_t m = with_order ? rnd() % 300 : n;
		const uint64_t seg_cap = rnd() % 4 ? m : rnd() % (m + 1), open_cap = rnd() % 4 ? m : rnd() % (m + 1);
		const uint32_t fstride = 62 + rnd() % 40, base = 1000;
		const uint64_t fbase = rnd() % 200;
		const uint64_t txlen = rnd() % 4 ? fbase + seg_cap * fstride : rnd() % (fbase + seg_cap * fstride + 1);
		uint32_t slots = 0;
		uint8_t *frames = exact(flen), *tx = exact(txlen);
		uint16_t *plen = exact(2 * (size_t)n);
		uint64_t *offs = with_offs ? exact(8 * (size_t)n) : NULL;
		uint32_t *sock = exact(4 * (size_t)n), *order = with_order ? exact(4 * (size_t)m) : NULL;
		uint8_t *st = with_st ? exact(n) : NULL;
		uint32_t *iss = exact(4 * (size_t)m);
		struct gcl_tcp_listen *listen = exact16(16 * (size_t)nlisten);
		uint8_t *verdict = exact(m);
		uint32_t *later_of = exact(4 * (size_t)m), *rst_seq = exact(4 * (size_t)m);
		uint32_t *backlog_out = exact(4 * (size_t)nlisten);
		struct gcl_tcp_open *open = exact16(64 * (size_t)open_cap);
		struct gcl_txh_desc *desc = exact16(32 * (size_t)seg_cap);
		uint64_t *frame_off = exact(8 * (size_t)seg_cap), ototals[2], stotals[2];
		uint32_t *seg_conn = exact(4 * (size_t)seg_cap), *seg_src = exact(4 * (size_t)seg_cap);
		uint8_t *seg_kind = exact(seg_cap);

		if (rnd() & 1)
			for (slots = 2; slots < 2 * m; slots <<= 1)
				;
		for (uint32_t i = 0; i < n; i++) {
			const uint64_t o = (uint64_t)i * stride;
			plen[i] = sane || rnd() % 4 ? 0 : (uint16_t)rnd();
			if (o < flen && (sane || rnd() % 4))
				plen[i] = (uint16_t)make_frame(frames + o, (uint32_t)(flen - o < stride ? flen - o : stride), 1 + n / 3);
			if (!sane && rnd() % 8 == 0)
				plen[i] = (uint16_t)rnd();
			sock[i] = rnd() % 10 < 6 ? base + rnd() % (nlisten + 1) : rnd() % 10 < 8 ? GCL_SOCK_MISS :
			          rnd() % 2 ? (uint32_t)rnd() : GCL_SOCK_MULTI + rnd() % 3;
			if (offs)
				offs[i] = rnd() % 4 ? o + rnd() % 3 : rnd();
			if (st)
				st[i] = rnd() % 8 ? GCL_L4_GOOD : (uint8_t)rnd();
		}
		for (uint64_t j = 0; order && j < m; j++)
			order[j] = rnd() % 16 ? (uint32_t)(rnd() % (n + 1)) : (uint32_t)rnd();
		for (uint32_t l = 0; l < nlisten; l++) {
			listen[l].backlog = rnd() % 3 ? rnd() % 20 : rnd() % 3 ? 0 : (uint32_t)rnd();
			listen[l].flags = rnd() % 8 ? 0 : (uint8_t)rnd();
		}
		const struct gcl_batch b = {.frames = frames, .frames_len = flen, .stride = offs ? 0 : stride, .offs = offs,
		                            .pkt_len = plen, .n = n};
		const struct gcl_tcpopen_in in = {.size = sizeof(in), .blocks = (uint32_t)(rnd() % 5), .order = order, .m = m,
		                                  .sock = sock, .l4_status = st, .hash_slots = slots, .listen_base = base,
		                                  .nlisten = nlisten, .frame_stride = fstride, .listen = listen, .iss = iss,
		                                  .seg_cap = seg_cap, .frame_base = fbase, .open_cap = open_cap,
		                                  .tx_frames = tx, .tx_frames_len = txlen};
		const struct gcl_tcpopen_out out = {verdict, later_of, rst_seq, open, backlog_out, ototals};
		const struct gcl_ctlseg_out seg = {desc, frame_off, seg_conn, seg_kind, seg_src, stotals};
		const int ret = gcl_tcp_rx_open_host(&b, &in, &out, &seg, counts);

		if (ret) {
			printf("tcpopen refused round %llu: %d\n", (unsigned long long)r, ret);
			return 1;
		}
		for (uint64_t k = 0; m && k < stotals[1]; k++)
			if (seg_kind[k] == GCL_CTL_SYNACK) {
				const uint8_t *o = tx + frame_off[k] + 54;
				if (desc[k].tcp_off > 5 && o[0] == 1)
					words[0]++;
				if (desc[k].tcp_off > 5 && o[4 * (desc[k].tcp_off - 6)] == 2)
					words[1]++;
				if (seg_conn[k] < ototals[1] && open[seg_conn[k]].src != seg_src[k])
					abort();
			}
		free(frames); free(tx); free(plen); free(offs); free(sock); free(order); free(st); free(iss);
		free(listen); free(verdict); free(later_of); free(rst_seq); free(backlog_out); free(open); free(desc);
		free(frame_off); free(seg_conn); free(seg_src); free(seg_kind);
	}
	printf("tcpopen ok");
	for (int k = 0; k < GCL_OPENC_NR; k++)
		printf(" %llu", (unsigned long long)counts[k]);
	printf(" : %llu %llu\n", (unsigned long long)words[0], (unsigned long long)words[1]);
	return 0;
}
