/*
 * tcptmr_fuzz.c - stand-alone ASan + UBSan driver of gcl_tcp_tick_host and
 * gcl_tcp_rx_acks_host (csrc/gcl_host.c with the rules of csrc/gcl_tcptmr.h):
 * hostile timer words, connection words, addresses, orders, cookies, verdicts
 * and caps over heap arrays of their exact size, so that a read or write past
 * any of them traps.  About half of the sweeps keep their timestamps near the
 * clock reading, so that every action bit is reached.  Usage: tcptmr_fuzz SEED
 * ROUNDS.  Prints "tcptmr ok" and the counts of FIRED ACK PROBE RETRANSMIT FAIL
 * CLOSE NOSPACE SEGS, then of the ACKs WANTED WRITTEN SKIPPED, then how often
 * each of the two guards (i >= n, cookie >= nconn) did the skipping.
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
	const size_t sz = (bytes + 15) & ~(size_t)15;
	void *p = aligned_alloc(16, sz ? sz : 16);

	if (!p)
		abort();
	for (size_t i = 0; i < bytes; i++)
		((uint8_t *)p)[i] = (uint8_t)rnd();
	return p;
}

struct segs {
	struct gcl_ctlseg_out o;
	uint64_t cap;
};

/* per-segment arrays of exactly @cap elements (desc: a multiple of 16 B anyway) */
static struct segs segs_new(uint64_t cap)
{
	struct segs s;

	s.cap = cap;
	s.o.desc = exact16(32 * cap);
	s.o.frame_off = exact(8 * cap);
	s.o.seg_conn = exact(4 * cap);
	s.o.seg_kind = exact(cap);
	s.o.seg_src = exact(4 * cap);
	s.o.totals = exact(16);
	return s;
}

static void segs_free(struct segs *s)
{
	free(s->o.desc); free(s->o.frame_off); free(s->o.seg_conn); free(s->o.seg_kind); free(s->o.seg_src);
	free(s->o.totals);
}

/* what every call must leave behind, whatever the input */
static int segs_check(const struct segs *s, uint64_t base, uint32_t stride, uint32_t nconn, const char *what,
                      uint64_t round)
{
	const uint64_t wanted = s->o.totals[0], written = s->o.totals[1];

	if (written != (wanted < s->cap ? wanted : s->cap)) {
		printf("%s round %llu: totals %llu %llu with cap %llu\n", what, (unsigned long long)round,
		       (unsigned long long)wanted, (unsigned long long)written, (unsigned long long)s->cap);
		return 1;
	}
	for (uint64_t k = 0; k < written; k++) {
		const struct gcl_txh_desc *d = &s->o.desc[k];

		if (d->proto != 6 || d->tcp_flags != 0x10 || d->tcp_off != 5 || d->ecn || d->paylen || d->pad ||
		    s->o.frame_off[k] != base + k * stride || s->o.seg_conn[k] >= nconn || s->o.seg_kind[k] > GCL_CTL_PROBE ||
		    (k && s->o.seg_src[k] < s->o.seg_src[k - 1])) {
			printf("%s round %llu: segment %llu is malformed\n", what, (unsigned long long)round,
			       (unsigned long long)k);
			return 1;
		}
	}
	return 0;
}

int main(int argc, char **argv)
{
	const uint64_t rounds = argc > 2 ? strtoull(argv[2], NULL, 0) : 1000;
	uint64_t tick[GCL_TICKC_NR] = {0}, acks[GCL_TICKC_NR] = {0}, guard[2] = {0, 0};

	rs = (argc > 1 ? strtoull(argv[1], NULL, 0) : 1) * 0x9E3779B97F4A7C15ull + 1;
	for (uint64_t r = 0; r < rounds; r++) {
		const int sane = rnd() & 1;
		const uint32_t nconn = rnd() % 300;
		const uint32_t stride = GCL_CTL_MIN_STRIDE + rnd() % 2000;
		const uint64_t base = rnd() & 3 ? rnd() % (1ull << 40) : rnd();
		const uint64_t now = sane ? 1ull << 40 : rnd();
		struct gcl_tcp_tmr *tmr = exact16(64 * (size_t)nconn);
		struct gcl_tcp_conn *conn = exact16(48 * (size_t)nconn);
		struct gcl_tcp_addr *addr = exact16(16 * (size_t)nconn);
		struct gcl_tcp_tmr_out *ot = exact16(32 * (size_t)nconn);
		struct segs s = segs_new(rnd() & 1 ? rnd() % (2 * nconn + 2) : 2 * (uint64_t)nconn);

		if (sane) {
			static const uint64_t T[] = {10000, 5000000, 1000000, 300000};
			for (uint32_t c = 0; c < nconn; c++) {
				uint64_t *w = &tmr[c].next_timeout;
				for (int x = 0; x < 6; x++)
					w[x] = now - T[rnd() & 3] + rnd() % 5 - 2;
				tmr[c].next_timeout = now - rnd() % 3 + (rnd() & 3 ? 0 : 2);
				tmr[c].state = rnd() % 10;
				tmr[c].flags = (uint8_t)(rnd() | (rnd() & 7 ? GCL_TMR_LIVE : 0));
			}
		}
		const struct gcl_tick_in in = {.size = sizeof(in), .blocks = rnd() % (GCL_TICK_MAX_BLOCKS + 1), .now = now,
		                               .tmr = tmr, .conn = conn, .addr = addr, .nconn = nconn,
		                               .frame_stride = stride, .seg_cap = s.cap, .frame_base = base};
		const struct gcl_tick_out out = {ot, s.o};
		uint64_t c[GCL_TICKC_NR] = {0};
		int rc = gcl_tcp_tick_host(&in, &out, c);

		if (rc != 0) {
			printf("tick round %llu: %d\n", (unsigned long long)r, rc);
			return 1;
		}
		if (segs_check(&s, base, stride, nconn, "tick", r))
			return 1;
		if (c[GCL_TICKC_SEGS] != s.o.totals[1] || c[GCL_TICKC_ACK] + c[GCL_TICKC_PROBE] != s.o.totals[0] ||
		    (c[GCL_TICKC_NOSPACE] != 0) != (s.o.totals[0] > s.cap)) {
			printf("tick round %llu: the counters do not agree with totals\n", (unsigned long long)r);
			return 1;
		}
		for (uint32_t k = 0; k < nconn; k++) {
			const uint8_t a = ot[k].action;
			if ((a & ~GCL_TMRA_FIRED) && !(a & GCL_TMRA_FIRED)) {
				printf("tick round %llu: connection %u acted without firing\n", (unsigned long long)r, k);
				return 1;
			}
		}
		for (int k = 0; k < GCL_TICKC_NR; k++)
			tick[k] += c[k];
		segs_free(&s);
		free(tmr);
		free(ot);

		/* the ACKs of a list: verdicts that often ask, orders and cookies that often point outside */
		const uint32_t n = rnd() % 200;
		const int with_order = rnd() & 1;
		const uint64_t m = with_order ? rnd() % 300 : n;
		uint32_t *sock = exact(4 * (size_t)n), *order = with_order ? exact(4 * (size_t)m) : NULL;
		uint8_t *verdict = exact(m), *sflags = exact(m);
		uint32_t *after = exact(4 * (size_t)m);
		struct segs a = segs_new(rnd() & 1 ? rnd() % (m + 2) : m);

		for (uint32_t i = 0; i < n; i++)
			if (rnd() & 7)
				sock[i] = (uint32_t)(rnd() % (nconn + 2));
		for (uint64_t j = 0; j < m; j++) {
			if (with_order && (rnd() & 7))
				order[j] = (uint32_t)(rnd() % (n + 2));
			if (rnd() & 3)
				verdict[j] = rnd() % 5;
		}
		const struct gcl_rxack_in rin = {.size = sizeof(rin), .blocks = rnd() % (GCL_TICK_MAX_BLOCKS + 1),
		                                 .order = order, .m = m, .n = n, .sock = sock, .verdict = verdict,
		                                 .sflags = sflags, .rcv_nxt_after = after, .conn = conn, .addr = addr,
		                                 .nconn = nconn, .frame_stride = stride, .seg_cap = a.cap,
		                                 .frame_base = base};
		uint64_t ca[GCL_TICKC_NR] = {0};

		rc = gcl_tcp_rx_acks_host(&rin, &a.o, ca);
		if (rc != 0) {
			printf("acks round %llu: %d\n", (unsigned long long)r, rc);
			return 1;
		}
		if (segs_check(&a, base, stride, nconn, "acks", r))
			return 1;
		if (ca[GCL_RXACKC_WANTED] != a.o.totals[0] || ca[GCL_RXACKC_WRITTEN] != a.o.totals[1] ||
		    ca[GCL_RXACKC_WANTED] + ca[GCL_RXACKC_SKIPPED] > m) {
			printf("acks round %llu: the counters do not agree with totals\n", (unsigned long long)r);
			return 1;
		}
		uint64_t gd[2] = {0, 0};
		for (uint64_t j = 0; j < m; j++) {
			if (verdict[j] != GCL_TCPRX_FAST || !(sflags[j] & GCL_TCPRX_SF_ACK_NOW))
				continue;
			const uint64_t i = order ? order[j] : j;
			if (i >= n)
				gd[0]++;
			else if (sock[i] >= nconn)
				gd[1]++;
		}
		if (gd[0] + gd[1] != ca[GCL_RXACKC_SKIPPED]) {
			printf("acks round %llu: SKIPPED is not what the guards skip\n", (unsigned long long)r);
			return 1;
		}
		guard[0] += gd[0];
		guard[1] += gd[1];
		for (int k = 0; k < GCL_TICKC_NR; k++)
			acks[k] += ca[k];
		segs_free(&a);
		free(conn); free(addr); free(sock); free(order); free(verdict); free(sflags); free(after);
	}
	printf("tcptmr ok");
	for (int k = 0; k < GCL_TICKC_NR; k++)
		printf(" %llu", (unsigned long long)tick[k]);
	printf(" %llu %llu %llu %llu %llu\n", (unsigned long long)acks[GCL_RXACKC_WANTED],
	       (unsigned long long)acks[GCL_RXACKC_WRITTEN], (unsigned long long)acks[GCL_RXACKC_SKIPPED],
	       (unsigned long long)guard[0], (unsigned long long)guard[1]);
	return 0;
}
