/*
 * txq_fuzz.c - stand-alone ASan + UBSan driver of gcl_tcp_txq_host
 * (csrc/gcl_host.c with the rule of csrc/gcl_txq.h): garbage queue offsets,
 * entries, connection words, wants and caps over heap arrays of their exact
 * size, so that a read or write past any of them traps.  About half of the
 * rounds keep an orderly CSR, sequence numbers around snd_una and timestamps
 * near the clock reading, so that every branch of the rule is reached.  Usage:
 * txq_fuzz SEED ROUNDS.  Prints "txq ok" and the counts of ACKED RETX COPIED
 * TRIMMED REFUSED NOSPACE DEFERRED BYTES, then of the connections flagged EMPTY
 * BATCH BADRANGE and of the entries left NOSPACE.
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

#define FAIL(...) do { printf(__VA_ARGS__); return 1; } while (0)

int main(int argc, char **argv)
{
	const uint64_t rounds = argc > 2 ? strtoull(argv[2], NULL, 0) : 1000;
	uint64_t sum[GCL_TXQC_NR] = {0}, flagged[3] = {0, 0, 0}, nospace_ent = 0;

	rs = (argc > 1 ? strtoull(argv[1], NULL, 0) : 1) * 0x9E3779B97F4A7C15ull + 1;
	for (uint64_t r = 0; r < rounds; r++) {
		const int sane = rnd() & 1;
		const uint32_t nconn = rnd() & 3 ? rnd() % 200 : rnd() % 6; /* a few connections: long queues */
		const uint64_t nent = rnd() % 600;
		const uint32_t stride = GCL_CTL_MIN_STRIDE + rnd() % 2000;
		const uint64_t base = rnd() & 3 ? rnd() % (1ull << 40) : rnd();
		const uint64_t now = sane ? 1ull << 40 : rnd();
		const uint64_t cap = rnd() & 1 ? rnd() % (nent + 2) : 17 * (uint64_t)nconn;
		uint32_t *qoff = exact(4 * ((size_t)nconn + 1));
		struct gcl_txq_ent *ent = exact16(16 * nent);
		struct gcl_txq_cold *cold = exact16(16 * nent);
		struct gcl_tcp_conn *conn = exact16(48 * (size_t)nconn);
		struct gcl_tcp_addr *addr = exact16(16 * (size_t)nconn);
		uint8_t *want = rnd() & 7 ? exact(nconn) : NULL;
		struct gcl_txq_out o = {.out_conn = exact16(32 * (size_t)nconn), .state = exact(nent),
		                        .desc = exact16(32 * cap), .frame_off = exact(8 * cap), .src_off = exact(8 * cap),
		                        .len = exact(2 * cap), .dst_off = exact(8 * cap), .seg_conn = exact(4 * cap),
		                        .seg_ent = exact(4 * cap), .totals = exact(24)};

		if (sane) {
			/* an orderly CSR (now and then one garbage offset), queues that start a little before snd_una */
			uint64_t at = 0;
			for (uint32_t c = 0; c <= nconn; c++) {
				qoff[c] = (uint32_t)at;
				if (c < nconn)
					at += (nent - at) * (rnd() % 4) / (2 * (nconn - c) + 1) + (at < nent && !(rnd() & 3));
				if (at > nent)
					at = nent;
			}
			if (nconn)
				qoff[nconn] = (uint32_t)nent;
			if (!(rnd() & 3))
				qoff[rnd() % (nconn + 1)] = (uint32_t)rnd();
			for (uint32_t c = 0; c < nconn; c++) {
				const uint32_t lo = qoff[c], hi = qoff[c + 1];
				uint32_t seq = conn[c].snd_una - (uint32_t)(rnd() % 300);
				uint64_t ts = now - 300000 - 400 + rnd() % 420;

				if (want)
					want[c] = rnd() & 7 ? (uint8_t)(rnd() & 3) : (uint8_t)rnd();
				if (lo > hi || hi > nent)
					continue;
				for (uint32_t e = lo; e < hi; e++) {
					const uint32_t ln = rnd() & 7 ? (uint32_t)(rnd() % 1500) : (uint32_t)rnd();
					ent[e].seg_seq = seq;
					ent[e].seg_end = seq + ln;
					ent[e].ts = rnd() & 15 ? ts : rnd();
					cold[e].tcp_off = rnd() & 7 ? 5 : (uint8_t)(rnd() % 18);
					cold[e].tcp_flags = rnd() & 3 ? 0x10 : (uint8_t)rnd();
					cold[e].flags = (uint8_t)(rnd() & 3 ? 0 : rnd());
					seq += ln;
					ts += rnd() % 3;
				}
			}
		}
		const struct gcl_txq_in in = {.size = sizeof(in), .blocks = rnd() % (GCL_TXQ_MAX_BLOCKS + 1), .now = now,
		                              .qoff = qoff, .ent = ent, .cold = cold, .nent = nent, .conn = conn,
		                              .addr = addr, .want = want, .nconn = nconn, .frame_stride = stride,
		                              .seg_cap = cap, .frame_base = base};
		uint64_t c[GCL_TXQC_NR] = {0};
		const int rc = gcl_tcp_txq_host(&in, &o, c);

		if (rc != 0)
			FAIL("round %llu: %d\n", (unsigned long long)r, rc);
		/* what every call must leave behind, whatever the input */
		const uint64_t wanted = o.totals[0], written = o.totals[1];
		uint64_t bytes = 0, nretx = 0, nacked = 0;

		if (written != (wanted < cap ? wanted : cap) || c[GCL_TXQC_RETX] != written || o.totals[2] != c[GCL_TXQC_BYTES])
			FAIL("round %llu: totals %llu %llu with cap %llu\n", (unsigned long long)r, (unsigned long long)wanted,
			     (unsigned long long)written, (unsigned long long)cap);
		for (uint64_t k = 0; k < written; k++) {
			const struct gcl_txh_desc *d = &o.desc[k];
			const uint32_t e = o.seg_ent[k], cn = o.seg_conn[k];
			const int copy = o.len[k] != 0 || o.frame_off[k] == base + k * stride;

			if (d->proto != 6 || d->ecn || d->pad || d->tcp_off < 5 || d->tcp_off > 15 || cn >= nconn || e >= nent ||
			    (k && cn < o.seg_conn[k - 1]) || o.dst_off[k] != o.frame_off[k] + 54 ||
			    (copy && (uint32_t)54 + o.len[k] > stride) || d->tcp_off != cold[e].tcp_off ||
			    (o.len[k] && o.len[k] != 4 * (d->tcp_off - 5) + d->paylen))
				FAIL("round %llu: segment %llu is malformed\n", (unsigned long long)r, (unsigned long long)k);
			bytes += o.len[k];
		}
		for (uint32_t k = 0; k < nconn; k++) {
			const struct gcl_txq_conn_out *oc = &o.out_conn[k];
			const int bad = qoff[k] > qoff[k + 1] || qoff[k + 1] > nent;
			const uint32_t n = bad ? 0 : qoff[k + 1] - qoff[k];

			if (oc->nacked > n || oc->nretx > 17 || ((oc->flags & GCL_TXQO_BADRANGE) != 0) != bad ||
			    ((oc->flags & GCL_TXQO_EMPTY) != 0) != (oc->nacked == n) || oc->first > cap ||
			    (uint64_t)oc->first + oc->nretx > cap ||
			    ((oc->flags & GCL_TXQO_DEFERRED) && (oc->nacked || oc->nretx)))
				FAIL("round %llu: connection %u is malformed\n", (unsigned long long)r, k);
			for (int x = 0; x < 11; x++)
				if (oc->pad[x])
					FAIL("round %llu: connection %u has pad bytes\n", (unsigned long long)r, k);
			nretx += oc->nretx;
			nacked += oc->nacked;
			flagged[0] += (oc->flags & GCL_TXQO_EMPTY) != 0;
			flagged[1] += (oc->flags & GCL_TXQO_BATCH) != 0;
			flagged[2] += bad;
			if (!bad)
				for (uint32_t e = qoff[k]; e < qoff[k + 1]; e++) {
					if ((o.state[e] & 0x7F) > GCL_TXQS_REFUSED)
						FAIL("round %llu: state %u of entry %u\n", (unsigned long long)r, o.state[e], e);
					nospace_ent += (o.state[e] & 0x7F) == GCL_TXQS_NOSPACE;
				}
		}
		if (bytes != o.totals[2] || nretx != written || nacked != c[GCL_TXQC_ACKED])
			FAIL("round %llu: the counters do not agree with the arrays\n", (unsigned long long)r);
		for (int k = 0; k < GCL_TXQC_NR; k++)
			sum[k] += c[k];
		free(qoff); free(ent); free(cold); free(conn); free(addr); free(want);
		free(o.out_conn); free(o.state); free(o.desc); free(o.frame_off); free(o.src_off); free(o.len);
		free(o.dst_off); free(o.seg_conn); free(o.seg_ent); free(o.totals);
	}
	printf("txq ok");
	for (int k = 0; k < GCL_TXQC_NR; k++)
		printf(" %llu", (unsigned long long)sum[k]);
	printf(" %llu %llu %llu %llu\n", (unsigned long long)flagged[0], (unsigned long long)flagged[1],
	       (unsigned long long)flagged[2], (unsigned long long)nospace_ent);
	return 0;
}
