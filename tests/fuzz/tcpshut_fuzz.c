/*
 * tcpshut_fuzz.c - stand-alone ASan + UBSan driver of gcl_tcp_shut_host
 * (csrc/gcl_host.c with the rule of csrc/gcl_tcpshut.h): hostile requests,
 * timer words, connection words, addresses and caps over heap arrays of their
 * exact size, so that a read or write past any of them traps.  About half of
 * the rounds keep ops, how, states and flags in or near their ranges, so that
 * every status is reached; the rest is garbage bytes.  Usage: tcpshut_fuzz SEED
 * ROUNDS.  Prints "tcpshut ok" and the counts: one per status (NONE DONE BLOCK
 * ABORT_WAIT EINVAL REFUSED NOSPACE), then FIN RST FAIL PUT WARN.
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

/* every record here is a multiple of 16 B, so the block is exactly @bytes long */
static void *exact16(size_t bytes)
{
	void *p = aligned_alloc(16, bytes ? bytes : 16);

	if (!p)
		abort();
	for (size_t i = 0; i < bytes; i++)
		((uint8_t *)p)[i] = (uint8_t)rnd();
	return p;
}

#define FAIL(...) do { printf("round %llu: ", (unsigned long long)r); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

int main(int argc, char **argv)
{
	const uint64_t rounds = argc > 2 ? strtoull(argv[2], NULL, 0) : 1000;
	uint64_t sum[GCL_SHUTC_NR] = {0};

	rs = (argc > 1 ? strtoull(argv[1], NULL, 0) : 1) * 0x9E3779B97F4A7C15ull + 1;
	for (uint64_t r = 0; r < rounds; r++) {
		const int sane = rnd() & 1;
		const uint32_t nconn = rnd() % 300;
		const uint32_t stride = GCL_CTL_MIN_STRIDE + rnd() % 2000;
		const uint64_t base = rnd() & 3 ? rnd() % (1ull << 40) : rnd();
		const uint64_t now = sane ? 1ull << 40 : rnd();
		const uint64_t cap = rnd() & 1 ? rnd() % (nconn + 2) : nconn;
		struct gcl_tcp_shut *shut = exact16(16 * (size_t)nconn);
		struct gcl_tcp_tmr *tmr = exact16(64 * (size_t)nconn);
		struct gcl_tcp_conn *conn = exact16(48 * (size_t)nconn);
		struct gcl_tcp_addr *addr = exact16(16 * (size_t)nconn);
		struct gcl_shut_conn_out *oc = exact16(48 * (size_t)nconn);
		struct gcl_shut_out out;
		uint64_t frames_len = 0, fcap = cap;

		out.out_conn = oc;
		out.seg.desc = exact16(32 * cap);
		out.seg.frame_off = exact(8 * cap);
		out.seg.seg_conn = exact(4 * cap);
		out.seg.seg_kind = exact(cap);
		out.seg.seg_src = exact(4 * cap);
		out.seg.totals = exact(16);
		out.txq_ent = exact16(16 * cap);
		out.txq_cold = exact16(16 * cap);
		if (!(rnd() & 3)) { /* the frames run out before the arrays do, or frame_base lies past them */
			fcap = rnd() % (cap + 1);
			frames_len = base + fcap * stride + rnd() % stride;
			if (frames_len < base || !frames_len) {
				frames_len = 1;
				fcap = base > 1 ? 0 : (1 - base) / stride;
			}
		}
		if (sane)
			for (uint32_t c = 0; c < nconn; c++) {
				shut[c].op = rnd() % 5;
				shut[c].how = (int32_t)(rnd() % 5) - 1;
				shut[c].flags = rnd() & 7 & rnd();
				tmr[c].state = rnd() % 11;
				tmr[c].flags = (uint8_t)((rnd() & rnd()) | (rnd() & 7 ? GCL_TMR_LIVE : 0));
				tmr[c].txq_ts = now - rnd() % 400000;
			}
		const struct gcl_shut_in in = {.size = sizeof(in), .blocks = rnd() % (GCL_SHUT_MAX_BLOCKS + 1), .now = now,
		                               .shut = shut, .tmr = tmr, .conn = conn, .addr = addr, .nconn = nconn,
		                               .frame_stride = stride, .seg_cap = cap, .frame_base = base,
		                               .frames_len = frames_len};
		uint64_t cnt[GCL_SHUTC_NR] = {0}, k = 0, st = 0;
		const int rc = gcl_tcp_shut_host(&in, &out, cnt);

		if (rc != 0)
			FAIL("%d", rc);
		const uint64_t wanted = out.seg.totals[0], written = out.seg.totals[1];
		if (written != (wanted < fcap ? wanted : fcap) || written > cap)
			FAIL("totals %llu %llu with caps %llu %llu", (unsigned long long)wanted, (unsigned long long)written,
			     (unsigned long long)cap, (unsigned long long)fcap);
		if (cnt[GCL_SHUTC_FIN] + cnt[GCL_SHUTC_RST] != written || cnt[GCL_SHUTS_NOSPACE] != wanted - written)
			FAIL("the counters do not agree with totals");
		for (uint32_t c = 0; c < nconn; c++) {
			const struct gcl_shut_conn_out *o = &oc[c];

			if (o->status >= GCL_SHUTS_NR || o->nseg > 1 || o->nput > 2 || memcmp(o->pad, "\0\0\0\0\0\0\0", 7))
				FAIL("connection %u: status %u nseg %u nput %u", c, o->status, o->nseg, o->nput);
			st++;
			if (o->status == GCL_SHUTS_NONE || o->status == GCL_SHUTS_BLOCK || o->status == GCL_SHUTS_EINVAL ||
			    o->status == GCL_SHUTS_REFUSED || o->status == GCL_SHUTS_NOSPACE) {
				if (o->flags || o->err || o->nput || o->nseg || o->state != tmr[c].state ||
				    o->tmr_flags != tmr[c].flags || o->snd_nxt != conn[c].snd_nxt ||
				    o->next_timeout != tmr[c].next_timeout || o->txq_ts != tmr[c].txq_ts)
					FAIL("connection %u: status %u changed something", c, o->status);
			}
			if (!o->nseg)
				continue;
			const struct gcl_txh_desc *d = &out.seg.desc[k];
			const int fin = out.seg.seg_kind[k] == GCL_CTL_FIN;
			if (o->first_seg != k || out.seg.seg_conn[k] != c || out.seg.seg_src[k] != c ||
			    out.seg.frame_off[k] != base + k * stride || d->proto != 6 || d->tcp_off != 5 || d->ecn || d->paylen ||
			    d->pad || d->seq != conn[c].snd_nxt || (!fin && out.seg.seg_kind[k] != GCL_CTL_RST) ||
			    d->tcp_flags != (fin ? 0x11 : 0x04) || (fin && o->snd_nxt != conn[c].snd_nxt + 1) ||
			    (fin && (out.txq_ent[k].seg_seq != d->seq || out.txq_ent[k].seg_end != d->seq + 1 ||
			             out.txq_ent[k].ts != now || out.txq_cold[k].frame_off != out.seg.frame_off[k] ||
			             out.txq_cold[k].tcp_flags != 0x11 || out.txq_cold[k].flags != GCL_TXQE_INFLIGHT)) ||
			    (!fin && (out.txq_ent[k].ts || out.txq_cold[k].frame_off || o->state != GCL_TCP_STATE_CLOSED)))
				FAIL("segment %llu of connection %u is malformed", (unsigned long long)k, c);
			k++;
		}
		if (k != written)
			FAIL("%llu segments claimed, %llu written", (unsigned long long)k, (unsigned long long)written);
		for (int i = 0; i < GCL_SHUTS_NR; i++)
			st -= cnt[i];
		if (st)
			FAIL("the status counters do not sum to nconn");
		for (int i = 0; i < GCL_SHUTC_NR; i++)
			sum[i] += cnt[i];
		free(out.seg.desc); free(out.seg.frame_off); free(out.seg.seg_conn); free(out.seg.seg_kind);
		free(out.seg.seg_src); free(out.seg.totals); free(out.txq_ent); free(out.txq_cold);
		free(shut); free(tmr); free(conn); free(addr); free(oc);
	}
	printf("tcpshut ok");
	for (int i = 0; i < GCL_SHUTC_NR; i++)
		printf(" %llu", (unsigned long long)sum[i]);
	printf("\n");
	return 0;
}
