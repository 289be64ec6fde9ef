/*
 * tcprxs_fuzz.c - stand-alone ASan + UBSan driver of gcl_tcp_rx_states_host and
 * gcl_tcp_rx_ctl_host (csrc/gcl_host.c with the rules of csrc/gcl_tcprxs.h and
 * csrc/gcl_tcptmr.h): tcprxo_fuzz.c's garbage frames, cookies, connection
 * words, orders, hostile q_off and queue entries, and on top random states
 * (also SYN_SENT and values past CLOSED, and no state array at all), FIN, RST,
 * SYN and URG on the segments and FIN on queue entries, over heap arrays of
 * their exact size, so that a read or write past any of them traps.  The
 * outputs of every call then go through gcl_tcp_rx_ctl_host with a random
 * seg_cap.  Usage: tcprxs_fuzz SEED ROUNDS.  Prints "tcprxs ok", the
 * twenty-three counters and the branch counts: tcprxo_fuzz.c's eleven, then
 * entries with RST, RST_ACK, FAIL, STATE, FIN and PUT in ev, and the RST and
 * RST|ACK segments gcl_tcp_rx_ctl_host wrote.
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

static void put32(uint8_t *p, uint32_t v)
{
	p[0] = v >> 24;
	p[1] = v >> 16;
	p[2] = v >> 8;
	p[3] = v;
}

enum { B_KEPT, B_FREED, B_DRAINED, B_REFUSED, B_HEADCLIP, B_LATE_DRAINED, B_LATE_FREED, B_HELD, B_ZERO, B_QSKIP,
       B_FULL, B_RST, B_RST_ACK, B_FAIL, B_STATE, B_FIN, B_PUT, B_SEG_RST, B_SEG_RST_ACK, B_NR };

int main(int argc, char **argv)
{
	const uint64_t rounds = argc > 2 ? strtoull(argv[2], NULL, 0) : 1000;
	uint64_t counts[GCL_TCPRXSC_NR] = {0}, br[B_NR] = {0};

	rs = (argc > 1 ? strtoull(argv[1], NULL, 0) : 1) * 0x9E3779B97F4A7C15ull + 1;
	for (uint64_t r = 0; r < rounds; r++) {
		const int sane = rnd() & 1, crowd = sane && rnd() % 8 == 0;
		const uint32_t n = crowd ? 300 : rnd() % 200, nconn = crowd ? 1 : sane ? 1 + rnd() % 8 : rnd() % 12;
		const uint32_t stride = 16 * (4 + rnd() % 100);
		const uint64_t flen = (uint64_t)n * stride - (n && !sane ? rnd() % stride : 0);
		const int with_order = !sane && (rnd() & 1), with_st = rnd() & 1, with_offs = !sane && (rnd() & 1);
		const uint64_t m = with_order ? rnd() % 300 : n;
		const uint32_t nq = rnd() % 4 == 0 ? 0 : rnd() % (sane ? 40 : 300);
		const int with_qoff = nq || (rnd() & 1);
		const uint32_t cap = rnd() % (nq + m + 2);
		uint8_t *frames = exact(flen);
		uint16_t *plen = exact(2 * (size_t)n);
		uint64_t *offs = with_offs ? exact(8 * (size_t)n) : NULL;
		uint32_t *sock = exact(4 * (size_t)n);
		uint8_t *st = with_st ? exact(n) : NULL;
		uint32_t *order = with_order ? exact(4 * (size_t)m) : NULL;
		struct gcl_tcp_conn *conn = exact16(48 * (size_t)nconn);
		struct gcl_tcp_conn_out *oc = exact16(48 * (size_t)nconn);
		struct gcl_tcp_conn_ext *ext = exact16(16 * (size_t)nconn);
		uint8_t *rep = rnd() & 3 ? exact(nconn) : NULL;
		uint8_t *verdict = exact(m), *sflags = exact(m), *oflags = exact(m);
		uint32_t *after = exact(4 * m);
		uint16_t *clen = exact(2 * m), *skip = exact(2 * m);
		uint64_t *doff = exact(8 * m), *coff = exact(8 * ((size_t)nconn + 1));
		uint32_t *q_off = with_qoff ? exact(4 * ((size_t)nconn + 1)) : NULL;
		struct gcl_tcp_ooo_ent *q = exact16(16 * (size_t)nq), *qout = exact16(16 * (size_t)cap);
		uint8_t *qstate = exact(nq);
		uint16_t *qskip = exact(2 * (size_t)nq), *qlen = exact(2 * (size_t)nq);
		uint64_t *qdst = exact(8 * (size_t)nq), totals[1];
		uint32_t *qout_off = exact(4 * ((size_t)nconn + 1));
		uint8_t *state = rnd() % 5 ? exact(nconn) : NULL;
		uint8_t *ev = exact(m), *state_after = exact(m), *state_out = exact(nconn);
		uint32_t *rst_seq = exact(4 * m);
		struct gcl_tcp_addr *addr = exact16(16 * (size_t)nconn);
		const uint64_t seg_cap = rnd() % (m + 2);
		struct gcl_txh_desc *desc = exact16(32 * (size_t)seg_cap);
		uint64_t *frame_off = exact(8 * (size_t)seg_cap), ctotals[2];
		uint32_t *seg_conn = exact(4 * (size_t)seg_cap), *seg_src = exact(4 * (size_t)seg_cap);
		uint8_t *seg_kind = exact(seg_cap);

		for (uint32_t c = 0; state && c < nconn; c++)
			state[c] = sane ? 1 + rnd() % 9 : rnd() % 12;

		for (uint32_t i = 0; i < n; i++) {
			if (with_offs && (rnd() & 3))
				offs[i] = rnd() % (flen + 64);
			if (rnd() & 7)
				sock[i] = (uint32_t)(rnd() % (nconn + 2));
			if (with_order && (rnd() & 7) && i < m)
				order[i] = (uint32_t)(rnd() % (n + 2));
		}
		if (q_off && (rnd() & 3)) /* near nq, in any order */
			for (uint32_t c = 0; c <= nconn; c++)
				q_off[c] = (uint32_t)(rnd() % (nq + 3));
		if (!sane)
			for (uint32_t c = 0; c < nconn; c++)
				if (rnd() & 1)
					conn[c].flags |= GCL_TCPC_ESTABLISHED;
		if (sane) { /* streams with reordering and overlap over sorted queues */
			uint32_t nxt[8], qat = 0;
			for (uint32_t c = 0; c < nconn; c++) {
				const uint32_t mine = crowd ? 0 : nq / nconn;

				memset(&conn[c], 0, sizeof(conn[c]));
				conn[c].snd_una = (uint32_t)rnd();
				conn[c].snd_nxt = conn[c].snd_una + 1000;
				conn[c].snd_wnd = 1u << 20;
				conn[c].rcv_nxt = nxt[c] = rnd() & 1 ? 0xFFFFFF00u : (uint32_t)rnd();
				conn[c].snd_wl1 = nxt[c] - 1;
				conn[c].rcv_wnd = rnd() & 3 ? 1u << 20 : 200 + rnd() % 3000;
				conn[c].rcv_mss = 200;
				conn[c].flags = (rnd() & 1 ? GCL_TCPC_ELIGIBLE : GCL_TCPC_ESTABLISHED) | (rnd() & 6);
				conn[c].acks_delayed_cnt = rnd() & 1;
				if (q_off)
					q_off[c] = qat;
				for (uint32_t k = 0; k < mine && qat < nq; k++, qat++) {
					q[qat].seq = nxt[c] + 100 * (1 + k) + rnd() % 50;
					q[qat].end = q[qat].seq + 1 + rnd() % 100;
					q[qat].flags = 0x10 | (rnd() % 20 == 0 ? 0x01 : 0);
				}
			}
			if (q_off)
				q_off[nconn] = qat;
			for (uint32_t i = 0; i < n; i++) {
				uint8_t *f = frames + (uint64_t)i * stride;
				const uint32_t c = rnd() % nconn, fault = rnd() % 40;
				const uint32_t len = crowd ? 1 : fault == 0 ? 201 : fault == 1 || rnd() % 8 == 0 ? 0 : 1 + rnd() % 200;
				const uint32_t tot = 40 + len, how = rnd() % 8;
				/* in order; ahead by a few segments; overlapping what was received; a crowd: 2-byte slots */
				const uint32_t seq = crowd ? nxt[c] + 2 + 2 * (i % 70) :
				                     how < 3 ? nxt[c] : how < 6 ? nxt[c] + 50 * (1 + rnd() % 12) : nxt[c] - rnd() % 150;

				plen[i] = (uint16_t)(14 + tot);
				sock[i] = fault == 2 ? nconn : c;
				f[12] = 0x08; f[13] = 0x00; f[14] = 0x45;
				f[16] = tot >> 8; f[17] = tot;
				f[20] = 0x40; f[21] = 0;
				f[23] = fault == 3 ? 17 : 6;
				put32(f + 38, seq);
				put32(f + 42, conn[c].snd_una + (fault == 5 ? 2000 : rnd() % 6 == 0 ? 1000 : rnd() & 1 ? 0 : rnd() % 500));
				f[46] = 0x50;
				f[48] = rnd() & 1 ? 0 : 0xFF;
				f[49] = 0;
				f[47] = (rnd() % 16 ? 0x10 : 0) | (fault == 6 || rnd() % 12 == 0 ? 0x01 : 0) | (rnd() & 8) |
				        (rnd() % 24 == 0 ? 0x04 : 0) | (rnd() % 24 == 0 ? 0x02 : 0) | (rnd() % 16 == 0 ? 0x20 : 0);
				if (st)
					st[i] = fault == 7 ? GCL_L4_BAD : GCL_L4_GOOD;
				if (how < 3 && fault > 7 && !crowd)
					nxt[c] += len; /* a guess that keeps the chains going */
			}
		}
		const struct gcl_batch b = {.frames = frames, .frames_len = flen, .stride = stride, .offs = offs,
		                            .pkt_len = plen, .n = n};
		const struct gcl_tcprxs_in in = {.size = sizeof(in), .align = 1u << (rnd() % 9) >> 1, .order = order,
		                                 .m = m, .sock = sock, .l4_status = st, .conn = conn, .nconn = nconn,
		                                 .blocks = rnd() % (GCL_TCPRX_MAX_BLOCKS + 1), .rep_acks = rep,
		                                 .q_off = q_off, .q = q, .nq = nq, .q_out_cap = cap, .state = state};
		const struct gcl_tcprxs_out so = {ev, rst_seq, state_after, state_out};
		const struct gcl_tcprx_out out = {verdict, sflags, after, clen, doff, oc, coff};
		const struct gcl_tcprxo_out oo = {oflags, skip, qstate, qskip, qlen, qdst, qout_off, qout, totals};
		uint64_t c[GCL_TCPRXSC_NR] = {0};
		const int rc = gcl_tcp_rx_states_host(&b, &in, &out, ext, &oo, &so, c);

		if (rc != 0) {
			printf("tcprxs round %llu: %d\n", (unsigned long long)r, rc);
			return 1;
		}
		if (c[0] + c[1] + c[2] + c[3] + c[4] != m || totals[0] != qout_off[nconn]) {
			printf("tcprxs round %llu: the counts do not add up\n", (unsigned long long)r);
			return 1;
		}
		for (uint64_t j = 0; j < m; j++) {
			if ((clen[j] && verdict[j] != GCL_TCPRX_FAST) || (clen[j] && doff[j] + clen[j] > coff[nconn])) {
				printf("tcprxs round %llu: entry %llu lies outside the layout\n", (unsigned long long)r,
				       (unsigned long long)j);
				return 1;
			}
			br[B_REFUSED] += (oflags[j] & (GCL_OOOF_OOO | GCL_OOOF_QUEUED)) == GCL_OOOF_OOO;
			br[B_HEADCLIP] += (oflags[j] & GCL_OOOF_HEADCLIP) != 0;
			br[B_LATE_DRAINED] += (oflags[j] & GCL_OOOF_LATE_DRAINED) != 0;
			br[B_LATE_FREED] += (oflags[j] & GCL_OOOF_LATE_FREED) != 0;
			br[B_HELD] += (oflags[j] & GCL_OOOF_HELD) != 0;
			br[B_ZERO] += (oflags[j] & GCL_OOOF_LATE_DRAINED) && !clen[j];
		}
		{ /* the control segments of the call, with any seg_cap */
			const struct gcl_rxctl_in cin = {.size = sizeof(cin), .blocks = 0, .order = order, .m = m, .n = n,
			                                 .sock = sock, .verdict = verdict, .sflags = sflags,
			                                 .rcv_nxt_after = after, .conn = conn, .addr = addr, .nconn = nconn,
			                                 .frame_stride = 64, .seg_cap = seg_cap, .frame_base = rnd(), .ev = ev,
			                                 .rst_seq = rst_seq};
			const struct gcl_ctlseg_out co = {desc, frame_off, seg_conn, seg_kind, seg_src, ctotals};
			const int rc2 = gcl_tcp_rx_ctl_host(&cin, &co, NULL);

			if (rc2 != 0 || ctotals[1] > seg_cap || ctotals[1] > ctotals[0] || ctotals[0] > m) {
				printf("tcprxs round %llu: ctl %d\n", (unsigned long long)r, rc2);
				return 1;
			}
			for (uint64_t k = 0; k < ctotals[1]; k++) {
				if (seg_kind[k] > GCL_CTL_RST_ACK || seg_kind[k] == GCL_CTL_PROBE || seg_src[k] >= m ||
				    seg_conn[k] >= nconn) {
					printf("tcprxs round %llu: control segment %llu\n", (unsigned long long)r, (unsigned long long)k);
					return 1;
				}
				br[B_SEG_RST] += seg_kind[k] == GCL_CTL_RST;
				br[B_SEG_RST_ACK] += seg_kind[k] == GCL_CTL_RST_ACK;
			}
		}
		for (uint64_t j = 0; j < m; j++) {
			if ((ev[j] & GCL_TCPS_RST) && (ev[j] & GCL_TCPS_RST_ACK)) {
				printf("tcprxs round %llu: entry %llu has both RSTs\n", (unsigned long long)r, (unsigned long long)j);
				return 1;
			}
			for (int x = 0; x < 6; x++)
				br[B_RST + x] += (ev[j] >> x) & 1;
		}
		for (uint32_t i = 0; i < nq; i++) {
			if (qstate[i] > GCL_OOOQ_DRAINED) {
				printf("tcprxs round %llu: qin_state[%u] = %u\n", (unsigned long long)r, i, qstate[i]);
				return 1;
			}
			if (qstate[i])
				br[B_KEPT + qstate[i] - 1]++;
		}
		for (uint32_t k = 0; k < nconn; k++) {
			br[B_QSKIP] += (ext[k].xflags & GCL_TCPX_QSKIP) != 0;
			br[B_FULL] += (oc[k].flags & GCL_TCPO_STOPPED) && qout_off[k + 1] - qout_off[k] == GCL_TCPOOO_CAP;
		}
		for (int k = 0; k < GCL_TCPRXSC_NR; k++)
			counts[k] += c[k];
		free(frames); free(plen); free(offs); free(sock); free(st); free(order); free(conn); free(oc); free(ext); free(rep);
		free(verdict); free(sflags); free(oflags); free(after); free(clen); free(skip); free(doff); free(coff);
		free(q_off); free(q); free(qout); free(qstate); free(qskip); free(qlen); free(qdst); free(qout_off);
		free(state); free(ev); free(state_after); free(state_out); free(rst_seq); free(addr); free(desc); free(frame_off);
		free(seg_conn); free(seg_src); free(seg_kind);
	}
	printf("tcprxs ok");
	for (int k = 0; k < GCL_TCPRXSC_NR; k++)
		printf(" %llu", (unsigned long long)counts[k]);
	printf(" :");
	for (int k = 0; k < B_NR; k++)
		printf(" %llu", (unsigned long long)br[k]);
	printf("\n");
	return 0;
}
