/*
 * tcpread_fuzz.c - a stand-alone driver of gcl_tcp_read_host for the ASan +
 * UBSan build (caladan_amd/build.py: build_sanitized_tcpread).  Every array is
 * a heap block of its exact size, so a read or write one element past any of
 * them traps.  Rounds alternate between consistent CSR offsets and garbage
 * ones (decreasing, past nent / nvec, 0xFFFFFFFF), with and without vectors,
 * with caps that are enough, one short, tiny and 0.
 *
 *   tcpread_fuzz SEED ROUNDS   ->   "tcpread ok" and the twelve summed counts
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"
#include "../../include/gclassify.h"

static uint64_t s[2];

static uint64_t rnd(void)
{
	uint64_t a = s[0], b = s[1];
	const uint64_t r = a + b;

	b ^= a;
	s[0] = (a << 55 | a >> 9) ^ b ^ (b << 14);
	s[1] = b << 36 | b >> 28;
	return r;
}

static uint32_t below(uint32_t n)
{
	return n ? (uint32_t)(rnd() % n) : 0;
}

static void *blk(size_t n, size_t sz)
{
	/* the exact size, 16-B aligned; an empty array still gets an address */
	void *p = NULL;

	if (posix_memalign(&p, 16, n && sz ? n * sz : 1))
		abort();
	memset(p, 0xA5, n && sz ? n * sz : 1);
	return p;
}

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], NULL, 0) : 1;
	const int rounds = argc > 2 ? atoi(argv[2]) : 200;
	static const uint16_t lens[] = {0, 0, 1, 7, 64, 1448, 65535};
	uint64_t counts[GCL_RDC_NR] = {0};

	s[0] = seed * 0x9E3779B97F4A7C15ull + 1;
	s[1] = seed ^ 0xD1B54A32D192ED03ull;
	for (int round = 0; round < rounds; round++) {
		const uint32_t nconn = below(40);
		const int garbage = round % 3 == 2, vectors = round & 1;
		uint32_t *qoff = blk(nconn + 1, 4), *voff = blk(nconn + 1, 4);
		uint64_t nent = 0, nvec = 0;

		qoff[0] = voff[0] = 0;
		for (uint32_t c = 0; c < nconn; c++) {
			nent += below(8) == 0 ? below(300) : below(6);
			nvec += below(5);
			qoff[c + 1] = (uint32_t)nent;
			voff[c + 1] = (uint32_t)nvec;
		}
		if (garbage)
			for (uint32_t c = 0; c <= nconn; c++) {
				if (below(4) == 0)
					qoff[c] = below(3) ? below((uint32_t)nent + 4) : 0xFFFFFFFFu - below(2);
				if (below(4) == 0)
					voff[c] = below(3) ? below((uint32_t)nvec + 4) : 0xFFFFFFFFu - below(2);
			}
		struct gcl_rdq_ent *ent = blk(nent, sizeof(*ent));
		struct gcl_rd_iov *iov = blk(nvec, sizeof(*iov));
		struct gcl_tcp_rd *rd = blk(nconn, sizeof(*rd));
		struct gcl_tcp_conn *conn = blk(nconn, sizeof(*conn));
		struct gcl_tcp_addr *addr = blk(nconn, sizeof(*addr));

		for (uint64_t e = 0; e < nent; e++) {
			ent[e].off = rnd();
			ent[e].len = lens[below(7)];
			ent[e].flags = below(12) == 0 ? GCL_RDQE_FIN : (garbage ? (uint8_t)rnd() & 0xFE : 0);
		}
		for (uint64_t v = 0; v < nvec; v++) {
			iov[v].off = rnd();
			iov[v].len = below(4) ? below(3000) : (uint32_t)rnd();
		}
		for (uint32_t c = 0; c < nconn; c++) {
			rd[c].dst_off = rnd();
			rd[c].len = below(3) ? below(9000) : (uint32_t)rnd();
			rd[c].tx_last_ack = (uint32_t)rnd();
			rd[c].tx_last_win = (uint32_t)rnd();
			rd[c].winmax = below(2) ? 0 : (uint32_t)rnd();
			rd[c].err = (int32_t)rnd();
			rd[c].flags = below(5) ? (uint8_t)(GCL_RD_WANT | (below(4) ? 0 : (uint8_t)rnd())) : (uint8_t)rnd();
			for (size_t k = 0; k < sizeof(*conn); k++)
				((uint8_t *)&conn[c])[k] = (uint8_t)rnd();
			for (size_t k = 0; k < sizeof(*addr); k++)
				((uint8_t *)&addr[c])[k] = (uint8_t)rnd();
		}
		const uint64_t enough = nent + (nvec > nconn ? nvec : nconn);
		const uint64_t caps[4] = {enough, enough ? enough - 1 : 0, 3, 0};
		const uint64_t item_cap = caps[below(4)], seg_cap = below(3) ? nconn : below(nconn + 1);
		struct gcl_rd_in in = {0};
		struct gcl_rd_out out = {0};
		uint64_t totals[4], seg_totals[2];

		in.size = sizeof(in);
		in.blocks = below(8);
		in.qoff = qoff;
		in.ent = ent;
		in.nent = nent;
		in.voff = vectors ? voff : NULL;
		in.iov = iov;
		in.nvec = nvec;
		in.rd = rd;
		in.conn = conn;
		in.addr = addr;
		in.nconn = nconn;
		in.frame_stride = GCL_CTL_MIN_STRIDE + below(100);
		in.item_cap = item_cap;
		in.seg_cap = seg_cap;
		in.frame_base = rnd();
		out.out_conn = blk(nconn, sizeof(*out.out_conn));
		out.src_off = blk(item_cap, 8);
		out.len = blk(item_cap, 2);
		out.dst_off = blk(item_cap, 8);
		out.item_conn = blk(item_cap, 4);
		out.item_ent = blk(item_cap, 4);
		out.totals = totals;
		out.seg.desc = blk(seg_cap, sizeof(*out.seg.desc));
		out.seg.frame_off = blk(seg_cap, 8);
		out.seg.seg_conn = blk(seg_cap, 4);
		out.seg.seg_kind = blk(seg_cap, 1);
		out.seg.seg_src = blk(seg_cap, 4);
		out.seg.totals = seg_totals;

		const int rc = gcl_tcp_read_host(&in, &out, counts);
		if (rc) {
			printf("tcpread refused round %d: %d\n", round, rc);
			return 1;
		}
		/* what must hold whatever the input was */
		uint64_t items = 0, segs = 0;
		for (uint32_t c = 0; c < nconn; c++) {
			const struct gcl_rd_conn_out *o = &out.out_conn[c];

			if (o->status > GCL_RDS_BADRANGE || o->pad[0] || o->pad[1] || o->first_item != items ||
			    o->first_item + (uint64_t)o->nitems > item_cap) {
				printf("tcpread bad out_conn round %d conn %u\n", round, c);
				return 1;
			}
			items += o->nitems;
			segs += (o->flags & GCL_RDO_ACK) && !(o->flags & GCL_RDO_SEG_NOSPACE);
			for (uint64_t k = o->first_item; k < items; k++)
				if (out.item_conn[k] != c || out.item_ent[k] >= nent) {
					printf("tcpread bad item round %d conn %u\n", round, c);
					return 1;
				}
		}
		if (items != totals[1] || totals[1] > totals[0] || totals[1] > item_cap || segs != seg_totals[1] ||
		    seg_totals[1] > seg_cap) {
			printf("tcpread bad totals round %d\n", round);
			return 1;
		}
		free(qoff); free(voff); free(ent); free(iov); free(rd); free(conn); free(addr);
		free(out.out_conn); free(out.src_off); free(out.len); free(out.dst_off); free(out.item_conn);
		free(out.item_ent); free(out.seg.desc); free(out.seg.frame_off); free(out.seg.seg_conn);
		free(out.seg.seg_kind); free(out.seg.seg_src);
	}
	printf("tcpread ok");
	for (int i = 0; i < GCL_RDC_NR; i++)
		printf(" %llu", (unsigned long long)counts[i]);
	printf("\n");
	return 0;
}
