/*
 * tcpwrite_fuzz.c - a stand-alone driver of gcl_tcp_write_host for the ASan +
 * UBSan build (caladan_amd/build.py: build_sanitized_tcpwrite).  Every array
 * is a heap block of its exact size, so a read or write one element past any
 * of them traps.  Rounds alternate between consistent vector offsets and
 * garbage ones (decreasing, past nvec, 0xFFFFFFFF), with and without voff.
 * Each round runs three times: with caps that surely hold everything, with
 * the caps the first run asked for exactly, and with one of the three caps
 * one short, tiny or 0.  Windows and lengths stay small: the twin's time
 * grows with the segments.
 *
 *   tcpwrite_fuzz SEED ROUNDS   ->   "tcpwrite ok" and the fourteen summed counts
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

struct outs {
	struct gcl_wr_out o;
	uint64_t totals[6];
};

static void outs_new(struct outs *x, uint32_t nconn, uint64_t seg_cap, uint64_t item_cap)
{
	x->o.out_conn = blk(nconn, sizeof(*x->o.out_conn));
	x->o.desc = blk(seg_cap, sizeof(*x->o.desc));
	x->o.frame_off = blk(seg_cap, 8);
	x->o.seg_conn = blk(seg_cap, 4);
	x->o.txq_ent = blk(seg_cap, sizeof(*x->o.txq_ent));
	x->o.txq_cold = blk(seg_cap, sizeof(*x->o.txq_cold));
	x->o.src_off = blk(item_cap, 8);
	x->o.len = blk(item_cap, 2);
	x->o.dst_off = blk(item_cap, 8);
	x->o.item_conn = blk(item_cap, 4);
	x->o.item_seg = blk(item_cap, 4);
	x->o.totals = x->totals;
}

static void outs_free(struct outs *x)
{
	free(x->o.out_conn); free(x->o.desc); free(x->o.frame_off); free(x->o.seg_conn); free(x->o.txq_ent);
	free(x->o.txq_cold); free(x->o.src_off); free(x->o.len); free(x->o.dst_off); free(x->o.item_conn);
	free(x->o.item_seg);
}

/* what must hold whatever the input was */
static int verify(const struct gcl_wr_in *in, const struct outs *x, int round, int run)
{
	uint64_t segs = 0, items = 0;

	for (uint32_t c = 0; c < in->nconn; c++) {
		const struct gcl_wr_conn_out *o = &x->o.out_conn[c];
		int bad = o->status > GCL_WRS_NOSPACE || o->pad[0] || o->pad[5];

		if (o->status == GCL_WRS_DONE) {
			bad |= o->first_seg != segs || o->first_item != items || o->ret < 0 ||
			       o->pend_len > in->wr[c].snd_mss || segs + o->nseg > in->seg_cap ||
			       items + o->nitems > in->item_cap;
			for (uint64_t k = segs; !bad && k < segs + o->nseg; k++)
				bad |= x->o.seg_conn[k] != c || x->o.desc[k].paylen > in->wr[c].snd_mss ||
				       x->o.txq_ent[k].seg_end - x->o.txq_ent[k].seg_seq != x->o.desc[k].paylen ||
				       x->o.txq_cold[k].frame_off != x->o.frame_off[k];
			for (uint64_t k = items; !bad && k < items + o->nitems; k++)
				bad |= x->o.item_conn[k] != c || x->o.len[k] > in->wr[c].snd_mss ||
				       (x->o.item_seg[k] != GCL_WR_SEG_HELD &&
				        (x->o.item_seg[k] < segs || x->o.item_seg[k] >= segs + o->nseg));
			segs += o->nseg;
			items += o->nitems;
		} else {
			bad |= o->nseg || o->nitems || o->snd_nxt != in->conn[c].snd_nxt || o->pend_len != in->wr[c].pend_len;
		}
		if (bad) {
			printf("tcpwrite bad out_conn round %d run %d conn %u\n", round, run, c);
			return 1;
		}
	}
	if (segs != x->totals[1] || items != x->totals[3] || x->totals[1] > x->totals[0] || x->totals[3] > x->totals[2]) {
		printf("tcpwrite bad totals round %d run %d\n", round, run);
		return 1;
	}
	return 0;
}

int main(int argc, char **argv)
{
	const uint64_t seed = argc > 1 ? strtoull(argv[1], NULL, 0) : 1;
	const int rounds = argc > 2 ? atoi(argv[2]) : 200;
	static const uint16_t msss[] = {0, 1, 19, 20, 21, 100, 536, 1448};
	uint64_t counts[GCL_WRC_NR] = {0};

	s[0] = seed * 0x9E3779B97F4A7C15ull + 1;
	s[1] = seed ^ 0xD1B54A32D192ED03ull;
	for (int round = 0; round < rounds; round++) {
		const uint32_t nconn = below(40);
		const int garbage = round % 3 == 2, vectors = round % 4 != 3;
		uint32_t *voff = blk(nconn + 1, 4);
		uint64_t nvec = 0, bound = 0;

		voff[0] = 0;
		for (uint32_t c = 0; c < nconn; c++) {
			nvec += below(9) == 0 ? below(40) : below(6);
			voff[c + 1] = (uint32_t)nvec;
		}
		if (garbage)
			for (uint32_t c = 0; c <= nconn; c++)
				if (below(4) == 0)
					voff[c] = below(3) ? below((uint32_t)nvec + 4) : 0xFFFFFFFFu - below(2);
		struct gcl_rd_iov *iov = blk(nvec, sizeof(*iov));
		struct gcl_tcp_wr *wr = blk(nconn, sizeof(*wr));
		struct gcl_tcp_conn *conn = blk(nconn, sizeof(*conn));
		struct gcl_tcp_addr *addr = blk(nconn, sizeof(*addr));

		for (uint64_t v = 0; v < nvec; v++) {
			iov[v].off = rnd();
			iov[v].len = below(4) == 0 ? 0 : below(5) == 0 ? (uint32_t)rnd() : below(400);
		}
		for (uint32_t c = 0; c < nconn; c++) {
			for (size_t k = 0; k < sizeof(*conn); k++)
				((uint8_t *)&conn[c])[k] = (uint8_t)rnd();
			for (size_t k = 0; k < sizeof(*addr); k++)
				((uint8_t *)&addr[c])[k] = (uint8_t)rnd();
			for (size_t k = 0; k < sizeof(*wr); k++)
				((uint8_t *)&wr[c])[k] = (uint8_t)rnd();
			/* a window of at most 4095 bytes, sometimes full or behind snd_nxt */
			conn[c].snd_wnd = conn[c].snd_nxt - conn[c].snd_una + (below(6) ? below(4096) : 0u - below(3));
			wr[c].snd_mss = msss[below(8)];
			wr[c].len = below(3) ? below(3000) : (uint32_t)rnd();
			wr[c].pend_len = below(3) ? 0 : below(4) ? below(wr[c].snd_mss + 1u) : below(2000);
			wr[c].flags = below(6) ? (uint8_t)(GCL_WR_WANT | (below(2) ? GCL_WR_VEC : 0) |
			                                  (below(4) ? 0 : GCL_WR_NO_PARTIAL) |
			                                  (below(3) ? 0 : (uint8_t)rnd())) : (uint8_t)rnd();
			wr[c].err = below(2) ? 0 : (int32_t)rnd();
			/* at most window / mss passes, one for the held segment and two more per vector */
			bound += 4096 + 128;
		}
		struct gcl_wr_in in = {0};

		in.size = sizeof(in);
		in.blocks = below(8);
		in.now = rnd();
		in.voff = vectors ? voff : NULL;
		in.iov = iov;
		in.nvec = nvec;
		in.wr = wr;
		in.conn = conn;
		in.addr = addr;
		in.nconn = nconn;
		in.frame_stride = below(3) ? 2048 : 54 + below(1500);
		in.frame_base = rnd();
		for (int run = 0; run < 3; run++) {
			static uint64_t want[3];
			struct outs x;

			if (run == 0) {
				in.seg_cap = in.item_cap = bound;
				in.frames_len = 0;
			} else {
				in.seg_cap = want[0];
				in.item_cap = want[1];
				in.frames_len = below(2) ? 0 : in.frame_base + want[2] * in.frame_stride;
				if (in.frames_len && in.frames_len < in.frame_base) /* wrapped */
					in.frames_len = 0;
			}
			if (run == 2)
				switch (below(5)) {
				case 0: in.seg_cap = in.seg_cap ? in.seg_cap - 1 : 0; break;
				case 1: in.item_cap = in.item_cap ? in.item_cap - 1 : 0; break;
				case 2: in.frames_len = in.frames_len > 1 ? in.frames_len - 1 : 1; break;
				case 3: in.seg_cap = below(4); in.item_cap = below(4); break;
				default: in.seg_cap = in.item_cap = 0; break;
				}
			outs_new(&x, nconn, in.seg_cap, in.item_cap);
			const int rc = gcl_tcp_write_host(&in, &x.o, counts);
			if (rc) {
				printf("tcpwrite refused round %d run %d: %d\n", round, run, rc);
				return 1;
			}
			if (verify(&in, &x, round, run))
				return 1;
			if (run == 0) {
				want[0] = x.totals[0];
				want[1] = x.totals[2];
				want[2] = x.totals[4];
				if (x.totals[0] != x.totals[1] || x.totals[2] != x.totals[3]) {
					printf("tcpwrite: the bound did not hold round %d\n", round);
					return 1;
				}
			} else if (run == 1 && (x.totals[0] != x.totals[1] || x.totals[2] != x.totals[3] ||
			                        x.totals[4] != want[2])) {
				printf("tcpwrite: the exact caps did not hold round %d\n", round);
				return 1;
			}
			outs_free(&x);
		}
		free(voff); free(iov); free(wr); free(conn); free(addr);
	}
	printf("tcpwrite ok");
	for (int i = 0; i < GCL_WRC_NR; i++)
		printf(" %llu", (unsigned long long)counts[i]);
	printf("\n");
	return 0;
}
