/*
 * pack_fuzz.c - CPU fuzz driver for gcl_host_deliver_packed, built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_pack; tests/test_pack_sanitize.py runs it).
 *
 *   pack_fuzz SEED ITERS   random packed records (cmd, payload and garbage v4
 *                          bytes) with random index lists, entries at or above
 *                          n included, into worlds of small rings that fill,
 *                          missing clients and rings, and a sched_add_core that
 *                          rewrites the tables; bcast_hash and ops NULL or not.
 *                          The record arrays are heap blocks of exactly m
 *                          elements and bcast_hash one of exactly n, so a read
 *                          past a list position, or through an entry >= n, is a
 *                          sanitizer report.  Every callback checks that it is
 *                          given a packet of the batch.
 *
 * Exit 0 when every call returned; a sanitizer report aborts with non-zero.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"

static uint64_t rng_state;

static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

#define NPROC 8
#define MAXR 12 /* ids 8..11 have no client */

struct world {
	struct gcl_host_proc procs[NPROC];
	struct gcl_host_proc *by_id[MAXR];
	struct gcl_host_proc *clients[NPROC];
	struct gcl_lrpc_chan_out chans[NPROC][GCL_NCPU];
	struct gcl_lrpc_msg *tbl[NPROC][GCL_NCPU];
	uint32_t head_wb[NPROC][GCL_NCPU];
	uint64_t n, calls;
};

static void w_init(struct world *w)
{
	for (int p = 0; p < NPROC; p++) {
		struct gcl_host_proc *pr = &w->procs[p];
		uint16_t tc = (uint16_t)(1 + rnd() % (p == 7 ? GCL_NCPU : 8));
		uint16_t act = (uint16_t)(rnd() % (tc + 1));
		uint16_t idx[GCL_NCPU];

		pr->uniqid = (uint16_t)p;
		pr->thread_count = tc;
		pr->active_thread_count = act;
		pr->idle_top = (int16_t)((rnd() & 3) ? (int)(rnd() % tc) : -1);
		for (uint16_t i = 0; i < act; i++)
			idx[i] = i;
		if (act)
			gcl_steer_flows(tc, idx, act, pr->flow_tbl);
		for (int t = 0; t < tc; t++) {
			unsigned size = 1u << (rnd() % 4);
			if ((rnd() & 7) == 0)
				continue;
			w->tbl[p][t] = calloc(size, sizeof(struct gcl_lrpc_msg));
			gcl_lrpc_init_out(&w->chans[p][t], w->tbl[p][t], size, &w->head_wb[p][t]);
			pr->rxq[t] = &w->chans[p][t];
		}
		w->clients[p] = pr;
		if (p != 3)
			w->by_id[p] = pr;
	}
}

static void w_free(struct world *w)
{
	for (int p = 0; p < NPROC; p++)
		for (int t = 0; t < GCL_NCPU; t++)
			free(w->tbl[p][t]);
}

static void cb_add_core(void *arg, struct gcl_host_proc *p)
{
	(void)arg;
	if (rnd() & 1) {
		uint16_t idx[GCL_NCPU];
		for (uint16_t i = 0; i < p->thread_count; i++)
			idx[i] = i;
		gcl_steer_flows(p->thread_count, idx, p->thread_count, p->flow_tbl);
		p->active_thread_count = p->thread_count;
	}
}
/* every callback must be given a packet of the batch */
static void seen(void *arg, uint64_t i)
{
	struct world *w = arg;
	if (i >= w->n)
		abort();
	w->calls++;
}
static void cb_poll(void *arg, struct gcl_host_proc *p, unsigned th)
{
	(void)arg;
	if (th >= p->thread_count)
		abort();
}
static void cb_free(void *arg, uint64_t i) { seen(arg, i); }
static void cb_owned(void *arg, struct gcl_host_proc *p, uint64_t i) { (void)p; seen(arg, i); }
static void cb_refcnt(void *arg, uint64_t i, int d) { (void)d; seen(arg, i); }
static bool cb_arp(void *arg, uint64_t i) { seen(arg, i); return (i & 1) != 0; }

int main(int argc, char **argv)
{
	uint64_t stats[GCL_NR_STATS] = { 0 };
	uint64_t delivered = 0, calls = 0, skipped = 0;

	if (argc < 3) {
		fprintf(stderr, "usage: pack_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);
	for (uint64_t it = 0; it < iters; it++) {
		struct world *w = calloc(1, sizeof(*w));
		struct gcl_host_ops ops = { w, cb_add_core, cb_poll, cb_free, cb_owned, cb_refcnt, cb_arp };
		const struct gcl_host_ops *o = (rnd() & 3) ? &ops : NULL;
		const uint64_t n = rnd() % 300, m = rnd() % 400; /* n == 0: every entry is outside */
		uint64_t inside = 0;
		/* exact-size heap blocks (malloc(0) is avoided, not padded) */
		uint64_t *cmd = malloc((m ? m : 1) * sizeof(*cmd));
		uint64_t *payload = malloc((m ? m : 1) * sizeof(*payload));
		struct gcl_verdict4 *v4 = malloc((m ? m : 1) * sizeof(*v4));
		uint32_t *idx = malloc((m ? m : 1) * sizeof(*idx));
		uint32_t *bh = malloc((n ? n : 1) * sizeof(*bh));

		w->n = n;
		w_init(w);
		for (uint64_t i = 0; i < n; i++)
			bh[i] = (uint32_t)rnd();
		for (uint64_t j = 0; j < m; j++) {
			const uint64_t r = rnd();
			uint8_t b[4];

			/* the ring's parity bit is the post-pass's, as gcl_rx_make_cmd leaves it */
			cmd[j] = rnd() & ~GCL_LRPC_DONE_PARITY;
			payload[j] = rnd();
			/* garbage bytes, mostly unicast-looking so the rings see traffic */
			for (int k = 0; k < 4; k++) {
				const uint64_t x = rnd();
				b[k] = (uint8_t)((x & 0x300) ? x % MAXR : x);
			}
			if (r & 0x3000)
				b[1] = 0; /* a uniqid below 256, action DELIVER or WAKE */
			if (r & 0xC000)
				b[3] &= 1;
			memcpy(&v4[j], b, 4);
			/* one entry in five names no packet: at n, just above, far above */
			switch (n ? (r >> 16) % 10 : 0) {
			case 0: idx[j] = (uint32_t)(n + (rnd() & 3)); break;
			case 1: idx[j] = (uint32_t)((rnd() & 1) ? UINT32_MAX - (rnd() & 7) : n + rnd() % (1u << 31)); break;
			default: idx[j] = (uint32_t)(rnd() % n); break;
			}
			inside += idx[j] < n;
		}
		const uint64_t d = gcl_host_deliver_packed(w->by_id, MAXR, w->clients, NPROC, cmd, payload, v4,
		                                           idx, m, n, (rnd() & 1) ? bh : NULL, o, stats);
		if (d > inside)
			abort();
		/* a missing required array delivers nothing */
		if (gcl_host_deliver_packed(w->by_id, MAXR, w->clients, NPROC, (it & 1) ? NULL : cmd,
		                            (it & 2) ? payload : NULL, (it & 4) ? v4 : NULL,
		                            (it & 8) ? idx : NULL, m, n, NULL, o, stats) != 0 &&
		    (it & 15) != 14)
			abort();
		delivered += d;
		calls += w->calls;
		skipped += m - inside;
		free(cmd); free(payload); free(v4); free(idx); free(bh);
		w_free(w);
		free(w);
	}
	printf("pack ok %llu %llu %llu %llu\n", (unsigned long long)delivered, (unsigned long long)calls,
	       (unsigned long long)skipped, (unsigned long long)stats[GCL_RX_UNICAST_FAIL]);
	return 0;
}
