/*
 * plan_fuzz.c - CPU fuzz driver for gcl_host_deliver_idx, built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_plan; tests/test_plan_sanitize.py runs it).
 *
 *   plan_fuzz SEED ITERS   random verdict BYTES of each width (1, 2, 4, 8, and
 *                          widths and thread_bits the call refuses) with
 *                          in-range index lists (repeats, any order, empty)
 *                          into worlds of small rings that fill, missing
 *                          clients and rings, and a sched_add_core that
 *                          rewrites the tables.  The arrays are heap blocks of
 *                          exactly n elements, so any index past a list entry
 *                          is a sanitizer report.
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
	static const uint8_t widths[] = { 1, 2, 4, 8, 1, 2, 4, 8, 3, 0 };
	uint64_t stats[GCL_NR_STATS] = { 0 };
	uint64_t delivered = 0, calls = 0;

	if (argc < 3) {
		fprintf(stderr, "usage: plan_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);
	for (uint64_t it = 0; it < iters; it++) {
		struct world *w = calloc(1, sizeof(*w));
		struct gcl_host_ops ops = { w, cb_add_core, cb_poll, cb_free, cb_owned, cb_refcnt, cb_arp };
		const struct gcl_host_ops *o = (rnd() & 3) ? &ops : NULL;
		const uint64_t n = 1 + rnd() % 300, m = rnd() % 400;
		const uint8_t vb = widths[rnd() % sizeof(widths)];
		const uint8_t tb = (uint8_t)(rnd() % 10); /* 8 (1-B) and 9: refused */
		/* exact-size heap blocks: a read past entry n - 1 is caught */
		uint8_t *v = malloc(n * (vb ? vb : 1));
		uint16_t *plen = malloc(n * sizeof(*plen));
		uint8_t *olf = malloc(n);
		uint32_t *bh = malloc(n * sizeof(*bh));
		uint64_t *shm = malloc(n * sizeof(*shm));
		uint32_t *idx = malloc((m ? m : 1) * sizeof(*idx));

		w->n = n;
		w_init(w);
		for (uint64_t i = 0; i < n * (vb ? vb : 1); i++) {
			const uint64_t r = rnd();
			/* mostly unicast-looking bytes, so the rings see traffic */
			v[i] = (uint8_t)((r & 0x300) ? r % MAXR : r);
		}
		for (uint64_t i = 0; i < n; i++) {
			const uint64_t r = rnd();
			plen[i] = (uint16_t)r;
			olf[i] = (uint8_t)(r >> 16);
			bh[i] = (uint32_t)(r >> 24);
			shm[i] = r;
		}
		for (uint64_t j = 0; j < m; j++)
			idx[j] = (uint32_t)(rnd() % n);
		const uint64_t d = gcl_host_deliver_idx(
		        w->by_id, MAXR, w->clients, NPROC, v, vb, tb, (rnd() & 1) ? bh : NULL,
		        (rnd() & 1) ? plen : NULL, (rnd() & 1) ? olf : NULL, 0x09,
		        (rnd() & 1) ? shm : NULL, idx, m, o, stats);
		if (d > m || ((vb != 1 && vb != 2 && vb != 4 && vb != 8) && d))
			abort();
		if ((tb > 8 || (vb == 1 && tb > 7)) && d)
			abort();
		delivered += d;
		calls += w->calls;
		free(v); free(plen); free(olf); free(bh); free(shm); free(idx);
		w_free(w);
		free(w);
	}
	printf("plan ok %llu %llu %llu\n", (unsigned long long)delivered, (unsigned long long)calls,
	       (unsigned long long)stats[GCL_RX_UNICAST_FAIL]);
	return 0;
}
