/*
 * sock_fuzz.c - CPU fuzz driver for the socket table (csrc/gcl_sock.c and the
 * probe of csrc/gcl_sock.h that the GPU kernel shares), built with
 * AddressSanitizer + UndefinedBehaviorSanitizer by caladan_amd/build.py
 * (build_sanitized_sock; tests/test_sock_sanitize.py runs it).
 *
 *   sock_fuzz SEED ITERS   ITERS rounds.  A round sets random entry sets for a
 *                          few runtimes (small pools of addresses and ports,
 *                          so that keys collide; some sets invalid: port 0, a
 *                          bad match, proto or cookie, a repeated 5-tuple --
 *                          those must be refused and change nothing), every
 *                          fourth round with the internal hash cut to a few
 *                          bits, deletes a runtime now and then, and looks up
 *                          one frame of every length in [0, 80], each in a
 *                          heap block of exactly that size, with random
 *                          verdict bytes of every width in an exactly sized
 *                          block.  A read past either block is a sanitizer
 *                          report.  Every answer is compared with a linear
 *                          search over the entries that were accepted.
 *
 * Exit 0 when every call returned what the rule says; a sanitizer report
 * aborts with non-zero.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"

#define NRT 6       /* runtimes in play; max_runtimes is NRT + 1, with no entries for the last */
#define MAXE 40

static uint64_t rng_state;

static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

static struct gcl_sock_entry model[NRT][MAXE];
static uint32_t model_n[NRT];

static uint32_t pool_ip(void) { return rnd() % 4 ? 0x0A000001u + (uint32_t)(rnd() % 3) : 0; }
static uint16_t pool_port(void) { return (uint16_t)(1 + rnd() % 5); }

/* the answer by linear search (transport.c:370-396) */
static uint32_t linear(uint32_t u, uint8_t proto, uint32_t lip, uint16_t lport, uint32_t rip,
                       uint16_t rport, int *klass)
{
	const struct gcl_sock_entry *e = model[u];

	for (uint32_t i = 0; i < model_n[u]; i++)
		if (e[i].match == GCL_SOCK_MATCH_5TUPLE && e[i].proto == proto && e[i].lip == lip &&
		    e[i].lport == lport && e[i].rip == rip && e[i].rport == rport) {
			*klass = GCL_SOCK_HIT5;
			return e[i].cookie;
		}
	for (int pass = 0; pass < 2; pass++) {
		const uint32_t ip = pass ? 0 : lip;
		uint32_t found = 0, cookie = 0;
		for (uint32_t i = 0; i < model_n[u]; i++)
			if (e[i].match == GCL_SOCK_MATCH_3TUPLE && e[i].proto == proto && e[i].lip == ip &&
			    e[i].lport == lport && !found++)
				cookie = e[i].cookie;
		if (found) {
			*klass = found > 1 ? GCL_SOCK_N_MULTI : pass ? GCL_SOCK_HIT3_ANY : GCL_SOCK_HIT3;
			return found > 1 ? GCL_SOCK_MULTI : cookie;
		}
	}
	*klass = GCL_SOCK_N_MISS;
	return GCL_SOCK_MISS;
}

/* a random set for runtime @u; returns what gcl_sock_tbl_set must answer */
static int random_set(struct gcl_sock_entry *e, uint32_t *n)
{
	int want = 0;

	*n = (uint32_t)(rnd() % MAXE);
	for (uint32_t i = 0; i < *n; i++) {
		e[i].lip = pool_ip();
		e[i].rip = 0xC0A80000u + (uint32_t)(rnd() % 3);
		e[i].lport = pool_port();
		e[i].rport = pool_port();
		e[i].proto = rnd() & 1 ? 6 : 17;
		e[i].match = rnd() % 3 ? GCL_SOCK_MATCH_5TUPLE : GCL_SOCK_MATCH_3TUPLE;
		e[i].pad = (uint16_t)rnd();
		e[i].cookie = (uint32_t)(rnd() % 1000);
	}
	if (*n && rnd() % 4 == 0) { /* one invalid entry */
		struct gcl_sock_entry *b = &e[rnd() % *n];
		switch (rnd() % 4) {
		case 0: b->lport = 0; break;
		case 1: b->match = (uint8_t)(rnd() % 2 ? 4 : 0); break;
		case 2: b->proto = (uint8_t)(rnd() % 2 ? 1 : 0); break;
		default: b->cookie = GCL_SOCK_COOKIE_MAX + 1 + (uint32_t)(rnd() % 16); break;
		}
		want = -EINVAL;
	}
	if (!want)
		for (uint32_t i = 0; i < *n && !want; i++)
			for (uint32_t j = 0; j < i; j++)
				if (e[i].match == GCL_SOCK_MATCH_5TUPLE && e[j].match == GCL_SOCK_MATCH_5TUPLE &&
				    e[i].proto == e[j].proto && e[i].lip == e[j].lip && e[i].lport == e[j].lport &&
				    e[i].rip == e[j].rip && e[i].rport == e[j].rport)
					want = -EADDRINUSE;
	return want;
}

int main(int argc, char **argv)
{
	uint64_t seen[GCL_SOCK_NR] = { 0 }, refused = 0, unplaced = 0;
	static const uint8_t widths[4] = { 8, 4, 2, 1 };

	if (argc < 3) {
		fprintf(stderr, "usage: sock_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);
	struct gcl_sock_tbl *t = gcl_sock_tbl_new();
	if (!t)
		return 3;
	for (uint64_t it = 0; it < iters; it++) {
		if (gcl_sock_tbl_hash_bits(t, it % 4 == 3 ? 1 + (uint32_t)(rnd() % 4) : 32))
			abort();
		for (int s = 0; s < 3; s++) {
			struct gcl_sock_entry e[MAXE];
			uint32_t n;
			const uint32_t u = (uint32_t)(rnd() % NRT);
			if (rnd() % 8 == 0) {
				if (gcl_sock_tbl_del(t, (uint16_t)u))
					abort();
				model_n[u] = 0;
				continue;
			}
			const int want = random_set(e, &n);
			/* exactly sized: a read past the n entries is a report */
			struct gcl_sock_entry *h = n ? malloc(n * sizeof(*h)) : NULL;
			if (n)
				memcpy(h, e, n * sizeof(*h));
			const int got = gcl_sock_tbl_set(t, (uint16_t)u, h, n);
			free(h);
			if (got == -ENOSPC && !want && it % 4 == 3) {
				unplaced++; /* the knob: a clean refusal, the previous set kept */
			} else if (got != want) {
				fprintf(stderr, "set: got %d want %d\n", got, want);
				abort();
			} else if (!got) {
				memcpy(model[u], e, n * sizeof(*e));
				model_n[u] = n;
			} else {
				refused++;
			}
		}
		for (size_t len = 0; len <= 80; len++) {
			uint8_t pad[96] = { 0 };
			uint8_t *frame = malloc(len ? len : 1); /* len bytes are readable */
			const uint8_t vb = widths[rnd() % 4], tb = vb <= 2 ? (uint8_t)(rnd() % 3) : 0;
			uint8_t *verd = malloc(vb);
			uint32_t sock = 0x5A5A5A5A;
			uint64_t cnt[GCL_SOCK_NR] = { 0 }, raw = rnd();

			for (size_t i = 0; i < len; i++)
				pad[i] = (uint8_t)rnd();
			if (rnd() % 8) { /* mostly a frame net_rx_trans would see, from the pools */
				const uint32_t lip = rnd() % 4 ? 0x0A000001u + (uint32_t)(rnd() % 3) : 0;
				const uint32_t rip = 0xC0A80000u + (uint32_t)(rnd() % 3);
				const uint16_t lport = pool_port(), rport = pool_port();
				pad[12] = 0x08, pad[13] = 0x00, pad[14] = 0x45;
				pad[21] &= 0xDF;
				pad[23] = rnd() & 1 ? 6 : 17;
				pad[26] = (uint8_t)(rip >> 24), pad[27] = (uint8_t)(rip >> 16);
				pad[28] = (uint8_t)(rip >> 8), pad[29] = (uint8_t)rip;
				pad[30] = (uint8_t)(lip >> 24), pad[31] = (uint8_t)(lip >> 16);
				pad[32] = (uint8_t)(lip >> 8), pad[33] = (uint8_t)lip;
				pad[34] = (uint8_t)(rport >> 8), pad[35] = (uint8_t)rport;
				pad[36] = (uint8_t)(lport >> 8), pad[37] = (uint8_t)lport;
				if (rnd() % 8 == 0)
					pad[12 + rnd() % 12] ^= (uint8_t)(1u << (rnd() % 8));
			}
			memset(pad + len, 0, sizeof(pad) - len);
			memcpy(frame, pad, len);
			if (rnd() % 4) { /* mostly a verdict that delivers to a runtime in play */
				const uint64_t u = rnd() % (NRT + 2), slot = rnd() & ((1u << tb) - 1);
				raw = vb == 8 ? (u | (rnd() & 0xC1) << 24) << 32 | (uint32_t)rnd() :
				      vb == 4 ? u | (rnd() & 0xC1) << 24 :
				      vb == 2 ? (u << tb | slot) | (rnd() & 1 ? GCL_V2_WAKE : 0) : (u << tb | slot);
			}
			memcpy(verd, &raw, vb);

			/* the rule, written out */
			uint32_t u = 0xFFFFFFFFu, want = GCL_SOCK_NA;
			int klass = GCL_SOCK_N_NA;
			if (vb >= 4) {
				const uint32_t w = vb == 8 ? (uint32_t)(raw >> 32) : (uint32_t)raw;
				if ((w >> 24 & GCL_ACT_MASK) <= GCL_ACT_WAKE)
					u = w & 0xFFFF;
			} else if (vb == 2) {
				const struct gcl_verdict4 w = gcl_verdict2_to4((uint16_t)raw, tb);
				if ((raw & GCL_V2_KIND) != 0x8000 && (w.action & GCL_ACT_MASK) <= GCL_ACT_WAKE)
					u = w.uniqid;
			} else {
				const struct gcl_verdict4 w = gcl_verdict1_to4((uint8_t)raw, tb);
				if ((w.action & GCL_ACT_MASK) <= GCL_ACT_WAKE)
					u = w.uniqid;
			}
			if (u < NRT + 1 && pad[12] == 0x08 && pad[13] == 0x00 && pad[14] == 0x45 &&
			    !(pad[21] & 0x20) && (pad[23] == 6 || pad[23] == 17)) {
				const uint32_t rip = (uint32_t)pad[26] << 24 | pad[27] << 16 | pad[28] << 8 | pad[29];
				const uint32_t lip = (uint32_t)pad[30] << 24 | pad[31] << 16 | pad[32] << 8 | pad[33];
				if (u < NRT) {
					want = linear(u, pad[23], lip, (uint16_t)(pad[36] << 8 | pad[37]), rip,
					              (uint16_t)(pad[34] << 8 | pad[35]), &klass);
				} else {
					want = GCL_SOCK_MISS;
					klass = GCL_SOCK_N_MISS;
				}
			}

			struct gcl_batch b = { .frames = frame, .frames_len = len, .stride = 64, .n = 1 };
			uint64_t off = rnd() % 4 ? 0 : rnd() % 3 ? len + rnd() % 3 : rnd() | 1ull << 40;
			if (off) { /* an offset at or past frames_len: a frame of zeros */
				b.offs = &off;
				want = GCL_SOCK_NA;
				klass = GCL_SOCK_N_NA;
			}
			if (gcl_sock_tbl_lookup_host(t, vb, tb, NRT + 1, &b, verd, &sock, cnt))
				abort();
			if (sock != want || cnt[klass] != 1) {
				fprintf(stderr, "len %zu vb %u raw %#llx: got %#x want %#x (class %d)\n", len, vb,
				        (unsigned long long)raw, sock, want, klass);
				abort();
			}
			seen[klass]++;
			free(frame);
			free(verd);
		}
	}
	gcl_sock_tbl_free(t);
	printf("sock ok");
	for (int j = 0; j <= GCL_SOCK_N_NA; j++)
		printf(" %llu", (unsigned long long)seen[j]);
	printf(" %llu %llu\n", (unsigned long long)refused, (unsigned long long)unplaced);
	return 0;
}
