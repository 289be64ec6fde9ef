/*
 * txh_fuzz.c - CPU fuzz driver for gcl_tx_hdr_host and the neighbour table,
 * built with AddressSanitizer + UndefinedBehaviorSanitizer by
 * caladan_amd/build.py (build_sanitized_txh; tests/test_txh_sanitize.py runs
 * it).
 *
 *   txh_fuzz SEED ITERS   ITERS batches of up to 64 segments over a heap tx
 *                         region of exactly frames_len bytes (1..4096; a write
 *                         at or past it is a sanitizer report).  Descriptors
 *                         start plausible and get hostile fields: any proto,
 *                         any tcp_off, paylens up to 65535, offsets near, at
 *                         or far past frames_len (UINT64_MAX too), any cap and
 *                         min_pkt_size.  The neighbour table holds a random
 *                         set under a random hash truncation; in one batch of
 *                         four its image is overwritten with random bytes
 *                         first, which must change answers only, never an
 *                         address: every index is masked.  Every array is a
 *                         heap block of its exact size.
 *
 * Checked besides the sanitizers: the four status counters are the census of
 * status[] and sum to m, LOCAL and BYTES agree with the outputs; a refused
 * entry has all outputs 0; an entry that is not refused lies inside the
 * region with its padding; cmd carries pkt_len and tx_olflags and has its top
 * byte clear; with an intact image the table answers every key it was given
 * and no other.
 */
#include <errno.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../caladan_amd/csrc/gcl_neigh.h"
#include "../../include/gcl_host.h"

#define MAXM 64
#define MAXN 200

static uint64_t rng_state;

static uint64_t rnd(void)
{
	uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, __VA_ARGS__); abort(); } } while (0)

int main(int argc, char **argv)
{
	uint64_t seen[4] = {0};
	uint8_t key[40];

	if (argc < 3) {
		fprintf(stderr, "usage: txh_fuzz SEED ITERS\n");
		return 2;
	}
	rng_state = strtoull(argv[1], NULL, 0);
	const uint64_t iters = strtoull(argv[2], NULL, 0);
	for (int i = 0; i < 40; i++)
		key[i] = (uint8_t)rnd();

	for (uint64_t it = 0; it < iters; it++) {
		const uint64_t flen = it % 7 == 0 ? 1 + rnd() % 80 : 1 + rnd() % 4096;
		const uint64_t m = 1 + rnd() % MAXM;
		const uint32_t nn = (uint32_t)(rnd() % MAXN);
		const bool scribble = it % 4 == 3, use_hash = rnd() & 1, use_counts = rnd() % 4 != 0;
		struct gcl_txh_net net = { .addr = 0x0A000005, .netmask = rnd() & 1 ? 0xFFFFFF00u : 0xFFFF0000u,
		                           .gateway = 0x0A000001, .mac = {2, 0, 0, 0, 0, 5},
		                           .min_pkt_size = rnd() % 3 ? (rnd() & 1 ? 60 : (uint8_t)rnd()) : 0,
		                           .flags = rnd() & 1 };
		struct gcl_neigh_tbl *t = gcl_neigh_tbl_new();
		struct gcl_neigh_entry *ne = malloc((nn ? nn : 1) * sizeof(*ne));
		CHECK(t && ne, "no memory\n");

		for (uint32_t i = 0; i < nn; i++) {
			memset(&ne[i], 0, sizeof(ne[i]));
			ne[i].ip = 0x0A000000u + 2 * i + (i == 0 ? 1 : 0); /* distinct; the gateway first */
			for (int b = 0; b < 6; b++)
				ne[i].mac[b] = rnd() % 3 ? net.mac[b] : (uint8_t)rnd();
		}
		if (rnd() & 1)
			CHECK(gcl_neigh_tbl_hash_bits(t, 1 + rnd() % 32) == 0, "hash_bits\n");
		int ret = gcl_neigh_tbl_set(t, nn ? ne : NULL, nn);
		CHECK(ret == 0 || ret == -ENOSPC, "tbl_set %d\n", ret);
		const uint32_t have = ret == 0 ? nn : 0;
		CHECK(gcl_neigh_tbl_count(t) == have, "count\n");
		for (uint32_t i = 0; i < have; i++) {
			uint8_t mac[6];
			CHECK(gcl_neigh_tbl_lookup(t, ne[i].ip, mac) == 1 && !memcmp(mac, ne[i].mac, 6), "key %u lost\n", i);
			CHECK(gcl_neigh_tbl_lookup(t, ne[i].ip + 0x01000000u, mac) == 0, "ghost key\n");
		}
		if (have > 1) { /* errors keep the set */
			ne[1].ip = ne[0].ip;
			CHECK(gcl_neigh_tbl_set(t, ne, have) == -EEXIST && gcl_neigh_tbl_count(t) == have, "dup\n");
		}
		if (scribble)
			for (size_t i = 0; i < t->image_bytes; i++)
				t->image[i] = (uint8_t)rnd();

		uint8_t *frames = malloc(flen);
		struct gcl_txh_desc *desc = malloc(m * sizeof(*desc));
		uint64_t *offs = malloc(m * 8), *cmd = malloc(m * 8), *pay = malloc(m * 8);
		uint16_t *pl = malloc(m * 2);
		uint8_t *fl = malloc(m), *st = malloc(m);
		uint32_t *hash = use_hash ? malloc(m * 4) : NULL;
		uint64_t counts[GCL_TXHC_NR] = {0}, want[GCL_TXHC_NR] = {0};
		CHECK(frames && desc && offs && cmd && pay && pl && fl && st && (!use_hash || hash), "no memory\n");
		memset(frames, 0xA5, flen);
		for (uint64_t j = 0; j < m; j++) {
			struct gcl_txh_desc *d = &desc[j];
			for (size_t b = 0; b < sizeof(*d); b++)
				((uint8_t *)d)[b] = (uint8_t)rnd();
			if (rnd() % 8)
				d->proto = rnd() & 1 ? 6 : 17;
			if (rnd() % 8)
				d->tcp_off = 5 + rnd() % 11;
			if (rnd() % 16)
				d->paylen = rnd() % 100;
			switch (rnd() % 6) {
			case 0: d->rip = net.addr; break;
			case 1: d->rip = rnd() & 1 ? 0x7F000001u : (uint32_t)rnd(); break;
			default: d->rip = 0x0A000000u + rnd() % (2 * MAXN); break;
			}
			switch (rnd() % 8) {
			case 0: offs[j] = flen - rnd() % (flen < 200 ? flen : 200); break;
			case 1: offs[j] = flen + rnd() % 3; break;
			case 2: offs[j] = rnd() & 1 ? UINT64_MAX - rnd() % 100 : rnd(); break;
			default: offs[j] = rnd() % flen; break;
			}
		}
		struct gcl_txh_in in = { .size = sizeof(in), .desc = desc, .frame_off = offs, .m = m, .frames = frames,
		                         .frames_len = flen, .shm_base = rnd() >> 20,
		                         .cap = rnd() % 3 ? 0 : (uint32_t)(rnd() % 300), .net = net };
		struct gcl_txh_out out = { cmd, pay, pl, fl, hash, st };

		ret = gcl_tx_hdr_host(rnd() % 16 ? t : NULL, key, &in, &out, use_counts ? counts : NULL);
		CHECK(ret == 0, "tx_hdr_host %d\n", ret);
		for (uint64_t j = 0; j < m; j++) {
			CHECK(st[j] <= GCL_TXH_REFUSED, "status %u\n", st[j]);
			want[st[j]]++;
			seen[st[j]]++;
			if (st[j] == GCL_TXH_REFUSED) {
				CHECK(!cmd[j] && !pay[j] && !pl[j] && !fl[j] && (!hash || !hash[j]), "refused entry not zero\n");
				continue;
			}
			CHECK(offs[j] <= flen && pl[j] <= flen - offs[j] && pl[j] >= 42, "frame outside the region\n");
			if (st[j] != GCL_TXH_OK) {
				CHECK(!cmd[j] && !pay[j] && (!hash || !hash[j]), "cmd of an entry that is not sent\n");
				continue;
			}
			CHECK(cmd[j] >> 56 == 0 && (cmd[j] >> 48 & 0xFF) == fl[j] && (cmd[j] >> 32 & 0xFFFF) == pl[j], "cmd\n");
			CHECK(pl[j] >= net.min_pkt_size, "padding\n");
			want[GCL_TXHC_LOCAL] += fl[j] >> 6 & 1;
			want[GCL_TXHC_BYTES] += pl[j];
			CHECK(!hash || (pay[j] >> 48) == (hash[j] & 0xFFFF) || (in.shm_base + offs[j]) >> 48, "payload\n");
		}
		if (use_counts)
			CHECK(!memcmp(counts, want, sizeof(want)), "counts\n");
		in.size--;
		CHECK(gcl_tx_hdr_host(t, key, &in, &out, NULL) == -EINVAL, "size\n");

		free(frames); free(desc); free(offs); free(cmd); free(pay); free(pl); free(fl); free(st); free(hash);
		free(ne);
		gcl_neigh_tbl_free(t);
	}
	printf("txh ok %llu %llu %llu %llu\n", (unsigned long long)seen[0], (unsigned long long)seen[1],
	       (unsigned long long)seen[2], (unsigned long long)seen[3]);
	return 0;
}
