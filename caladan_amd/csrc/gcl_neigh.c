/*
 * gcl_neigh.c - the neighbour table on the host (gcl_host.h: gcl_neigh_tbl_*):
 * the entry set, its checks, the two-choice cuckoo placement that builds the
 * table image (gcl_neigh.h), and the lookup of one address on the CPU with the
 * probe the GPU kernel shares.  Plain C, no HIP.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"
#include "gcl_neigh.h"

#define NEIGH_SEEDS    16   /* hash seeds tried before a placement counts as failed */
#define NEIGH_MAX_KICK 1000 /* evictions one insert may cause */

struct neigh_img {
	uint8_t *bytes;
	size_t len;
	uint32_t lg, seed, bits;
	struct gcl_neigh_view v;
	struct gcl_neigh_slot *slots; /* the view's array, writable */
	uint64_t rng;
};

static int img_alloc(struct neigh_img *im, uint32_t log2_buckets, uint32_t seed, uint32_t hash_bits)
{
	struct gcl_neigh_img_hdr h = { GCL_NEIGH_MAGIC, log2_buckets, seed, hash_bits };

	im->len = gcl_neigh_image_bytes(log2_buckets);
	im->bytes = calloc(1, im->len);
	if (!im->bytes)
		return -ENOMEM;
	memcpy(im->bytes, &h, sizeof(h));
	im->lg = log2_buckets;
	im->seed = seed;
	im->bits = hash_bits;
	im->v = gcl_neigh_view_of(log2_buckets, seed, hash_bits, im->bytes);
	im->slots = (struct gcl_neigh_slot *)im->v.slots;
	im->rng = 0x9E3779B97F4A7C15ull ^ seed;
	return 0;
}

static uint32_t img_rand(struct neigh_img *im)
{
	im->rng ^= im->rng << 13;
	im->rng ^= im->rng >> 7;
	im->rng ^= im->rng << 17;
	return (uint32_t)(im->rng >> 32);
}

/* Insert one entry whose address is not in the image yet: it takes a free
 * slot of its two buckets, or evicts a random resident, which then moves to
 * its other bucket, and so on (random walk); -ENOSPC after NEIGH_MAX_KICK
 * evictions. */
static int img_insert(struct neigh_img *im, const struct gcl_neigh_entry *e)
{
	struct gcl_neigh_slot cur;
	uint32_t from = GCL_NEIGH_NO_SLOT, s[2];

	cur.w[0] = e->ip;
	cur.w[1] = e->mac[0] | (uint32_t)e->mac[1] << 8 | (uint32_t)e->mac[2] << 16 | (uint32_t)e->mac[3] << 24;
	cur.w[2] = e->mac[4] | (uint32_t)e->mac[5] << 8 | GCL_NEIGH_S_VALID;
	cur.w[3] = 0;
	for (int kick = 0; kick <= NEIGH_MAX_KICK; kick++) {
		gcl_neigh_buckets(&im->v, cur.w[0], s);
		for (int i = 0; i < 4; i++) {
			const uint32_t slot = s[i >> 1] + (i & 1);
			if (!(im->slots[slot].w[2] & GCL_NEIGH_S_VALID)) {
				im->slots[slot] = cur;
				return 0;
			}
		}
		const uint32_t r = img_rand(im);
		uint32_t b = r & 1;
		if (s[b] == from && s[b ^ 1] != from)
			b ^= 1; /* not straight back where it came from */
		const uint32_t slot = s[b] + (r >> 1 & 1);
		const struct gcl_neigh_slot k2 = im->slots[slot];
		im->slots[slot] = cur;
		cur = k2;
		from = s[b];
	}
	return -ENOSPC;
}

static int img_build(uint32_t hash_bits, const struct gcl_neigh_entry *e, uint32_t n, struct neigh_img *out)
{
	uint32_t lg = 3;
	int ret = 0;

	while (((uint32_t)1 << lg) < n && lg < GCL_NEIGH_LOG2_MAX)
		lg++; /* 2 slots per bucket: load <= 1/2 */
	for (uint32_t seed = 0; seed < NEIGH_SEEDS; seed++) {
		ret = img_alloc(out, lg, seed, hash_bits ? hash_bits : 32);
		if (ret)
			return ret;
		for (uint32_t i = 0; i < n && !ret; i++)
			ret = img_insert(out, &e[i]);
		if (ret != -ENOSPC)
			break;
		free(out->bytes);
		out->bytes = NULL;
	}
	if (ret) {
		free(out->bytes);
		out->bytes = NULL;
	}
	return ret;
}

static int ip_cmp(const void *a, const void *b)
{
	const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
	return x < y ? -1 : x > y;
}

/* -EEXIST when two entries of @e share their address */
static int dup_check(const struct gcl_neigh_entry *e, uint32_t n)
{
	uint32_t *k = malloc(((size_t)n + 1) * sizeof(*k));
	int ret = 0;

	if (!k)
		return -ENOMEM;
	for (uint32_t i = 0; i < n; i++)
		k[i] = e[i].ip;
	qsort(k, n, sizeof(*k), ip_cmp);
	for (uint32_t i = 1; i < n && !ret; i++)
		if (k[i - 1] == k[i])
			ret = -EEXIST;
	free(k);
	return ret;
}

static void tbl_take(struct gcl_neigh_tbl *t, struct neigh_img *im)
{
	free(t->image);
	t->image = im->bytes;
	t->image_bytes = im->len;
	t->log2_buckets = im->lg;
	t->seed = im->seed;
	t->img_bits = im->bits;
	t->dirty = 1;
}

struct gcl_neigh_tbl *gcl_neigh_tbl_new(void)
{
	struct gcl_neigh_tbl *t = calloc(1, sizeof(*t));
	struct neigh_img im;

	if (!t)
		return NULL;
	if (img_build(0, NULL, 0, &im)) {
		free(t);
		return NULL;
	}
	tbl_take(t, &im);
	return t;
}

void gcl_neigh_tbl_free(struct gcl_neigh_tbl *t)
{
	if (!t)
		return;
	free(t->set);
	free(t->image);
	free(t);
}

int gcl_neigh_tbl_hash_bits(struct gcl_neigh_tbl *t, uint32_t bits)
{
	if (!t || bits < 1 || bits > 32)
		return -EINVAL;
	t->hash_bits = bits;
	return 0;
}

int gcl_neigh_tbl_set(struct gcl_neigh_tbl *t, const struct gcl_neigh_entry *e, uint32_t n)
{
	struct gcl_neigh_entry *copy = NULL;
	struct neigh_img im;

	if (!t || (n && !e))
		return -EINVAL;
	if (n > GCL_NEIGH_MAX_ENTRIES)
		return -ENOSPC;
	const int dup = dup_check(e, n);
	if (dup)
		return dup;
	if (n) {
		copy = malloc((size_t)n * sizeof(*e));
		if (!copy)
			return -ENOMEM;
		memcpy(copy, e, (size_t)n * sizeof(*e));
	}
	const int ret = img_build(t->hash_bits, copy, n, &im);
	if (ret) {
		free(copy);
		return ret;
	}
	free(t->set);
	t->set = copy;
	t->cnt = n;
	tbl_take(t, &im);
	return 0;
}

uint32_t gcl_neigh_tbl_count(const struct gcl_neigh_tbl *t)
{
	return t ? t->cnt : 0;
}

int gcl_neigh_tbl_lookup(const struct gcl_neigh_tbl *t, uint32_t ip, uint8_t mac[6])
{
	uint32_t m[2];

	if (!t || !mac)
		return -EINVAL;
	const struct gcl_neigh_view v = gcl_neigh_tbl_view(t);
	if (gcl_neigh_probe(&v, ip, m) == GCL_NEIGH_NO_SLOT)
		return 0;
	for (int i = 0; i < 4; i++)
		mac[i] = (uint8_t)(m[0] >> (8 * i));
	mac[4] = (uint8_t)m[1];
	mac[5] = (uint8_t)(m[1] >> 8);
	return 1;
}
