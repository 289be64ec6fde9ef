/*
 * gcl_sock.c - the socket table on the host (gcl_host.h: gcl_sock_tbl_*): the
 * per-runtime entry sets, their checks (__trans_table_add,
 * runtime/net/transport.c:177-245), the two-choice cuckoo placement that
 * builds the table image (gcl_sock.h), and the lookup of a batch on the CPU
 * with the probe the GPU kernel shares.  Plain C, no HIP.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"
#include "gcl_sock.h"

#define SOCK_SEEDS    16   /* hash seeds tried before a placement counts as failed */
#define SOCK_MAX_KICK 1000 /* evictions one insert may cause */

struct sock_img {
	uint8_t *bytes;
	size_t len;
	struct gcl_sock_view v;
	struct gcl_sock_key *keys; /* the view's arrays, writable */
	uint32_t *cookies;
	uint64_t rng;
};

static int img_alloc(struct sock_img *im, uint32_t log2_buckets, uint32_t seed, uint32_t hash_bits)
{
	struct gcl_sock_img_hdr h = { GCL_SOCK_MAGIC, log2_buckets, seed, hash_bits };

	im->len = gcl_sock_image_bytes(log2_buckets);
	im->bytes = calloc(1, im->len);
	if (!im->bytes)
		return -ENOMEM;
	memcpy(im->bytes, &h, sizeof(h));
	im->v = gcl_sock_view_of(&h, im->bytes);
	im->keys = (struct gcl_sock_key *)im->v.keys;
	im->cookies = (uint32_t *)im->v.cookies;
	im->rng = 0x9E3779B97F4A7C15ull ^ seed;
	return 0;
}

static uint32_t img_rand(struct sock_img *im)
{
	im->rng ^= im->rng << 13;
	im->rng ^= im->rng >> 7;
	im->rng ^= im->rng << 17;
	return (uint32_t)(im->rng >> 32);
}

/* Insert one entry.  A key already there is a conflict for a 5-tuple
 * (-EADDRINUSE) and one more reuse_port listener for a 3-tuple (the slot's
 * cookie becomes GCL_SOCK_MULTI).  A new key takes a free slot of its two
 * buckets, or evicts a random resident, which then moves to its other
 * bucket, and so on (random walk); -ENOSPC after SOCK_MAX_KICK evictions. */
static int img_insert(struct sock_img *im, uint16_t uniqid, const struct gcl_sock_entry *e)
{
	struct gcl_sock_key cur = gcl_sock_make_key(uniqid, e->match, e->proto, e->lip, e->lport,
	                                            e->rip, e->rport);
	uint32_t cookie = e->cookie, from = GCL_SOCK_NO_SLOT, s[2];
	const uint32_t at = gcl_sock_probe(&im->v, &cur);

	if (at != GCL_SOCK_NO_SLOT) {
		if (e->match == GCL_SOCK_MATCH_5TUPLE)
			return -EADDRINUSE;
		im->cookies[at] = GCL_SOCK_MULTI;
		return 0;
	}
	for (int kick = 0; kick <= SOCK_MAX_KICK; kick++) {
		gcl_sock_buckets(&im->v, &cur, s);
		for (int i = 0; i < 4; i++) {
			const uint32_t slot = s[i >> 1] + (i & 1);
			if (!(im->keys[slot].w[3] & GCL_SOCK_K_VALID)) {
				im->keys[slot] = cur;
				im->cookies[slot] = cookie;
				return 0;
			}
		}
		const uint32_t r = img_rand(im);
		uint32_t b = r & 1;
		if (s[b] == from && s[b ^ 1] != from)
			b ^= 1; /* not straight back where it came from */
		const uint32_t slot = s[b] + (r >> 1 & 1);
		const struct gcl_sock_key k2 = im->keys[slot];
		const uint32_t c2 = im->cookies[slot];
		im->keys[slot] = cur;
		im->cookies[slot] = cookie;
		cur = k2;
		cookie = c2;
		from = s[b];
	}
	return -ENOSPC;
}

/* The image of @t's sets with @uniqid's replaced by @e[0..n). */
static int img_build(const struct gcl_sock_tbl *t, uint16_t uniqid, const struct gcl_sock_entry *e,
                     uint32_t n, uint64_t total, struct sock_img *out)
{
	uint32_t lg = 3;
	int ret = 0;

	while (((uint64_t)1 << lg) < total && lg < GCL_SOCK_LOG2_MAX)
		lg++; /* 2 slots per bucket: load <= 1/2 */
	for (uint32_t seed = 0; seed < SOCK_SEEDS; seed++) {
		ret = img_alloc(out, lg, seed, t->hash_bits ? t->hash_bits : 32);
		if (ret)
			return ret;
		for (uint32_t u = 0; u < GCL_MAX_PROC && !ret; u++) {
			const struct gcl_sock_entry *se = u == uniqid ? e : t->set[u];
			const uint32_t sn = u == uniqid ? n : t->cnt[u];
			for (uint32_t i = 0; i < sn && !ret; i++)
				ret = img_insert(out, (uint16_t)u, &se[i]);
		}
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

static int key_cmp(const void *a, const void *b)
{
	return memcmp(a, b, sizeof(struct gcl_sock_key));
}

/* -EADDRINUSE when two 5-tuple entries of @e share their key
 * (__trans_table_add, transport.c:202-214), whatever else is wrong with
 * placing the set */
static int conflict_check(const struct gcl_sock_entry *e, uint32_t n)
{
	struct gcl_sock_key *k = malloc(((size_t)n + 1) * sizeof(*k));
	uint32_t m = 0;
	int ret = 0;

	if (!k)
		return -ENOMEM;
	for (uint32_t i = 0; i < n; i++)
		if (e[i].match == GCL_SOCK_MATCH_5TUPLE)
			k[m++] = gcl_sock_make_key(0, e[i].match, e[i].proto, e[i].lip, e[i].lport, e[i].rip,
			                           e[i].rport);
	qsort(k, m, sizeof(*k), key_cmp);
	for (uint32_t i = 1; i < m && !ret; i++)
		if (gcl_sock_key_eq(&k[i - 1], &k[i]))
			ret = -EADDRINUSE;
	free(k);
	return ret;
}

struct gcl_sock_tbl *gcl_sock_tbl_new(void)
{
	struct gcl_sock_tbl *t = calloc(1, sizeof(*t));
	struct sock_img im;

	if (!t)
		return NULL;
	if (img_build(t, 0, NULL, 0, 0, &im)) {
		free(t);
		return NULL;
	}
	t->image = im.bytes;
	t->image_bytes = im.len;
	t->dirty = 1;
	return t;
}

void gcl_sock_tbl_free(struct gcl_sock_tbl *t)
{
	if (!t)
		return;
	for (uint32_t u = 0; u < GCL_MAX_PROC; u++)
		free(t->set[u]);
	free(t->image);
	free(t);
}

int gcl_sock_tbl_hash_bits(struct gcl_sock_tbl *t, uint32_t bits)
{
	if (!t || bits < 1 || bits > 32)
		return -EINVAL;
	t->hash_bits = bits;
	return 0;
}

int gcl_sock_tbl_set(struct gcl_sock_tbl *t, uint16_t uniqid, const struct gcl_sock_entry *e, uint32_t n)
{
	struct gcl_sock_entry *copy = NULL;
	struct sock_img im;

	if (!t || uniqid >= GCL_MAX_PROC || (n && !e))
		return -EINVAL;
	for (uint32_t i = 0; i < n; i++)
		if (e[i].lport == 0 || (e[i].match != GCL_SOCK_MATCH_3TUPLE && e[i].match != GCL_SOCK_MATCH_5TUPLE) ||
		    (e[i].proto != 6 && e[i].proto != 17) || e[i].cookie > GCL_SOCK_COOKIE_MAX)
			return -EINVAL;
	const uint64_t total = t->total - t->cnt[uniqid] + n;
	if (total > GCL_SOCK_MAX_ENTRIES)
		return -ENOSPC;
	const int dup = conflict_check(e, n);
	if (dup)
		return dup;
	if (n) {
		copy = malloc((size_t)n * sizeof(*e));
		if (!copy)
			return -ENOMEM;
		memcpy(copy, e, (size_t)n * sizeof(*e));
	}
	const int ret = img_build(t, uniqid, copy, n, total, &im);
	if (ret) {
		free(copy);
		return ret;
	}
	free(t->set[uniqid]);
	t->set[uniqid] = copy;
	t->cnt[uniqid] = n;
	t->total = total;
	free(t->image);
	t->image = im.bytes;
	t->image_bytes = im.len;
	t->dirty = 1;
	return 0;
}

/* In place: the slots of @uniqid's keys are emptied, which cannot fail and
 * leaves every other key where a probe finds it. */
int gcl_sock_tbl_del(struct gcl_sock_tbl *t, uint16_t uniqid)
{
	struct gcl_sock_img_hdr h;

	if (!t || uniqid >= GCL_MAX_PROC)
		return -EINVAL;
	if (!t->cnt[uniqid])
		return 0;
	memcpy(&h, t->image, sizeof(h));
	const struct gcl_sock_view v = gcl_sock_view_of(&h, t->image);
	for (uint32_t i = 0; i < t->cnt[uniqid]; i++) {
		const struct gcl_sock_entry *e = &t->set[uniqid][i];
		const struct gcl_sock_key k = gcl_sock_make_key(uniqid, e->match, e->proto, e->lip, e->lport,
		                                                e->rip, e->rport);
		const uint32_t at = gcl_sock_probe(&v, &k);
		if (at != GCL_SOCK_NO_SLOT) { /* a reuse_port listener's slot goes with the first */
			memset((struct gcl_sock_key *)&v.keys[at], 0, sizeof(k));
			((uint32_t *)v.cookies)[at] = 0;
		}
	}
	free(t->set[uniqid]);
	t->set[uniqid] = NULL;
	t->total -= t->cnt[uniqid];
	t->cnt[uniqid] = 0;
	t->dirty = 1;
	return 0;
}

int gcl_sock_tbl_lookup_host(const struct gcl_sock_tbl *t, uint8_t vbytes, uint8_t thread_bits,
                             uint32_t max_runtimes, const struct gcl_batch *b, const void *verdicts,
                             uint32_t *sock, uint64_t *counts)
{
	struct gcl_sock_img_hdr h;
	uint64_t cnt[GCL_SOCK_NR] = { 0 };

	if (!t || !b || !verdicts || !sock || thread_bits > 8 ||
	    (vbytes != 8 && vbytes != 4 && vbytes != 2 && vbytes != 1))
		return -EINVAL;
	if (b->n == 0)
		return 0;
	if (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	    (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))))
		return -EINVAL;
	memcpy(&h, t->image, sizeof(h));
	const struct gcl_sock_view v = gcl_sock_view_of(&h, t->image);
	for (uint64_t i = 0; i < b->n; i++) {
		uint64_t raw = 0, off = i * b->stride;
		uint8_t hb[28] = { 0 };
		uint32_t d[7], klass, res;

		memcpy(&raw, (const uint8_t *)verdicts + i * vbytes, vbytes); /* little-endian host */
		if (b->offs)
			memcpy(&off, (const uint8_t *)b->offs + i * 8, 8);
		/* frame bytes [12, 40), a byte at or past frames_len as 0 */
		if (off < b->frames_len && b->frames_len - off > 12) {
			const uint64_t avail = b->frames_len - off - 12;
			memcpy(hb, b->frames + off + 12, avail < sizeof(hb) ? avail : sizeof(hb));
		}
		for (int j = 0; j < 7; j++)
			d[j] = hb[4 * j] | (uint32_t)hb[4 * j + 1] << 8 | (uint32_t)hb[4 * j + 2] << 16 |
			       (uint32_t)hb[4 * j + 3] << 24;
		res = gcl_sock_rule(&v, gcl_sock_verdict_rt(raw, vbytes, thread_bits, max_runtimes), d, &klass);
		memcpy((uint8_t *)sock + i * 4, &res, 4);
		cnt[klass]++;
	}
	if (counts)
		for (int j = 0; j < GCL_SOCK_NR; j++)
			counts[j] += cnt[j];
	return 0;
}
