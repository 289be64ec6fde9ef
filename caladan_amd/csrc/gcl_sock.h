/*
 * gcl_sock.h - the socket table's image and the lookup of one packet in it,
 * shared by the host table object (gcl_sock.c, plain C) and the GPU kernel
 * (gcl_sock.hip): both include this file, so the CPU tests and the sanitizer
 * driver run the very probe the GPU runs.  Not installed; the ABI is in
 * include/gclassify.h (gcl_sock_set, gcl_sock_lookup) and include/gcl_host.h
 * (the host-only table object).
 *
 * The image: a 16-B header, then the key array (one 16-B key per slot), then
 * the cookie array (one u32 per slot).  Slots come in buckets of two; a key
 * lives in one of the two buckets its hash names (two-choice cuckoo, placed
 * on the host), so one key is found or ruled out by reading exactly four
 * 16-B keys, whatever the table holds.  The cookie of the winning slot is one
 * more 4-B read.  Every index is masked with the bucket mask before use: no
 * image content and no key indexes outside the two arrays.
 *
 * A key is exact: {lip, rip, lport | rport << 16, uniqid | udp << 16 |
 * 5-tuple << 17 | valid << 31}; a 3-tuple key has rip = rport = 0.  An empty
 * slot is all zeros and equals no key (valid is clear).  Several listeners on
 * one 3-tuple share one slot whose cookie is GCL_SOCK_MULTI.
 */
#ifndef GCL_SOCK_H
#define GCL_SOCK_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_SOCK_FN __host__ __device__ static inline
#else
#define GCL_SOCK_FN static inline
#endif

#define GCL_SOCK_MAGIC      0x4B434F53u /* "SOCK" */
#define GCL_SOCK_HDR_BYTES  16u
#define GCL_SOCK_LOG2_MAX   21u         /* buckets: 2 slots each, load <= 1/2 at 2^20 entries */
#define GCL_SOCK_K_UDP      0x00010000u
#define GCL_SOCK_K_5TUPLE   0x00020000u
#define GCL_SOCK_K_VALID    0x80000000u
#define GCL_SOCK_NO_SLOT    0xFFFFFFFFu
#define GCL_SOCK_NO_RT      0xFFFFFFFFu /* the verdict names no runtime: NA */

struct gcl_sock_key {
	uint32_t w[4];
} __attribute__((aligned(16)));

struct gcl_sock_img_hdr {
	uint32_t magic;
	uint32_t log2_buckets; /* <= GCL_SOCK_LOG2_MAX */
	uint32_t seed;
	uint32_t hash_bits;    /* 1..32: bits of the internal hash in use (32 in production) */
};

/* what a lookup needs of an image, with the two arrays at their addresses in
 * the memory the lookup runs in (host, or the device copy) */
struct gcl_sock_view {
	const struct gcl_sock_key *keys;
	const uint32_t *cookies;
	uint32_t mask;   /* buckets - 1 */
	uint32_t seed;
	uint32_t hmask;  /* the hash_bits low bits */
};

GCL_SOCK_FN size_t gcl_sock_image_bytes(uint32_t log2_buckets)
{
	return GCL_SOCK_HDR_BYTES + ((size_t)2 << log2_buckets) * (sizeof(struct gcl_sock_key) + 4);
}

/* The view of the image whose header is @h and whose bytes lie at @base (the
 * header is read on the host; @base may be a device address). */
GCL_SOCK_FN struct gcl_sock_view gcl_sock_view_of(const struct gcl_sock_img_hdr *h, const void *base)
{
	struct gcl_sock_view v;
	const uint32_t lg = h->log2_buckets <= GCL_SOCK_LOG2_MAX ? h->log2_buckets : GCL_SOCK_LOG2_MAX;
	const uint32_t bits = h->hash_bits >= 1 && h->hash_bits < 32 ? h->hash_bits : 32;

	v.keys = (const struct gcl_sock_key *)((const uint8_t *)base + GCL_SOCK_HDR_BYTES);
	v.cookies = (const uint32_t *)((const uint8_t *)base + GCL_SOCK_HDR_BYTES +
	                               ((size_t)2 << lg) * sizeof(struct gcl_sock_key));
	v.mask = (1u << lg) - 1;
	v.seed = h->seed;
	v.hmask = bits == 32 ? 0xFFFFFFFFu : (1u << bits) - 1;
	return v;
}

GCL_SOCK_FN struct gcl_sock_key gcl_sock_make_key(uint32_t uniqid, uint32_t match, uint32_t proto,
                                                  uint32_t lip, uint32_t lport, uint32_t rip,
                                                  uint32_t rport)
{
	struct gcl_sock_key k;
	const int five = match == GCL_SOCK_MATCH_5TUPLE;

	k.w[0] = lip;
	k.w[1] = five ? rip : 0;
	k.w[2] = (lport & 0xFFFFu) | (five ? (rport & 0xFFFFu) << 16 : 0);
	k.w[3] = (uniqid & 0xFFFFu) | (proto == 17 ? GCL_SOCK_K_UDP : 0) |
	         (five ? GCL_SOCK_K_5TUPLE : 0) | GCL_SOCK_K_VALID;
	return k;
}

GCL_SOCK_FN int gcl_sock_key_eq(const struct gcl_sock_key *a, const struct gcl_sock_key *b)
{
	return ((a->w[0] ^ b->w[0]) | (a->w[1] ^ b->w[1]) | (a->w[2] ^ b->w[2]) | (a->w[3] ^ b->w[3])) == 0;
}

GCL_SOCK_FN uint32_t gcl_sock_mix(uint32_t h)
{
	h ^= h >> 16;
	h *= 0x85EBCA6Bu;
	h ^= h >> 13;
	h *= 0xC2B2AE35u;
	h ^= h >> 16;
	return h;
}

/* The first slots of the two buckets of @k (each < 2 * buckets, even). */
GCL_SOCK_FN void gcl_sock_buckets(const struct gcl_sock_view *v, const struct gcl_sock_key *k,
                                  uint32_t s[2])
{
	uint32_t h = v->seed;

	for (int i = 0; i < 4; i++) {
		h = (h ^ k->w[i]) * 0x9E3779B1u;
		h = h << 13 | h >> 19;
	}
	h = gcl_sock_mix(h) & v->hmask;
	s[0] = 2 * (gcl_sock_mix(h ^ 0x5BD1E995u) & v->mask);
	s[1] = 2 * (gcl_sock_mix(h + 0x9E3779B9u) & v->mask);
}

/* The slot that holds @k, or GCL_SOCK_NO_SLOT: four key reads. */
GCL_SOCK_FN uint32_t gcl_sock_probe(const struct gcl_sock_view *v, const struct gcl_sock_key *k)
{
	uint32_t s[2], slot = GCL_SOCK_NO_SLOT;
	struct gcl_sock_key e[4];

	gcl_sock_buckets(v, k, s);
	for (int i = 0; i < 4; i++)
		e[i] = v->keys[s[i >> 1] + (i & 1)];
	for (int i = 0; i < 4; i++)
		if (gcl_sock_key_eq(&e[i], k))
			slot = s[i >> 1] + (i & 1);
	return slot;
}

/*
 * trans_lookup (runtime/net/transport.c:361-397) for a packet of runtime
 * @uniqid: the 5-tuple entry, else the 3-tuple entry of laddr, else the one
 * of (0, laddr.port).  The three keys are known at once, so their twelve key
 * reads are issued together and the winner chosen afterwards; its cookie is
 * the only dependent read.  *@klass gets the GCL_SOCK_* counter slot.
 */
GCL_SOCK_FN uint32_t gcl_sock_resolve(const struct gcl_sock_view *v, uint32_t uniqid, uint32_t proto,
                                      uint32_t lip, uint32_t lport, uint32_t rip, uint32_t rport,
                                      uint32_t *klass)
{
	struct gcl_sock_key k[3], e[3][4];
	uint32_t s[3][2], slot[3];

	k[0] = gcl_sock_make_key(uniqid, GCL_SOCK_MATCH_5TUPLE, proto, lip, lport, rip, rport);
	k[1] = gcl_sock_make_key(uniqid, GCL_SOCK_MATCH_3TUPLE, proto, lip, lport, 0, 0);
	k[2] = gcl_sock_make_key(uniqid, GCL_SOCK_MATCH_3TUPLE, proto, 0, lport, 0, 0);
	for (int j = 0; j < 3; j++)
		gcl_sock_buckets(v, &k[j], s[j]);
	for (int j = 0; j < 3; j++)
		for (int i = 0; i < 4; i++)
			e[j][i] = v->keys[s[j][i >> 1] + (i & 1)];
	for (int j = 0; j < 3; j++) {
		slot[j] = GCL_SOCK_NO_SLOT;
		for (int i = 0; i < 4; i++)
			if (gcl_sock_key_eq(&e[j][i], &k[j]))
				slot[j] = s[j][i >> 1] + (i & 1);
	}
	const uint32_t step = slot[0] != GCL_SOCK_NO_SLOT ? 0 : slot[1] != GCL_SOCK_NO_SLOT ? 1 :
	                      slot[2] != GCL_SOCK_NO_SLOT ? 2 : 3;
	if (step == 3) {
		*klass = GCL_SOCK_N_MISS;
		return GCL_SOCK_MISS;
	}
	/* a found slot is 2 * (masked bucket) + 0 or 1: inside the cookie array */
	const uint32_t cookie = v->cookies[step == 0 ? slot[0] : step == 1 ? slot[1] : slot[2]];
	*klass = step != 0 && cookie == GCL_SOCK_MULTI ? (uint32_t)GCL_SOCK_N_MULTI :
	         step == 0 ? (uint32_t)GCL_SOCK_HIT5 : step == 1 ? (uint32_t)GCL_SOCK_HIT3 :
	                                                           (uint32_t)GCL_SOCK_HIT3_ANY;
	return cookie;
}

/* The runtime a verdict delivers to (DELIVER or WAKE, uniqid < @max_runtimes),
 * or GCL_SOCK_NO_RT.  @raw is the verdict's @vbytes bytes, little endian. */
GCL_SOCK_FN uint32_t gcl_sock_verdict_rt(uint64_t raw, uint32_t vbytes, uint32_t thread_bits,
                                         uint32_t max_runtimes)
{
	uint32_t u = GCL_SOCK_NO_RT;

	if (vbytes == 8 || vbytes == 4) { /* struct gcl_verdict's last four bytes, gcl_verdict4 */
		const uint32_t w = vbytes == 8 ? (uint32_t)(raw >> 32) : (uint32_t)raw;
		const uint32_t act = w >> 24 & GCL_ACT_MASK;
		if (act == GCL_ACT_DELIVER || act == GCL_ACT_WAKE)
			u = w & 0xFFFFu;
	} else if (vbytes == 2) {         /* gcl_verdict2_to4 */
		const uint32_t kind = (uint32_t)raw & GCL_V2_KIND;
		if (kind == GCL_V2_DELIVER || kind == GCL_V2_WAKE)
			u = ((uint32_t)raw & GCL_V2_Q_MASK) >> thread_bits;
	} else if (!(raw & GCL_V1_OTHER)) { /* gcl_verdict1_to4 */
		u = ((uint32_t)raw & GCL_V1_Q_MASK) >> thread_bits;
	}
	return u < max_runtimes ? u : GCL_SOCK_NO_RT;
}

GCL_SOCK_FN uint32_t gcl_sock_bswap32(uint32_t x)
{
	return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}

/*
 * The rule of gcl_sock_lookup for one packet.  @uniqid is gcl_sock_verdict_rt
 * of its verdict; @d are the little-endian dwords of frame bytes [12, 40)
 * (bytes 38-39 are not looked at), bytes at or past frames_len as 0.  The
 * frame predicate is the one that sets GCL_ACT_F_TRANS (classify_core,
 * gcl_kern.h): ethertype 0x0800, version 4, IHL 5, IP_MF (0x2000) clear in
 * the fragment field as the little-endian load sees it (the MF test of
 * ip_hdr_supported as written, runtime/net/core.c:203-209), TCP or UDP.
 */
GCL_SOCK_FN uint32_t gcl_sock_rule(const struct gcl_sock_view *v, uint32_t uniqid, const uint32_t d[7],
                                   uint32_t *klass)
{
	const uint32_t proto = d[2] >> 24;

	if (uniqid == GCL_SOCK_NO_RT || (d[0] & 0xFFFFFFu) != 0x450008u || (d[2] & 0x2000u) ||
	    (proto != 6 && proto != 17)) {
		*klass = GCL_SOCK_N_NA;
		return GCL_SOCK_NA;
	}
	/* transport.c:361-365: laddr = (daddr, dport), raddr = (saddr, sport) */
	const uint32_t rip = gcl_sock_bswap32(d[3] >> 16 | d[4] << 16);   /* bytes 26-29 */
	const uint32_t lip = gcl_sock_bswap32(d[4] >> 16 | d[5] << 16);   /* bytes 30-33 */
	const uint32_t rport = (d[5] >> 8 & 0xFF00u) | d[5] >> 24;         /* bytes 34-35 */
	const uint32_t lport = (d[6] << 8 & 0xFF00u) | (d[6] >> 8 & 0xFFu); /* bytes 36-37 */
	return gcl_sock_resolve(v, uniqid, proto, lip, lport, rip, rport, klass);
}

/* The host table object (gcl_host.h).  The image is rebuilt by every
 * successful gcl_sock_tbl_set and edited in place by gcl_sock_tbl_del. */
struct gcl_sock_tbl {
	struct gcl_sock_entry *set[GCL_MAX_PROC]; /* the entries of each runtime, as given */
	uint32_t cnt[GCL_MAX_PROC];
	uint64_t total;
	uint8_t *image;       /* header | keys | cookies; never NULL */
	size_t image_bytes;
	uint32_t hash_bits;   /* test knob: 1..31 truncate the internal hash; 0 or 32: all of it */
	int dirty;            /* the image changed since a user last cleared this */
};

#endif
