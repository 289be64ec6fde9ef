/*
 * gcl_neigh.h - the neighbour table's image and the lookup of one address in
 * it, shared by the host table object (gcl_neigh.c, plain C), the host twin of
 * gcl_tx_hdr (gcl_host.c) and the GPU kernel (gcl_txhdr.hip): all include this
 * file, so the CPU tests and the sanitizer driver run the very probe the GPU
 * runs.  Not installed; the ABI is in include/gclassify.h (gcl_neigh_set,
 * gcl_tx_hdr) and include/gcl_host.h (the host-only table object).
 *
 * The table is a context's ARP cache: the arp_entry records whose state is
 * not ARP_STATE_PROBING (runtime/net/arp.c:331-344), an address and the mac
 * that answers for it.
 *
 * The image: a 16-B header, then the slot array, one 16-B slot {ip, mac,
 * valid} per entry.  Slots come in buckets of two; an address lives in one of
 * the two buckets its hash names (two-choice cuckoo, placed on the host), so
 * an address is found or ruled out by reading exactly four 16-B slots,
 * whatever the table holds.  The hash is the library's own.  Every index is
 * masked with the bucket mask before use, and the mask comes from the table
 * object (the context), never from the image: no image content and no address
 * indexes outside the slot array.  An empty slot is all zeros and equals no
 * address (valid is clear).
 */
#ifndef GCL_NEIGH_H
#define GCL_NEIGH_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_NEIGH_FN __host__ __device__ static inline
#else
#define GCL_NEIGH_FN static inline
#endif

#define GCL_NEIGH_MAGIC     0x4847494Eu /* "NIGH" */
#define GCL_NEIGH_HDR_BYTES 16u
#define GCL_NEIGH_LOG2_MAX  16u         /* buckets: 2 slots each, load <= 1/2 at 2^16 entries */
#define GCL_NEIGH_S_VALID   0x80000000u
#define GCL_NEIGH_NO_SLOT   0xFFFFFFFFu

/* w[0] = ip (host order); w[1] = mac bytes 0-3, little endian; w[2] = mac
 * bytes 4-5 | GCL_NEIGH_S_VALID; w[3] = 0 */
struct gcl_neigh_slot {
	uint32_t w[4];
} __attribute__((aligned(16)));

struct gcl_neigh_img_hdr {
	uint32_t magic;
	uint32_t log2_buckets; /* <= GCL_NEIGH_LOG2_MAX */
	uint32_t seed;
	uint32_t hash_bits;    /* 1..32: bits of the internal hash in use (32 in production) */
};

/* what a lookup needs of an image, the slot array at its address in the
 * memory the lookup runs in (host, or the device copy) */
struct gcl_neigh_view {
	const struct gcl_neigh_slot *slots;
	uint32_t mask;   /* buckets - 1 */
	uint32_t seed;
	uint32_t hmask;  /* the hash_bits low bits */
};

GCL_NEIGH_FN size_t gcl_neigh_image_bytes(uint32_t log2_buckets)
{
	return GCL_NEIGH_HDR_BYTES + ((size_t)2 << log2_buckets) * sizeof(struct gcl_neigh_slot);
}

/* The view of the image of 2^@log2_buckets buckets whose bytes lie at @base
 * (which may be a device address).  The three numbers are the owner's record
 * of what it built, not the image's header. */
GCL_NEIGH_FN struct gcl_neigh_view gcl_neigh_view_of(uint32_t log2_buckets, uint32_t seed,
                                                     uint32_t hash_bits, const void *base)
{
	struct gcl_neigh_view v;
	const uint32_t lg = log2_buckets <= GCL_NEIGH_LOG2_MAX ? log2_buckets : GCL_NEIGH_LOG2_MAX;
	const uint32_t bits = hash_bits >= 1 && hash_bits < 32 ? hash_bits : 32;

	v.slots = (const struct gcl_neigh_slot *)((const uint8_t *)base + GCL_NEIGH_HDR_BYTES);
	v.mask = (1u << lg) - 1;
	v.seed = seed;
	v.hmask = bits == 32 ? 0xFFFFFFFFu : (1u << bits) - 1;
	return v;
}

GCL_NEIGH_FN uint32_t gcl_neigh_mix(uint32_t h)
{
	h ^= h >> 16;
	h *= 0x85EBCA6Bu;
	h ^= h >> 13;
	h *= 0xC2B2AE35u;
	h ^= h >> 16;
	return h;
}

/* The first slots of the two buckets of @ip (each < 2 * buckets, even). */
GCL_NEIGH_FN void gcl_neigh_buckets(const struct gcl_neigh_view *v, uint32_t ip, uint32_t s[2])
{
	const uint32_t h = gcl_neigh_mix((v->seed ^ ip) * 0x9E3779B1u + 0x7F4A7C15u) & v->hmask;

	s[0] = 2 * (gcl_neigh_mix(h ^ 0x5BD1E995u) & v->mask);
	s[1] = 2 * (gcl_neigh_mix(h + 0x9E3779B9u) & v->mask);
}

/* The slot that holds @ip, or GCL_NEIGH_NO_SLOT: four slot reads.  On a hit
 * @mac gets the mac: bytes 0-3 little endian, then bytes 4-5. */
GCL_NEIGH_FN uint32_t gcl_neigh_probe(const struct gcl_neigh_view *v, uint32_t ip, uint32_t mac[2])
{
	uint32_t s[2], slot = GCL_NEIGH_NO_SLOT;
	struct gcl_neigh_slot e[4];

	gcl_neigh_buckets(v, ip, s);
	for (int i = 0; i < 4; i++)
		e[i] = v->slots[s[i >> 1] + (i & 1)];
	mac[0] = mac[1] = 0;
	for (int i = 0; i < 4; i++)
		if (e[i].w[0] == ip && (e[i].w[2] & GCL_NEIGH_S_VALID)) {
			slot = s[i >> 1] + (i & 1);
			mac[0] = e[i].w[1];
			mac[1] = e[i].w[2] & 0xFFFFu;
		}
	return slot;
}

/* The host table object (gcl_host.h).  The image is rebuilt by every
 * successful gcl_neigh_tbl_set. */
struct gcl_neigh_tbl {
	struct gcl_neigh_entry *set; /* the entries, as given */
	uint32_t cnt;
	uint8_t *image;        /* header | slots; never NULL */
	size_t image_bytes;
	uint32_t log2_buckets; /* of the image */
	uint32_t seed;         /* of the image */
	uint32_t img_bits;     /* hash bits the image was built with */
	uint32_t hash_bits;    /* test knob for the next set: 1..31 truncate the hash; 0 or 32: all of it */
	int dirty;             /* the image changed since a user last cleared this */
};

GCL_NEIGH_FN struct gcl_neigh_view gcl_neigh_tbl_view(const struct gcl_neigh_tbl *t)
{
	return gcl_neigh_view_of(t->log2_buckets, t->seed, t->img_bits, t->image);
}

#endif /* GCL_NEIGH_H */
