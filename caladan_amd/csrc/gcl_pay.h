/*
 * gcl_pay.h - the rule of gcl_l4_payload (include/gclassify.h) for one list
 * entry, shared by the host twin (gcl_host.c, plain C) and the GPU kernel
 * (gcl_payload.hip): both include this file, so the CPU tests and the
 * sanitizer driver run the very rule the GPU runs.  Not installed.
 *
 * The rule reads frame bytes [12, 48) only, given as nine little-endian
 * dwords (dword k holds bytes 12 + 4 k .. 15 + 4 k), and uses a byte only
 * when it lies below L: the header bytes [12, 38) after L >= 34 and
 * 14 + tot <= L with tot >= 28 have been seen, the TCP bytes [38, 48) only for
 * a TCP packet, whose tot >= 40 puts L at 54 or more.
 */
#ifndef GCL_PAY_H
#define GCL_PAY_H

#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_PAY_FN __host__ __device__ static inline
#else
#define GCL_PAY_FN static inline
#endif

#define GCL_PAY_KINDS 6u /* GCL_PAY_NA .. GCL_PAY_OOR */

/* what one entry gets: the three per-entry outputs and the meta record */
struct gcl_pay_desc {
	uint64_t src_off;
	uint32_t len;
	uint32_t kind;
	uint32_t meta[4]; /* struct gcl_pay_meta as four dwords */
};

/* frame byte @k, 12 <= k < 48 */
#define GCL_PAY_B(d, k) (((d)[((k) - 12) >> 2] >> (8 * (((k) - 12) & 3))) & 0xFFu)

/* align: 0 or 1 = dense, else a power of two <= 256 */
GCL_PAY_FN int gcl_pay_align_ok(uint32_t align)
{
	return align <= 256 && !(align & (align - 1));
}

/* @len rounded up to the alignment whose mask (align - 1, 0 for dense) is @amask */
GCL_PAY_FN uint32_t gcl_pay_pad(uint32_t len, uint32_t amask)
{
	return (len + amask) & ~amask;
}

/* index of kind's counter in counts[] */
GCL_PAY_FN uint32_t gcl_pay_counter(uint32_t kind)
{
	return kind == GCL_PAY_UDP ? GCL_PAYC_UDP : kind == GCL_PAY_TCP ? GCL_PAYC_TCP :
	       kind == GCL_PAY_NOSOCK ? GCL_PAYC_NOSOCK : kind == GCL_PAY_BADCSUM ? GCL_PAYC_BADCSUM :
	       kind == GCL_PAY_OOR ? GCL_PAYC_OOR : GCL_PAYC_NA;
}

/*
 * Packet i < n at clamped offset @o with @L bytes that exist; @d its frame
 * bytes [12, 48) (bytes that do not exist may hold anything: none is used).
 * @st / @sock are l4_status[i] / sock[i], looked at when @has_st / @has_sock.
 */
GCL_PAY_FN struct gcl_pay_desc gcl_pay_rule(const uint32_t d[9], uint64_t o, uint64_t L, int has_st,
                                            uint32_t st, int has_sock, uint32_t sock)
{
	struct gcl_pay_desc r = {0, 0, GCL_PAY_NA, {0, 0, 0, 0}};

	if (L < 34)
		return r;
	const uint32_t frag = GCL_PAY_B(d, 20) << 8 | GCL_PAY_B(d, 21);
	const uint32_t proto = GCL_PAY_B(d, 23);
	const uint32_t tot = GCL_PAY_B(d, 16) << 8 | GCL_PAY_B(d, 17);
	const int tcp = proto == 6;

	if (GCL_PAY_B(d, 12) != (GCL_ETHTYPE_IP >> 8) || GCL_PAY_B(d, 13) != (GCL_ETHTYPE_IP & 0xFF) ||
	    GCL_PAY_B(d, 14) != 0x45 || (frag & 0x3FFF) || (proto != 6 && proto != 17) ||
	    tot < 20u + (tcp ? 20u : 8u) || 14ull + tot > L)
		return r;
	const uint32_t hl = tcp ? 4 * (GCL_PAY_B(d, 46) >> 4) : 8;
	if (tcp && (hl < 20 || hl > tot - 20))
		return r;
	if (has_st && (st & 0xF) == GCL_L4_BAD) {
		r.kind = GCL_PAY_BADCSUM;
		return r;
	}
	if (has_sock && sock > GCL_SOCK_COOKIE_MAX) {
		r.kind = GCL_PAY_NOSOCK;
		return r;
	}
	r.kind = tcp ? GCL_PAY_TCP : GCL_PAY_UDP;
	r.len = tot - 20 - hl;
	r.src_off = o + 34 + hl;
	r.meta[0] = GCL_PAY_B(d, 26) << 24 | GCL_PAY_B(d, 27) << 16 | GCL_PAY_B(d, 28) << 8 | GCL_PAY_B(d, 29);
	r.meta[1] = GCL_PAY_B(d, 34) << 8 | GCL_PAY_B(d, 35) | proto << 16 |
	            (tcp ? GCL_PAY_B(d, 47) << 24 : 0);
	if (tcp) {
		r.meta[2] = GCL_PAY_B(d, 38) << 24 | GCL_PAY_B(d, 39) << 16 | GCL_PAY_B(d, 40) << 8 |
		            GCL_PAY_B(d, 41);
		r.meta[3] = GCL_PAY_B(d, 42) << 24 | GCL_PAY_B(d, 43) << 16 | GCL_PAY_B(d, 44) << 8 |
		            GCL_PAY_B(d, 45);
	}
	return r;
}

#endif /* GCL_PAY_H */
