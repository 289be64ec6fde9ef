/*
 * gcl_seg.h - the rule of gcl_tx_seg (include/gclassify.h), shared by the host
 * twin (gcl_host.c, plain C) and the GPU kernels (gcl_seg.hip): both include
 * this file, so the CPU tests and the sanitizer driver run the very rule the
 * GPU runs.  Not installed.
 *
 * A write is given as the twelve little-endian dwords of its struct
 * gcl_seg_send.  gcl_seg_rule is the per-write half: refused or not, L, the
 * segment count and the bytes the write's frames take in the layout.
 * gcl_seg_emit is the per-(write, k) half: the descriptor and the offsets of
 * segment k.  It needs no division and no segment count: paylen and the push
 * bit follow from L - k * mss alone, so the expansion recomputes nothing of
 * the per-write half.
 *
 * Sums.  A write has fewer than 2^32 segments and m <= 2^31, so a sum of
 * segment counts stays below 2^63.  A write's layout bytes are at most
 * GCL_SEG_WB_MAX (2^32 frames of at most 2^20 bytes); sums of them are formed
 * with gcl_seg_sat, which stops at GCL_SEG_SAT = 2^62 and cannot wrap.  A write
 * that is OK lies below seg_cap <= 2^31 segments, so its byte offsets are below
 * 2^51 and exact; a saturated sum belongs to a write that the segment test
 * alone already makes NOSPACE.
 */
#ifndef GCL_SEG_H
#define GCL_SEG_H

#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_SEG_FN __host__ __device__ static inline
#else
#define GCL_SEG_FN static inline
#endif

#define GCL_SEG_SAT      (1ull << 62)
#define GCL_SEG_WB_MAX   (1ull << 52)
#define GCL_SEG_MAX_STRIDE (1u << 20)
#define GCL_SEG_MAX_LEAD 65535u
#define GCL_SEG_MAX_UDP  65507u /* 65535 - 20 - 8 */
#define GCL_SEG_TCP_ACK  0x10u  /* TCP_ACK, TCP_PUSH (inc/net/tcp.h) */
#define GCL_SEG_TCP_PUSH 0x08u
#define GCL_SEG_ST_TCP   0x80u  /* the kernels' provisional status: OK | this for a TCP write */

/* the per-write half */
struct gcl_seg_plan {
	uint32_t status; /* GCL_SEG_OK or GCL_SEG_REFUSED: NOSPACE is the scan's */
	uint32_t tcp;
	uint32_t L;      /* min(len, winlen), or len for UDP; 0 when refused */
	uint32_t nseg;   /* 0 when refused */
	uint64_t wbytes; /* stride != 0: nseg * stride; packed: the padded frames; 0 when refused */
};

/* a + b for a, b <= GCL_SEG_SAT, stopping there */
GCL_SEG_FN uint64_t gcl_seg_sat(uint64_t a, uint64_t b)
{
	return a + b < GCL_SEG_SAT ? a + b : GCL_SEG_SAT;
}

/* a frame of @paylen bytes behind @hl header bytes as the packed layout holds it */
GCL_SEG_FN uint64_t gcl_seg_pad(uint32_t hl, uint32_t paylen)
{
	return (34ull + hl + paylen + 15) & ~15ull;
}

/*
 * The bytes the layout may take behind frame_base + lead, from frames_len (0:
 * no limit).  In both layouts a write is NOSPACE when the layout bytes of the
 * non-refused writes up to and including it exceed this.
 */
GCL_SEG_FN uint64_t gcl_seg_byte_cap(uint64_t frames_len, uint64_t frame_base, uint32_t stride, uint32_t lead)
{
	if (!frames_len)
		return UINT64_MAX;
	if (frames_len < frame_base)
		return 0;
	const uint64_t room = frames_len - frame_base;
	if (stride) /* whole slots; a slot holds its lead */
		return room;
	return room < lead ? 0 : room - lead;
}

GCL_SEG_FN struct gcl_seg_plan gcl_seg_rule(const uint32_t s[12], uint32_t udp_max, uint32_t stride,
                                            uint32_t lead)
{
	struct gcl_seg_plan p = {GCL_SEG_REFUSED, 0, 0, 0, 0};
	const uint32_t proto = s[3] & 0xFFu, mss = s[3] >> 16, len = s[7], winlen = s[8];
	uint32_t L, nseg, full, last, hl;

	if (proto == 6) {
		if (mss == 0)
			return p;
		L = len < winlen ? len : winlen;                   /* tcp.c:1374 */
		nseg = L ? L / mss + (L % mss != 0) : 1;           /* the do ... while runs once for L == 0 */
		full = L < mss ? L : mss;
		last = L - (nseg - 1) * mss;
		hl = 20;
		p.tcp = 1;
	} else if (proto == 17) {
		if (len > udp_max)                                 /* udp.c:590 */
			return p;
		L = full = last = len;
		nseg = 1;
		hl = 8;
	} else {
		return p;
	}
	if (stride && (uint64_t)lead + 34 + hl + full > stride)
		return p;
	p.status = GCL_SEG_OK;
	p.L = L;
	p.nseg = nseg;
	p.wbytes = stride ? (uint64_t)nseg * stride : (uint64_t)(nseg - 1) * gcl_seg_pad(hl, full) + gcl_seg_pad(hl, last);
	return p;
}

/* segment @k of a write that was not refused */
struct gcl_seg_one {
	uint32_t d[8];      /* struct gcl_txh_desc as eight dwords */
	uint64_t frame_off, src_off, dst_off;
	uint32_t paylen;
};

/*
 * @first_byte: frame_base + lead + the layout bytes of the non-refused writes
 * before this one (mod 2^64).  k < nseg of the write, so k * mss < max(L, 1).
 */
GCL_SEG_FN struct gcl_seg_one gcl_seg_emit(const uint32_t s[12], uint32_t k, uint64_t first_byte, uint32_t stride)
{
	struct gcl_seg_one r;
	const uint32_t tcp = (s[3] & 0xFFu) == 6, mss = s[3] >> 16;
	const uint32_t hl = tcp ? 20 : 8;
	const uint32_t L = tcp ? (s[7] < s[8] ? s[7] : s[8]) : s[7];
	const uint32_t done = tcp ? k * mss : 0;          /* bytes in the segments before: < max(L, 1) */
	const uint32_t rest = L - done;
	const uint32_t full = tcp ? mss : L;
	const uint32_t paylen = rest < full ? rest : full;
	const uint32_t flags = tcp ? GCL_SEG_TCP_ACK | (rest <= full ? GCL_SEG_TCP_PUSH : 0) : 0;

	r.d[0] = s[0];
	r.d[1] = s[1];
	r.d[2] = s[2];
	r.d[3] = (tcp ? 6u : 17u) | flags << 8 | (tcp ? 5u << 16 : 0) | (s[3] >> 8 & 0xFFu) << 24;
	r.d[4] = tcp ? s[4] + done : 0;
	r.d[5] = tcp ? s[5] : 0;
	r.d[6] = (tcp ? s[6] & 0xFFFFu : 0) | paylen << 16;
	r.d[7] = 0;
	r.paylen = paylen;
	r.frame_off = first_byte + (uint64_t)k * (stride ? stride : gcl_seg_pad(hl, full));
	r.dst_off = r.frame_off + 34 + hl;
	r.src_off = ((uint64_t)s[11] << 32 | s[10]) + done;
	return r;
}

#endif /* GCL_SEG_H */
