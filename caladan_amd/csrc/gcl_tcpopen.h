/*
 * gcl_tcpopen.h - the rule of gcl_tcp_rx_open (include/gclassify.h) for one
 * list entry, shared by the host twin (gcl_host.c, plain C) and the GPU kernels
 * (gcl_tcpopen.hip): both include this file, so the CPU tests and the
 * sanitizer driver run the very rule the GPU runs.  Not installed.  Plain C
 * without libc.
 *
 * It restates tcp_rx_closed (runtime/net/tcp_in.c:696-723), tcp_rx_listener up
 * to tcp_conn_alloc (:614-656), tcp_parse_options (:298-348) and the option
 * words of tcp_put_options (runtime/net/tcp_out.c:230-251) in the pieces the
 * kernels need apart:
 *
 *   gcl_open_head   the route and everything the header bytes [12, 56) decide:
 *                   a provisional verdict that ignores the backlog and the
 *                   entries before this one, the tuple, and the sequence
 *                   number an RST or a new connection takes from the packet
 *   gcl_open_walk   tcp_parse_options over the 4 * off - 20 option bytes
 *   gcl_open_final  what the backlog and an earlier ACCEPT of the same tuple
 *                   make of the provisional verdict (tcp_queue_recv,
 *                   runtime/net/tcp.c:488-522, and tcp_conn_attach)
 *   gcl_open_record / gcl_open_synack_desc / gcl_open_optwords
 *                   what an ACCEPT writes
 *
 * gcl_open_walk is the one place the call declines to follow the reference:
 * on an option other than EOL or NOP whose length byte is 0, tcp_parse_options
 * does not return (ptr += opsize - 2; len -= opsize makes no progress); the
 * walk stops there and the entry is GCL_OPEN_BADOPT.  A read at or past the
 * end of the option bytes reads 0, where the reference reads whatever follows
 * in the mbuf; the two differ only on malformed options.
 *
 * The walk is pinned to the reference's own tcp_in.c through snd_wscale and the
 * WSCALE bit (tests/test_tcpopen_ref.py); snd_mss is not visible through that
 * driver and rests on the independent model and the hand-derived cases of
 * tests/tcpopencases.py.
 */
#ifndef GCL_TCPOPEN_H
#define GCL_TCPOPEN_H

#include <stdint.h>

#include "../../include/gclassify.h"
#include "gcl_pay.h"
#include "gcl_tcptmr.h"

#if defined(__HIPCC__)
#define GCL_OPEN_FN __host__ __device__ static inline
#else
#define GCL_OPEN_FN static inline
#endif

#define GCL_OPEN_TCP_FIN 0x01u
#define GCL_OPEN_TCP_SYN 0x02u
#define GCL_OPEN_TCP_RST 0x04u
#define GCL_OPEN_TCP_ACK 0x10u
#define GCL_OPEN_MIN_MSS 88u       /* TCP_MIN_MSS, runtime/net/tcp.h:19 */
#define GCL_OPEN_DEFAULT_MSS 1460u /* tcp_calculate_mss(ETH_DEFAULT_MTU) */
#define GCL_OPEN_MAX_OPT 40u       /* 4 * 15 - 20 */
#define GCL_OPEN_NONE 0xFFFFFFFFu  /* no leader, no later_of, no connection record */

/* what the header bytes of one entry decide */
struct gcl_open_ent {
	uint32_t cls;      /* the provisional verdict */
	uint32_t listener; /* listener-route entries */
	uint32_t lip, rip; /* the packet's daddr and saddr */
	uint32_t ports;    /* lport | rport << 16 */
	uint32_t val;      /* rst_seq of an RST; irs of a candidate */
	uint32_t optlen;   /* a candidate's option bytes, <= GCL_OPEN_MAX_OPT */
};

/* tcp_parse_options' results */
struct gcl_open_opts {
	uint32_t opt_en; /* GCL_OPEN_OPT_* that counted */
	uint32_t mss;    /* the last MSS option's value */
	uint32_t wscale; /* the last WSCALE option's, clamped to 14 */
	uint32_t bad;    /* a length byte of 0 */
};

/* the verdicts tcp_queue_recv reaches: the listener route */
GCL_OPEN_FN int gcl_open_listener_route(uint32_t cls)
{
	return cls == GCL_OPEN_DROP || cls == GCL_OPEN_RST || cls == GCL_OPEN_BADOPT || cls == GCL_OPEN_ACCEPT;
}

/* cookie @sock names listener sock - base */
GCL_OPEN_FN int gcl_open_is_listener(uint32_t sock, uint32_t base, uint32_t nlisten)
{
	return sock <= GCL_SOCK_COOKIE_MAX && sock >= base && sock - base < nlisten;
}

/*
 * Packet i < n with @L bytes that exist; @d its frame bytes [12, 56) as eleven
 * little-endian dwords (a byte is used only below L).  Lines 2 to 5c of the
 * rule, the backlog and the entries before this one left aside.
 */
GCL_OPEN_FN struct gcl_open_ent gcl_open_head(const uint32_t d[11], uint64_t L, int has_st, uint32_t st,
                                              uint32_t sock, uint32_t base, uint32_t nlisten)
{
	struct gcl_open_ent e = {GCL_OPEN_NA, 0, 0, 0, 0, 0, 0};
	const int listener = gcl_open_is_listener(sock, base, nlisten);

	if ((sock != GCL_SOCK_MISS && !listener) || L < 34)
		return e;
	const uint32_t frag = GCL_PAY_B(d, 20) << 8 | GCL_PAY_B(d, 21);
	const uint32_t tot = GCL_PAY_B(d, 16) << 8 | GCL_PAY_B(d, 17);

	if (GCL_PAY_B(d, 12) != (GCL_ETHTYPE_IP >> 8) || GCL_PAY_B(d, 13) != (GCL_ETHTYPE_IP & 0xFF) ||
	    GCL_PAY_B(d, 14) != 0x45 || (frag & 0x3FFF) || GCL_PAY_B(d, 23) != 6 || tot < 20 || 14ull + tot > L)
		return e;
	if (has_st && (st & 0xF) == GCL_L4_BAD)
		return e;
	/* mbuf_pull_hdr_or_null, tcp_in.c:627 and :704 */
	if (tot - 20 < 20 || L < 54) {
		e.cls = GCL_OPEN_SHORT;
		return e;
	}
	const uint32_t seq = GCL_PAY_B(d, 38) << 24 | GCL_PAY_B(d, 39) << 16 | GCL_PAY_B(d, 40) << 8 | GCL_PAY_B(d, 41);
	const uint32_t ack = GCL_PAY_B(d, 42) << 24 | GCL_PAY_B(d, 43) << 16 | GCL_PAY_B(d, 44) << 8 | GCL_PAY_B(d, 45);
	const uint32_t hl = 4 * (GCL_PAY_B(d, 46) >> 4), fl = GCL_PAY_B(d, 47);

	e.rip = GCL_PAY_B(d, 26) << 24 | GCL_PAY_B(d, 27) << 16 | GCL_PAY_B(d, 28) << 8 | GCL_PAY_B(d, 29);
	e.lip = GCL_PAY_B(d, 30) << 24 | GCL_PAY_B(d, 31) << 16 | GCL_PAY_B(d, 32) << 8 | GCL_PAY_B(d, 33);
	e.ports = (GCL_PAY_B(d, 36) << 8 | GCL_PAY_B(d, 37)) | (GCL_PAY_B(d, 34) << 8 | GCL_PAY_B(d, 35)) << 16;
	if (!listener) {
		/* tcp_rx_closed, tcp_in.c:708-722 */
		if (fl & GCL_OPEN_TCP_RST) {
			e.cls = GCL_OPEN_CLOSED_DROP;
		} else if (fl & GCL_OPEN_TCP_ACK) {
			e.cls = GCL_OPEN_CLOSED_RST;
			e.val = ack;
		} else {
			e.cls = GCL_OPEN_CLOSED_RST_ACK;
			e.val = seq + (tot - 20 - hl); /* :720, as written: it may wrap */
		}
		return e;
	}
	/* tcp_rx_listener, tcp_in.c:638-656 */
	e.listener = sock - base;
	e.cls = GCL_OPEN_DROP;
	if (fl & GCL_OPEN_TCP_RST)
		return e;
	if (fl & GCL_OPEN_TCP_ACK) {
		e.cls = GCL_OPEN_RST;
		e.val = ack;
		return e;
	}
	if (!(fl & GCL_OPEN_TCP_SYN) || tot - 20 != hl || 34ull + hl > L)
		return e;
	e.cls = GCL_OPEN_ACCEPT;
	e.val = seq;
	e.optlen = hl - 20; /* hl == tot - 20 >= 20, and hl <= 60 */
	return e;
}

/*
 * tcp_parse_options over @optlen <= 40 option bytes, @w their little-endian
 * dwords.  The reference's pointer only moves forward (a length of 1 steps
 * back onto the length byte, which then reads as a NOP), so the walk is one
 * pass over the byte positions with where the next opcode, the pending length
 * byte and the pending values stand; every index into @w is a constant once
 * the loop is unrolled.
 */
GCL_OPEN_FN struct gcl_open_opts gcl_open_walk(const uint32_t w[10], uint32_t optlen)
{
	struct gcl_open_opts r = {0, 0, 0, 0};
	uint32_t next = 0, lenpos = 64, op = 0, mss_at = 64, ws_at = 64;
	int done = 0;

#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (uint32_t p = 0; p < GCL_OPEN_MAX_OPT; p++) {
		const uint32_t b = (w[p >> 2] >> (8 * (p & 3))) & 0xFFu;

		if (p >= optlen) /* len <= 0; a value byte out here reads 0, which mss and wscale already hold */
			done = 1;
		if (done)
			continue;
		if (p == mss_at)
			r.mss |= b << 8;
		if (p == mss_at + 1)
			r.mss |= b;
		if (p == ws_at)
			r.wscale = b > 14 ? 14 : b;
		if (p == lenpos) {
			lenpos = 64;
			if (b == 0) {
				r.bad = 1;
				done = 1;
				continue;
			}
			next = b == 1 ? p + 1 : p - 1 + b;
			if (op == 2 && b == 4) {
				r.opt_en |= GCL_OPEN_OPT_MSS;
				r.mss = 0;
				mss_at = p + 1;
			}
			if (op == 3 && b == 3) {
				r.opt_en |= GCL_OPEN_OPT_WSCALE;
				r.wscale = 0;
				ws_at = p + 1;
			}
		} else if (p == next) {
			if (b == 0) {
				done = 1;
			} else if (b == 1) {
				next = p + 1;
			} else if (p + 1 >= optlen) { /* its length byte lies past the end: it reads 0 */
				r.bad = 1;
				done = 1;
			} else {
				op = b;
				lenpos = p + 1;
			}
		}
	}
	return r;
}

/*
 * Lines 5a, 5b and what is left of a listener-route entry.  @later: an earlier
 * entry with this tuple was accepted; @before: the ACCEPTs of this entry's
 * listener before it cannot be fewer than min(@before, backlog), @before being
 * the first entries of their tuples that reach line 5e before this one.
 */
GCL_OPEN_FN uint32_t gcl_open_final(uint32_t cls, int later, uint32_t lflags, uint32_t backlog, uint32_t before)
{
	if (!gcl_open_listener_route(cls))
		return cls;
	if (later)
		return GCL_OPEN_LATER;
	if ((lflags & GCL_LISTEN_SHUTDOWN) || before >= backlog)
		return GCL_OPEN_FULL;
	return cls;
}

/* struct gcl_tcp_listen as four dwords */
GCL_OPEN_FN uint32_t gcl_open_l_backlog(const uint32_t l[4]) { return l[0]; }
GCL_OPEN_FN uint32_t gcl_open_l_flags(const uint32_t l[4]) { return l[2] >> 24; }

/*
 * struct gcl_tcp_open of an ACCEPT as sixteen dwords: tcp_rx_listener :659-690
 * with tcp_parse_options' tail (:338-346) and tcp_tx_ctl's snd_nxt + 1.
 */
GCL_OPEN_FN void gcl_open_record(const struct gcl_open_ent *e, const struct gcl_open_opts *o, uint32_t j,
                                 uint32_t iss, const uint32_t l[4], uint32_t r[16])
{
	const uint32_t rcv_mss = l[2] & 0xFFFFu;
	uint32_t winmax = l[1], rcv_wscale = (l[2] >> 16) & 0xFFu, snd_mss;

	snd_mss = o->mss > GCL_OPEN_MIN_MSS ? o->mss : GCL_OPEN_MIN_MSS;
	if (snd_mss > rcv_mss)
		snd_mss = rcv_mss;
	if (!(o->opt_en & GCL_OPEN_OPT_WSCALE)) {
		if (winmax > 65535u)
			winmax = 65535u;
		rcv_wscale = 0;
	}
	if (!(o->opt_en & GCL_OPEN_OPT_MSS))
		snd_mss = GCL_OPEN_DEFAULT_MSS;
	r[0] = j;
	r[1] = e->listener;
	r[2] = e->lip;
	r[3] = e->rip;
	r[4] = e->ports;
	r[5] = e->val;
	r[6] = e->val + 1;
	r[7] = iss;
	r[8] = iss;
	r[9] = iss + 1;
	r[10] = winmax; /* rcv_wnd */
	r[11] = winmax;
	r[12] = snd_mss | (o->opt_en & GCL_OPEN_OPT_WSCALE ? o->wscale : 0) << 16 | rcv_wscale << 24;
	r[13] = o->opt_en | GCL_TCP_STATE_SYN_RECEIVED << 8;
	r[14] = 0;
	r[15] = 0;
}

GCL_OPEN_FN uint32_t gcl_open_popcount2(uint32_t opt_en)
{
	return (opt_en & 1u) + ((opt_en >> 1) & 1u);
}

/* the SYN|ACK of record @r: tcp_tx_ctl(TCP_SYN | TCP_ACK) with __tcp_add_tcphdr */
GCL_OPEN_FN void gcl_open_synack_desc(const uint32_t r[16], uint32_t d[8])
{
	const uint32_t opt_en = r[13] & 0xFFu;

	d[0] = r[2];
	d[1] = r[3];
	d[2] = r[4];
	d[3] = 6u | 0x12u << 8 | (5u + gcl_open_popcount2(opt_en)) << 16;
	d[4] = r[7];
	d[5] = r[6];
	d[6] = (r[10] >> ((r[12] >> 24) & 31u)) & 0xFFFFu;
	d[7] = 0;
}

/* tcp_put_options: the option bytes behind the TCP header, WSCALE first; returns how many */
GCL_OPEN_FN uint32_t gcl_open_optbytes(const uint32_t r[16], const uint32_t l[4], uint8_t o[8])
{
	const uint32_t opt_en = r[13] & 0xFFu, rcv_mss = l[2] & 0xFFFFu;
	uint32_t n = 0;

	if (opt_en & GCL_OPEN_OPT_WSCALE) {
		o[n++] = 1;
		o[n++] = 3;
		o[n++] = 3;
		o[n++] = (uint8_t)(r[12] >> 24);
	}
	if (opt_en & GCL_OPEN_OPT_MSS) {
		o[n++] = 2;
		o[n++] = 4;
		o[n++] = (uint8_t)(rcv_mss >> 8);
		o[n++] = (uint8_t)rcv_mss;
	}
	return n;
}

/* the slot a tuple's probe starts at */
GCL_OPEN_FN uint32_t gcl_open_hash(uint32_t lip, uint32_t rip, uint32_t ports, uint32_t listener)
{
	uint32_t h = lip * 0x9E3779B1u;

	h = (h ^ rip) * 0x85EBCA6Bu;
	h = (h ^ ports) * 0xC2B2AE35u;
	h = (h ^ listener) * 0x27D4EB2Fu;
	return h ^ h >> 15;
}

/* the library's choice of in->hash_slots */
GCL_OPEN_FN uint64_t gcl_open_slots(uint64_t m)
{
	uint64_t s = 64;

	while (s < 2 * m)
		s <<= 1;
	return s;
}

/* segments at and past this are not written: seg_cap, and the slots that lie inside the tx region */
GCL_OPEN_FN uint64_t gcl_open_seg_lim(uint64_t seg_cap, uint64_t frame_base, uint32_t frame_stride,
                                      uint64_t tx_frames_len)
{
	const uint64_t fit = frame_base <= tx_frames_len ? (tx_frames_len - frame_base) / frame_stride : 0;

	return seg_cap < fit ? seg_cap : fit;
}

/* what gcl_tcp_rx_open and its host twin both refuse, the ctx and the workspace apart (host code) */
static inline int gcl_open_refused(const struct gcl_batch *b, const struct gcl_tcpopen_in *in,
                                   const struct gcl_tcpopen_out *out, const struct gcl_ctlseg_out *seg,
                                   const uint64_t *counts)
{
	if (!b || !in || !out || !seg || in->size != sizeof(*in) || (!in->order && in->m != b->n) ||
	    in->m > (1ull << 31) || in->nlisten > GCL_OPEN_MAX_LISTEN || in->blocks > GCL_OPEN_MAX_BLOCKS ||
	    (in->hash_slots && ((in->hash_slots & (in->hash_slots - 1)) || in->hash_slots < 2 * in->m)) ||
	    in->seg_cap > (1ull << 31) || in->open_cap > (1ull << 31) || in->frame_stride < GCL_CTL_MIN_STRIDE + 8 ||
	    !seg->totals || !out->totals)
		return 1;
	if (in->nlisten && (!in->listen || !out->backlog_out))
		return 1;
	if (in->m && (!in->sock || !in->iss || !out->verdict || !out->later_of || !out->rst_seq ||
	              (in->open_cap && !out->open) || (in->tx_frames_len && !in->tx_frames) ||
	              (in->seg_cap && (!seg->desc || !seg->frame_off || !seg->seg_conn || !seg->seg_kind ||
	                               !seg->seg_src))))
		return 1;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->listen & 15) ||
	    ((uintptr_t)in->iss & 3) || ((uintptr_t)out->later_of & 3) || ((uintptr_t)out->rst_seq & 3) ||
	    ((uintptr_t)out->open & 15) || ((uintptr_t)out->backlog_out & 3) || ((uintptr_t)out->totals & 7) ||
	    ((uintptr_t)seg->desc & 15) || ((uintptr_t)seg->frame_off & 7) || ((uintptr_t)seg->seg_conn & 3) ||
	    ((uintptr_t)seg->seg_src & 3) || ((uintptr_t)seg->totals & 7) || ((uintptr_t)counts & 7))
		return 1;
	return in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	                 (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	                 !b->pkt_len || ((uintptr_t)b->pkt_len & 1));
}

#endif /* GCL_TCPOPEN_H */
