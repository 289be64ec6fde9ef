/*
 * gcl_tcprx.h - the rule of gcl_tcp_rx (include/gclassify.h), shared by the
 * host twin (gcl_host.c, plain C) and the GPU kernels (gcl_tcprx.hip): both
 * include this file, so the CPU tests and the sanitizer driver run the very
 * rule the GPU runs.  Not installed.
 *
 * It restates tcp_rx_conn's fast path (runtime/net/tcp_in.c:197-296) in the
 * pieces the kernels need apart: the slow_path terms that depend on nothing
 * that moves inside a call (gcl_tcprx_slow_fixed), the two receive-window
 * terms, which along a chain of FAST segments are a prefix sum of len
 * (gcl_tcprx_slow_rcv), the send-window term and the ack / window / delayed
 * ACK steps, which are carried serially (gcl_tcprx_snd_full,
 * gcl_tcprx_ack_step, gcl_tcprx_rx_step).  gcl_tcprx_one is the whole rule for
 * one segment, composed of exactly those pieces.
 */
#ifndef GCL_TCPRX_H
#define GCL_TCPRX_H

#include <stdint.h>

#include "../../include/gclassify.h"
#include "gcl_pay.h"

#if defined(__HIPCC__)
#define GCL_TCPRX_FN __host__ __device__ static inline
#else
#define GCL_TCPRX_FN static inline
#endif

#define GCL_TCPRX_FIN 0x01u
#define GCL_TCPRX_RST 0x04u
#define GCL_TCPRX_PSH 0x08u
#define GCL_TCPRX_URG 0x20u
#define GCL_TCPRX_SLOWPATH_FLAGS (GCL_TCPRX_FIN | GCL_TCPRX_RST | GCL_TCPRX_URG)
#define GCL_TCPRX_NONE 0xFFFFFFFFu /* first_slow of a connection that did not stop; no cookie */

/* inc/base/stddef.h:144-178 */
GCL_TCPRX_FN int gcl_tcprx_wraps_lt(uint32_t a, uint32_t b)
{
	return (int32_t)(a - b) < 0;
}
GCL_TCPRX_FN int gcl_tcprx_wraps_lte(uint32_t a, uint32_t b)
{
	return (int32_t)(a - b) <= 0;
}
GCL_TCPRX_FN int gcl_tcprx_wraps_gt(uint32_t a, uint32_t b)
{
	return (int32_t)(b - a) < 0;
}

/* a connection's region: fast_bytes is any u32, so the padded length is 64-bit */
GCL_TCPRX_FN uint64_t gcl_tcprx_pad(uint32_t bytes, uint32_t amask)
{
	return ((uint64_t)bytes + amask) & ~(uint64_t)amask;
}

/* what the call reads of one segment: frame bytes 38-41, 42-45, 47, 48-49 and gcl_pay_rule's len */
struct gcl_tcprx_seg {
	uint32_t seq, ack;
	uint32_t win;   /* the 16 bits of the header, not shifted */
	uint32_t len;
	uint32_t flags;
};

/* the words of a connection that move during a call */
struct gcl_tcprx_live {
	uint32_t snd_una, snd_wnd, snd_wl1, snd_wl2, rcv_nxt, rcv_wnd;
	uint32_t cnt;    /* acks_delayed_cnt */
	uint32_t flags;  /* GCL_TCPC_RXQ, GCL_TCPC_ACK_DELAYED, GCL_TCPO_* */
};

/* frame bytes 38.. of a kept TCP entry, out of the dwords of bytes [12, 52) */
GCL_TCPRX_FN struct gcl_tcprx_seg gcl_tcprx_parse(const uint32_t d[10], uint32_t len)
{
	struct gcl_tcprx_seg s;

	s.seq = GCL_PAY_B(d, 38) << 24 | GCL_PAY_B(d, 39) << 16 | GCL_PAY_B(d, 40) << 8 | GCL_PAY_B(d, 41);
	s.ack = GCL_PAY_B(d, 42) << 24 | GCL_PAY_B(d, 43) << 16 | GCL_PAY_B(d, 44) << 8 | GCL_PAY_B(d, 45);
	s.flags = GCL_PAY_B(d, 47);
	s.win = GCL_PAY_B(d, 48) << 8 | GCL_PAY_B(d, 49);
	s.len = len;
	return s;
}

GCL_TCPRX_FN struct gcl_tcprx_live gcl_tcprx_live_of(const struct gcl_tcp_conn *c)
{
	struct gcl_tcprx_live l;

	l.snd_una = c->snd_una;
	l.snd_wnd = c->snd_wnd;
	l.snd_wl1 = c->snd_wl1;
	l.snd_wl2 = c->snd_wl2;
	l.rcv_nxt = c->rcv_nxt;
	l.rcv_wnd = c->rcv_wnd;
	l.cnt = c->acks_delayed_cnt;
	l.flags = c->flags & (GCL_TCPC_RXQ | GCL_TCPC_ACK_DELAYED);
	return l;
}

/* tcp_in.c:221-222, :227, :233 (the rxq_ooo half), :239: the terms nothing in a call moves */
GCL_TCPRX_FN int gcl_tcprx_slow_fixed(uint32_t flags, uint32_t len, uint32_t ack, uint32_t snd_nxt,
                                      uint32_t cflags)
{
	return (flags & GCL_TCPRX_SLOWPATH_FLAGS) != 0 || len == 0 || gcl_tcprx_wraps_gt(ack, snd_nxt) ||
	       !(cflags & GCL_TCPC_ELIGIBLE);
}

/* tcp_in.c:230, tcp.h:224: tcp_is_snd_full */
GCL_TCPRX_FN int gcl_tcprx_snd_full(uint32_t snd_una, uint32_t snd_wnd, uint32_t snd_nxt)
{
	return gcl_tcprx_wraps_lte(snd_una + snd_wnd, snd_nxt);
}

/* tcp_in.c:233 (the seq half), :236 */
GCL_TCPRX_FN int gcl_tcprx_slow_rcv(uint32_t seq, uint32_t len, uint32_t rcv_nxt, uint32_t rcv_wnd)
{
	return seq != rcv_nxt || rcv_wnd < len;
}

/* tcp_in.c:246-264 for a FAST segment; @win is already shifted.  Returns ACKED | WND. */
GCL_TCPRX_FN uint32_t gcl_tcprx_ack_step(struct gcl_tcprx_live *l, uint32_t seq, uint32_t ack, uint32_t win)
{
	uint32_t sf = 0;

	if (gcl_tcprx_wraps_lte(l->snd_una, ack)) {
		if (l->snd_una != ack) {
			l->snd_una = ack;
			sf |= GCL_TCPRX_SF_ACKED;
		}
		if (gcl_tcprx_wraps_lt(l->snd_wl1, seq) ||
		    (l->snd_wl1 == seq && gcl_tcprx_wraps_lte(l->snd_wl2, ack))) {
			l->snd_wnd = win;
			l->snd_wl1 = seq;
			l->snd_wl2 = ack;
			sf |= GCL_TCPRX_SF_WND;
		}
	}
	if (sf)
		l->flags |= GCL_TCPO_REP_ACKS_RESET;
	return sf;
}

/* tcp_in.c:266-287 for a FAST segment.  Returns WAKE | ACK_NOW. */
GCL_TCPRX_FN uint32_t gcl_tcprx_rx_step(struct gcl_tcprx_live *l, uint32_t len, uint32_t flags)
{
	uint32_t sf = 0;

	l->rcv_nxt += len;
	l->rcv_wnd -= len;
	if ((l->flags & GCL_TCPC_RXQ) || (flags & GCL_TCPRX_PSH)) {
		sf |= GCL_TCPRX_SF_WAKE;
		l->flags |= GCL_TCPO_WOKEN;
	}
	if (l->cnt + 1 >= 2) {
		l->flags &= ~(uint32_t)GCL_TCPC_ACK_DELAYED;
		sf |= GCL_TCPRX_SF_ACK_NOW;
		l->cnt = 0;
	} else {
		l->cnt = l->cnt + 1;
		if (!(l->flags & GCL_TCPC_ACK_DELAYED))
			l->flags |= GCL_TCPC_ACK_DELAYED | GCL_TCPO_TIMER_ARMED;
	}
	l->flags |= GCL_TCPC_RXQ;
	return sf;
}

/*
 * One segment of connection @c, whose live words are @l, that passed the
 * NA / NOCONN / DROP lines.  Returns GCL_TCPRX_FAST or GCL_TCPRX_SLOW; a FAST
 * segment moves @l and sets *sflags, a SLOW one sets GCL_TCPO_STOPPED.
 */
GCL_TCPRX_FN uint32_t gcl_tcprx_one(const struct gcl_tcp_conn *c, struct gcl_tcprx_live *l,
                                    const struct gcl_tcprx_seg *s, uint32_t *sflags)
{
	*sflags = 0;
	if ((l->flags & GCL_TCPO_STOPPED) || gcl_tcprx_slow_fixed(s->flags, s->len, s->ack, c->snd_nxt, c->flags) ||
	    gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt) ||
	    gcl_tcprx_slow_rcv(s->seq, s->len, l->rcv_nxt, l->rcv_wnd)) {
		l->flags |= GCL_TCPO_STOPPED;
		return GCL_TCPRX_SLOW;
	}
	*sflags = gcl_tcprx_ack_step(l, s->seq, s->ack, s->win << (c->snd_wscale & 31));
	*sflags |= gcl_tcprx_rx_step(l, s->len, s->flags);
	return GCL_TCPRX_FAST;
}

#endif /* GCL_TCPRX_H */
