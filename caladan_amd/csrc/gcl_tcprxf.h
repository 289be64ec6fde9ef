/*
 * gcl_tcprxf.h - the rule of gcl_tcp_rx_full (include/gclassify.h), shared by
 * the host twin (gcl_host.c, plain C) and the GPU walk (gcl_tcprx.hip): both
 * include this file, so the CPU tests and the sanitizer driver run the very
 * rule the GPU runs.  Not installed.
 *
 * On top of gcl_tcprx.h (tcp_rx_conn's fast path) it restates __tcp_rx_conn
 * (runtime/net/tcp_in.c:352-611) as it reads for state == ESTABLISHED and an
 * empty out-of-order queue: the acceptability test (gcl_tcprxf_acceptable),
 * what still leaves for the runtime (gcl_tcprxf_stops), the ACK / window
 * update (gcl_tcprxf_ack_step), the duplicate-ACK block (gcl_tcprxf_dupack)
 * and tcp_rx_text's in-order branch with tcp_rx_append_text's tail clip
 * (gcl_tcprxf_text).  gcl_tcprxf_slow is one handled segment in the
 * reference's order, gcl_tcprxf_one the whole rule for one segment: the fast
 * path where gcl_tcprx_one takes it, else the slow rule.
 */
#ifndef GCL_TCPRXF_H
#define GCL_TCPRXF_H

#include "gcl_tcprx.h"

#define GCL_TCPRXF_SYN 0x02u
#define GCL_TCPRXF_ACK 0x10u
#define GCL_TCPRXF_STOP_FLAGS (GCL_TCPRX_FIN | GCL_TCPRX_RST | GCL_TCPRX_URG | GCL_TCPRXF_SYN)
#define GCL_TCPRXF_FAST_RETRANSMIT_THRESH 3u /* runtime/net/tcp.h: TCP_FAST_RETRANSMIT_THRESH */
/* above the eight bits of sflags[j]: this segment was a rep_acks++ event */
#define GCL_TCPRXF_EV_DUPACK 0x100u

/* the words of a connection that move during a call */
struct gcl_tcprxf_live {
	struct gcl_tcprx_live l;
	uint32_t rep_acks;     /* c->rep_acks, the reference's int */
	uint32_t fast_rtx_ack; /* the ack of the last FASTRTX */
	uint32_t xflags;       /* GCL_TCPX_* */
};

/* tcp_in.c:27-51: is_acceptable, @len without the FIN increment */
GCL_TCPRX_FN int gcl_tcprxf_acceptable(uint32_t rcv_nxt, uint32_t rcv_wnd, uint32_t len, uint32_t seq,
                                       uint32_t flags)
{
	if (len == 0 && rcv_wnd == 0) {
		if (flags & (GCL_TCPRXF_ACK | GCL_TCPRX_URG | GCL_TCPRX_RST))
			return 1;
		return seq == rcv_nxt;
	} else if (len == 0) {
		return gcl_tcprx_wraps_lte(rcv_nxt, seq) && gcl_tcprx_wraps_lt(seq, rcv_nxt + rcv_wnd);
	} else if (rcv_wnd == 0) {
		return 0;
	}
	return (gcl_tcprx_wraps_lte(rcv_nxt, seq) && gcl_tcprx_wraps_lt(seq, rcv_nxt + rcv_wnd)) ||
	       (gcl_tcprx_wraps_lte(rcv_nxt, seq + len - 1) && gcl_tcprx_wraps_lt(seq + len - 1, rcv_nxt + rcv_wnd));
}

/*
 * What a flat snapshot cannot carry: every other state and the out-of-order
 * queue (not ELIGIBLE), the flags whose steps end or reset the connection, and
 * acceptable text that does not start at rcv_nxt (tcp_rx_text's out-of-order
 * branch, or tcp_rx_append_text's head clip).
 */
GCL_TCPRX_FN int gcl_tcprxf_stops(uint32_t cflags, const struct gcl_tcprx_live *l, const struct gcl_tcprx_seg *s)
{
	if (!(cflags & GCL_TCPC_ELIGIBLE) || (s->flags & GCL_TCPRXF_STOP_FLAGS))
		return 1;
	return s->len > 0 && s->seq != l->rcv_nxt &&
	       gcl_tcprxf_acceptable(l->rcv_nxt, l->rcv_wnd, s->len, s->seq, s->flags);
}

/*
 * tcp_in.c:477-497 for snd_una <= ack <= snd_nxt; @win is already shifted.
 * Returns ACKED | WND; *ack_same and *wnd_updated as the reference's locals.
 */
GCL_TCPRX_FN uint32_t gcl_tcprxf_ack_step(struct gcl_tcprx_live *l, uint32_t seq, uint32_t ack, uint32_t win,
                                          int *ack_same, int *wnd_updated)
{
	uint32_t sf = 0;

	if (l->snd_una != ack) {
		l->snd_una = ack;
		sf |= GCL_TCPRX_SF_ACKED;
	} else {
		*ack_same = 1;
	}
	if (gcl_tcprx_wraps_lt(l->snd_wl1, seq) || (l->snd_wl1 == seq && gcl_tcprx_wraps_lte(l->snd_wl2, ack))) {
		if (!*ack_same || l->snd_wnd <= win) {
			if (l->snd_wnd != win || l->snd_wl2 != ack)
				*wnd_updated = 1;
			l->snd_wnd = win;
			l->snd_wl1 = seq;
			l->snd_wl2 = ack;
			sf |= GCL_TCPRX_SF_WND;
		}
	}
	return sf;
}

/* tcp_in.c:514-528.  Returns FASTRTX | GCL_TCPRXF_EV_DUPACK. */
GCL_TCPRX_FN uint32_t gcl_tcprxf_dupack(struct gcl_tcprxf_live *x, uint32_t snd_nxt, uint32_t ack, uint32_t len,
                                        int ack_same, int wnd_updated)
{
	uint32_t sf = 0;

	if (ack_same && x->l.snd_una != snd_nxt && len == 0 && !wnd_updated) {
		x->rep_acks++;
		sf |= GCL_TCPRXF_EV_DUPACK;
		if (x->rep_acks >= GCL_TCPRXF_FAST_RETRANSMIT_THRESH) {
			sf |= GCL_TCPRX_SF_FASTRTX;
			x->fast_rtx_ack = ack;
			x->xflags |= GCL_TCPX_FASTRTX;
			x->rep_acks = 0;
			x->l.flags |= GCL_TCPO_REP_ACKS_RESET;
		}
	} else if (x->l.snd_una == ack) {
		x->rep_acks = 0;
		x->l.flags |= GCL_TCPO_REP_ACKS_RESET;
	}
	return sf;
}

/*
 * tcp_in.c:98-169 and :64-95 for text that starts at rcv_nxt into a window
 * that is not 0, then :562-573.  Returns WAKE; *copy is what joined rxq and
 * *do_ack the reference's local.  The tail clip compares rcv_wnd < len plainly:
 * the same as :83's wraps_lt for every window below 2^31, and for the others,
 * which no PCB holds, never longer than the segment.
 */
GCL_TCPRX_FN uint32_t gcl_tcprxf_text(struct gcl_tcprx_live *l, uint32_t len, uint32_t flags, uint32_t *copy,
                                      int *do_ack)
{
	uint32_t sf = 0;
	int wake = (flags & GCL_TCPRX_PSH) != 0 || (l->flags & GCL_TCPC_RXQ) != 0;

	if (l->rcv_wnd < len)
		len = l->rcv_wnd;
	l->rcv_nxt += len;
	l->rcv_wnd -= len;
	l->flags |= GCL_TCPC_RXQ;
	if (l->rcv_wnd == 0)
		wake = 1;
	if (wake) {
		sf |= GCL_TCPRX_SF_WAKE;
		l->flags |= GCL_TCPO_WOKEN;
	}
	l->cnt = l->cnt + 1;
	if (l->cnt >= 2)
		*do_ack = 1;
	else if (!(l->flags & GCL_TCPC_ACK_DELAYED))
		l->flags |= GCL_TCPC_ACK_DELAYED | GCL_TCPO_TIMER_ARMED;
	*copy = len;
	return sf;
}

/*
 * One segment that gcl_tcprxf_stops lets through, in __tcp_rx_conn's order
 * from step 1 to done.  Returns its sflags and GCL_TCPRXF_EV_DUPACK; *copy is
 * the accepted byte count.
 */
GCL_TCPRX_FN uint32_t gcl_tcprxf_slow(const struct gcl_tcp_conn *c, struct gcl_tcprxf_live *x,
                                      const struct gcl_tcprx_seg *s, uint32_t *copy)
{
	struct gcl_tcprx_live *l = &x->l;
	uint32_t sf = GCL_TCPRX_SF_RULE2;
	int do_ack = 0, do_drop = 1, ack_same = 0, wnd_updated = 0;

	*copy = 0;
	if (!gcl_tcprxf_acceptable(l->rcv_nxt, l->rcv_wnd, s->len, s->seq, s->flags)) {
		do_ack = 1;
		goto done;
	}
	if (!(s->flags & GCL_TCPRXF_ACK))
		goto done;
	{
		const int snd_was_full = gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt);

		if (gcl_tcprx_wraps_lte(l->snd_una, s->ack) && gcl_tcprx_wraps_lte(s->ack, c->snd_nxt)) {
			sf |= gcl_tcprxf_ack_step(l, s->seq, s->ack, s->win << (c->snd_wscale & 31), &ack_same,
			                          &wnd_updated);
		} else if (gcl_tcprx_wraps_gt(s->ack, c->snd_nxt)) {
			do_ack = 1;
			goto done;
		}
		if (snd_was_full && !gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt)) {
			sf |= GCL_TCPRX_SF_TXWAKE;
			x->xflags |= GCL_TCPX_TXWAKE;
		}
	}
	sf |= gcl_tcprxf_dupack(x, c->snd_nxt, s->ack, s->len, ack_same, wnd_updated);
	if (s->len > 0) {
		sf |= gcl_tcprxf_text(l, s->len, s->flags, copy, &do_ack);
		do_drop = 0;
	}
done:
	if (do_ack) {
		l->flags &= ~(uint32_t)GCL_TCPC_ACK_DELAYED;
		l->cnt = 0;
		sf |= GCL_TCPRX_SF_ACK_NOW;
	}
	if (do_drop)
		sf |= GCL_TCPRX_SF_DROPPED;
	return sf;
}

/*
 * One segment of connection @c, whose live words are @x, that passed the
 * NA / NOCONN / DROP lines.  Returns GCL_TCPRX_FAST (handled, by either rule)
 * or GCL_TCPRX_SLOW; a handled segment moves @x and sets *sflags (with
 * GCL_TCPRXF_EV_DUPACK above the byte) and *copy, a SLOW one sets
 * GCL_TCPO_STOPPED.
 */
GCL_TCPRX_FN uint32_t gcl_tcprxf_one(const struct gcl_tcp_conn *c, struct gcl_tcprxf_live *x,
                                     const struct gcl_tcprx_seg *s, uint32_t *sflags, uint32_t *copy)
{
	*sflags = 0;
	*copy = 0;
	if (x->l.flags & GCL_TCPO_STOPPED)
		return GCL_TCPRX_SLOW;
	if (!gcl_tcprx_slow_fixed(s->flags, s->len, s->ack, c->snd_nxt, c->flags) &&
	    !gcl_tcprx_snd_full(x->l.snd_una, x->l.snd_wnd, c->snd_nxt) &&
	    !gcl_tcprx_slow_rcv(s->seq, s->len, x->l.rcv_nxt, x->l.rcv_wnd)) {
		*sflags = gcl_tcprx_ack_step(&x->l, s->seq, s->ack, s->win << (c->snd_wscale & 31));
		if (*sflags)
			x->rep_acks = 0;
		*sflags |= gcl_tcprx_rx_step(&x->l, s->len, s->flags);
		*copy = s->len;
		return GCL_TCPRX_FAST;
	}
	if (gcl_tcprxf_stops(c->flags, &x->l, s)) {
		x->l.flags |= GCL_TCPO_STOPPED;
		return GCL_TCPRX_SLOW;
	}
	*sflags = gcl_tcprxf_slow(c, x, s, copy);
	return GCL_TCPRX_FAST;
}

#endif /* GCL_TCPRXF_H */
