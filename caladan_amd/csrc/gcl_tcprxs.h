/*
 * gcl_tcprxs.h - the rule of gcl_tcp_rx_states (include/gclassify.h), shared
 * by the host twin (gcl_host.c, plain C) and the GPU walk (gcl_tcprx.hip):
 * both include this file, so the CPU tests run the very rule the GPU runs.
 * Not installed.
 *
 * On top of gcl_tcprxo.h it restates the rest of __tcp_rx_conn
 * (runtime/net/tcp_in.c:352-611): the FIN octet of len (:369-370), state
 * CLOSED (:372-376), :439's do_ack, RST (:444-447), SYN (:452-456), the ACK
 * step of SYN_RECEIVED (:462-473), the three transitions on snd_una ==
 * snd_nxt (:530-542), step 7's state test (:547-550), the fin that comes out
 * of tcp_rx_text (:114, :161) and step 8 (:578-590).  SYN_SENT (:378-428) is
 * not restated: it needs iss, winmax and the options.  The pieces:
 *
 *   gcl_tcprxs_head    one segment up to the text step, the live state moving;
 *                      FASTED, DONE or TEXT as gcl_tcprxo_head.
 *   gcl_tcprxs_append  tcp_rx_append_text for a piece whose last octet may be
 *                      a FIN: what moves in sequence space, and the bytes the
 *                      mbuf keeps.
 *   gcl_tcprxs_fin     step 8.
 * The queue tests, gcl_tcprxo_text_tail and gcl_tcprxo_done are gcl_tcprxo.h's.
 *
 * Two things the reference does are kept as they are.  m->seg_end counts the
 * FIN (:552), so tcp_rx_append_text's tail clip (:83-87) trims the mbuf by a
 * length that counts the FIN octet: a clipped FIN segment loses one more byte
 * of text than the window took, while rcv_nxt moves by the window.  And fin is
 * set whether or not the clip removed the FIN's own octet.
 */
#ifndef GCL_TCPRXS_H
#define GCL_TCPRXS_H

#include "gcl_tcprxo.h"

/* enum tcp state, runtime/net/tcp.h:41-52 */
enum {
	GCL_TCPRXS_SYN_SENT = 0, GCL_TCPRXS_SYN_RECEIVED, GCL_TCPRXS_ESTABLISHED, GCL_TCPRXS_FIN_WAIT1,
	GCL_TCPRXS_FIN_WAIT2, GCL_TCPRXS_CLOSE_WAIT, GCL_TCPRXS_CLOSING, GCL_TCPRXS_LAST_ACK, GCL_TCPRXS_TIME_WAIT,
	GCL_TCPRXS_CLOSED
};

/* the locals of __tcp_rx_conn that outlive the text step, and what the segment leaves for ev / rst_seq */
struct gcl_tcprxs_mid {
	struct gcl_tcprxo_mid o;
	uint32_t ev, rst_seq;
	uint32_t slen; /* :367-370: len with the FIN octet */
	int fin;
};

/* the state a connection enters with: state[c], or what the two flag bits say (GCL_TCPS_NOSTATE: not taken) */
GCL_TCPRX_FN uint32_t gcl_tcprxs_state_of(const uint8_t *state, uint32_t c, uint32_t cflags)
{
	if (state)
		return state[c];
	return gcl_tcprxo_state_ok(cflags) ? (uint32_t)GCL_TCPRXS_ESTABLISHED : (uint32_t)GCL_TCPS_NOSTATE;
}

/* may the call walk a connection in this state at all, its queue apart */
GCL_TCPRX_FN int gcl_tcprxs_state_ok(uint32_t st)
{
	return st >= GCL_TCPRXS_SYN_RECEIVED && st <= GCL_TCPRXS_CLOSED;
}

/* :547-550: the states that take text */
GCL_TCPRX_FN int gcl_tcprxs_text_state(uint32_t st)
{
	return st == GCL_TCPRXS_ESTABLISHED || st == GCL_TCPRXS_FIN_WAIT1 || st == GCL_TCPRXS_FIN_WAIT2;
}

/* tcp_conn_set_state (tcp.c:230-260) as far as the call carries it */
GCL_TCPRX_FN void gcl_tcprxs_set_state(uint32_t *st, uint32_t to, struct gcl_tcprxs_mid *mid)
{
	*st = to;
	mid->ev |= GCL_TCPS_STATE;
}

/* send_rst, :54-62 */
GCL_TCPRX_FN void gcl_tcprxs_send_rst(struct gcl_tcprxs_mid *mid, int acked, uint32_t seq, uint32_t ack)
{
	if (acked) {
		mid->ev |= GCL_TCPS_RST;
		mid->rst_seq = ack;
	} else {
		mid->ev |= GCL_TCPS_RST_ACK;
		mid->rst_seq = seq + mid->slen;
	}
}

/*
 * One segment of a taken connection that has not stopped, up to the text step;
 * *st is the live state, @qn the live queue's length.  FASTED: tcp_rx_conn's
 * fast path took it (only in ESTABLISHED with an empty live queue), *copy
 * bytes.  DONE: __tcp_rx_conn went to done without text.  TEXT: tcp_rx_text is
 * next.  ev, rst_seq, the state and xflags are as the steps passed leave them.
 */
GCL_TCPRX_FN uint32_t gcl_tcprxs_head(const struct gcl_tcp_conn *c, struct gcl_tcprxf_live *x, uint32_t *st,
                                      const struct gcl_tcprx_seg *s, uint32_t qn, struct gcl_tcprxs_mid *mid,
                                      uint32_t *copy)
{
	struct gcl_tcprx_live *l = &x->l;
	const uint32_t win = s->win << (c->snd_wscale & 31);
	int ack_same = 0, wnd_updated = 0;

	mid->o.sf = 0;
	mid->o.do_ack = 0;
	mid->o.do_drop = 1;
	mid->ev = 0;
	mid->rst_seq = 0;
	mid->fin = 0;
	/* :367-370 */
	mid->slen = s->len + ((s->flags & GCL_TCPRX_FIN) ? 1u : 0u);
	*copy = 0;
	/* :221-242 */
	if (*st == GCL_TCPRXS_ESTABLISHED && qn == 0 &&
	    !gcl_tcprx_slow_fixed(s->flags, s->len, s->ack, c->snd_nxt, GCL_TCPC_ELIGIBLE) &&
	    !gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt) &&
	    !gcl_tcprx_slow_rcv(s->seq, s->len, l->rcv_nxt, l->rcv_wnd)) {
		mid->o.sf = gcl_tcprx_ack_step(l, s->seq, s->ack, win);
		if (mid->o.sf)
			x->rep_acks = 0;
		mid->o.sf |= gcl_tcprx_rx_step(l, s->len, s->flags);
		*copy = s->len;
		return GCL_TCPRXO_FASTED;
	}
	mid->o.sf = GCL_TCPRX_SF_RULE2;
	/* :372-376 */
	if (*st == GCL_TCPRXS_CLOSED) {
		if (!(s->flags & GCL_TCPRX_RST))
			gcl_tcprxs_send_rst(mid, 0, s->seq, s->ack);
		return GCL_TCPRXO_DONE;
	}
	/* step 1, :438-441 */
	if (!gcl_tcprxf_acceptable(l->rcv_nxt, l->rcv_wnd, mid->slen, s->seq, s->flags)) {
		mid->o.do_ack = !(s->flags & GCL_TCPRX_RST);
		return GCL_TCPRXO_DONE;
	}
	/* step 2, :444-447 */
	if (s->flags & GCL_TCPRX_RST) {
		mid->ev |= GCL_TCPS_FAIL;
		x->xflags |= GCL_TCPX_FAILED;
		return GCL_TCPRXO_DONE;
	}
	/* step 4, :452-456 */
	if (s->flags & GCL_TCPRXF_SYN) {
		gcl_tcprxs_send_rst(mid, (s->flags & GCL_TCPRXF_ACK) != 0, s->seq, s->ack);
		mid->ev |= GCL_TCPS_FAIL;
		x->xflags |= GCL_TCPX_FAILED;
		return GCL_TCPRXO_DONE;
	}
	/* step 5, :459-473 */
	if (!(s->flags & GCL_TCPRXF_ACK))
		return GCL_TCPRXO_DONE;
	if (*st == GCL_TCPRXS_SYN_RECEIVED) {
		if (!(gcl_tcprx_wraps_lte(l->snd_una, s->ack) && gcl_tcprx_wraps_lte(s->ack, c->snd_nxt))) {
			gcl_tcprxs_send_rst(mid, 1, s->seq, s->ack);
			return GCL_TCPRXO_DONE;
		}
		l->snd_wnd = win;
		l->snd_wl1 = s->seq;
		l->snd_wl2 = s->ack;
		mid->o.sf |= GCL_TCPRX_SF_WND;
		gcl_tcprxs_set_state(st, GCL_TCPRXS_ESTABLISHED, mid);
		x->xflags |= GCL_TCPX_OPENED;
	}
	/* :476-505 */
	{
		const int snd_was_full = gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt);

		if (gcl_tcprx_wraps_lte(l->snd_una, s->ack) && gcl_tcprx_wraps_lte(s->ack, c->snd_nxt)) {
			mid->o.sf |= gcl_tcprxf_ack_step(l, s->seq, s->ack, win, &ack_same, &wnd_updated);
		} else if (gcl_tcprx_wraps_gt(s->ack, c->snd_nxt)) {
			mid->o.do_ack = 1;
			return GCL_TCPRXO_DONE;
		}
		if (snd_was_full && !gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt)) {
			mid->o.sf |= GCL_TCPRX_SF_TXWAKE;
			x->xflags |= GCL_TCPX_TXWAKE;
		}
	}
	/* :514-528: a FIN counts in len */
	mid->o.sf |= gcl_tcprxf_dupack(x, c->snd_nxt, s->ack, mid->slen, ack_same, wnd_updated);
	/* :530-542 */
	if (*st == GCL_TCPRXS_FIN_WAIT1 && l->snd_una == c->snd_nxt) {
		gcl_tcprxs_set_state(st, GCL_TCPRXS_FIN_WAIT2, mid);
	} else if (*st == GCL_TCPRXS_CLOSING && l->snd_una == c->snd_nxt) {
		x->xflags |= GCL_TCPX_TIMEWAIT;
		gcl_tcprxs_set_state(st, GCL_TCPRXS_TIME_WAIT, mid);
	} else if (*st == GCL_TCPRXS_LAST_ACK && l->snd_una == c->snd_nxt) {
		gcl_tcprxs_set_state(st, GCL_TCPRXS_CLOSED, mid);
		mid->ev |= GCL_TCPS_PUT;
		x->xflags |= GCL_TCPX_PUT;
		return GCL_TCPRXO_DONE;
	}
	/* step 7, :547-550 */
	return mid->slen > 0 && gcl_tcprxs_text_state(*st) ? GCL_TCPRXO_TEXT : GCL_TCPRXO_DONE;
}

/* tcp_in.c:111-115: wake of the in-order branch, asked before the append; a FIN also sets fin there */
GCL_TCPRX_FN int gcl_tcprxs_in_order_wake(const struct gcl_tcprx_live *l, uint32_t flags)
{
	return (flags & (GCL_TCPRX_PSH | GCL_TCPRX_FIN)) != 0 || (l->flags & GCL_TCPC_RXQ) != 0;
}

/*
 * tcp_in.c:64-95 for [@seq, @end) whose last octet is a FIN when @fin: *head
 * and the move of rcv_nxt and rcv_wnd are gcl_tcprxo_append's, in sequence
 * space; *bytes is the length mbuf_pull and mbuf_trim leave.  The mbuf holds
 * end - seq - 1 bytes, the pull takes *head and the trim the whole of
 * seg_end - (rcv_nxt + rcv_wnd), the FIN octet counted: one byte less than
 * the sequence space taken, and none when that is 0.
 */
GCL_TCPRX_FN void gcl_tcprxs_append(struct gcl_tcprx_live *l, uint32_t seq, uint32_t end, int fin, uint32_t *head,
                                    uint32_t *bytes)
{
	uint32_t ln;

	gcl_tcprxo_append(l, seq, end, head, &ln);
	*bytes = fin && ln ? ln - 1 : ln;
}

/* step 8, :578-590 */
GCL_TCPRX_FN void gcl_tcprxs_fin(struct gcl_tcprxf_live *x, uint32_t *st, struct gcl_tcprxs_mid *mid)
{
	if (!mid->fin)
		return;
	mid->ev |= GCL_TCPS_FIN;
	if (*st == GCL_TCPRXS_ESTABLISHED) {
		gcl_tcprxs_set_state(st, GCL_TCPRXS_CLOSE_WAIT, mid);
	} else if (*st == GCL_TCPRXS_FIN_WAIT1) {
		gcl_tcprxs_set_state(st, GCL_TCPRXS_CLOSING, mid);
	} else if (*st == GCL_TCPRXS_FIN_WAIT2) {
		x->xflags |= GCL_TCPX_TIMEWAIT;
		mid->o.do_ack = 1;
		gcl_tcprxs_set_state(st, GCL_TCPRXS_TIME_WAIT, mid);
	}
}

/* after this segment the connection is the runtime's: tcp_conn_fail's frees, or tcp_conn_put */
GCL_TCPRX_FN int gcl_tcprxs_ends(uint32_t ev)
{
	return (ev & (GCL_TCPS_FAIL | GCL_TCPS_PUT)) != 0;
}

#endif /* GCL_TCPRXS_H */
