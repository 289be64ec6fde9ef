/*
 * gcl_tcprxo.h - the rule of gcl_tcp_rx_ooo (include/gclassify.h), shared by
 * the host twin (gcl_host.c, plain C) and the GPU walk (gcl_tcprx.hip): both
 * include this file, so the CPU tests and the sanitizer driver run the very
 * rule the GPU runs.  Not installed.
 *
 * On top of gcl_tcprxf.h it restates tcp_rx_append_text and tcp_rx_text
 * (runtime/net/tcp_in.c:64-169) and the lines around their call (:547-575)
 * with the out-of-order queue.  The queue is an ordered array of at most
 * GCL_TCPOOO_CAP entries; the host twin keeps it in memory and the GPU walk in
 * the registers of a wave, entry i in lane i, so the rule comes in the pieces
 * both can compose without naming the queue's storage:
 *
 *   gcl_tcprxo_reaches_ooo  would this segment get to tcp_rx_text's
 *                           out-of-order branch?  Pure; asked before anything
 *                           moves, for the stop at a full queue.
 *   gcl_tcprxo_head         one segment up to the text step: the fast path
 *                           (only with an empty live queue, :233), the flags
 *                           that stop, gcl_tcprxf_slow's steps unchanged.
 *   gcl_tcprxo_pos_test     :125 and :129 for one queue entry, two bits; the
 *                           walk from the tail takes the entry nearest the
 *                           tail that has either bit (gcl_tcprxo_pos).
 *   gcl_tcprxo_drain_test   :146 and :154 for the head of the queue.
 *   gcl_tcprxo_append       tcp_rx_append_text: the head clip, then the tail
 *                           clip, then rcv_nxt and rcv_wnd.
 *   gcl_tcprxo_text_tail    :562-574 after tcp_rx_text returned.
 *   gcl_tcprxo_done         done: of __tcp_rx_conn.
 *
 * The reference bounds the queue by TCP_OOO_MAX_SIZE (2048, :121); with a cap
 * of 64 that line can never hold, so it is not restated.  A segment that would
 * be inserted into a queue of GCL_TCPOOO_CAP entries STOPS the connection: it
 * is not dropped as the reference drops the 2049th, the runtime takes it.
 *
 * The rule assumes no order on a queue that came from outside: every test is
 * the reference's own on the entries as they lie.  As in gcl_tcprxf.h the tail
 * clip compares rcv_wnd < len plainly, the same as :83 for windows below 2^31.
 */
#ifndef GCL_TCPRXO_H
#define GCL_TCPRXO_H

#include "gcl_tcprxf.h"

enum { GCL_TCPRXO_FASTED = 0, GCL_TCPRXO_STOP, GCL_TCPRXO_DONE, GCL_TCPRXO_TEXT };
enum { GCL_TCPRXO_FREE = 0, GCL_TCPRXO_BREAK, GCL_TCPRXO_APPEND };
#define GCL_TCPRXO_POS_END 1u /* :125 wraps_gt(m->seg_end, pos->seg_end) */
#define GCL_TCPRXO_POS_SEQ 2u /* :129 wraps_gte(m->seg_seq, pos->seg_seq) */
#define GCL_TCPRXO_REJECT 0xFFFFFFFFu

/* the locals of __tcp_rx_conn that outlive the text step */
struct gcl_tcprxo_mid {
	uint32_t sf;
	int do_ack, do_drop;
};

/* inc/base/stddef.h:144-178 */
GCL_TCPRX_FN int gcl_tcprxo_wraps_gte(uint32_t a, uint32_t b)
{
	return (int32_t)(a - b) >= 0;
}

/* may the call walk this connection at all, its queue apart */
GCL_TCPRX_FN int gcl_tcprxo_state_ok(uint32_t cflags)
{
	return (cflags & (GCL_TCPC_ELIGIBLE | GCL_TCPC_ESTABLISHED)) != 0;
}

/*
 * Does the segment reach :117?  Nothing before the text step moves rcv_nxt or
 * rcv_wnd, so this is decided on the state as it stands before the segment.
 */
GCL_TCPRX_FN int gcl_tcprxo_reaches_ooo(const struct gcl_tcp_conn *c, const struct gcl_tcprx_live *l,
                                        const struct gcl_tcprx_seg *s)
{
	return !(s->flags & GCL_TCPRXF_STOP_FLAGS) && s->len > 0 && (s->flags & GCL_TCPRXF_ACK) &&
	       !gcl_tcprx_wraps_gt(s->ack, c->snd_nxt) && !gcl_tcprx_wraps_lte(s->seq, l->rcv_nxt) &&
	       gcl_tcprxf_acceptable(l->rcv_nxt, l->rcv_wnd, s->len, s->seq, s->flags);
}

/*
 * One segment of a taken connection that has not stopped, up to the text step;
 * @c->flags has GCL_TCPC_ELIGIBLE (the caller sets it: the live queue, not the
 * flag, says whether the queue is empty), @qn is the live queue's length.
 * FASTED: the fast path took it, *copy bytes.  STOP: the runtime's.  DONE: the
 * slow rule went to done without text.  TEXT: tcp_rx_text is next.
 */
GCL_TCPRX_FN uint32_t gcl_tcprxo_head(const struct gcl_tcp_conn *c, struct gcl_tcprxf_live *x,
                                      const struct gcl_tcprx_seg *s, uint32_t qn, struct gcl_tcprxo_mid *mid,
                                      uint32_t *copy)
{
	struct gcl_tcprx_live *l = &x->l;
	int ack_same = 0, wnd_updated = 0;

	mid->sf = 0;
	mid->do_ack = 0;
	mid->do_drop = 1;
	*copy = 0;
	if (qn == 0 && !gcl_tcprx_slow_fixed(s->flags, s->len, s->ack, c->snd_nxt, c->flags) &&
	    !gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt) &&
	    !gcl_tcprx_slow_rcv(s->seq, s->len, l->rcv_nxt, l->rcv_wnd)) {
		mid->sf = gcl_tcprx_ack_step(l, s->seq, s->ack, s->win << (c->snd_wscale & 31));
		if (mid->sf)
			x->rep_acks = 0;
		mid->sf |= gcl_tcprx_rx_step(l, s->len, s->flags);
		*copy = s->len;
		return GCL_TCPRXO_FASTED;
	}
	if (s->flags & GCL_TCPRXF_STOP_FLAGS)
		return GCL_TCPRXO_STOP;
	mid->sf = GCL_TCPRX_SF_RULE2;
	if (!gcl_tcprxf_acceptable(l->rcv_nxt, l->rcv_wnd, s->len, s->seq, s->flags)) {
		mid->do_ack = 1;
		return GCL_TCPRXO_DONE;
	}
	if (!(s->flags & GCL_TCPRXF_ACK))
		return GCL_TCPRXO_DONE;
	{
		const int snd_was_full = gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt);

		if (gcl_tcprx_wraps_lte(l->snd_una, s->ack) && gcl_tcprx_wraps_lte(s->ack, c->snd_nxt)) {
			mid->sf |= gcl_tcprxf_ack_step(l, s->seq, s->ack, s->win << (c->snd_wscale & 31), &ack_same,
			                               &wnd_updated);
		} else if (gcl_tcprx_wraps_gt(s->ack, c->snd_nxt)) {
			mid->do_ack = 1;
			return GCL_TCPRXO_DONE;
		}
		if (snd_was_full && !gcl_tcprx_snd_full(l->snd_una, l->snd_wnd, c->snd_nxt)) {
			mid->sf |= GCL_TCPRX_SF_TXWAKE;
			x->xflags |= GCL_TCPX_TXWAKE;
		}
	}
	mid->sf |= gcl_tcprxf_dupack(x, c->snd_nxt, s->ack, s->len, ack_same, wnd_updated);
	return s->len > 0 ? GCL_TCPRXO_TEXT : GCL_TCPRXO_DONE;
}

/* tcp_in.c:108: the in-order branch */
GCL_TCPRX_FN int gcl_tcprxo_in_order(const struct gcl_tcprx_live *l, uint32_t seq)
{
	return gcl_tcprx_wraps_lte(seq, l->rcv_nxt);
}

/* tcp_in.c:111-115, without FIN: wake of the in-order branch, asked before the append */
GCL_TCPRX_FN int gcl_tcprxo_in_order_wake(const struct gcl_tcprx_live *l, uint32_t flags)
{
	return (flags & GCL_TCPRX_PSH) != 0 || (l->flags & GCL_TCPC_RXQ) != 0;
}

/* tcp_in.c:125 and :129 for segment [@seq, @end) against entry [@eseq, @eend) */
GCL_TCPRX_FN uint32_t gcl_tcprxo_pos_test(uint32_t seq, uint32_t end, uint32_t eseq, uint32_t eend)
{
	return (gcl_tcprx_wraps_gt(end, eend) ? GCL_TCPRXO_POS_END : 0u) |
	       (gcl_tcprxo_wraps_gte(seq, eseq) ? GCL_TCPRXO_POS_SEQ : 0u);
}

/*
 * tcp_in.c:124-135 out of the entries' tests: bit i of @ends and @seqs is
 * entry i's POS_END and POS_SEQ.  The walk from the tail ends at the entry
 * nearest the tail with either bit, and :125 is tested first: after it with
 * POS_END, else the segment is refused; no such entry: at the head.
 */
GCL_TCPRX_FN uint32_t gcl_tcprxo_pos(uint64_t ends, uint64_t seqs)
{
	const uint64_t any = ends | seqs;

	if (!any)
		return 0;
	const uint32_t h = 63u - (uint32_t)__builtin_clzll(any);
	return (ends >> h & 1) ? h + 1 : GCL_TCPRXO_REJECT;
}

/* tcp_in.c:146 and :154 for the head of the queue: the free test comes first */
GCL_TCPRX_FN uint32_t gcl_tcprxo_drain_test(uint32_t eseq, uint32_t eend, uint32_t rcv_nxt)
{
	if (gcl_tcprx_wraps_lte(eend, rcv_nxt))
		return GCL_TCPRXO_FREE;
	if (gcl_tcprx_wraps_gt(eseq, rcv_nxt))
		return GCL_TCPRXO_BREAK;
	return GCL_TCPRXO_APPEND;
}

/*
 * tcp_in.c:64-95 for [@seq, @end) with wraps_lte(seq, rcv_nxt) and
 * wraps_gt(end, rcv_nxt): *head bytes are pulled off the front first (:76-80),
 * then the window trims the tail (:83-87), and *ln bytes join rxq.  A window
 * of 0 leaves ln == 0: the mbuf joins rxq empty, as in the reference.
 */
GCL_TCPRX_FN void gcl_tcprxo_append(struct gcl_tcprx_live *l, uint32_t seq, uint32_t end, uint32_t *head,
                                    uint32_t *ln)
{
	*head = l->rcv_nxt - seq;
	*ln = end - l->rcv_nxt;
	if (l->rcv_wnd < *ln)
		*ln = l->rcv_wnd;
	l->rcv_nxt += *ln;
	l->rcv_wnd -= *ln;
	l->flags |= GCL_TCPC_RXQ;
}

/*
 * tcp_in.c:165-166 and :559-574 once tcp_rx_text has returned @used with its
 * @wake; @qn is the queue's length now.  A refused segment (@used == 0) ran no
 * drain and gets no wake, and its delayed-ACK lines still run.
 */
GCL_TCPRX_FN void gcl_tcprxo_text_tail(struct gcl_tcprx_live *l, struct gcl_tcprxo_mid *mid, int used, int wake,
                                       uint32_t qn)
{
	if (used && l->rcv_wnd == 0)
		wake = 1;
	mid->do_drop = !used;
	if (wake) {
		mid->sf |= GCL_TCPRX_SF_WAKE;
		l->flags |= GCL_TCPO_WOKEN;
	}
	l->cnt = l->cnt + 1;
	if (l->cnt >= 2)
		mid->do_ack = 1;
	else if (!(l->flags & GCL_TCPC_ACK_DELAYED))
		l->flags |= GCL_TCPC_ACK_DELAYED | GCL_TCPO_TIMER_ARMED;
	/* :574: the duplicate ACKs that drive the peer's fast retransmit */
	if (qn)
		mid->do_ack = 1;
}

/* tcp_in.c:592-610: the segment's sflags */
GCL_TCPRX_FN uint32_t gcl_tcprxo_done(struct gcl_tcprx_live *l, const struct gcl_tcprxo_mid *mid)
{
	uint32_t sf = mid->sf;

	if (mid->do_ack) {
		l->flags &= ~(uint32_t)GCL_TCPC_ACK_DELAYED;
		l->cnt = 0;
		sf |= GCL_TCPRX_SF_ACK_NOW;
	}
	if (mid->do_drop)
		sf |= GCL_TCPRX_SF_DROPPED;
	return sf;
}

/* qin_skip and qin_len are 16 bits: an input entry longer than any frame saturates */
GCL_TCPRX_FN uint16_t gcl_tcprxo_u16(uint32_t v)
{
	return (uint16_t)(v < 0xFFFFu ? v : 0xFFFFu);
}

#endif /* GCL_TCPRXO_H */
