/*
 * gcl_tcpshut.h - the rule of gcl_tcp_shut (include/gclassify.h), shared by
 * the host twin (gcl_host.c, plain C) and the GPU kernels (gcl_tcpshut.hip):
 * both include this file, so the CPU tests and the sanitizer driver run the
 * very rule the GPU runs.  Not installed.  Plain C without libc.
 *
 * gcl_shut_rule restates tcp_shutdown, tcp_close and tcp_abort
 * (runtime/net/tcp.c:1555-1633) with tcp_conn_shutdown_tx (:1504-1546),
 * tcp_conn_shutdown_rx (:1492-1502), tcp_conn_fail (:1453-1484),
 * tcp_conn_set_state (:248-263) and tcp_timer_update (:46-77) for one
 * connection at one clock reading, without the layout of the segments: it
 * says which one segment the connection wants, and the caller, who knows how
 * many were wanted before it, turns the result into NOSPACE with
 * gcl_shut_nospace when that segment has no room.
 *
 * gcl_shut_seg_words is the segment as a gcl_txh_desc with its gcl_txq_ent and
 * gcl_txq_cold: tcp_tx_ctl(FIN | ACK) (runtime/net/tcp_out.c:264-295 with
 * __tcp_add_tcphdr, :54-81) or tcp_tx_raw_rst (:98-128, gcl_ctl_rst_desc of
 * gcl_tcptmr.h).
 *
 * Not modelled: the interrupted wait of tcp_shutdown (-EINTR), which needs a
 * signal; a connection whose writer is busy is BLOCK whoever asks.
 * tx_pending is left as the reference leaves it: tcp_conn_shutdown_tx does not
 * flush it (the FIN takes snd_nxt, which already counts its bytes), and only a
 * fail without TX_EXCLUSIVE frees it (FREE_PEND).
 */
#ifndef GCL_TCPSHUT_H
#define GCL_TCPSHUT_H

#include <stdint.h>

#include "../../include/gclassify.h"
#include "gcl_tcptmr.h"

#define GCL_SHUT_FN GCL_TMR_FN

#define GCL_SHUT_ECONNABORTED 103
#define GCL_SHUT_EINVAL       22
#define GCL_SHUT_ENOBUFS      105
#define GCL_SHUT_TCP_FIN_ACK  0x11u

/* what the connection wants sent */
#define GCL_SHUT_WANT_NONE 0u
#define GCL_SHUT_WANT_FIN  1u
#define GCL_SHUT_WANT_RST  2u

/* one connection as the rule reads it */
struct gcl_shut_one {
	uint64_t next_timeout, attach_ts, time_wait_ts, ack_ts, zero_wnd_ts, txq_ts;
	uint32_t state, tflags; /* gcl_tcp_tmr's bytes */
	uint32_t op, sflags;    /* gcl_tcp_shut's bytes */
	int32_t  how;
	uint32_t snd_nxt;
};

/* and what the rule says of it */
struct gcl_shut_res {
	uint64_t next_timeout, txq_ts;
	int32_t  ret, err;
	uint32_t snd_nxt, flags;
	uint32_t status, state, tflags, nput;
	uint32_t want;          /* GCL_SHUT_WANT_* */
};

/* tcp_timer_update (tcp.c:46-77) on the given words; the out-of-order term takes @now, as gcl_tmr_sweep's */
GCL_SHUT_FN uint64_t gcl_shut_timer(const struct gcl_shut_one *t, uint32_t state, uint32_t tflags, uint64_t txq_ts,
                                    uint64_t now)
{
	uint64_t nt = UINT64_MAX;

	if (state == GCL_TCP_STATE_TIME_WAIT)
		nt = t->time_wait_ts + GCL_TMR_T_TIME_WAIT;
	if (state < GCL_TCP_STATE_ESTABLISHED)
		nt = t->attach_ts + GCL_TMR_T_CONNECT;
	if (tflags & GCL_TMR_ACK_DELAYED)
		nt = gcl_tmr_min(nt, t->ack_ts + GCL_TMR_T_ACK);
	if (tflags & GCL_TMR_ZERO_WND)
		nt = gcl_tmr_min(nt, t->zero_wnd_ts + GCL_TMR_T_ZERO_WND);
	if (!(tflags & GCL_TMR_TX_EXCLUSIVE) && (tflags & GCL_TMR_TXQ))
		nt = gcl_tmr_min(nt, txq_ts + GCL_TMR_T_RETRANSMIT);
	if (tflags & GCL_TMR_OOO)
		nt = gcl_tmr_min(nt, now + GCL_TMR_T_OOQ_ACK);
	return nt;
}

/* tcp_conn_shutdown_rx, tcp.c:1492-1502 */
GCL_SHUT_FN void gcl_shut_rx(const struct gcl_shut_one *t, struct gcl_shut_res *r)
{
	if ((t->sflags & GCL_SHUT_RX_CLOSED) || (r->flags & GCL_SHO_RX_CLOSED_SET))
		return;
	r->flags |= GCL_SHO_POLLRDHUP_IN | GCL_SHO_RX_CLOSED_SET | GCL_SHO_RXWAKE;
}

/* tcp_conn_fail, tcp.c:1453-1484 */
GCL_SHUT_FN void gcl_shut_fail(const struct gcl_shut_one *t, uint64_t now, int32_t err, struct gcl_shut_res *r)
{
	r->err = err;                                   /* :1458 */
	if (t->state < GCL_TCP_STATE_ESTABLISHED)       /* tcp_conn_set_state, :254-258 */
		r->flags |= GCL_SHO_POLLOUT;
	r->state = GCL_TCP_STATE_CLOSED;                /* :1459, and its tcp_timer_update: before the frees */
	r->next_timeout = gcl_shut_timer(t, GCL_TCP_STATE_CLOSED, t->tflags, t->txq_ts, now);
	gcl_shut_rx(t, r);                              /* :1461 */
	if (!(t->sflags & GCL_SHUT_TX_CLOSED))          /* :1463-1467 */
		r->flags |= GCL_SHO_TX_CLOSED_SET | GCL_SHO_TXWAKE | GCL_SHO_POLLHUP;
	if (!(t->tflags & GCL_TMR_TX_EXCLUSIVE)) {      /* :1470-1476 */
		r->flags |= GCL_SHO_FREE_TXQ | GCL_SHO_FREE_PEND;
		r->tflags &= ~(uint32_t)GCL_TMR_TXQ;
	}
	if (!(t->sflags & GCL_SHUT_RX_EXCL))            /* :1477-1478 */
		r->flags |= GCL_SHO_FREE_RXQ;
	r->flags |= GCL_SHO_FREE_OOO;                   /* :1479 */
	r->tflags &= ~(uint32_t)GCL_TMR_OOO;
	if (t->state != GCL_TCP_STATE_CLOSED)           /* :1482-1483 */
		r->nput++;
}

/* the connection with nothing changed */
GCL_SHUT_FN void gcl_shut_echo(const struct gcl_shut_one *t, uint32_t status, int32_t ret, struct gcl_shut_res *r)
{
	r->next_timeout = t->next_timeout;
	r->txq_ts = t->txq_ts;
	r->ret = ret;
	r->err = 0;
	r->snd_nxt = t->snd_nxt;
	r->flags = 0;
	r->status = status;
	r->state = t->state;
	r->tflags = t->tflags;
	r->nput = 0;
	r->want = GCL_SHUT_WANT_NONE;
}

/* a cap took the room of its segment: tcp_tx_ctl's -ENOMEM is not played out, nothing happens */
GCL_SHUT_FN void gcl_shut_nospace(const struct gcl_shut_one *t, struct gcl_shut_res *r)
{
	gcl_shut_echo(t, GCL_SHUTS_NOSPACE, -GCL_SHUT_ENOBUFS, r);
}

/* The rule of one connection: fills every field of *@r. */
GCL_SHUT_FN void gcl_shut_rule(const struct gcl_shut_one *t, uint64_t now, struct gcl_shut_res *r)
{
	const uint32_t S = t->state, X = t->tflags & GCL_TMR_TX_EXCLUSIVE;
	int tx, rx;

	gcl_shut_echo(t, GCL_SHUTS_NONE, 0, r);
	if (t->op == GCL_SHUT_OP_NONE || !(t->tflags & GCL_TMR_LIVE))
		return;
	if (t->op > GCL_SHUT_OP_ABORT || S > GCL_TCP_STATE_CLOSED) {
		r->status = GCL_SHUTS_REFUSED;
		return;
	}
	if (t->op == GCL_SHUT_OP_SHUTDOWN && (t->how < 0 || t->how > 2)) { /* :1560-1561 */
		r->status = GCL_SHUTS_EINVAL;
		r->ret = -GCL_SHUT_EINVAL;
		return;
	}
	r->status = GCL_SHUTS_DONE;
	if (t->op == GCL_SHUT_OP_ABORT) { /* :1585-1606 */
		if (S == GCL_TCP_STATE_CLOSED)
			return;
		gcl_shut_fail(t, now, GCL_SHUT_ECONNABORTED, r);
		if (X)
			r->status = GCL_SHUTS_ABORT_WAIT; /* :1600-1601: the RST waits for the writer's snd_nxt */
		else
			r->want = GCL_SHUT_WANT_RST;
		return;
	}
	tx = t->op == GCL_SHUT_OP_CLOSE || t->how != 0;
	rx = t->op == GCL_SHUT_OP_CLOSE || t->how != 1;
	if (tx && !(t->sflags & GCL_SHUT_TX_CLOSED)) { /* tcp_conn_shutdown_tx */
		if (S < GCL_TCP_STATE_ESTABLISHED) { /* :1513-1517 */
			gcl_shut_fail(t, now, GCL_SHUT_ECONNABORTED, r);
			r->want = GCL_SHUT_WANT_RST;
		} else if (X) { /* :1519-1527: asleep before the rx part and the put */
			r->status = GCL_SHUTS_BLOCK;
			return;
		} else { /* :1529-1543 */
			r->want = GCL_SHUT_WANT_FIN;
			r->snd_nxt = t->snd_nxt + 1;
			if (!(t->tflags & GCL_TMR_TXQ))
				r->txq_ts = now; /* the FIN is the queue's head */
			r->tflags |= GCL_TMR_TXQ;
			if (S == GCL_TCP_STATE_ESTABLISHED)
				r->state = GCL_TCP_STATE_FIN_WAIT1;
			else if (S == GCL_TCP_STATE_CLOSE_WAIT)
				r->state = GCL_TCP_STATE_LAST_ACK;
			else
				r->flags |= GCL_SHO_WARN; /* no tcp_conn_set_state: no timer update */
			if (r->state != S)
				r->next_timeout = gcl_shut_timer(t, r->state, r->tflags, r->txq_ts, now);
			r->flags |= GCL_SHO_POLLHUP | GCL_SHO_TX_CLOSED_SET | GCL_SHO_TXWAKE;
		}
	}
	if (rx)
		gcl_shut_rx(t, r);
	if (t->op == GCL_SHUT_OP_CLOSE) { /* :1627-1632 */
		r->flags |= GCL_SHO_DETACH_POLL;
		r->nput++;
	}
}

/* struct gcl_shut_conn_out as twelve dwords */
GCL_SHUT_FN void gcl_shut_conn_words(const struct gcl_shut_res *r, uint32_t first_seg, uint32_t nseg, uint32_t o[12])
{
	o[0] = (uint32_t)r->next_timeout;
	o[1] = (uint32_t)(r->next_timeout >> 32);
	o[2] = (uint32_t)r->txq_ts;
	o[3] = (uint32_t)(r->txq_ts >> 32);
	o[4] = (uint32_t)r->ret;
	o[5] = (uint32_t)r->err;
	o[6] = r->snd_nxt;
	o[7] = first_seg;
	o[8] = r->flags;
	o[9] = (r->status & 0xFFu) | (r->state & 0xFFu) << 8 | (r->tflags & 0xFFu) << 16 | (nseg & 0xFFu) << 24;
	o[10] = r->nput & 0xFFu;
	o[11] = 0;
}

/* struct gcl_tcp_tmr, struct gcl_tcp_shut and snd_nxt as dwords -> *@t; @m: the timer record's sixteen, @s: the request's four */
GCL_SHUT_FN void gcl_shut_load(const uint32_t m[16], const uint32_t s[4], uint32_t snd_nxt, struct gcl_shut_one *t)
{
	t->next_timeout = (uint64_t)m[1] << 32 | m[0];
	t->attach_ts = (uint64_t)m[3] << 32 | m[2];
	t->time_wait_ts = (uint64_t)m[5] << 32 | m[4];
	t->ack_ts = (uint64_t)m[7] << 32 | m[6];
	t->zero_wnd_ts = (uint64_t)m[9] << 32 | m[8];
	t->txq_ts = (uint64_t)m[11] << 32 | m[10];
	t->state = m[12] & 0xFFu;
	t->tflags = (m[12] >> 8) & 0xFFu;
	t->how = (int32_t)s[0];
	t->op = s[1] & 0xFFu;
	t->sflags = (s[1] >> 8) & 0xFFu;
	t->snd_nxt = snd_nxt;
}

/* the slots that fit: min(seg_cap, the frames behind frame_base); the fit test is gcl_tcp_write's */
GCL_SHUT_FN uint64_t gcl_shut_cap(uint64_t seg_cap, uint64_t frames_len, uint64_t frame_base, uint32_t stride)
{
	uint64_t slots;

	if (!frames_len)
		return seg_cap;
	slots = frames_len < frame_base ? 0 : (frames_len - frame_base) / stride;
	return slots < seg_cap ? slots : seg_cap;
}

/*
 * The segment as sixteen dwords: d[0..7] its gcl_txh_desc, d[8..11] its
 * gcl_txq_ent, d[12..15] its gcl_txq_cold (all zero for an RST, which never
 * joins the queue).  @a: struct gcl_tcp_addr as four dwords; @snd_nxt: as it
 * came, the segment's seq.
 */
GCL_SHUT_FN void gcl_shut_seg_words(const uint32_t a[4], uint32_t want, uint32_t snd_nxt, uint32_t rcv_nxt,
                                    uint32_t rcv_wnd, uint64_t frame_off, uint64_t now, uint32_t d[16])
{
	if (want == GCL_SHUT_WANT_RST) {
		gcl_ctl_rst_desc(a, GCL_CTL_RST, snd_nxt, d);
		for (int i = 8; i < 16; i++)
			d[i] = 0;
		return;
	}
	gcl_ctl_desc(a, snd_nxt, rcv_nxt, rcv_wnd, d);
	d[3] = 6u | GCL_SHUT_TCP_FIN_ACK << 8 | 5u << 16;
	d[8] = snd_nxt;
	d[9] = snd_nxt + 1;
	d[10] = (uint32_t)now;
	d[11] = (uint32_t)(now >> 32);
	d[12] = (uint32_t)frame_off;
	d[13] = (uint32_t)(frame_off >> 32);
	d[14] = GCL_SHUT_TCP_FIN_ACK | 5u << 8 | (uint32_t)GCL_TXQE_INFLIGHT << 16;
	d[15] = 0;
}

#endif /* GCL_TCPSHUT_H */
