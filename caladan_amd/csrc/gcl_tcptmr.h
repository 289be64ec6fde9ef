/*
 * gcl_tcptmr.h - the rules of gcl_tcp_tick and gcl_tcp_rx_acks
 * (include/gclassify.h), shared by the host twins (gcl_host.c, plain C) and
 * the GPU kernels (gcl_tcptmr.hip): both include this file, so the CPU tests
 * and the sanitizer driver run the very rules the GPU runs.  Not installed.
 * Plain C without libc.
 *
 * gcl_tmr_sweep restates tcp_worker's test, tcp_handle_timeouts and
 * tcp_timer_update (runtime/net/tcp.c:166, :80-140, :46-77) for one
 * connection at one clock reading.  The one departure: tcp_timer_update reads
 * microtime() again for its out-of-order term (tcp.c:74); a sweep has one
 * clock reading, so that term is now + OOQ_ACK.
 *
 * gcl_ctl_desc is the segment tcp_tx_ack and tcp_tx_probe_window send
 * (runtime/net/tcp_out.c:178-228 with __tcp_add_tcphdr, :54-81) as a
 * gcl_txh_desc; gcl_rxack_want and gcl_rxack_wnd are the guards and the
 * window of an ACK that follows a gcl_tcp_rx call.
 */
#ifndef GCL_TCPTMR_H
#define GCL_TCPTMR_H

#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_TMR_FN __host__ __device__ static inline
#else
#define GCL_TMR_FN static inline
#endif

/* runtime/net/tcp.h:21-26, in microseconds */
#define GCL_TMR_T_ACK        10000ull
#define GCL_TMR_T_CONNECT    5000000ull
#define GCL_TMR_T_OOQ_ACK    300000ull
#define GCL_TMR_T_TIME_WAIT  1000000ull
#define GCL_TMR_T_ZERO_WND   300000ull
#define GCL_TMR_T_RETRANSMIT 300000ull

GCL_TMR_FN uint64_t gcl_tmr_min(uint64_t a, uint64_t b)
{
	return a < b ? a : b;
}

/*
 * The sweep of one connection: fills every byte of *@o and returns the action
 * (without GCL_TMRA_NOSPACE, which only the layout of the segments knows).
 */
GCL_TMR_FN uint32_t gcl_tmr_sweep(const struct gcl_tcp_tmr *t, uint64_t now, struct gcl_tcp_tmr_out *o)
{
	uint32_t flags = t->flags, action = 0;
	const uint32_t state = t->state;
	uint64_t zero_wnd_ts = t->zero_wnd_ts, nt;

	o->next_timeout = t->next_timeout;
	o->zero_wnd_ts = zero_wnd_ts;
	o->state = (uint8_t)state;
	o->flags = (uint8_t)flags;
	o->action = 0;
	for (int i = 0; i < 13; i++)
		o->pad[i] = 0;
	/* tcp.c:166 */
	if (!(flags & GCL_TMR_LIVE) || t->next_timeout > now)
		return 0;
	action = GCL_TMRA_FIRED;
	o->action = (uint8_t)action;
	/* :85-88 */
	if (state == GCL_TCP_STATE_CLOSED)
		return action;
	/* :90-95 */
	if (state < GCL_TCP_STATE_ESTABLISHED && now - t->attach_ts >= GCL_TMR_T_CONNECT) {
		action |= GCL_TMRA_FAIL;
		o->state = GCL_TCP_STATE_CLOSED;
		o->action = (uint8_t)action;
		return action;
	}
	/* :97-104 */
	if (state == GCL_TCP_STATE_TIME_WAIT && now - t->time_wait_ts >= GCL_TMR_T_TIME_WAIT) {
		action |= GCL_TMRA_CLOSE;
		o->state = GCL_TCP_STATE_CLOSED;
		o->action = (uint8_t)action;
		return action;
	}
	/* :106-110 */
	if ((flags & GCL_TMR_ACK_DELAYED) && now - t->ack_ts >= GCL_TMR_T_ACK) {
		flags &= ~(uint32_t)GCL_TMR_ACK_DELAYED;
		action |= GCL_TMRA_ACK;
	}
	/* :112-116 */
	if ((flags & GCL_TMR_ZERO_WND) && now - zero_wnd_ts >= GCL_TMR_T_ZERO_WND) {
		zero_wnd_ts = now;
		action |= GCL_TMRA_PROBE;
	}
	/* :118-126 */
	if (!(flags & GCL_TMR_TX_EXCLUSIVE) && (flags & GCL_TMR_TXQ) && now - t->txq_ts >= GCL_TMR_T_RETRANSMIT)
		action |= GCL_TMRA_RETRANSMIT;
	/* :128 */
	if (flags & GCL_TMR_OOO)
		action |= GCL_TMRA_ACK;
	/* :130, tcp_timer_update, :46-77 */
	nt = UINT64_MAX;
	if (state == GCL_TCP_STATE_TIME_WAIT)
		nt = t->time_wait_ts + GCL_TMR_T_TIME_WAIT;
	if (state < GCL_TCP_STATE_ESTABLISHED)
		nt = t->attach_ts + GCL_TMR_T_CONNECT;
	if (flags & GCL_TMR_ACK_DELAYED)
		nt = gcl_tmr_min(nt, t->ack_ts + GCL_TMR_T_ACK);
	if (flags & GCL_TMR_ZERO_WND)
		nt = gcl_tmr_min(nt, zero_wnd_ts + GCL_TMR_T_ZERO_WND);
	if (!(flags & GCL_TMR_TX_EXCLUSIVE) && (flags & GCL_TMR_TXQ))
		nt = gcl_tmr_min(nt, t->txq_ts + GCL_TMR_T_RETRANSMIT);
	if (flags & GCL_TMR_OOO)
		nt = gcl_tmr_min(nt, now + GCL_TMR_T_OOQ_ACK); /* the reference: microtime() again */
	o->next_timeout = nt;
	o->zero_wnd_ts = zero_wnd_ts;
	o->flags = (uint8_t)flags;
	o->action = (uint8_t)action;
	return action;
}

/* the segments an action asks for: bit 0 the ACK, bit 1 the probe, in send order */
GCL_TMR_FN uint32_t gcl_tmr_segs(uint32_t action)
{
	return ((action & GCL_TMRA_ACK) ? 1u : 0u) | ((action & GCL_TMRA_PROBE) ? 2u : 0u);
}

/* tcp_tx_ack (@kind GCL_CTL_ACK) and tcp_tx_probe_window: m->seg_seq, tcp_out.c:188, :219 */
GCL_TMR_FN uint32_t gcl_ctl_seq(uint32_t kind, uint32_t snd_una, uint32_t snd_nxt)
{
	return kind == GCL_CTL_PROBE ? snd_una - 1 : snd_nxt;
}

/*
 * struct gcl_txh_desc as eight dwords: TCP_ACK, off 5, no payload, no ECN;
 * @a: struct gcl_tcp_addr as four dwords.  win: tcp_out.c:74, hton16 of
 * win >> rcv_wscale truncates.
 */
GCL_TMR_FN void gcl_ctl_desc(const uint32_t a[4], uint32_t seq, uint32_t ack, uint32_t rcv_wnd, uint32_t d[8])
{
	d[0] = a[0];
	d[1] = a[1];
	d[2] = a[2];
	d[3] = 6u | 0x10u << 8 | 5u << 16;
	d[4] = seq;
	d[5] = ack;
	d[6] = (rcv_wnd >> (a[3] & 31u)) & 0xFFFFu;
	d[7] = 0;
}

/* the entry of a gcl_tcp_rx call asks for an ACK (tcp_in.c:289-290) */
GCL_TMR_FN int gcl_rxack_asked(uint32_t verdict, uint32_t sflags)
{
	return verdict == GCL_TCPRX_FAST && (sflags & GCL_TCPRX_SF_ACK_NOW) != 0;
}

/* the receive window as it stood after the segment that left rcv_nxt at @after */
GCL_TMR_FN uint32_t gcl_rxack_wnd(uint32_t rcv_wnd, uint32_t rcv_nxt, uint32_t after)
{
	return rcv_wnd - (after - rcv_nxt);
}

/*
 * gcl_tcp_rx_ctl: the one control segment list entry j of a gcl_tcp_rx_states
 * call asks for, or GCL_RXCTL_NONE.  Every send_rst path of __tcp_rx_conn goes
 * to done with do_ack false (tcp_in.c:372-376, :452-456, :462-468), so an entry
 * has at most one; the ACK is asked first, as gcl_tcp_rx_acks asks it.
 */
#define GCL_RXCTL_NONE 0xFFu
GCL_TMR_FN uint32_t gcl_rxctl_kind(uint32_t verdict, uint32_t sflags, uint32_t ev)
{
	if (verdict != GCL_TCPRX_FAST)
		return GCL_RXCTL_NONE;
	if (sflags & GCL_TCPRX_SF_ACK_NOW)
		return GCL_CTL_ACK;
	if (ev & GCL_TCPS_RST)
		return GCL_CTL_RST;
	if (ev & GCL_TCPS_RST_ACK)
		return GCL_CTL_RST_ACK;
	return GCL_RXCTL_NONE;
}

/*
 * struct gcl_txh_desc of tcp_tx_raw_rst (runtime/net/tcp_out.c:98-128: flags
 * RST, seq = @rst_seq, ack 0) or tcp_tx_raw_rst_ack (:139-170: flags RST|ACK,
 * seq 0, ack = @rst_seq): off 5, win 0, no payload.
 */
GCL_TMR_FN void gcl_ctl_rst_desc(const uint32_t a[4], uint32_t kind, uint32_t rst_seq, uint32_t d[8])
{
	const uint32_t fl = kind == GCL_CTL_RST ? 0x04u : 0x14u;

	d[0] = a[0];
	d[1] = a[1];
	d[2] = a[2];
	d[3] = 6u | fl << 8 | 5u << 16;
	d[4] = kind == GCL_CTL_RST ? rst_seq : 0;
	d[5] = kind == GCL_CTL_RST ? 0 : rst_seq;
	d[6] = 0;
	d[7] = 0;
}

#endif /* GCL_TCPTMR_H */
