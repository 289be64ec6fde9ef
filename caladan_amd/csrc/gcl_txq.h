/*
 * gcl_txq.h - the rule of gcl_tcp_txq (include/gclassify.h), shared by the
 * host twin (gcl_host.c, plain C) and the GPU kernels (gcl_txq.hip): both
 * include this file, so the CPU tests and the sanitizer driver run the very
 * rule the GPU runs.  Not installed.  Plain C without libc.
 *
 * gcl_txq_conn restates, for one connection at one clock reading,
 * tcp_tx_retransmit (runtime/net/tcp_out.c:480-506), tcp_conn_ack
 * (runtime/net/tcp.c:217-238) and tcp_tx_fast_retransmit_start
 * (tcp_out.c:450-466), in the order tcp_retransmit and tcp_write_finish run
 * them (tcp.c:1425-1444, :1309-1349); gcl_txq_one is tcp_tx_retransmit_one
 * (tcp_out.c:388-444).  Two departures from the reference:
 *   - it computes l4len before the partial-ACK pull and never again (:395
 *     against :431), and so seeds the checksum with the untrimmed length; the
 *     descriptor here carries the trimmed length;
 *   - with options and a partial ACK it pulls option bytes; such an entry is
 *     refused here.  Only a SYN carries options and a SYN has sequence length
 *     1, so consistent input never gets there.
 * The walk and the pops read one entry each per step and do not depend on one
 * another, so they share one pass over the queue.
 */
#ifndef GCL_TXQ_H
#define GCL_TXQ_H

#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_TXQ_FN __host__ __device__ static inline
#else
#define GCL_TXQ_FN static inline
#endif

#define GCL_TXQ_T_RETRANSMIT 300000ull /* TCP_RETRANSMIT_TIMEOUT, runtime/net/tcp.h, us */
#define GCL_TXQ_BATCH 16u              /* TCP_RETRANSMIT_BATCH */
#define GCL_TXQ_HDR 54u                /* Ethernet + IPv4 + TCP without options */
#define GCL_TXQ_NOROOM UINT64_MAX      /* gcl_txq_conn's @room when only the count is asked for */

/* inc/base/stddef.h:144-178 */
GCL_TXQ_FN int gcl_txq_wraps_lt(uint32_t a, uint32_t b)
{
	return (int32_t)(a - b) < 0;
}
GCL_TXQ_FN int gcl_txq_wraps_gt(uint32_t a, uint32_t b)
{
	return (int32_t)(b - a) < 0;
}
GCL_TXQ_FN int gcl_txq_wraps_gte(uint32_t a, uint32_t b)
{
	return (int32_t)(b - a) <= 0;
}

/* the walk's test of one entry: 0 young (break), 1 acknowledged (continue), 2 wanted */
GCL_TXQ_FN uint32_t gcl_txq_due(const struct gcl_txq_ent *h, uint32_t snd_una, uint64_t now)
{
	if (now - h->ts < GCL_TXQ_T_RETRANSMIT) /* tcp_out.c:492 */
		return 0;
	return gcl_txq_wraps_gte(snd_una, h->seg_end) ? 1 : 2; /* :495 */
}

struct gcl_txq_pick {
	uint32_t trim, seq, paylen;
	uint32_t copy, len; /* by copy, and the bytes to copy */
};

/* tcp_tx_retransmit_one up to the header: 0 when the entry is refused */
GCL_TXQ_FN int gcl_txq_one(const struct gcl_txq_ent *h, const struct gcl_txq_cold *q, uint32_t snd_una, int fast,
                           uint32_t frame_stride, struct gcl_txq_pick *p)
{
	const uint32_t off = q->tcp_off;

	/* :430-433 */
	p->trim = gcl_txq_wraps_lt(h->seg_seq, snd_una) ? snd_una - h->seg_seq : 0;
	p->seq = h->seg_seq + p->trim;
	/* :395-397, on the trimmed segment */
	p->paylen = h->seg_end - p->seq - ((q->tcp_flags & 0x03) ? 1u : 0u); /* TCP_SYN | TCP_FIN */
	p->copy = fast || (q->flags & GCL_TXQE_INFLIGHT);                    /* :407, :462 */
	p->len = 0;
	if (off < 5 || off > 15 || p->paylen > 0xFFFFu || (p->trim && off > 5))
		return 0;
	if (p->copy) {
		p->len = 4 * (off - 5) + p->paylen; /* :408 */
		if (p->len > 0xFFFFu || GCL_TXQ_HDR + p->len > frame_stride)
			return 0;
	}
	return 1;
}

/* what a call gives every connection */
struct gcl_txq_call {
	const struct gcl_txq_out *out;
	uint64_t now, frame_base;
	uint32_t frame_stride;
};

/* connection @c's own words */
struct gcl_txq_cx {
	uint32_t c, snd_una, ack, win; /* win as it goes on the wire */
	uint32_t a[3];                 /* the first three dwords of its gcl_tcp_addr */
	uint32_t want;
};

struct gcl_txq_res {
	uint64_t head_ts, bytes;
	uint32_t nacked, nretx, flags;
	uint32_t refused, copied, trimmed;
};

GCL_TXQ_FN void gcl_txq_res_zero(struct gcl_txq_res *r)
{
	r->head_ts = r->bytes = 0;
	r->nacked = r->nretx = r->flags = r->refused = r->copied = r->trimmed = 0;
}

/* struct gcl_txh_desc as eight dwords */
GCL_TXQ_FN void gcl_txq_desc(const struct gcl_txq_cx *x, const struct gcl_txq_cold *q, const struct gcl_txq_pick *p,
                             uint32_t d[8])
{
	d[0] = x->a[0];
	d[1] = x->a[1];
	d[2] = x->a[2];
	d[3] = 6u | (uint32_t)q->tcp_flags << 8 | (uint32_t)q->tcp_off << 16;
	d[4] = p->seq;
	d[5] = x->ack;
	d[6] = x->win | p->paylen << 16;
	d[7] = 0;
}

/* segment @k < seg_cap of the call: entry @e (its index in ent) of connection x->c */
GCL_TXQ_FN void gcl_txq_store(const struct gcl_txq_call *k_, uint64_t k, const struct gcl_txq_cx *x, uint32_t e,
                              const struct gcl_txq_cold *q, const struct gcl_txq_pick *p)
{
	const struct gcl_txq_out *o = k_->out;
	const uint64_t fo = p->copy ? k_->frame_base + k * k_->frame_stride : q->frame_off + p->trim;
	uint32_t d[8];

	gcl_txq_desc(x, q, p, d);
#if defined(__HIP_DEVICE_COMPILE__)
	((uint4 *)&o->desc[k])[0] = make_uint4(d[0], d[1], d[2], d[3]);
	((uint4 *)&o->desc[k])[1] = make_uint4(d[4], d[5], d[6], d[7]);
#else
	struct gcl_txh_desc *t = &o->desc[k];
	t->lip = d[0];
	t->rip = d[1];
	t->lport = (uint16_t)d[2];
	t->rport = (uint16_t)(d[2] >> 16);
	t->proto = 6;
	t->tcp_flags = q->tcp_flags;
	t->tcp_off = q->tcp_off;
	t->ecn = 0;
	t->seq = d[4];
	t->ack = d[5];
	t->win = (uint16_t)d[6];
	t->paylen = (uint16_t)(d[6] >> 16);
	t->pad = 0;
#endif
	o->frame_off[k] = fo;
	o->src_off[k] = q->frame_off + GCL_TXQ_HDR + p->trim;
	o->len[k] = (uint16_t)p->len;
	o->dst_off[k] = fo + GCL_TXQ_HDR;
	o->seg_conn[k] = x->c;
	o->seg_ent[k] = e;
}

/* one wanted entry that is not refused: its state; stores segment @k when @emit */
GCL_TXQ_FN uint32_t gcl_txq_send(const struct gcl_txq_call *k_, uint64_t k, const struct gcl_txq_cx *x, uint32_t e,
                                 const struct gcl_txq_cold *q, const struct gcl_txq_pick *p, int emit,
                                 struct gcl_txq_res *r)
{
	if (emit)
		gcl_txq_store(k_, k, x, e, q, p);
	r->copied += p->copy ? 1u : 0u;
	r->trimmed += p->trim ? 1u : 0u;
	r->bytes += p->len;
	return (p->copy ? GCL_TXQS_RETX_COPY : GCL_TXQS_RETX) | (p->trim ? GCL_TXQS_TRIMMED : 0u);
}

/* step 4 of the rule on the head @e0 + r->nacked, whose state so far is @st; returns its state */
GCL_TXQ_FN uint32_t gcl_txq_fast(const struct gcl_txq_call *k_, const struct gcl_txq_cx *x,
                                 const struct gcl_txq_ent *h, const struct gcl_txq_cold *q, uint32_t e, uint32_t st,
                                 uint64_t first, uint64_t room, int emit, struct gcl_txq_res *r)
{
	struct gcl_txq_pick p;
	const uint32_t was = st & 0x7Fu;

	if (was == GCL_TXQS_RETX || was == GCL_TXQS_RETX_COPY)
		return st;
	if (!gcl_txq_one(h, q, x->snd_una, 1, k_->frame_stride, &p)) {
		r->refused += was == GCL_TXQS_REFUSED ? 0u : 1u;
		return GCL_TXQS_REFUSED;
	}
	if (r->nretx >= room) {
		r->flags |= GCL_TXQO_NOSPACE;
		return GCL_TXQS_NOSPACE;
	}
	st = gcl_txq_send(k_, first + r->nretx, x, e, q, &p, emit, r);
	r->nretx++;
	return st;
}

/* the tail of the rule: head_ts and EMPTY; @head_ts0 is the head's timestamp as it came */
GCL_TXQ_FN void gcl_txq_finish(struct gcl_txq_res *r, uint32_t n, uint32_t head_st, uint64_t head_ts0, uint64_t now)
{
	if (r->nacked >= n) {
		r->flags |= GCL_TXQO_EMPTY;
		r->head_ts = 0;
	} else {
		r->head_ts = (head_st & 0x7Fu) >= GCL_TXQS_RETX ? now : head_ts0;
	}
}

/*
 * The queue [e0, e0 + n) of connection *@x.  @room: the segments that still
 * fit, seg_cap - first, or GCL_TXQ_NOROOM; with @emit the segments are stored
 * at @first onwards.  Writes state[e0, e0 + n) and *@r.
 */
GCL_TXQ_FN void gcl_txq_conn(const struct gcl_txq_call *k_, const struct gcl_txq_cx *x,
                             const struct gcl_txq_ent *ent, const struct gcl_txq_cold *cold, uint32_t e0, uint32_t n,
                             uint64_t first, uint64_t room, int emit, struct gcl_txq_res *r)
{
	uint8_t *state = k_->out->state;
	int walking = (x->want & GCL_TXQ_W_RTO) != 0, popping = 1;
	uint32_t head_st = GCL_TXQS_KEPT;
	uint64_t head_ts0 = 0;

	gcl_txq_res_zero(r);
	if (x->want & GCL_TXQ_W_EXCL) { /* tcp.c:224, :1431, tcp_out.c:456 */
		for (uint32_t i = 0; i < n; i++)
			state[e0 + i] = GCL_TXQS_KEPT;
		r->flags = GCL_TXQO_DEFERRED;
		gcl_txq_finish(r, n, GCL_TXQS_KEPT, n ? ent[e0].ts : 0, k_->now);
		return;
	}
	for (uint32_t i = 0; i < n; i++) {
		const uint32_t e = e0 + i;
		uint32_t st = GCL_TXQS_KEPT;

		if (walking || popping) {
			const struct gcl_txq_ent h = ent[e];

			if (walking) { /* tcp_out.c:490-505 */
				const uint32_t due = gcl_txq_due(&h, x->snd_una, k_->now);

				if (due == 0) {
					walking = 0;
				} else if (due == 2) {
					const struct gcl_txq_cold q = cold[e];
					struct gcl_txq_pick p;

					if (!gcl_txq_one(&h, &q, x->snd_una, 0, k_->frame_stride, &p)) {
						st = GCL_TXQS_REFUSED;
						r->refused++;
					} else if (r->nretx >= room) {
						st = GCL_TXQS_NOSPACE;
						r->flags |= GCL_TXQO_NOSPACE;
						walking = 0;
					} else {
						st = gcl_txq_send(k_, first + r->nretx, x, e, &q, &p, emit, r);
						if (++r->nretx >= GCL_TXQ_BATCH) {
							r->flags |= GCL_TXQO_BATCH;
							walking = 0;
						}
					}
				}
			}
			if (popping) { /* tcp.c:228-237 */
				if (gcl_txq_wraps_gt(h.seg_end, x->snd_una)) {
					popping = 0;
					head_st = st;
					head_ts0 = h.ts;
				} else {
					st = GCL_TXQS_ACKED;
					r->nacked++;
				}
			}
		}
		state[e] = (uint8_t)st;
	}
	if ((x->want & GCL_TXQ_W_FAST) && r->nacked < n) {
		const uint32_t e = e0 + r->nacked;
		const struct gcl_txq_ent h = ent[e];
		const struct gcl_txq_cold q = cold[e];

		head_st = gcl_txq_fast(k_, x, &h, &q, e, head_st, first, room, emit, r);
		state[e] = (uint8_t)head_st;
	}
	gcl_txq_finish(r, n, head_st, head_ts0, k_->now);
}

/* connection @c's range of the CSR: 0 and BADRANGE when it is not inside [0, nent] */
GCL_TXQ_FN uint32_t gcl_txq_range(uint32_t lo, uint32_t hi, uint64_t nent, uint32_t *e0, uint32_t *flags)
{
	*e0 = lo;
	*flags = 0;
	if (lo > hi || hi > nent) {
		*e0 = 0;
		*flags = GCL_TXQO_BADRANGE;
		return 0;
	}
	return hi - lo;
}

/* gcl_txq_cx of connection @c: @c0, @c1 the first two 16-B words of its gcl_tcp_conn, @ad its gcl_tcp_addr */
GCL_TXQ_FN void gcl_txq_cx_fill(struct gcl_txq_cx *x, uint32_t c, uint32_t snd_una, uint32_t rcv_nxt,
                                uint32_t rcv_wnd, const uint32_t ad[4], uint32_t want)
{
	x->c = c;
	x->snd_una = snd_una;
	x->ack = rcv_nxt;
	x->win = (rcv_wnd >> (ad[3] & 31u)) & 0xFFFFu; /* tcp_out.c:74 */
	x->a[0] = ad[0];
	x->a[1] = ad[1];
	x->a[2] = ad[2];
	x->want = want;
}

/* out_conn[c], every byte */
GCL_TXQ_FN void gcl_txq_conn_out(struct gcl_txq_conn_out *o, const struct gcl_txq_res *r, uint32_t flags,
                                 uint64_t first)
{
	o->head_ts = r->head_ts;
	o->nacked = r->nacked;
	o->nretx = r->nretx;
	o->first = (uint32_t)first;
	o->flags = (uint8_t)(r->flags | flags);
	for (int i = 0; i < 11; i++)
		o->pad[i] = 0;
}

#endif /* GCL_TXQ_H */
