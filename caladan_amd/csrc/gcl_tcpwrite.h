/*
 * gcl_tcpwrite.h - the rule of gcl_tcp_write (include/gclassify.h), shared by
 * the host twin (gcl_host.c, plain C) and the GPU kernels (gcl_tcpwrite.hip):
 * both include this file.  Not installed.  Plain C without libc.
 *
 * One connection's write restates tcp_write_wait (runtime/net/tcp.c:
 * 1259-1307), tcp_write3 / tcp_writev2 (:1362-1422), tcp_write_finish
 * (:1309-1349) and tcp_tx_send (tcp_out.c:313-386).  The host twin runs the
 * reference's loops, one pass of tcp_tx_send's do ... while after the other;
 * the kernels reach the same numbers through the closed forms below
 * (gcl_wr_send_rule for one tcp_tx_send, gcl_wr_pass_at for its pass j) and
 * share with the twin everything that is not a loop: the ranges, the wait, the
 * flags and the words of a connection, a segment and an item.
 *
 * A write is given as the twelve little-endian dwords of its struct
 * gcl_tcp_wr: w[0..1] src_off, w[2] len, w[3] tx_last_ack, w[4..5]
 * pend_frame_off, w[6] pend_len, w[7] err, w[8] snd_mss | ecn << 16 | flags <<
 * 24.
 */
#ifndef GCL_TCPWRITE_H
#define GCL_TCPWRITE_H

#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_WR_FN __host__ __device__ static inline
#else
#define GCL_WR_FN static inline
#endif

#define GCL_WR_EAGAIN  11
#define GCL_WR_EPIPE   32
#define GCL_WR_ENOSPC  28
#define GCL_WR_ENOBUFS 105
#define GCL_WR_HDR     54u    /* Ethernet + IPv4 + TCP without options */
#define GCL_WR_TCPHDR  20u    /* sizeof(struct tcp_hdr): tcp_out.c:359-360 */
#define GCL_WR_TCP_ACK  0x10u
#define GCL_WR_TCP_PUSH 0x08u
#define GCL_WR_NOSLOT  0xFFFFFFFFu /* the held segment is the tx_pending that came in */

/* inc/base/stddef.h: a <= b on the sequence circle */
GCL_WR_FN int gcl_wr_wraps_lte(uint32_t a, uint32_t b)
{
	return (int32_t)(a - b) <= 0;
}

GCL_WR_FN uint32_t gcl_wr_mss(const uint32_t w[12])
{
	return w[8] & 0xFFFFu;
}

GCL_WR_FN uint32_t gcl_wr_flags(const uint32_t w[12])
{
	return w[8] >> 24;
}

/*
 * The vectors of connection @c: their number, *first, and *bad when the write
 * is refused for them (rule 2): no voff, a range that is inverted or not
 * inside [0, nvec], or more than GCL_WR_MAX_IOV of them.
 */
GCL_WR_FN uint32_t gcl_wr_range(const uint32_t *voff, uint32_t c, uint64_t nvec, uint32_t *first, uint32_t *bad)
{
	*first = 0;
	if (!voff) {
		*bad = 1;
		return 0;
	}
	const uint32_t lo = voff[c], hi = voff[c + 1];
	if (lo > hi || hi > nvec || hi - lo > GCL_WR_MAX_IOV) {
		*bad = 1;
		return 0;
	}
	*first = lo;
	return hi - lo;
}

/* the vectors a write names that take room in the walk's table: counted for every wanted vector write */
GCL_WR_FN uint32_t gcl_wr_named(const uint32_t w[12], const uint32_t *voff, uint32_t c, uint64_t nvec)
{
	uint32_t first, bad = 0;
	const uint32_t fl = gcl_wr_flags(w);

	if ((fl & (GCL_WR_WANT | GCL_WR_VEC)) != (GCL_WR_WANT | GCL_WR_VEC))
		return 0;
	return gcl_wr_range(voff, c, nvec, &first, &bad);
}

struct gcl_wr_res {
	int64_t  ret;
	uint32_t status, flags, winlen;
};

/*
 * Rules 1-4: fills *@r for a connection that does not go ahead and returns 0,
 * or returns 1 with r->winlen and r->flags as rule 5 starts.  @bad: rule 2's
 * vector causes (looked at with GCL_WR_VEC alone).
 */
GCL_WR_FN int gcl_wr_wait(const uint32_t w[12], uint32_t bad, uint32_t snd_una, uint32_t snd_wnd, uint32_t snd_nxt,
                          uint32_t frame_stride, struct gcl_wr_res *r)
{
	const uint32_t fl = gcl_wr_flags(w), mss = gcl_wr_mss(w);
	const int full = gcl_wr_wraps_lte(snd_una + snd_wnd, snd_nxt);

	r->ret = 0;
	r->flags = 0;
	r->winlen = 0;
	r->status = GCL_WRS_NONE;
	if (!(fl & GCL_WR_WANT))
		return 0;
	if (((fl & GCL_WR_VEC) && bad) || mss == 0 || w[6] > mss || GCL_WR_HDR + mss > frame_stride) {
		r->status = GCL_WRS_REFUSED;
		return 0;
	}
	/* tcp.c:1267 */
	if (!(fl & GCL_WR_TX_CLOSED) && ((fl & (GCL_WR_BELOW_EST | GCL_WR_TX_EXCL)) || full)) {
		if (full && !(fl & GCL_WR_ZERO_WND))
			r->flags = GCL_WRO_ZWND_ARM;
		if (fl & GCL_WR_NONBLOCK) {
			r->status = GCL_WRS_AGAIN;
			r->ret = -GCL_WR_EAGAIN;
		} else {
			r->status = GCL_WRS_BLOCK;
		}
		return 0;
	}
	if (fl & GCL_WR_ZERO_WND) /* :1285 */
		r->flags = GCL_WRO_ZWND_CLEAR;
	if (fl & GCL_WR_TX_CLOSED) {
		const int32_t err = (int32_t)w[7];
		r->status = GCL_WRS_CLOSED;
		r->ret = err ? -(int64_t)err : -GCL_WR_EPIPE;
		return 0;
	}
	r->winlen = snd_una + snd_wnd - snd_nxt;
	if (!(fl & GCL_WR_VEC) && (fl & GCL_WR_NO_PARTIAL) && r->winlen < w[2]) {
		r->status = GCL_WRS_NOSPC;
		r->ret = -GCL_WR_ENOSPC;
		return 0;
	}
	r->flags |= GCL_WRO_ACKS_RESET | GCL_WRO_TXWAKE;
	r->status = GCL_WRS_DONE;
	return 1;
}

/* rule 8 and the NOSPACE test of a write that went ahead, once its numbers are known */
GCL_WR_FN uint32_t gcl_wr_finish_flags(uint32_t flags, uint32_t nseg, uint32_t rcv_nxt, uint32_t tx_last_ack,
                                       uint32_t snd_una, uint32_t snd_wnd, uint32_t snd_nxt_out)
{
	if (nseg == 0 && rcv_nxt != tx_last_ack) /* tcp.c:1322 with tcp_out.c:60 */
		flags |= GCL_WRO_ACK_TS;
	if (gcl_wr_wraps_lte(snd_una + snd_wnd, snd_nxt_out)) /* :1341 */
		flags |= GCL_WRO_POLLOUT_CLEAR;
	return flags;
}

/* the slots that fit behind frame_base: UINT64_MAX without frames_len */
GCL_WR_FN uint64_t gcl_wr_slot_cap(uint64_t frames_len, uint64_t frame_base, uint32_t stride)
{
	if (!frames_len)
		return UINT64_MAX;
	return frames_len < frame_base ? 0 : (frames_len - frame_base) / stride;
}

GCL_WR_FN int gcl_wr_fits(uint64_t S, uint32_t nseg, uint64_t seg_cap, uint64_t I, uint32_t nitems, uint64_t item_cap,
                          uint64_t K, uint32_t nslots, uint64_t slot_cap)
{
	return S + nseg <= seg_cap && I + nitems <= item_cap && K + nslots <= slot_cap;
}

/* one tcp_tx_send(X, push) that finds @h bytes held, in closed form */
struct gcl_wr_send {
	uint32_t passes;  /* of the do ... while: the items */
	uint32_t sent;    /* segments sent: passes, less the one that ends held */
	uint32_t slots;   /* new segments: passes, less the continued one */
	uint32_t h_out;   /* bytes held behind it */
	uint32_t is_short; /* its tail went out by the under-20 rule */
	uint32_t a0;      /* what the continued segment took */
};

GCL_WR_FN struct gcl_wr_send gcl_wr_send_rule(uint32_t mss, uint32_t h, uint32_t X, uint32_t push)
{
	struct gcl_wr_send r;
	uint32_t fill;

	r.a0 = h ? (X < mss - h ? X : mss - h) : 0;
	const uint32_t R = X - r.a0, nnew = R ? (R - 1) / mss + 1 : 0; /* the bytes and the passes of new segments */
	if (h) {
		r.passes = 1 + nnew;
		fill = nnew ? R - (nnew - 1) * mss : h + r.a0;
	} else {
		r.passes = nnew ? nnew : 1; /* X == 0 still makes a pass */
		fill = nnew ? R - (nnew - 1) * mss : 0;
	}
	const uint32_t held = !push && fill >= GCL_WR_TCPHDR; /* (size_t)(fill - 20) < mss with fill <= mss */
	r.is_short = !push && fill < GCL_WR_TCPHDR;
	r.sent = r.passes - held;
	r.slots = r.passes - (h ? 1u : 0u);
	r.h_out = held ? fill : 0;
	return r;
}

/* where the walk over a connection's vectors stands */
struct gcl_wr_walk {
	uint32_t S;      /* bytes taken */
	uint32_t h;      /* bytes held */
	uint32_t segs, items, slots; /* sent, passes, new segments so far */
	uint32_t hslot;  /* the held segment's slot among the connection's, or GCL_WR_NOSLOT */
	uint32_t shorts, pushes;
};

GCL_WR_FN void gcl_wr_walk_init(struct gcl_wr_walk *s, uint32_t pend_len)
{
	s->S = s->segs = s->items = s->slots = s->shorts = s->pushes = 0;
	s->h = pend_len;
	s->hslot = GCL_WR_NOSLOT;
}

/*
 * What vector (@len, @last) sends with @left of the window: returns 0 when
 * tcp_writev2's loop passes it over (:1406-1409), else 1 with *X and *push.
 * @plain: tcp_write3's one call, which is made whatever len is.
 */
GCL_WR_FN int gcl_wr_vec_send(uint32_t len, uint32_t left, int last, int plain, uint32_t *X, uint32_t *push)
{
	*X = len < left ? len : left;
	*push = plain ? 1u : (last && len <= left);
	return plain || (left != 0 && len != 0);
}

/* the walk steps over one vector */
GCL_WR_FN void gcl_wr_step(struct gcl_wr_walk *s, uint32_t mss, uint32_t winlen, uint32_t len, int last, int plain)
{
	uint32_t X, push;

	if (!gcl_wr_vec_send(len, winlen - s->S, last, plain, &X, &push))
		return;
	const struct gcl_wr_send r = gcl_wr_send_rule(mss, s->h, X, push);
	if (r.h_out && !(s->h && r.passes == 1))
		s->hslot = s->slots + r.slots - 1; /* the last new segment */
	s->S += X;
	s->h = r.h_out;
	s->segs += r.sent;
	s->items += r.passes;
	s->slots += r.slots;
	s->shorts += r.is_short;
	s->pushes += push;
}

/* pass @j < passes of a tcp_tx_send(X, push) that the walk reached in state *@s */
struct gcl_wr_pass {
	uint32_t off;    /* bytes of the send before it */
	uint32_t take;
	uint32_t fill0;  /* bytes in its segment before */
	uint32_t slot;   /* the segment's slot among the connection's, or GCL_WR_NOSLOT */
	uint32_t seq;    /* seg_seq less the connection's snd_nxt as it came */
	uint32_t tcp_flags;
	uint32_t sent;   /* 0: it ends held */
};

GCL_WR_FN struct gcl_wr_pass gcl_wr_pass_at(const struct gcl_wr_walk *s, uint32_t mss, uint32_t X, uint32_t push,
                                            uint32_t j)
{
	struct gcl_wr_pass p;
	const uint32_t h = s->h, a0 = h ? (X < mss - h ? X : mss - h) : 0;

	if (h && j == 0) {
		p.off = 0;
		p.take = a0;
		p.fill0 = h;
		p.slot = s->hslot;
	} else {
		const uint32_t jj = h ? j - 1 : j;
		p.off = a0 + jj * mss;
		p.take = X - p.off < mss ? X - p.off : mss;
		p.fill0 = 0;
		p.slot = s->slots + jj;
	}
	const uint32_t rest = X - p.off - p.take;
	p.seq = s->S + p.off - p.fill0;
	p.tcp_flags = GCL_WR_TCP_ACK | (push && rest == 0 ? GCL_WR_TCP_PUSH : 0);
	p.sent = !(rest == 0 && !push && p.fill0 + p.take >= GCL_WR_TCPHDR);
	return p;
}

/* where the segment in slot @slot of a connection whose first slot is @k0 lies */
GCL_WR_FN uint64_t gcl_wr_frame(uint32_t slot, uint64_t k0, uint64_t pend_frame_off, uint64_t frame_base,
                                uint32_t stride)
{
	return slot == GCL_WR_NOSLOT ? pend_frame_off : frame_base + (k0 + slot) * stride;
}

/* out_conn[c] as twelve dwords, every byte */
GCL_WR_FN void gcl_wr_conn_words(int64_t ret, uint32_t snd_nxt, uint32_t first_seg, uint32_t nseg, uint32_t first_item,
                                 uint32_t nitems, uint32_t pend_len, uint64_t pend_frame_off, uint32_t status,
                                 uint32_t flags, uint32_t w[12])
{
	w[0] = (uint32_t)(uint64_t)ret;
	w[1] = (uint32_t)((uint64_t)ret >> 32);
	w[2] = snd_nxt;
	w[3] = first_seg;
	w[4] = nseg;
	w[5] = first_item;
	w[6] = nitems;
	w[7] = pend_len;
	w[8] = (uint32_t)pend_frame_off;
	w[9] = (uint32_t)(pend_frame_off >> 32);
	w[10] = (status & 0xFFu) | (flags & 0xFFu) << 8;
	w[11] = 0;
}

/*
 * Sent segment @k < seg_cap of the call as sixteen dwords: d[0..7] its
 * gcl_txh_desc, d[8..11] its gcl_txq_ent, d[12..15] its gcl_txq_cold.  @a:
 * struct gcl_tcp_addr as four dwords.  win: tcp_out.c:74 as gcl_ctl_desc
 * (gcl_tcptmr.h) has it.
 */
GCL_WR_FN void gcl_wr_seg_words(const uint32_t a[4], uint32_t ecn, uint32_t tcp_flags, uint32_t seq, uint32_t ack,
                                uint32_t rcv_wnd, uint32_t paylen, uint64_t frame_off, uint64_t now, uint32_t d[16])
{
	d[0] = a[0];
	d[1] = a[1];
	d[2] = a[2];
	d[3] = 6u | tcp_flags << 8 | 5u << 16 | (ecn & 0xFFu) << 24;
	d[4] = seq;
	d[5] = ack;
	d[6] = ((rcv_wnd >> (a[3] & 31u)) & 0xFFFFu) | paylen << 16;
	d[7] = 0;
	d[8] = seq;
	d[9] = seq + paylen;
	d[10] = (uint32_t)now;
	d[11] = (uint32_t)(now >> 32);
	d[12] = (uint32_t)frame_off;
	d[13] = (uint32_t)(frame_off >> 32);
	d[14] = tcp_flags | 5u << 8 | (uint32_t)GCL_TXQE_INFLIGHT << 16;
	d[15] = 0;
}

#endif /* GCL_TCPWRITE_H */
