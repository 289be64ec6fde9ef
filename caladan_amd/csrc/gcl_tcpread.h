/*
 * gcl_tcpread.h - the rule of gcl_tcp_read (include/gclassify.h), shared by
 * the host twin (gcl_host.c, plain C) and the GPU kernels (gcl_tcpread.hip):
 * both include this file.  Not installed.  Plain C without libc.
 *
 * One connection's read restates tcp_wait_rx (runtime/net/tcp.c:850-876),
 * tcp_read_wait (:878-934) and tcp_read_wait_peek (:963-988); the copy items
 * are what copy_mbufs_to_buf (:1013-1038) and copy_into_iov (:1133-1185)
 * memcpy.  The host twin walks the queue as the reference does
 * (gcl_rd_walk, gcl_rd_items_walk); the kernels reach the same numbers
 * through prefix sums and searches and share with it everything that is not a
 * walk: the ranges, the wait, the ACK test, the flags and one item's words.
 */
#ifndef GCL_TCPREAD_H
#define GCL_TCPREAD_H

#include <stdint.h>

#include "../../include/gclassify.h"

#if defined(__HIPCC__)
#define GCL_RD_FN __host__ __device__ static inline
#else
#define GCL_RD_FN static inline
#endif

#define GCL_RD_EAGAIN 11

/* inc/base/stddef.h:176 */
GCL_RD_FN int gcl_rd_wraps_gte(uint32_t a, uint32_t b)
{
	return (int32_t)(b - a) <= 0;
}

/* a range of a CSR over @total elements: its length, 0 and *bad when it is not inside [0, total] */
GCL_RD_FN uint32_t gcl_rd_range(uint32_t lo, uint32_t hi, uint64_t total, uint32_t *first, uint32_t *bad)
{
	*first = lo;
	if (lo > hi || hi > total) {
		*first = 0;
		*bad = 1;
		return 0;
	}
	return hi - lo;
}

/* what a connection's read comes to */
struct gcl_rd_res {
	int64_t  ret;
	uint64_t nitems;       /* the items it wants: ne + nv - 1, or 0 */
	uint32_t npop, pull, rcv_wnd;
	uint32_t status, flags;
	uint32_t ne, nv;       /* entries and vectors the copy touches */
};

/*
 * Rules 1-3: fills *@r for a connection that is not read and returns 0, or
 * returns 1: the queue is read (rule 4 or 5).  @rdflags: gcl_tcp_rd.flags; @n:
 * the queue's length; @bad: a range of it was bad.
 */
GCL_RD_FN int gcl_rd_wait(uint32_t rdflags, uint32_t n, int32_t err, uint32_t bad, uint32_t rcv_wnd,
                          struct gcl_rd_res *r)
{
	r->ret = 0;
	r->nitems = 0;
	r->npop = r->pull = r->flags = r->ne = r->nv = 0;
	r->rcv_wnd = rcv_wnd;
	r->status = GCL_RDS_NONE;
	if (bad) {
		r->status = GCL_RDS_BADRANGE;
		return 0;
	}
	if (!(rdflags & GCL_RD_WANT))
		return 0;
	/* tcp.c:858 */
	if (!(rdflags & GCL_RD_RX_CLOSED) && ((rdflags & GCL_RD_RX_EXCL) || n == 0)) {
		if (rdflags & GCL_RD_NONBLOCK) {
			r->status = GCL_RDS_AGAIN;
			r->ret = -GCL_RD_EAGAIN;
		} else {
			r->status = GCL_RDS_BLOCK;
		}
		return 0;
	}
	/* :870 */
	if (rdflags & GCL_RD_RX_CLOSED) {
		r->status = GCL_RDS_CLOSED;
		r->ret = -(int64_t)err;
		return 0;
	}
	r->status = GCL_RDS_DONE;
	return 1;
}

/* rule 4 once ret = min(A_n, L) is known */
GCL_RD_FN void gcl_rd_peek_done(struct gcl_rd_res *r, uint64_t ret)
{
	r->ret = (int64_t)ret;
	r->flags = ret ? GCL_RDO_RXWAKE : GCL_RDO_EXCL_LEFT;
}

/*
 * Rule 5b, 5c once the walk's numbers are known: @readlen, @npop, @pull,
 * @closed (an examined entry had FIN); @n the queue's length.
 */
GCL_RD_FN void gcl_rd_read_done(struct gcl_rd_res *r, uint64_t readlen, uint32_t npop, uint32_t pull, int closed,
                                uint32_t n, uint32_t rcv_nxt, uint32_t tx_last_ack, uint32_t tx_last_win,
                                uint32_t winmax)
{
	r->ret = (int64_t)readlen;
	r->npop = npop;
	r->pull = pull;
	r->rcv_wnd += (uint32_t)readlen; /* tcp.c:920 */
	r->flags = (closed ? GCL_RDO_RX_CLOSED : 0u) | (pull ? GCL_RDO_PARTIAL | GCL_RDO_RXWAKE : 0u) |
	           (npop == n ? GCL_RDO_POLLIN_CLEAR : 0u);
	if (gcl_rd_wraps_gte(rcv_nxt + r->rcv_wnd, tx_last_ack + tx_last_win + winmax / 4)) /* :921 */
		r->flags |= GCL_RDO_ACK;
}

/* tcp_read_wait's loop (tcp.c:896-918) over the queue ent[e0, e0 + n) for a read of @len bytes */
GCL_RD_FN uint64_t gcl_rd_walk(const struct gcl_rdq_ent *ent, uint32_t e0, uint32_t n, uint64_t len,
                               uint32_t *npop, uint32_t *pull, int *closed)
{
	uint64_t readlen = 0;
	uint32_t i = 0;

	*pull = 0;
	*closed = 0;
	while (readlen < len) {
		if (i >= n) /* list_top: NULL */
			break;
		const struct gcl_rdq_ent *m = &ent[e0 + i];
		if (m->flags & GCL_RDQE_FIN) {
			*closed = 1;
			if (m->len == 0)
				break;
		}
		if (len - readlen < m->len) {
			*pull = (uint32_t)(len - readlen);
			readlen = len;
			break;
		}
		i++;
		readlen += m->len;
	}
	*npop = i;
	return readlen;
}

/* tcp_read_wait_peek's loop (tcp.c:977-984) */
GCL_RD_FN uint64_t gcl_rd_peek_walk(const struct gcl_rdq_ent *ent, uint32_t e0, uint32_t n, uint64_t len)
{
	uint64_t readlen = 0;

	for (uint32_t i = 0; i < n; i++) {
		readlen += ent[e0 + i].len;
		if (readlen >= len)
			break;
	}
	return readlen < len ? readlen : len;
}

/* out_conn[c] as eight dwords, every byte */
GCL_RD_FN void gcl_rd_conn_words(const struct gcl_rd_res *r, uint32_t first_item, uint32_t nitems, uint32_t flags,
                                 uint32_t w[8])
{
	w[0] = (uint32_t)(uint64_t)r->ret;
	w[1] = (uint32_t)((uint64_t)r->ret >> 32);
	w[2] = r->npop;
	w[3] = r->pull;
	w[4] = r->rcv_wnd;
	w[5] = first_item;
	w[6] = nitems;
	w[7] = (r->status & 0xFFu) | (flags & 0xFFu) << 8;
}

/*
 * The item that spans [@from, @to) of connection @c's stream, in the entry
 * with index @e in ent, data at @eoff, that starts at @ea of the stream, and
 * the vector at @voff that starts at @vb: item @k < item_cap of the call.
 */
GCL_RD_FN void gcl_rd_item_store(const struct gcl_rd_out *o, uint64_t k, uint32_t c, uint32_t e, uint64_t eoff,
                                 uint64_t ea, uint64_t voff, uint64_t vb, uint64_t from, uint64_t to)
{
	o->src_off[k] = eoff + (from - ea);
	o->len[k] = (uint16_t)(to - from);
	o->dst_off[k] = voff + (from - vb);
	o->item_conn[k] = c;
	o->item_ent[k] = e;
}

#endif /* GCL_TCPREAD_H */
