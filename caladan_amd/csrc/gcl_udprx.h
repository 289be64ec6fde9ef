/*
 * gcl_udprx.h - the rule of gcl_udp_rx (include/gclassify.h), shared by the
 * host twin (gcl_host.c, plain C) and the GPU kernels (gcl_udprx.hip): both
 * include this file.  Not installed.  Plain C without libc.
 *
 * It restates udp_conn_recv (runtime/net/udp.c:79-107) and udp_par_recv
 * (:811-840) in the pieces the two sides need apart:
 *
 *   gcl_udprx_class  what gcl_pay_rule's word and the cookie make of an entry:
 *                    NA, NOSOCK, or a datagram of socket s (both sides)
 *   gcl_udprx_step   one datagram against a socket's RUNNING inq_len, as the
 *                    reference does it under inq_lock (the host twin only)
 *   gcl_udprx_closed the same verdict from the datagram's rank k among its
 *                    socket's datagrams, with no running state (the kernels
 *                    only):  a datagram of a live, non-spawner socket is
 *                    QUEUED iff (int64)inq_len + k < inq_cap, and sets POLLIN
 *                    iff inq_len + k == 0
 *   gcl_udprx_after  a socket's words after a run of n datagrams, in closed
 *                    form (the kernels only; the twin counts as it walks)
 *
 * Why the closed form holds: only a QUEUED entry moves the running inq_len,
 * by one, and once an entry is FULL every later one is, so the first
 * min(n, max(0, inq_cap - inq_len)) datagrams of a run are QUEUED and datagram
 * k of them finds inq_len + k.  The twin does not use it, so the CPU tests and
 * the GPU tests check one form against the other.
 */
#ifndef GCL_UDPRX_H
#define GCL_UDPRX_H

#include <stdint.h>

#include "../../include/gclassify.h"
#include "gcl_pay.h"

#if defined(__HIPCC__)
#define GCL_UDPRX_FN __host__ __device__ static inline
#else
#define GCL_UDPRX_FN static inline
#endif

#define GCL_UDPRX_NONE 0xFFFFFFFFu /* no socket, no record */

/*
 * Entry whose packet gcl_pay_rule described as @r, with cookie @sock: returns
 * GCL_UDPRX_NA, GCL_UDPRX_NOSOCK, or GCL_UDPRX_QUEUED for a datagram, whose
 * socket index (below @nsock) is then in *@s.
 */
GCL_UDPRX_FN uint32_t gcl_udprx_class(const struct gcl_pay_desc *r, uint32_t sock, uint32_t base, uint32_t nsock,
                                      uint32_t *s)
{
	*s = GCL_UDPRX_NONE;
	if (r->kind != GCL_PAY_UDP)
		return GCL_UDPRX_NA;
	if (sock < base || sock - base >= nsock)
		return GCL_UDPRX_NOSOCK;
	*s = sock - base;
	return GCL_UDPRX_QUEUED;
}

/* the remote address and port of a datagram, host order: meta words 0 and 1 of gcl_pay_rule */
GCL_UDPRX_FN uint32_t gcl_udprx_rport(const struct gcl_pay_desc *r)
{
	return r->meta[1] & 0xFFFFu;
}

/* what the socket's flags alone decide: SPAWN, CLOSED, or QUEUED for "ask the queue" */
GCL_UDPRX_FN uint32_t gcl_udprx_sock_class(uint32_t flags)
{
	if (flags & GCL_UDPS_SPAWNER)
		return GCL_UDPRX_SPAWN;
	if (flags & (GCL_UDPS_ERR | GCL_UDPS_SHUTDOWN))
		return GCL_UDPRX_CLOSED;
	return GCL_UDPRX_QUEUED;
}

/* a QUEUED or SPAWN entry has bytes to copy and a record */
GCL_UDPRX_FN int gcl_udprx_taken(uint32_t verdict)
{
	return verdict == GCL_UDPRX_QUEUED || verdict == GCL_UDPRX_SPAWN;
}

/* udp_conn_recv / udp_par_recv for one datagram: *@inq_len is the socket's running word */
GCL_UDPRX_FN uint32_t gcl_udprx_step(int32_t *inq_len, int32_t inq_cap, uint32_t flags, uint32_t *sf)
{
	const uint32_t cls = gcl_udprx_sock_class(flags);

	*sf = 0;
	if (cls != GCL_UDPRX_QUEUED)
		return cls;
	if (*inq_len >= inq_cap)
		return GCL_UDPRX_FULL;
	if (*inq_len == 0)
		*sf = GCL_UDPRX_SF_POLLIN;
	*inq_len += 1; /* below inq_cap: no overflow */
	return GCL_UDPRX_QUEUED;
}

/* the verdict of the datagram that has @k datagrams of its socket before it */
GCL_UDPRX_FN uint32_t gcl_udprx_closed(int32_t inq_len, int32_t inq_cap, uint32_t flags, uint32_t k, uint32_t *sf)
{
	const uint32_t cls = gcl_udprx_sock_class(flags);
	const int64_t at = (int64_t)inq_len + (int64_t)k;

	*sf = 0;
	if (cls != GCL_UDPRX_QUEUED)
		return cls;
	if (at >= (int64_t)inq_cap)
		return GCL_UDPRX_FULL;
	if (at == 0)
		*sf = GCL_UDPRX_SF_POLLIN;
	return GCL_UDPRX_QUEUED;
}

/* struct gcl_udp_sock_out after a run of @n datagrams, as four dwords */
GCL_UDPRX_FN void gcl_udprx_after(int32_t inq_len, int32_t inq_cap, uint32_t flags, uint32_t n, uint32_t o[4])
{
	const uint32_t cls = gcl_udprx_sock_class(flags);
	uint32_t taken = 0, pollin = 0;
	int32_t after = inq_len;

	if (cls == GCL_UDPRX_SPAWN) {
		taken = n;
	} else if (cls == GCL_UDPRX_QUEUED) {
		const int64_t room = (int64_t)inq_cap - (int64_t)inq_len;

		taken = room <= 0 ? 0 : (int64_t)n < room ? n : (uint32_t)room;
		after = (int32_t)((int64_t)inq_len + taken); /* <= inq_cap */
		pollin = inq_len <= 0 && -(int64_t)inq_len < (int64_t)taken;
	}
	o[0] = (uint32_t)after;
	o[1] = taken;
	o[2] = n - taken;
	o[3] = pollin ? GCL_UDPRX_SF_POLLIN : 0;
}

/* what gcl_udp_rx and its host twin both refuse, the ctx and the workspace apart (host code) */
static inline int gcl_udprx_refused(const struct gcl_batch *b, const struct gcl_udprx_in *in,
                                    const struct gcl_udprx_out *out, const uint64_t *counts)
{
	if (!b || !in || !out || in->size != sizeof(*in) || !gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || in->m > (1ull << 31) || in->nsock > GCL_SOCK_MAX_ENTRIES ||
	    in->blocks > GCL_UDPRX_MAX_BLOCKS || !in->sock || !out->rec_off || !out->sock_off)
		return 1;
	if (in->nsock && (!in->usock || !out->out_sock))
		return 1;
	if (in->m && (!out->verdict || !out->sflags || !out->copy_len || !out->dst_off || !out->rec_idx || !out->rec))
		return 1;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->usock & 15) ||
	    ((uintptr_t)out->copy_len & 1) || ((uintptr_t)out->dst_off & 7) || ((uintptr_t)out->rec_idx & 3) ||
	    ((uintptr_t)out->rec & 15) || ((uintptr_t)out->out_sock & 15) || ((uintptr_t)out->rec_off & 3) ||
	    ((uintptr_t)out->sock_off & 7) || ((uintptr_t)counts & 7))
		return 1;
	return in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	                 (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	                 !b->pkt_len || ((uintptr_t)b->pkt_len & 1));
}

#endif /* GCL_UDPRX_H */
