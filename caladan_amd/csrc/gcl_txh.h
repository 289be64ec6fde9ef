/*
 * gcl_txh.h - the rule of gcl_tx_hdr (include/gclassify.h) for one entry,
 * shared by the host twin (gcl_host.c, plain C) and the GPU kernel
 * (gcl_txhdr.hip): both include this file, so the CPU tests and the sanitizer
 * driver run the very rule the GPU runs.  Not installed.
 *
 * The rule reads nothing but its arguments and the neighbour table (one
 * probe, gcl_neigh.h) and writes nothing: it returns the header as fourteen
 * little-endian dwords (dword k holds frame bytes 4 k .. 4 k + 3) and says
 * which of those bytes the caller stores.  The Toeplitz hash of a local entry
 * is the caller's (a key walk on the host, the LUT on the device); what
 * follows from it is gcl_txh_cmd and gcl_txh_payload.
 */
#ifndef GCL_TXH_H
#define GCL_TXH_H

#include <stdint.h>

#include "../../include/gclassify.h"
#include "gcl_neigh.h"

#define GCL_TXH_FN GCL_NEIGH_FN

#define GCL_TXH_LOOPBACK 0x7F000001u /* MAKE_IP_ADDR(127, 0, 0, 1) */
/* txpkt cmd.olflags (inc/iokernel/queue.h:36-42) */
#define GCL_TXH_OL_IP_CHKSUM  0x01u
#define GCL_TXH_OL_TCP_CHKSUM 0x02u
#define GCL_TXH_OL_IPV4       0x04u
#define GCL_TXH_OL_LOCAL      0x10u
#define GCL_TXH_OL_LOCAL_HINT 0x40u

/* what one entry gets */
struct gcl_txh_res {
	uint32_t status;   /* GCL_TXH_* */
	uint32_t w[14];    /* frame bytes [0, 56); meaningful where they are stored */
	uint32_t eth;      /* 1: bytes [0, 14) are stored (OK) */
	uint32_t l4end;    /* bytes [14, l4end) are stored unless REFUSED: 42 or 54 */
	uint32_t len;      /* 14 + tot */
	uint32_t pkt_len;  /* the pkt_len output; bytes [len, pkt_len) become 0 when OK */
	uint32_t olflags;  /* the tx_olflags output */
	uint32_t local;    /* OK and the neighbour's mac is net.mac */
	uint32_t nh;       /* the next hop, when looked up */
	uint32_t lport, rport;
};

/* a 16-bit value's two network-order bytes as a little-endian halfword */
GCL_TXH_FN uint32_t gcl_txh_be16(uint32_t x)
{
	return (x >> 8 & 0xFFu) | (x & 0xFFu) << 8;
}

GCL_TXH_FN uint32_t gcl_txh_be32(uint32_t x)
{
	return x >> 24 | (x >> 8 & 0xFF00u) | (x << 8 & 0xFF0000u) | x << 24;
}

/* __raw_cksum_reduce (inc/net/chksum.h:72-78) */
GCL_TXH_FN uint32_t gcl_txh_fold(uint32_t sum)
{
	sum = (sum >> 16) + (sum & 0xFFFFu);
	sum = (sum >> 16) + (sum & 0xFFFFu);
	return sum & 0xFFFFu;
}

/*
 * Entry with descriptor @d (struct gcl_txh_desc as eight little-endian
 * dwords) whose frame starts at @o of a region of @frames_len bytes.
 */
GCL_TXH_FN struct gcl_txh_res gcl_txh_rule(const struct gcl_neigh_view *v, const struct gcl_txh_net *net,
                                           const uint32_t d[8], uint64_t o, uint64_t frames_len,
                                           uint32_t cap)
{
	struct gcl_txh_res r;
	const uint32_t lip = d[0], rip = d[1], lport = d[2] & 0xFFFFu, rport = d[2] >> 16;
	const uint32_t proto = d[3] & 0xFFu, flags = d[3] >> 8 & 0xFFu, off = d[3] >> 16 & 0xFFu;
	const uint32_t ecn = d[3] >> 24, seq = d[4], ack = d[5], win = d[6] & 0xFFFFu, paylen = d[6] >> 16;
	const int tcp = proto == 6;
	const uint32_t hl = tcp ? 4 * off : 8;
	const uint32_t tot = 20 + hl + paylen, len = 14 + tot;
	const uint32_t elen = len > net->min_pkt_size ? len : net->min_pkt_size;

	for (int i = 0; i < 14; i++)
		r.w[i] = 0;
	r.status = GCL_TXH_REFUSED;
	r.eth = 0;
	r.l4end = tcp ? 54 : 42;
	r.len = len;
	r.pkt_len = 0;
	r.olflags = 0;
	r.local = 0;
	r.nh = 0;
	r.lport = lport;
	r.rport = rport;
	if ((proto != 6 && proto != 17) || (tcp && (off < 5 || off > 15)) || len > 65535 ||
	    (cap && elen > cap) || o > frames_len || elen > frames_len - o)
		return r;

	/* core.c:693-698 */
	const uint32_t saddr = lip ? lip : rip == GCL_TXH_LOOPBACK ? GCL_TXH_LOOPBACK : net->addr;
	const uint32_t S = gcl_txh_be32(saddr), D = gcl_txh_be32(rip);
	const uint32_t tos = ecn & 0x80u ? ecn & 3u : 0;
	uint32_t ipsum = 0, l4sum = 0;

	if (net->flags & GCL_TXH_IP_CSUM) /* ipv4_cksum, core.c:616-617 */
		ipsum = ~gcl_txh_fold((0x4500u | tos) + tot + 0x4000u + (64u << 8 | proto) + (saddr >> 16) +
		                      (saddr & 0xFFFFu) + (rip >> 16) + (rip & 0xFFFFu)) & 0xFFFFu;
	if (tcp) /* ipv4_phdr_cksum, tcp_out.c:34 */
		l4sum = gcl_txh_fold((saddr >> 16) + (saddr & 0xFFFFu) + (rip >> 16) + (rip & 0xFFFFu) + 6u +
		                     ((hl + paylen) & 0xFFFFu));
	r.w[3] = 0x0008u | 0x45u << 16 | tos << 24;
	r.w[4] = gcl_txh_be16(tot);                         /* id 0 */
	r.w[5] = 0x0040u | 64u << 16 | proto << 24;         /* IP_DF, ttl */
	r.w[6] = gcl_txh_be16(ipsum) | S << 16;
	r.w[7] = S >> 16 | D << 16;
	r.w[8] = D >> 16 | gcl_txh_be16(lport) << 16;
	if (tcp) {
		const uint32_t Q = gcl_txh_be32(seq), A = gcl_txh_be32(ack);
		r.w[9] = gcl_txh_be16(rport) | Q << 16;
		r.w[10] = Q >> 16 | A << 16;
		r.w[11] = A >> 16 | (off << 4 & 0xFFu) << 16 | flags << 24;
		r.w[12] = gcl_txh_be16(win) | gcl_txh_be16(l4sum) << 16;
	} else {
		r.w[9] = gcl_txh_be16(rport) | gcl_txh_be16(paylen + 8) << 16;
	}
	r.pkt_len = len;

	/* net_tx_local_loopback, core.c:705-706 */
	if (rip == net->addr || rip == GCL_TXH_LOOPBACK) {
		r.status = GCL_TXH_SELF;
		return r;
	}
	r.olflags = GCL_TXH_OL_IP_CHKSUM | GCL_TXH_OL_IPV4 | (tcp ? GCL_TXH_OL_TCP_CHKSUM : 0);
	/* net_get_ip_route, core.c:620-626 */
	r.nh = (rip & net->netmask) == (net->addr & net->netmask) ? rip : net->gateway;
	uint32_t mac[2];
	if (gcl_neigh_probe(v, r.nh, mac) == GCL_NEIGH_NO_SLOT) {
		r.status = GCL_TXH_NONEIGH;
		return r;
	}
	const uint32_t own0 = net->mac[0] | (uint32_t)net->mac[1] << 8 | (uint32_t)net->mac[2] << 16 |
	                      (uint32_t)net->mac[3] << 24;
	const uint32_t own1 = net->mac[4] | (uint32_t)net->mac[5] << 8;
	r.status = GCL_TXH_OK;
	r.eth = 1;
	r.w[0] = mac[0];
	r.w[1] = mac[1] | own0 << 16;
	r.w[2] = own0 >> 16 | own1 << 16;
	r.local = mac[0] == own0 && mac[1] == own1; /* is_local, arp.c:62-65 */
	if (r.local)
		r.olflags |= GCL_TXH_OL_LOCAL | GCL_TXH_OL_LOCAL_HINT;
	r.pkt_len = elen; /* net_tx_iokernel's padding, core.c:513-517 */
	return r;
}

/* txpkt_xmit_cmd.lrpc_cmd (inc/iokernel/queue.h:82-93), txcmd = TXPKT_NET_XMIT */
GCL_TXH_FN uint64_t gcl_txh_cmd(const struct gcl_txh_res *r)
{
	if (r->status != GCL_TXH_OK)
		return 0;
	return (r->local ? r->nh : 0) | (uint64_t)r->pkt_len << 32 | (uint64_t)r->olflags << 48;
}

/* txpkt_to_payload (queue.h:120-124); @hash is the entry's hash output */
GCL_TXH_FN uint64_t gcl_txh_payload(const struct gcl_txh_res *r, uint64_t shm_base, uint64_t o,
                                    uint32_t hash)
{
	if (r->status != GCL_TXH_OK)
		return 0;
	return (shm_base + o) | (uint64_t)(hash & 0xFFFFu) << 48;
}

#endif /* GCL_TXH_H */
