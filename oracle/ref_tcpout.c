/*
 * ref_tcpout.c - test infrastructure (oracle/_ref only, never linked into the
 * product): the reference's own tcp_push_tcphdr
 * (/root/reference/runtime/net/tcp_out.c:54-87, with the __tcp_hdr_chksum it
 * calls, tcp_out.c:27-52) and the checksum routines of inc/net/chksum.h,
 * compiled where they lie.
 *
 * oracle/Makefile passes the reference file's path as REF_TCP_OUT_C and this
 * file #includes it unmodified, against the reference's own headers.
 * tcp_push_tcphdr is a static inline that reads a tcpconn_t, an mbuf and the
 * runtime's `netcfg` global (runtime/defs.h:534-549, defined in core.c, which
 * is not part of this library); this file builds the first two by hand from
 * its arguments and defines netcfg -- the function's input, as ref_core.c
 * defines `iok`.  The one other symbol defined here is logk_bug, the handler
 * a failed BUG_ON of inc/net/mbuf.h calls: the mbuf below always has the
 * headroom the push needs, so it is never reached, and it aborts.  The rest
 * of tcp_out.c is unreachable from the exports and dropped by --gc-sections;
 * the library links with --no-undefined.
 */
#include <stdlib.h>

#include REF_TCP_OUT_C

struct net_cfg netcfg;

void logk_bug(bool fatal, const char *expr, const char *file, int line, const char *func)
{
	abort();
}

#define REF_EXPORT __attribute__((visibility("default")))
#define REF_HEADROOM 64

static unsigned char ref_buf[REF_HEADROOM + 65536];
static tcpconn_t ref_conn;

/* tcp_push_tcphdr(m, c, flags, off, l4len) with netcfg.no_tx_offloads =
 * @no_tx_offloads: c->e.laddr/raddr = (@lip, @lport)/(@rip, @rport) in host
 * order, c->pcb.rcv_nxt_wnd = @win << 32 | @ack, c->pcb.rcv_wscale = @wscale,
 * m->seg_seq = @seq, and m's data the @l4len bytes at @payload.  @hdr gets the
 * 20 header bytes as pushed.  @off must be 5: the header struct has no room
 * for options and the full checksum covers @l4len + 4 * @off bytes from it. */
REF_EXPORT int ref_tcp_push_tcphdr(int no_tx_offloads, uint32_t lip, uint16_t lport, uint32_t rip,
                                   uint16_t rport, uint32_t seq, uint32_t ack, uint32_t win,
                                   uint32_t wscale, uint8_t flags, uint8_t off, uint16_t l4len,
                                   const uint8_t *payload, uint8_t hdr[20])
{
	struct mbuf m;
	struct tcp_hdr *h;

	if (off != 5 || l4len > 65535 - 20)
		return -1;
	memset(&m, 0, sizeof(m));
	memset(&ref_conn, 0, sizeof(ref_conn));
	memset(&netcfg, 0, sizeof(netcfg));
	netcfg.no_tx_offloads = no_tx_offloads != 0;
	if (l4len)
		memcpy(ref_buf + REF_HEADROOM, payload, l4len);
	m.head = ref_buf;
	m.head_len = 65535;
	m.data = ref_buf + REF_HEADROOM;
	m.len = l4len;
	m.seg_seq = seq;
	ref_conn.e.laddr.ip = lip;
	ref_conn.e.laddr.port = lport;
	ref_conn.e.raddr.ip = rip;
	ref_conn.e.raddr.port = rport;
	ref_conn.pcb.rcv_nxt_wnd = (uint64_t)win << 32 | ack;
	ref_conn.pcb.rcv_wscale = wscale;
	h = tcp_push_tcphdr(&m, &ref_conn, flags, off, l4len);
	if ((unsigned char *)h != ref_buf + REF_HEADROOM - 20 || m.len != l4len + 20u)
		return -2;
	memcpy(hdr, h, 20);
	return 0;
}

/* inc/net/chksum.h, each over the caller's buffer; the result is the uint16_t
 * the routine returns, to be stored as the reference stores it (hdr->sum = v) */
REF_EXPORT uint16_t ref_raw_cksum(const uint8_t *buf, size_t len)
{
	return raw_cksum(buf, len);
}

REF_EXPORT uint16_t ref_ipv4_phdr_cksum(uint8_t proto, uint32_t saddr, uint32_t daddr, uint16_t l4len)
{
	return ipv4_phdr_cksum(proto, saddr, daddr, l4len);
}

REF_EXPORT uint16_t ref_ipv4_udptcp_cksum(uint8_t proto, uint32_t saddr, uint32_t daddr,
                                          uint16_t l4len, const uint8_t *l4hdr)
{
	return ipv4_udptcp_cksum(proto, saddr, daddr, l4len, l4hdr);
}

/* ipv4_cksum over the 20 bytes at @hdr (wire order, the field as it stands) */
REF_EXPORT uint16_t ref_ipv4_cksum(const uint8_t *hdr)
{
	struct ip_hdr ip;

	memcpy(&ip, hdr, sizeof(ip));
	return ipv4_cksum(&ip);
}
