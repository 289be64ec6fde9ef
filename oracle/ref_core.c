/*
 * ref_core.c - test infrastructure (oracle/_ref only, never linked into the
 * product): the reference's own do_toeplitz
 * (/root/reference/runtime/net/core.c:120-139) and ip_hdr_supported
 * (core.c:203-209, which frames reach the transport demux), compiled where
 * they lie.
 *
 * oracle/Makefile passes the reference file's path as REF_CORE_C and this
 * file #includes it unmodified, against the reference's own headers
 * (inc/, runtime/, runtime/net/).  do_toeplitz is static and reads the RSS
 * key from the runtime's `iok` global (runtime/defs.h:193-199), which the
 * runtime fills from the iokernel's shared memory at start-up; this file
 * defines that global -- the function's input, as tests/ set it -- and
 * exports entry points for the two static functions.  Nothing the reference references is stubbed:
 * the rest of core.c is unreachable from the export and dropped by
 * --gc-sections, and the library links with --no-undefined.
 *
 * The transmit side: net_push_iphdr and net_get_ip_route (core.c:592-626),
 * both static, read `netcfg`, which core.c itself defines (core.c:23) and the
 * entry points below set per call.  net_push_iphdr pushes onto an mbuf, built
 * here by hand; the failed-BUG_ON handler of inc/net/mbuf.h, logk_bug, is the
 * one symbol this file defines besides `iok`.  It is never reached (the mbuf
 * has the headroom) and aborts.
 */
#include <stdlib.h>

#include REF_CORE_C

struct iokernel_control iok;
static struct iokernel_info ref_info;

/* do_toeplitz(saddr, daddr, sport, dport) (host-order fields) with RSS key
 * @key (@key_len <= 52 bytes, iokernel_info.rss_key) */
__attribute__((visibility("default"))) uint32_t ref_do_toeplitz(const uint8_t *key,
                                                                uint32_t key_len,
                                                                uint32_t saddr, uint32_t daddr,
                                                                uint16_t sport, uint16_t dport)
{
	memset(ref_info.rss_key, 0, sizeof(ref_info.rss_key));
	memcpy(ref_info.rss_key, key,
	       key_len < sizeof(ref_info.rss_key) ? key_len : sizeof(ref_info.rss_key));
	ref_info.rss_key_len = key_len;
	iok.iok_info = &ref_info;
	return do_toeplitz(saddr, daddr, sport, dport);
}

/* ip_hdr_supported on the 20-byte IPv4 header at @hdr (wire order) */
__attribute__((visibility("default"))) int ref_ip_hdr_supported(const uint8_t *hdr)
{
	struct ip_hdr ip;

	memcpy(&ip, hdr, sizeof(ip));
	return ip_hdr_supported(&ip);
}

void logk_bug(bool fatal, const char *expr, const char *file, int line, const char *func)
{
	abort();
}

/* net_push_iphdr(m, proto, daddr, saddr, aux) with netcfg.no_tx_offloads =
 * @no_tx_offloads onto an mbuf that holds @l4bytes bytes (their content is
 * not read).  @aux_mode 0: aux == NULL; 1: aux->has_ecn = @has_ecn,
 * aux->ecn = @ecn.  @hdr gets the 20 header bytes. */
__attribute__((visibility("default"))) int ref_net_push_iphdr(int no_tx_offloads, uint8_t proto,
                                                              uint32_t daddr, uint32_t saddr,
                                                              uint16_t l4bytes, int aux_mode,
                                                              int has_ecn, uint8_t ecn,
                                                              uint8_t hdr[20])
{
	static unsigned char buf[64];
	struct aux_tx_pkt_data aux;
	struct mbuf m;

	if (l4bytes > 65535 - 20)
		return -1;
	memset(&m, 0, sizeof(m));
	memset(&aux, 0, sizeof(aux));
	memset(&netcfg, 0, sizeof(netcfg));
	netcfg.no_tx_offloads = no_tx_offloads != 0;
	aux.has_ecn = has_ecn != 0;
	aux.ecn = ecn;
	m.head = buf;
	m.head_len = 65535;
	m.data = buf + sizeof(buf);   /* the L4 bytes would lie behind; only their count is used */
	m.len = l4bytes;
	net_push_iphdr(&m, proto, daddr, saddr, aux_mode ? &aux : NULL);
	if (m.data != buf + sizeof(buf) - 20 || m.len != l4bytes + 20u)
		return -2;
	memcpy(hdr, m.data, 20);
	return 0;
}

/* net_get_ip_route(daddr) with netcfg.addr/netmask/gateway as given (host order) */
__attribute__((visibility("default"))) uint32_t ref_net_get_ip_route(uint32_t addr, uint32_t netmask,
                                                                     uint32_t gateway, uint32_t daddr)
{
	memset(&netcfg, 0, sizeof(netcfg));
	netcfg.addr = addr;
	netcfg.netmask = netmask;
	netcfg.gateway = gateway;
	return net_get_ip_route(daddr);
}
