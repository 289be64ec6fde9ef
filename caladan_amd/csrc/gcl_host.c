/*
 * gcl_host.c - host-side C of the rx classify path: table helpers, the CPU
 * forms of the two hashes, and the verdict post-pass that feeds lrpc rings.
 */
#include <errno.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/gcl_host.h"
#include "../../include/gclassify.h"
#include "gcl_pay.h"
#include "gcl_seg.h"
#include "gcl_tcprx.h"
#include "gcl_tcprxf.h"
#include "gcl_tcprxo.h"
#include "gcl_tcprxs.h"
#include "gcl_tcpopen.h"
#include "gcl_tcpread.h"
#include "gcl_tcpwrite.h"
#include "gcl_tcpshut.h"
#include "gcl_tcptmr.h"
#include "gcl_txq.h"
#include "gcl_txh.h"
#include "gcl_udprx.h"

#define ROT(x, k) (((x) << (k)) | ((x) >> (32 - (k))))

/*
 * gcl_jenkins_hash - lookup3 hashlittle, initval 0 (base/jenkins_hash.c:
 * 126-297), the function rte_jhash(key, len, 0) applies to the ip_to_proc
 * keys.  Reads 12-byte blocks as little-endian words (memcpy, any alignment).
 */
uint32_t gcl_jenkins_hash(const void *key, size_t length)
{
	const uint8_t *k = key;
	uint32_t a, b, c, w[3];

	a = b = c = 0xdeadbeefu + (uint32_t)length;
	while (length > 12) {
		memcpy(w, k, 12);
		a += w[0];
		b += w[1];
		c += w[2];
		a -= c; a ^= ROT(c, 4);  c += b;
		b -= a; b ^= ROT(a, 6);  a += c;
		c -= b; c ^= ROT(b, 8);  b += a;
		a -= c; a ^= ROT(c, 16); c += b;
		b -= a; b ^= ROT(a, 19); a += c;
		c -= b; c ^= ROT(b, 4);  b += a;
		length -= 12;
		k += 12;
	}
	if (length == 0)
		return c;
	w[0] = w[1] = w[2] = 0;
	memcpy(w, k, length); /* the masked tail of the aligned path, :166-181 */
	a += w[0];
	b += w[1];
	c += w[2];
	c ^= b; c -= ROT(b, 14);
	a ^= c; a -= ROT(c, 11);
	b ^= a; b -= ROT(a, 25);
	c ^= b; c -= ROT(b, 16);
	a ^= c; a -= ROT(c, 4);
	b ^= a; b -= ROT(a, 14);
	c ^= b; c -= ROT(b, 24);
	return c;
}

/*
 * gcl_toeplitz - Toeplitz hash of @input under @key, bit i of the input
 * (MSB first) selecting the 32-bit key window starting at bit i.  For the
 * 12-byte IPv4 tuple this equals do_toeplitz (runtime/net/core.c:120-139).
 */
uint32_t gcl_toeplitz(const uint8_t *key, size_t keylen, const uint8_t *input, size_t len)
{
	uint32_t ret = 0;
	uint64_t window = 0;
	size_t kb = 0;

	/* 64-bit sliding window over the key bits */
	for (; kb < 8; kb++)
		window = window << 8 | (kb < keylen ? key[kb] : 0);
	for (size_t i = 0; i < len; i++) {
		for (int bit = 7; bit >= 0; bit--) {
			int shift = 7 - bit; /* bits consumed from this byte so far */
			if (input[i] & (1u << bit))
				ret ^= (uint32_t)(window >> (32 - shift));
		}
		window = window << 8 | (kb < keylen ? key[kb] : 0);
		kb++;
	}
	return ret;
}

/* sched_steer_flows rule (iokernel/sched.c:122-147) */
int gcl_steer_flows(uint16_t thread_count, const uint16_t *active_idx,
                    uint16_t active_count, uint16_t *flow_tbl)
{
	unsigned int rr = 0;

	if (thread_count == 0 || thread_count > GCL_NCPU || active_count > thread_count ||
	    !flow_tbl || (active_count && !active_idx))
		return -EINVAL;
	if (active_count == 0)
		return 0; /* "don't do anything if zero threads are active" */
	for (unsigned int i = 0; i < active_count; i++)
		if (active_idx[i] >= thread_count)
			return -EINVAL;
	for (unsigned int i = 0; i < thread_count; i++)
		flow_tbl[i] = UINT16_MAX;
	for (unsigned int i = 0; i < active_count; i++)
		flow_tbl[active_idx[i]] = active_idx[i];
	for (unsigned int i = 0; i < thread_count; i++)
		if (flow_tbl[i] == UINT16_MAX)
			flow_tbl[i] = active_idx[rr++ % active_count];
	return 0;
}

/* tx_prepare_tx_mbuf (tx.c:81) + copy_batch (dma.c:182-185) */
uint8_t gcl_loopback_olflags(uint8_t tx_olflags)
{
	const uint8_t TXFLAG_LOCAL_HINT = 1u << 6; /* inc/iokernel/queue.h:42 */
	return (uint8_t)(((tx_olflags & TXFLAG_LOCAL_HINT) ? GCL_F_RSS_HASH : 0) |
	                 GCL_F_IP_CKSUM_GOOD);
}

/* rss_from_txpkt_payload, inc/iokernel/queue.h:131-134 */
uint32_t gcl_txpkt_rss(uint64_t payload)
{
	return (uint32_t)(payload >> 48);
}

/* CRC32C (Castagnoli, reflected 0x82F63B78) over the 8 little-endian bytes of
 * @val starting from @crc with no inversion: the crc32q instruction that
 * hash_crc32c_one/two use (inc/base/hash.h:23-40, inc/asm/ops.h:77-80). */
uint32_t gcl_crc32c_u64(uint32_t crc, uint64_t val)
{
	for (int i = 0; i < 8; i++) {
		crc ^= (uint8_t)(val >> (8 * i));
		for (int b = 0; b < 8; b++)
			crc = (crc >> 1) ^ (0x82F63B78u & (0u - (crc & 1)));
	}
	return crc;
}

/* trans_hash_5tuple / trans_hash_3tuple, runtime/net/transport.c:29-42 */
void gcl_trans_hash(uint32_t seed, uint8_t proto, uint32_t lip, uint16_t lport, uint32_t rip,
                    uint16_t rport, struct gcl_trans *out)
{
	uint64_t l = (uint64_t)lip | (uint64_t)lport << 32;
	uint64_t r = (uint64_t)rip | (uint64_t)rport << 32 | (uint64_t)proto << 48;
	out->h5 = gcl_crc32c_u64(gcl_crc32c_u64(seed, l), r);
	out->h3 = gcl_crc32c_u64(seed, l | (uint64_t)proto << 48);
}

uint32_t gcl_runtime_ip(uint32_t r)
{
	return 0x0A000000u + r + 1;
}

int gcl_zipf_cdf(uint32_t nflows, double s, uint64_t *cdf_out)
{
	double h = 0.0, acc = 0.0;

	if (!nflows || !cdf_out)
		return -EINVAL;
	for (uint32_t k = 0; k < nflows; k++)
		h += pow((double)k + 1.0, -s);
	for (uint32_t k = 0; k < nflows; k++) {
		double x;
		acc += pow((double)k + 1.0, -s);
		x = ldexp(acc / h, 64);
		cdf_out[k] = x >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)x;
	}
	cdf_out[nflows - 1] = UINT64_MAX;
	return 0;
}

/* ---------------------------------------------------------------------- */

int gcl_lrpc_init_out(struct gcl_lrpc_chan_out *chan, struct gcl_lrpc_msg *tbl,
                      unsigned int size, uint32_t *recv_head_wb)
{
	if (!size || (size & (size - 1)))
		return -EINVAL;
	memset(chan, 0, sizeof(*chan));
	chan->tbl = tbl;
	chan->size = size;
	chan->recv_head_wb = recv_head_wb;
	return 0;
}

bool gcl_lrpc_send(struct gcl_lrpc_chan_out *chan, uint64_t cmd, unsigned long payload)
{
	struct gcl_lrpc_msg *dst;

	if (chan->send_head - chan->send_tail >= chan->size) {
		/* __lrpc_send: refresh the consumer position (base/lrpc.c:16-19) */
		chan->send_tail = __atomic_load_n(chan->recv_head_wb, __ATOMIC_ACQUIRE);
		if (chan->send_head - chan->send_tail == chan->size)
			return false;
	}
	dst = &chan->tbl[chan->send_head & (chan->size - 1)];
	cmd |= (chan->send_head++ & chan->size) ? 0 : GCL_LRPC_DONE_PARITY;
	dst->payload = payload;
	__atomic_store_n(&dst->cmd, cmd, __ATOMIC_RELEASE);
	return true;
}

uint64_t gcl_rx_make_cmd(uint16_t pkt_len, uint8_t olflags)
{
	uint64_t csum = (olflags & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD ? 1 : 0;
	return 0 /* RX_NET_RECV */ | (uint64_t)pkt_len << 16 | csum << 48;
}

/* The rule of gcl_rx_csum (gclassify.h) for one frame: a frame that is not
 * IPv4 or is already IP_CKSUM_GOOD keeps its flags; any other gets the
 * verdict of chksum_internet over frame bytes [14, 34) (net_rx_one,
 * runtime/net/core.c:275-279), bytes at or past @len reading 0. */
uint8_t gcl_rx_csum_flags(const uint8_t *frame, size_t len, uint8_t olflags)
{
	uint8_t h[34] = {0};
	uint32_t sum = 0;

	if (len)
		memcpy(h, frame, len < sizeof(h) ? len : sizeof(h));
	if (h[12] != (GCL_ETHTYPE_IP >> 8) || h[13] != (GCL_ETHTYPE_IP & 0xFF) ||
	    (olflags & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD)
		return olflags;
	for (int i = 14; i < 34; i += 2)
		sum += h[i] | (uint32_t)h[i + 1] << 8;
	sum = (sum & 0xFFFF) + (sum >> 16);
	sum = (sum & 0xFFFF) + (sum >> 16);
	return (olflags & ~GCL_F_IP_CKSUM_MASK) |
	       (sum == 0xFFFF ? GCL_F_IP_CKSUM_GOOD : GCL_F_IP_CKSUM_BAD);
}

/* The rule of gcl_copy_batch (gclassify.h) on the CPU: copy_batch's loop
 * (iokernel/dma.c:179-188) with rte_pktmbuf_append's failure made a refusal
 * and the source bounded by src_len (bytes at or past it read 0). */
int gcl_copy_batch_host(const struct gcl_copy_in *in, const struct gcl_copy_out *out,
                        uint64_t *counts)
{
	uint64_t copied = 0, refused = 0, bytes = 0;

	if (!in || !out || in->size != sizeof(*in))
		return -EINVAL;
	if (in->n == 0)
		return 0;
	if (!in->src || !in->src_off || !in->len || !out->dst || !out->pkt_len ||
	    in->src_len == UINT64_MAX || out->dst_len == UINT64_MAX || in->n > (1ull << 40) ||
	    (!out->dst_off && (out->dst_stride < 16 || (out->dst_stride & 15) ||
	                       out->dst_stride > (1u << 20))))
		return -EINVAL;
	for (uint64_t i = 0; i < in->n; i++) {
		const uint64_t len = in->len[i], so = in->src_off[i];
		const uint64_t d = out->dst_off ? out->dst_off[i] : i * out->dst_stride;

		if (out->olflags)
			out->olflags[i] = gcl_loopback_olflags(in->tx_olflags ? in->tx_olflags[i] : 0);
		if (out->rss)
			out->rss[i] = in->hash ? in->hash[i] : 0;
		/* rte_pktmbuf_append(dst[i], bytes) */
		if ((in->dst_cap && len > in->dst_cap) || (!out->dst_off && len > out->dst_stride) ||
		    d > out->dst_len || len > out->dst_len - d) {
			out->pkt_len[i] = 0;
			refused++;
			continue;
		}
		const uint64_t avail = so < in->src_len ? in->src_len - so : 0;
		const uint64_t have = len < avail ? len : avail;
		if (have)
			memcpy(out->dst + d, in->src + so, have);
		if (len > have)
			memset(out->dst + d + have, 0, len - have);
		out->pkt_len[i] = (uint16_t)len;
		copied++;
		bytes += len;
	}
	if (counts) {
		counts[GCL_COPY_COPIED] += copied;
		counts[GCL_COPY_REFUSED] += refused;
		counts[GCL_COPY_BYTES] += bytes;
	}
	return 0;
}

/* __raw_cksum (inc/net/chksum.h) folded: @len bytes as 16-bit words in memory
 * order, an odd last byte the low byte of a last word, plus @sum */
static uint32_t l4_fold(const uint8_t *p, size_t len, uint64_t sum)
{
	size_t i;

	for (i = 0; i + 1 < len; i += 2)
		sum += p[i] | (uint32_t)p[i + 1] << 8;
	if (i < len)
		sum += p[i];
	while (sum >> 16)
		sum = (sum & 0xFFFF) + (sum >> 16);
	return (uint32_t)sum;
}

/* The rule of gcl_l4_csum (gclassify.h) on the CPU: ipv4_cksum and
 * ipv4_udptcp_cksum (inc/net/chksum.h) as the runtime fills them, and the
 * check of the same sum on receive. */
int gcl_l4_csum_host(const struct gcl_batch *b, const struct gcl_l4_in *in, uint8_t *status,
                     uint64_t *counts)
{
	uint64_t c[GCL_L4C_NR] = {0};

	if (!b || !in || !status || in->size != sizeof(*in) || in->mode > GCL_L4_FILL ||
	    (in->group != 0 && in->group != 4 && in->group != 16 && in->group != 64))
		return -EINVAL;
	if (b->n == 0)
		return 0;
	if (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	    (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	    !b->pkt_len || ((uintptr_t)b->pkt_len & 1))
		return -EINVAL;
	for (uint64_t i = 0; i < b->n; i++) {
		const uint64_t raw = b->offs ? b->offs[i] : i * b->stride;
		const uint64_t o = raw < b->frames_len ? raw : b->frames_len;
		const uint64_t avail = b->frames_len - o;
		const uint64_t L = b->pkt_len[i] < avail ? b->pkt_len[i] : avail;
		uint8_t *f = (uint8_t *)b->frames + o; /* FILL writes: the caller owns the memory */
		const uint8_t fl = in->mode != GCL_L4_FILL ? 0 : in->tx_olflags ? in->tx_olflags[i] : 3;
		uint8_t st = GCL_L4_NA;
		uint32_t tot = 0, l4len = 0;
		bool ip_ok, l4_ok = false;

		ip_ok = L >= 34 && f[12] == (GCL_ETHTYPE_IP >> 8) && f[13] == (GCL_ETHTYPE_IP & 0xFF) &&
		        f[14] == 0x45;
		if (ip_ok) {
			const uint32_t frag = (uint32_t)f[20] << 8 | f[21]; /* host order: MF 0x2000, offset 0x1FFF */
			const uint8_t proto = f[23];

			tot = (uint32_t)f[16] << 8 | f[17];
			l4_ok = !(frag & 0x3FFF) && (proto == 6 || proto == 17) &&
			        tot >= 20u + (proto == 6 ? 20u : 8u) && 14ull + tot <= L;
			l4len = tot - 20;
		}
		if (ip_ok && (fl & 1)) {
			f[24] = f[25] = 0;
			const uint32_t v = ~l4_fold(f + 14, 20, 0) & 0xFFFF;
			f[24] = (uint8_t)v;
			f[25] = (uint8_t)(v >> 8);
			st |= GCL_L4_FILLED_IP;
			c[GCL_L4C_FILLED_IP]++;
		}
		if (l4_ok) {
			const uint8_t proto = f[23];
			uint8_t *fld = f + (proto == 6 ? 50 : 40);
			/* the pseudo-header's words in memory order: the addresses
			 * as they lie in the frame, {0, proto}, hton16(l4len) */
			const uint64_t ph = l4_fold(f + 26, 8, 0) + ((uint32_t)proto << 8) +
			                    ((l4len >> 8) | (l4len & 0xFF) << 8);

			if (in->mode == GCL_L4_FILL) {
				if (fl & 2) {
					fld[0] = fld[1] = 0;
					uint32_t v = ~l4_fold(f + 34, l4len, ph) & 0xFFFF;
					if (v == 0)
						v = 0xFFFF;
					fld[0] = (uint8_t)v;
					fld[1] = (uint8_t)(v >> 8);
					st |= GCL_L4_FILLED_L4;
					c[GCL_L4C_FILLED_L4]++;
					c[GCL_L4C_BYTES] += l4len;
				}
			} else if (proto == 17 && !fld[0] && !fld[1]) {
				st = GCL_L4_NONE;
			} else {
				st = l4_fold(f + 34, l4len, ph) == 0xFFFF ? GCL_L4_GOOD : GCL_L4_BAD;
				c[GCL_L4C_BYTES] += l4len;
			}
		}
		status[i] = st;
		c[(st & 0xF) == GCL_L4_GOOD ? GCL_L4C_GOOD : (st & 0xF) == GCL_L4_BAD ? GCL_L4C_BAD :
		  (st & 0xF) == GCL_L4_NONE ? GCL_L4C_NONE : GCL_L4C_NA]++;
	}
	if (counts)
		for (int k = 0; k < GCL_L4C_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* The rule of gcl_l4_payload (gclassify.h) on the CPU: gcl_pay_rule of
 * gcl_pay.h for every list entry in turn, the layout a running sum. */
int gcl_l4_payload_host(const struct gcl_batch *b, const struct gcl_pay_in *in,
                        const struct gcl_pay_out *out, uint64_t *counts)
{
	uint64_t c[GCL_PAYC_NR] = {0}, at = 0;

	if (!b || !in || !out || in->size != sizeof(*in) || !gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || in->m > (1ull << 31) || in->blocks > GCL_PAY_MAX_BLOCKS)
		return -EINVAL;
	if (!out->src_off || !out->len || !out->dst_off || !out->kind || !out->total ||
	    !in->seg_off != !out->seg_bytes)
		return -EINVAL;
	if (((uintptr_t)out->src_off & 7) || ((uintptr_t)out->len & 1) || ((uintptr_t)out->dst_off & 7) ||
	    ((uintptr_t)out->meta & 15) || ((uintptr_t)out->seg_bytes & 7) || ((uintptr_t)out->total & 7) ||
	    ((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->seg_off & 3) ||
	    ((uintptr_t)counts & 7))
		return -EINVAL;
	if (in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	              (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	              !b->pkt_len || ((uintptr_t)b->pkt_len & 1)))
		return -EINVAL;
	const uint32_t amask = in->align ? in->align - 1 : 0;

	for (uint64_t j = 0; j < in->m; j++) {
		const uint64_t i = in->order ? in->order[j] : j;
		struct gcl_pay_desc r = {0, 0, GCL_PAY_OOR, {0, 0, 0, 0}};

		if (i < b->n) {
			const uint64_t raw = b->offs ? b->offs[i] : i * b->stride;
			const uint64_t o = raw < b->frames_len ? raw : b->frames_len;
			const uint64_t avail = b->frames_len - o;
			const uint64_t L = b->pkt_len[i] < avail ? b->pkt_len[i] : avail;
			uint8_t h[48] = {0};
			uint32_t d[9];

			if (avail)
				memcpy(h, b->frames + o, avail < sizeof(h) ? avail : sizeof(h));
			for (int x = 0; x < 9; x++)
				d[x] = h[12 + 4 * x] | (uint32_t)h[13 + 4 * x] << 8 | (uint32_t)h[14 + 4 * x] << 16 |
				       (uint32_t)h[15 + 4 * x] << 24;
			r = gcl_pay_rule(d, o, L, in->l4_status != NULL, in->l4_status ? in->l4_status[i] : 0,
			                 in->sock != NULL, in->sock ? in->sock[i] : 0);
		}
		out->src_off[j] = r.src_off;
		out->len[j] = (uint16_t)r.len;
		out->kind[j] = (uint8_t)r.kind;
		if (out->meta)
			memcpy(&out->meta[j], r.meta, sizeof(out->meta[j]));
		out->dst_off[j] = at;
		at += gcl_pay_pad(r.len, amask);
		c[gcl_pay_counter(r.kind)]++;
		c[GCL_PAYC_BYTES] += r.len;
	}
	*out->total = at;
	if (in->seg_off)
		for (uint64_t s = 0; s <= in->nseg; s++)
			out->seg_bytes[s] = in->seg_off[s] < in->m ? out->dst_off[in->seg_off[s]] : at;
	if (counts)
		for (int k = 0; k < GCL_PAYC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* The rule of gcl_tx_hdr (gclassify.h) on the CPU: gcl_txh_rule of gcl_txh.h
 * for every entry in turn, the header bytes it names stored with memcpy. */
int gcl_tx_hdr_host(const struct gcl_neigh_tbl *tbl, const uint8_t rss_key[40],
                    const struct gcl_txh_in *in, const struct gcl_txh_out *out, uint64_t *counts)
{
	static const struct gcl_neigh_slot none[1 + (2u << 3)]; /* an empty image: header | 8 buckets */
	uint64_t c[GCL_TXHC_NR] = {0};

	if (!rss_key || !in || !out || in->size != sizeof(*in) || in->m > (1ull << 31))
		return -EINVAL;
	if (in->m == 0)
		return 0;
	if (!in->desc || !in->frame_off || !in->frames || in->frames_len == UINT64_MAX || !out->cmd ||
	    !out->payload || !out->pkt_len || !out->tx_olflags || !out->status)
		return -EINVAL;
	const struct gcl_neigh_view v = tbl ? gcl_neigh_tbl_view(tbl) : gcl_neigh_view_of(3, 0, 32, none);

	for (uint64_t j = 0; j < in->m; j++) {
		uint32_t d[8], hash = 0;
		uint64_t o;
		uint8_t h[56];

		memcpy(d, (const uint8_t *)in->desc + 32 * j, 32); /* little-endian host */
		memcpy(&o, (const uint8_t *)in->frame_off + 8 * j, 8);
		const struct gcl_txh_res r = gcl_txh_rule(&v, &in->net, d, o, in->frames_len, in->cap);
		if (r.status != GCL_TXH_REFUSED) {
			uint8_t *f = in->frames + o;
			memcpy(h, r.w, sizeof(h));
			memcpy(f + 14, h + 14, r.l4end - 14);
			if (r.eth) {
				memcpy(f, h, 14);
				if (r.pkt_len > r.len)
					memset(f + r.len, 0, r.pkt_len - r.len);
			}
		}
		if (r.local) { /* do_toeplitz(netcfg.addr, daddr, sport, dport), core.c:730 */
			const uint32_t a = in->net.addr;
			const uint8_t t[12] = { a >> 24, a >> 16, a >> 8, a, r.nh >> 24, r.nh >> 16, r.nh >> 8, r.nh,
			                        r.lport >> 8, r.lport, r.rport >> 8, r.rport };
			hash = gcl_toeplitz(rss_key, 40, t, 12);
		}
		const uint64_t cmd = gcl_txh_cmd(&r), pay = gcl_txh_payload(&r, in->shm_base, o, hash);
		const uint16_t pl = (uint16_t)r.pkt_len;
		memcpy((uint8_t *)out->cmd + 8 * j, &cmd, 8);
		memcpy((uint8_t *)out->payload + 8 * j, &pay, 8);
		memcpy((uint8_t *)out->pkt_len + 2 * j, &pl, 2);
		out->tx_olflags[j] = (uint8_t)r.olflags;
		if (out->hash)
			memcpy((uint8_t *)out->hash + 4 * j, &hash, 4);
		out->status[j] = (uint8_t)r.status;
		c[r.status]++;
		c[GCL_TXHC_LOCAL] += r.local;
		c[GCL_TXHC_BYTES] += r.status == GCL_TXH_OK ? r.pkt_len : 0;
	}
	if (counts)
		for (int k = 0; k < GCL_TXHC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* The rule of gcl_tx_seg (gclassify.h) on the CPU: gcl_seg_rule of gcl_seg.h
 * for every write in turn, the two sums running, gcl_seg_emit for every
 * segment of a write that fits. */
int gcl_tx_seg_host(const struct gcl_seg_in *in, const struct gcl_seg_out *out, uint64_t *counts)
{
	uint64_t c[GCL_SEGC_NR] = {0}, S = 0, B = 0, segs = 0, bytes = 0;

	if (!in || !out || in->size != sizeof(*in) || in->m > (1ull << 31) || in->seg_cap > (1ull << 31) ||
	    in->stride > GCL_SEG_MAX_STRIDE || in->lead > GCL_SEG_MAX_LEAD || in->udp_max > GCL_SEG_MAX_UDP ||
	    in->blocks > GCL_SEG_MAX_BLOCKS || !out->total_segs || !out->total_bytes)
		return -EINVAL;
	if (in->m && (!in->send || !out->status || !out->sent || !out->snd_nxt_out || !out->seg_first ||
	              !out->nseg))
		return -EINVAL;
	if (in->m && in->seg_cap && (!out->desc || !out->frame_off || !out->src_off || !out->len ||
	                             !out->dst_off))
		return -EINVAL;
	if (((uintptr_t)in->send & 15) || ((uintptr_t)out->sent & 3) || ((uintptr_t)out->snd_nxt_out & 3) ||
	    ((uintptr_t)out->seg_first & 3) || ((uintptr_t)out->nseg & 3) || ((uintptr_t)out->desc & 15) ||
	    ((uintptr_t)out->frame_off & 7) || ((uintptr_t)out->src_off & 7) || ((uintptr_t)out->len & 1) ||
	    ((uintptr_t)out->dst_off & 7) || ((uintptr_t)out->send_idx & 3) || ((uintptr_t)out->total_segs & 7) ||
	    ((uintptr_t)out->total_bytes & 7) || ((uintptr_t)counts & 7))
		return -EINVAL;
	const uint64_t bcap = gcl_seg_byte_cap(in->frames_len, in->frame_base, in->stride, in->lead);

	for (uint64_t i = 0; i < in->m; i++) {
		uint32_t s[12];

		memcpy(s, &in->send[i], sizeof(s)); /* little-endian host */
		const struct gcl_seg_plan p = gcl_seg_rule(s, in->udp_max, in->stride, in->lead);
		uint32_t status = p.status;
		if (status == GCL_SEG_OK && (S + p.nseg > in->seg_cap || gcl_seg_sat(B, p.wbytes) > bcap))
			status = GCL_SEG_NOSPACE;
		const int ok = status == GCL_SEG_OK;

		out->status[i] = (uint8_t)status;
		out->sent[i] = ok ? p.L : 0;
		out->snd_nxt_out[i] = s[4] + (ok ? p.L : 0);
		out->seg_first[i] = (uint32_t)(S < in->seg_cap ? S : in->seg_cap);
		out->nseg[i] = ok ? p.nseg : 0;
		if (ok) {
			const uint64_t first_byte = in->frame_base + in->lead + B;
			for (uint32_t k = 0; k < p.nseg; k++) {
				const struct gcl_seg_one r = gcl_seg_emit(s, k, first_byte, in->stride);
				const uint64_t g = S + k;
				memcpy(&out->desc[g], r.d, sizeof(out->desc[g]));
				out->frame_off[g] = r.frame_off;
				out->src_off[g] = r.src_off;
				out->len[g] = (uint16_t)r.paylen;
				out->dst_off[g] = r.dst_off;
				if (out->send_idx)
					out->send_idx[g] = (uint32_t)i;
			}
			segs += p.nseg;
			bytes += p.wbytes;
			c[GCL_SEGC_BYTES] += p.L;
			c[GCL_SEGC_PUSH] += p.tcp;
		}
		c[status]++;
		S += p.nseg;
		B = gcl_seg_sat(B, p.wbytes);
	}
	c[GCL_SEGC_SEGS] = segs;
	*out->total_segs = segs;
	*out->total_bytes = bytes;
	if (counts)
		for (int k = 0; k < GCL_SEGC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* One list entry of gcl_tcp_rx: the frame's bytes [12, 52) as dwords and
 * gcl_pay_rule's word on them.  Returns the cookie of a TCP segment, or
 * GCL_TCPRX_NONE. */
static uint32_t tcprx_entry(const struct gcl_batch *b, const struct gcl_tcprx_in *in, uint64_t j,
                            struct gcl_tcprx_seg *s)
{
	const uint64_t i = in->order ? in->order[j] : j;

	if (i >= b->n)
		return GCL_TCPRX_NONE;
	const uint64_t raw = b->offs ? b->offs[i] : i * b->stride;
	const uint64_t o = raw < b->frames_len ? raw : b->frames_len;
	const uint64_t avail = b->frames_len - o;
	const uint64_t L = b->pkt_len[i] < avail ? b->pkt_len[i] : avail;
	uint8_t h[52] = {0};
	uint32_t d[10];

	if (avail)
		memcpy(h, b->frames + o, avail < sizeof(h) ? avail : sizeof(h));
	for (int x = 0; x < 10; x++)
		d[x] = h[12 + 4 * x] | (uint32_t)h[13 + 4 * x] << 8 | (uint32_t)h[14 + 4 * x] << 16 |
		       (uint32_t)h[15 + 4 * x] << 24;
	const struct gcl_pay_desc r = gcl_pay_rule(d, o, L, in->l4_status != NULL,
	                                           in->l4_status ? in->l4_status[i] : 0, 1, in->sock[i]);
	if (r.kind != GCL_PAY_TCP)
		return GCL_TCPRX_NONE;
	*s = gcl_tcprx_parse(d, r.len);
	return in->sock[i];
}

/* The rule of gcl_tcp_rx (gclassify.h) on the CPU: one walk over the list with
 * every connection's live words kept in out_conn, gcl_tcprx_one of gcl_tcprx.h
 * for every segment; then the layout, and a second walk for dst_off. */
int gcl_tcp_rx_host(const struct gcl_batch *b, const struct gcl_tcprx_in *in,
                    const struct gcl_tcprx_out *out, uint64_t *counts)
{
	uint64_t c[GCL_TCPRXC_NR] = {0}, at = 0;

	if (!b || !in || !out || in->size != sizeof(*in) || !gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || in->m > (1ull << 31) || in->nconn > GCL_TCPRX_MAX_CONN ||
	    in->blocks > GCL_TCPRX_MAX_BLOCKS || !in->sock || !out->conn_off)
		return -EINVAL;
	if (in->nconn && (!in->conn || !out->out_conn))
		return -EINVAL;
	if (in->m && (!out->verdict || !out->sflags || !out->rcv_nxt_after || !out->copy_len || !out->dst_off))
		return -EINVAL;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->conn & 15) ||
	    ((uintptr_t)out->rcv_nxt_after & 3) || ((uintptr_t)out->copy_len & 1) || ((uintptr_t)out->dst_off & 7) ||
	    ((uintptr_t)out->out_conn & 15) || ((uintptr_t)out->conn_off & 7) || ((uintptr_t)counts & 7))
		return -EINVAL;
	if (in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	              (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	              !b->pkt_len || ((uintptr_t)b->pkt_len & 1)))
		return -EINVAL;
	const uint32_t amask = in->align ? in->align - 1 : 0;

	for (uint32_t k = 0; k < in->nconn; k++) {
		const struct gcl_tcp_conn *cn = &in->conn[k];
		struct gcl_tcp_conn_out *o = &out->out_conn[k];

		memset(o, 0, sizeof(*o));
		o->snd_una = cn->snd_una;
		o->snd_wnd = cn->snd_wnd;
		o->snd_wl1 = cn->snd_wl1;
		o->snd_wl2 = cn->snd_wl2;
		o->rcv_nxt = cn->rcv_nxt;
		o->rcv_wnd = cn->rcv_wnd;
		o->first_slow = GCL_TCPRX_NONE;
		o->acks_delayed_cnt = cn->acks_delayed_cnt;
		o->flags = cn->flags & (GCL_TCPC_RXQ | GCL_TCPC_ACK_DELAYED);
	}
	for (uint64_t j = 0; j < in->m; j++) {
		struct gcl_tcprx_seg s = {0, 0, 0, 0, 0};
		const uint32_t k = tcprx_entry(b, in, j, &s);
		uint32_t verdict, sf = 0, after = 0, len = 0;

		if (k == GCL_TCPRX_NONE) {
			verdict = GCL_TCPRX_NA;
		} else if (k >= in->nconn) {
			verdict = GCL_TCPRX_NOCONN;
		} else if (s.len > in->conn[k].rcv_mss) {
			verdict = GCL_TCPRX_DROP;
		} else {
			struct gcl_tcp_conn_out *o = &out->out_conn[k];
			struct gcl_tcprx_live l = {o->snd_una, o->snd_wnd, o->snd_wl1, o->snd_wl2, o->rcv_nxt,
			                           o->rcv_wnd, o->acks_delayed_cnt, o->flags};
			const int stopped = (l.flags & GCL_TCPO_STOPPED) != 0;

			verdict = gcl_tcprx_one(&in->conn[k], &l, &s, &sf);
			if (verdict == GCL_TCPRX_FAST) {
				o->snd_una = l.snd_una;
				o->snd_wnd = l.snd_wnd;
				o->snd_wl1 = l.snd_wl1;
				o->snd_wl2 = l.snd_wl2;
				o->rcv_nxt = l.rcv_nxt;
				o->rcv_wnd = l.rcv_wnd;
				o->acks_delayed_cnt = (uint8_t)l.cnt;
				o->nfast++;
				o->nacks += (sf & GCL_TCPRX_SF_ACK_NOW) != 0;
				after = l.rcv_nxt;
				len = s.len;
				c[GCL_TCPRXC_BYTES] += len;
				c[GCL_TCPRXC_ACKS] += (sf & GCL_TCPRX_SF_ACK_NOW) != 0;
				c[GCL_TCPRXC_WAKES] += (sf & GCL_TCPRX_SF_WAKE) != 0;
			} else {
				o->nslow++;
				if (!stopped)
					o->first_slow = (uint32_t)j;
			}
			o->flags = (uint8_t)l.flags;
		}
		out->verdict[j] = (uint8_t)verdict;
		out->sflags[j] = (uint8_t)sf;
		out->rcv_nxt_after[j] = after;
		out->copy_len[j] = (uint16_t)len;
		/* for now the offset inside the connection's region */
		out->dst_off[j] = verdict == GCL_TCPRX_FAST ? (uint32_t)(s.seq - in->conn[k].rcv_nxt) : 0;
		c[verdict]++;
	}
	for (uint32_t k = 0; k < in->nconn; k++) {
		out->conn_off[k] = at;
		at += gcl_tcprx_pad((uint32_t)(out->out_conn[k].rcv_nxt - in->conn[k].rcv_nxt), amask);
	}
	out->conn_off[in->nconn] = at;
	for (uint64_t j = 0; j < in->m; j++)
		if (out->verdict[j] == GCL_TCPRX_FAST) {
			const uint64_t i = in->order ? in->order[j] : j;
			out->dst_off[j] += out->conn_off[in->sock[i]];
		}
	if (counts)
		for (int k = 0; k < GCL_TCPRXC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* The rule of gcl_tcp_rx_full (gclassify.h) on the CPU: gcl_tcp_rx_host's walk
 * with gcl_tcprxf_one of gcl_tcprxf.h for every segment, every connection's
 * live words kept in out_conn and out_ext. */
int gcl_tcp_rx_full_host(const struct gcl_batch *b, const struct gcl_tcprxf_in *fin,
                         const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext, uint64_t *counts)
{
	uint64_t c[GCL_TCPRXFC_NR] = {0}, at = 0;

	if (!b || !fin || !out || fin->size != sizeof(*fin))
		return -EINVAL;
	const struct gcl_tcprx_in rin = {sizeof(rin), fin->align, fin->order, fin->m, fin->sock, fin->l4_status,
	                                 fin->conn, fin->nconn, fin->blocks};
	const struct gcl_tcprx_in *in = &rin;

	if (!gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || in->m > (1ull << 31) || in->nconn > GCL_TCPRX_MAX_CONN ||
	    in->blocks > GCL_TCPRX_MAX_BLOCKS || !in->sock || !out->conn_off)
		return -EINVAL;
	if (in->nconn && (!in->conn || !out->out_conn || !out_ext))
		return -EINVAL;
	if (in->m && (!out->verdict || !out->sflags || !out->rcv_nxt_after || !out->copy_len || !out->dst_off))
		return -EINVAL;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->conn & 15) ||
	    ((uintptr_t)out->rcv_nxt_after & 3) || ((uintptr_t)out->copy_len & 1) || ((uintptr_t)out->dst_off & 7) ||
	    ((uintptr_t)out->out_conn & 15) || ((uintptr_t)out->conn_off & 7) || ((uintptr_t)counts & 7) ||
	    ((uintptr_t)out_ext & 15))
		return -EINVAL;
	if (in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	              (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	              !b->pkt_len || ((uintptr_t)b->pkt_len & 1)))
		return -EINVAL;
	const uint32_t amask = in->align ? in->align - 1 : 0;

	for (uint32_t k = 0; k < in->nconn; k++) {
		const struct gcl_tcp_conn *cn = &in->conn[k];
		struct gcl_tcp_conn_out *o = &out->out_conn[k];

		memset(o, 0, sizeof(*o));
		o->snd_una = cn->snd_una;
		o->snd_wnd = cn->snd_wnd;
		o->snd_wl1 = cn->snd_wl1;
		o->snd_wl2 = cn->snd_wl2;
		o->rcv_nxt = cn->rcv_nxt;
		o->rcv_wnd = cn->rcv_wnd;
		o->first_slow = GCL_TCPRX_NONE;
		o->acks_delayed_cnt = cn->acks_delayed_cnt;
		o->flags = cn->flags & (GCL_TCPC_RXQ | GCL_TCPC_ACK_DELAYED);
		memset(&out_ext[k], 0, sizeof(out_ext[k]));
		out_ext[k].rep_acks = fin->rep_acks ? fin->rep_acks[k] : 0;
	}
	for (uint64_t j = 0; j < in->m; j++) {
		struct gcl_tcprx_seg s = {0, 0, 0, 0, 0};
		const uint32_t k = tcprx_entry(b, in, j, &s);
		uint32_t verdict, sf = 0, after = 0, len = 0;

		if (k == GCL_TCPRX_NONE) {
			verdict = GCL_TCPRX_NA;
		} else if (k >= in->nconn) {
			verdict = GCL_TCPRX_NOCONN;
		} else if (s.len > in->conn[k].rcv_mss) {
			verdict = GCL_TCPRX_DROP;
		} else {
			struct gcl_tcp_conn_out *o = &out->out_conn[k];
			struct gcl_tcp_conn_ext *e = &out_ext[k];
			struct gcl_tcprxf_live x = {{o->snd_una, o->snd_wnd, o->snd_wl1, o->snd_wl2, o->rcv_nxt,
			                             o->rcv_wnd, o->acks_delayed_cnt, o->flags},
			                            e->rep_acks, e->fast_rtx_ack, e->xflags};
			const int stopped = (x.l.flags & GCL_TCPO_STOPPED) != 0;

			verdict = gcl_tcprxf_one(&in->conn[k], &x, &s, &sf, &len);
			if (verdict == GCL_TCPRX_FAST) {
				o->snd_una = x.l.snd_una;
				o->snd_wnd = x.l.snd_wnd;
				o->snd_wl1 = x.l.snd_wl1;
				o->snd_wl2 = x.l.snd_wl2;
				o->rcv_nxt = x.l.rcv_nxt;
				o->rcv_wnd = x.l.rcv_wnd;
				o->acks_delayed_cnt = (uint8_t)x.l.cnt;
				o->nfast++;
				o->nacks += (sf & GCL_TCPRX_SF_ACK_NOW) != 0;
				e->nrule2 += (sf & GCL_TCPRX_SF_RULE2) != 0;
				e->ndropped += (sf & GCL_TCPRX_SF_DROPPED) != 0;
				e->fast_rtx_ack = x.fast_rtx_ack;
				e->rep_acks = (uint8_t)x.rep_acks;
				e->xflags = (uint8_t)x.xflags;
				after = x.l.rcv_nxt;
				c[GCL_TCPRXC_BYTES] += len;
				c[GCL_TCPRXC_ACKS] += (sf & GCL_TCPRX_SF_ACK_NOW) != 0;
				c[GCL_TCPRXC_WAKES] += (sf & GCL_TCPRX_SF_WAKE) != 0;
				c[GCL_TCPRXFC_RULE2] += (sf & GCL_TCPRX_SF_RULE2) != 0;
				c[GCL_TCPRXFC_TXWAKES] += (sf & GCL_TCPRX_SF_TXWAKE) != 0;
				c[GCL_TCPRXFC_FASTRTX] += (sf & GCL_TCPRX_SF_FASTRTX) != 0;
				c[GCL_TCPRXFC_DUPACKS] += (sf & GCL_TCPRXF_EV_DUPACK) != 0;
				c[GCL_TCPRXFC_DROPPED] += (sf & GCL_TCPRX_SF_DROPPED) != 0;
			} else {
				o->nslow++;
				if (!stopped)
					o->first_slow = (uint32_t)j;
			}
			o->flags = (uint8_t)x.l.flags;
		}
		out->verdict[j] = (uint8_t)verdict;
		out->sflags[j] = (uint8_t)sf;
		out->rcv_nxt_after[j] = after;
		out->copy_len[j] = (uint16_t)len;
		/* for now the offset inside the connection's region */
		out->dst_off[j] = len ? (uint32_t)(s.seq - in->conn[k].rcv_nxt) : 0;
		c[verdict]++;
	}
	for (uint32_t k = 0; k < in->nconn; k++) {
		out->conn_off[k] = at;
		at += gcl_tcprx_pad((uint32_t)(out->out_conn[k].rcv_nxt - in->conn[k].rcv_nxt), amask);
	}
	out->conn_off[in->nconn] = at;
	for (uint64_t j = 0; j < in->m; j++)
		if (out->copy_len[j]) {
			const uint64_t i = in->order ? in->order[j] : j;
			out->dst_off[j] += out->conn_off[in->sock[i]];
		}
	if (counts)
		for (int k = 0; k < GCL_TCPRXFC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* a live queue entry of gcl_tcp_rx_ooo_host: @fl is flags | src << 16, @idx the index into q or the list */
struct tcprxo_ent {
	uint32_t seq, end, fl, idx;
};

struct tcprxo_cnt {
	uint32_t ooo, queued, drained, freed, headclip, held;
};

/* what a queue entry that leaves the queue gets: @t is GCL_TCPRXO_APPEND or GCL_TCPRXO_FREE */
static void tcprxo_fate(const struct gcl_tcprx_out *out, const struct gcl_tcprxo_out *oo,
                        const struct tcprxo_ent *e, uint32_t t, uint32_t head, uint32_t ln, uint32_t rel)
{
	if (e->fl >> 16) {
		const uint32_t j = e->idx;

		out->copy_len[j] = (uint16_t)ln;
		out->dst_off[j] = ln ? rel : 0;
		oo->oflags[j] = (uint8_t)(GCL_OOOF_OOO | GCL_OOOF_QUEUED | (head ? GCL_OOOF_HEADCLIP : 0) |
		                          (t == GCL_TCPRXO_APPEND ? GCL_OOOF_LATE_DRAINED : GCL_OOOF_LATE_FREED));
		oo->skip[j] = (uint16_t)head;
	} else {
		const uint32_t i = e->idx;

		oo->qin_state[i] = t == GCL_TCPRXO_APPEND ? GCL_OOOQ_DRAINED : GCL_OOOQ_FREED;
		oo->qin_skip[i] = gcl_tcprxo_u16(head);
		oo->qin_len[i] = gcl_tcprxo_u16(ln);
		oo->qin_dst_off[i] = ln ? rel : 0;
	}
}

/* tcp_in.c:124-135 over the live queue: the insert position, or GCL_TCPRXO_REJECT */
static uint32_t tcprxo_find(const struct tcprxo_ent *Q, uint32_t qn, uint32_t seq, uint32_t end)
{
	uint64_t ends = 0, seqs = 0;

	for (uint32_t i = 0; i < qn; i++) {
		const uint32_t t = gcl_tcprxo_pos_test(seq, end, Q[i].seq, Q[i].end);

		ends |= (uint64_t)(t & GCL_TCPRXO_POS_END ? 1 : 0) << i;
		seqs |= (uint64_t)(t & GCL_TCPRXO_POS_SEQ ? 1 : 0) << i;
	}
	return gcl_tcprxo_pos(ends, seqs);
}

/* The rule of gcl_tcp_rx_ooo (gclassify.h) on the CPU: the list is threaded
 * per connection (next[], in list order), then every connection walks its
 * segments with its queue in a local array of GCL_TCPOOO_CAP entries, composed
 * of the pieces of gcl_tcprxo.h as the GPU walk composes them. */
int gcl_tcp_rx_ooo_host(const struct gcl_batch *b, const struct gcl_tcprxo_in *oin,
                        const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                        const struct gcl_tcprxo_out *oo, uint64_t *counts)
{
	uint64_t c[GCL_TCPRXOC_NR] = {0}, at = 0;

	if (!b || !oin || !out || !oo || oin->size != sizeof(*oin))
		return -EINVAL;
	const struct gcl_tcprx_in rin = {sizeof(rin), oin->align, oin->order, oin->m, oin->sock, oin->l4_status,
	                                 oin->conn, oin->nconn, oin->blocks};
	const struct gcl_tcprx_in *in = &rin;
	const uint32_t nq = oin->nq;

	if (!gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || in->m > (1ull << 31) || in->nconn > GCL_TCPRX_MAX_CONN ||
	    in->blocks > GCL_TCPRX_MAX_BLOCKS || !in->sock || !out->conn_off || nq > (1u << 31) || !oo->qout_off ||
	    !oo->totals)
		return -EINVAL;
	if (in->nconn && (!in->conn || !out->out_conn || !out_ext))
		return -EINVAL;
	if (in->m && (!out->verdict || !out->sflags || !out->rcv_nxt_after || !out->copy_len || !out->dst_off ||
	              !oo->oflags || !oo->skip))
		return -EINVAL;
	if (nq && (!oin->q || !oo->qin_state || !oo->qin_skip || !oo->qin_len || !oo->qin_dst_off))
		return -EINVAL;
	if (oin->q_out_cap && !oo->qout)
		return -EINVAL;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->conn & 15) ||
	    ((uintptr_t)out->rcv_nxt_after & 3) || ((uintptr_t)out->copy_len & 1) || ((uintptr_t)out->dst_off & 7) ||
	    ((uintptr_t)out->out_conn & 15) || ((uintptr_t)out->conn_off & 7) || ((uintptr_t)counts & 7) ||
	    ((uintptr_t)out_ext & 15) || ((uintptr_t)oin->q_off & 3) || ((uintptr_t)oin->q & 15) ||
	    ((uintptr_t)oo->skip & 1) || ((uintptr_t)oo->qin_skip & 1) || ((uintptr_t)oo->qin_len & 1) ||
	    ((uintptr_t)oo->qin_dst_off & 7) || ((uintptr_t)oo->qout_off & 3) || ((uintptr_t)oo->qout & 15) ||
	    ((uintptr_t)oo->totals & 7))
		return -EINVAL;
	if (in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	              (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	              !b->pkt_len || ((uintptr_t)b->pkt_len & 1)))
		return -EINVAL;
	const uint32_t amask = in->align ? in->align - 1 : 0;
	/* first[k], last[k] and next[j]: connection k's segments in list order */
	uint32_t *link = malloc(4 * ((size_t)in->m + 2 * (size_t)in->nconn) + 4);

	if (!link)
		return -ENOMEM;
	uint32_t *first = link, *last = link + in->nconn, *next = link + 2 * (size_t)in->nconn;

	for (uint32_t k = 0; k < in->nconn; k++)
		first[k] = last[k] = GCL_TCPRX_NONE;
	for (uint32_t i = 0; i < nq; i++) {
		oo->qin_state[i] = GCL_OOOQ_UNTOUCHED;
		oo->qin_skip[i] = 0;
		oo->qin_len[i] = 0;
		oo->qin_dst_off[i] = 0;
	}
	for (uint64_t j = 0; j < in->m; j++) {
		struct gcl_tcprx_seg s = {0, 0, 0, 0, 0};
		const uint32_t k = tcprx_entry(b, in, j, &s);
		const uint32_t verdict = k == GCL_TCPRX_NONE ? GCL_TCPRX_NA : k >= in->nconn ? GCL_TCPRX_NOCONN :
		                         s.len > in->conn[k].rcv_mss ? GCL_TCPRX_DROP : GCL_TCPRX_FAST;

		out->verdict[j] = (uint8_t)verdict;
		out->sflags[j] = 0;
		out->rcv_nxt_after[j] = 0;
		out->copy_len[j] = 0;
		out->dst_off[j] = 0;
		oo->oflags[j] = 0;
		oo->skip[j] = 0;
		next[j] = GCL_TCPRX_NONE;
		if (verdict != GCL_TCPRX_FAST) {
			c[verdict]++;
			continue;
		}
		if (first[k] == GCL_TCPRX_NONE)
			first[k] = (uint32_t)j;
		else
			next[last[k]] = (uint32_t)j;
		last[k] = (uint32_t)j;
	}
	for (uint32_t k = 0; k < in->nconn; k++) {
		struct gcl_tcp_conn cn = in->conn[k];
		struct gcl_tcp_conn_out *o = &out->out_conn[k];
		struct gcl_tcp_conn_ext *e = &out_ext[k];
		struct gcl_tcprxf_live x = {gcl_tcprx_live_of(&cn), oin->rep_acks ? oin->rep_acks[k] : 0, 0, 0};
		struct tcprxo_ent Q[GCL_TCPOOO_CAP];
		struct tcprxo_cnt n = {0, 0, 0, 0, 0, 0};
		uint32_t qs = 0, qe = 0, qn = 0, nfast = 0, nslow = 0, nacks = 0, nrule2 = 0, ndropped = 0;
		uint32_t first_slow = GCL_TCPRX_NONE;

		if (oin->q_off) {
			qs = oin->q_off[k] < nq ? oin->q_off[k] : nq;
			qe = oin->q_off[k + 1] < nq ? oin->q_off[k + 1] : nq;
			if (qe < qs)
				qe = qs;
		}
		int taken = gcl_tcprxo_state_ok(cn.flags) && qe - qs <= GCL_TCPOOO_CAP;

		for (uint32_t i = qs; taken && i < qe; i++) {
			Q[i - qs] = (struct tcprxo_ent){oin->q[i].seq, oin->q[i].end, oin->q[i].flags, i};
			if (oin->q[i].flags & GCL_TCPRX_FIN)
				taken = 0;
		}
		if (taken) {
			qn = qe - qs;
			cn.flags |= GCL_TCPC_ELIGIBLE;
		} else if (qe != qs) {
			x.xflags |= GCL_TCPX_QSKIP;
		}
		for (uint32_t j = first[k]; j != GCL_TCPRX_NONE; j = next[j]) {
			struct gcl_tcprx_seg s = {0, 0, 0, 0, 0};
			struct gcl_tcprxo_mid mid;
			uint32_t sf = 0, len = 0, head = 0, of = 0;
			const uint32_t rel = x.l.rcv_nxt - in->conn[k].rcv_nxt; /* where an in-order piece lands */
			int stop = (x.l.flags & GCL_TCPO_STOPPED) != 0 || !taken;

			(void)tcprx_entry(b, in, j, &s);
			if (!stop && qn == GCL_TCPOOO_CAP && gcl_tcprxo_reaches_ooo(&cn, &x.l, &s))
				stop = tcprxo_find(Q, qn, s.seq, s.seq + s.len) != GCL_TCPRXO_REJECT;
			if (!stop) {
				const uint32_t st = gcl_tcprxo_head(&cn, &x, &s, qn, &mid, &len);

				if (st == GCL_TCPRXO_STOP) {
					stop = 1;
				} else if (st == GCL_TCPRXO_FASTED) {
					sf = mid.sf;
				} else {
					if (st == GCL_TCPRXO_TEXT) {
						int used = 1, wake = 0;

						if (gcl_tcprxo_in_order(&x.l, s.seq)) {
							wake = gcl_tcprxo_in_order_wake(&x.l, s.flags);
							gcl_tcprxo_append(&x.l, s.seq, s.seq + s.len, &head, &len);
							if (head) {
								of |= GCL_OOOF_HEADCLIP;
								n.headclip++;
							}
						} else {
							const uint32_t pos = tcprxo_find(Q, qn, s.seq, s.seq + s.len);

							of |= GCL_OOOF_OOO;
							n.ooo++;
							if (pos == GCL_TCPRXO_REJECT) {
								used = 0;
							} else {
								memmove(&Q[pos + 1], &Q[pos], (qn - pos) * sizeof(Q[0]));
								Q[pos] = (struct tcprxo_ent){s.seq, s.seq + s.len, s.flags | 1u << 16, j};
								qn++;
								of |= GCL_OOOF_QUEUED;
								n.queued++;
							}
						}
						while (used && qn) {
							const uint32_t t = gcl_tcprxo_drain_test(Q[0].seq, Q[0].end, x.l.rcv_nxt);
							uint32_t h = 0, ln = 0;
							const uint32_t r = x.l.rcv_nxt - in->conn[k].rcv_nxt;

							if (t == GCL_TCPRXO_BREAK)
								break;
							if (t == GCL_TCPRXO_APPEND) {
								wake = 1;
								gcl_tcprxo_append(&x.l, Q[0].seq, Q[0].end, &h, &ln);
								n.headclip += h != 0;
								n.drained++;
							} else {
								n.freed++;
							}
							tcprxo_fate(out, oo, &Q[0], t, h, ln, r);
							memmove(&Q[0], &Q[1], (qn - 1) * sizeof(Q[0]));
							qn--;
						}
						gcl_tcprxo_text_tail(&x.l, &mid, used, wake, qn);
					}
					sf = gcl_tcprxo_done(&x.l, &mid);
				}
			}
			if (stop) {
				if (!(x.l.flags & GCL_TCPO_STOPPED))
					first_slow = j;
				x.l.flags |= GCL_TCPO_STOPPED;
				nslow++;
				out->verdict[j] = GCL_TCPRX_SLOW;
				c[GCL_TCPRX_SLOW]++;
				continue;
			}
			nfast++;
			nacks += (sf & GCL_TCPRX_SF_ACK_NOW) != 0;
			nrule2 += (sf & GCL_TCPRX_SF_RULE2) != 0;
			ndropped += (sf & GCL_TCPRX_SF_DROPPED) != 0;
			c[GCL_TCPRX_FAST]++;
			c[GCL_TCPRXC_WAKES] += (sf & GCL_TCPRX_SF_WAKE) != 0;
			c[GCL_TCPRXFC_TXWAKES] += (sf & GCL_TCPRX_SF_TXWAKE) != 0;
			c[GCL_TCPRXFC_FASTRTX] += (sf & GCL_TCPRX_SF_FASTRTX) != 0;
			c[GCL_TCPRXFC_DUPACKS] += (sf & GCL_TCPRXF_EV_DUPACK) != 0;
			out->sflags[j] = (uint8_t)sf;
			out->rcv_nxt_after[j] = x.l.rcv_nxt;
			if (!(of & GCL_OOOF_QUEUED)) { /* a queued entry gets these with its fate */
				out->copy_len[j] = (uint16_t)len;
				out->dst_off[j] = len ? rel : 0;
				oo->oflags[j] = (uint8_t)of;
				oo->skip[j] = (uint16_t)head;
			}
		}
		for (uint32_t i = 0; i < qn; i++) {
			if (Q[i].fl >> 16) {
				oo->oflags[Q[i].idx] = GCL_OOOF_OOO | GCL_OOOF_QUEUED | GCL_OOOF_HELD;
				n.held++;
			} else {
				oo->qin_state[Q[i].idx] = GCL_OOOQ_KEPT;
			}
			if (at + i < oin->q_out_cap)
				oo->qout[at + i] = (struct gcl_tcp_ooo_ent){Q[i].seq, Q[i].end,
				                                            Q[i].fl >> 16 ? Q[i].idx : oin->q[Q[i].idx].ref,
				                                            (uint16_t)Q[i].fl, (uint16_t)(Q[i].fl >> 16)};
		}
		oo->qout_off[k] = (uint32_t)at;
		at += qn;
		memset(o, 0, sizeof(*o));
		o->snd_una = x.l.snd_una;
		o->snd_wnd = x.l.snd_wnd;
		o->snd_wl1 = x.l.snd_wl1;
		o->snd_wl2 = x.l.snd_wl2;
		o->rcv_nxt = x.l.rcv_nxt;
		o->rcv_wnd = x.l.rcv_wnd;
		o->nfast = nfast;
		o->nslow = nslow;
		o->nacks = nacks;
		o->first_slow = first_slow;
		o->acks_delayed_cnt = (uint8_t)x.l.cnt;
		o->flags = (uint8_t)x.l.flags;
		memset(e, 0, sizeof(*e));
		e->nrule2 = nrule2;
		e->ndropped = ndropped;
		e->fast_rtx_ack = x.fast_rtx_ack;
		e->rep_acks = (uint8_t)x.rep_acks;
		e->xflags = (uint8_t)x.xflags;
		c[GCL_TCPRXC_BYTES] += (uint32_t)(x.l.rcv_nxt - in->conn[k].rcv_nxt);
		c[GCL_TCPRXC_ACKS] += nacks;
		c[GCL_TCPRXFC_RULE2] += nrule2;
		c[GCL_TCPRXFC_DROPPED] += ndropped;
		c[GCL_TCPRXOC_OOO] += n.ooo;
		c[GCL_TCPRXOC_QUEUED] += n.queued;
		c[GCL_TCPRXOC_DRAINED] += n.drained;
		c[GCL_TCPRXOC_FREED] += n.freed;
		c[GCL_TCPRXOC_HEADCLIP] += n.headclip;
		c[GCL_TCPRXOC_HELD] += n.held;
	}
	oo->qout_off[in->nconn] = (uint32_t)at;
	oo->totals[0] = at;
	at = 0;
	for (uint32_t k = 0; k < in->nconn; k++) {
		out->conn_off[k] = at;
		at += gcl_tcprx_pad((uint32_t)(out->out_conn[k].rcv_nxt - in->conn[k].rcv_nxt), amask);
	}
	out->conn_off[in->nconn] = at;
	/* the layout: every accepted piece moves by its connection's offset */
	for (uint32_t k = 0; k < in->nconn; k++) {
		for (uint32_t j = first[k]; j != GCL_TCPRX_NONE; j = next[j])
			if (out->copy_len[j])
				out->dst_off[j] += out->conn_off[k];
		if (oin->q_off && gcl_tcprxo_state_ok(in->conn[k].flags)) {
			const uint32_t qs = oin->q_off[k] < nq ? oin->q_off[k] : nq;
			const uint32_t qe = oin->q_off[k + 1] < nq ? oin->q_off[k + 1] : nq;

			for (uint32_t i = qs; i < qe && qe - qs <= GCL_TCPOOO_CAP; i++)
				if (oo->qin_state[i] == GCL_OOOQ_DRAINED && oo->qin_len[i])
					oo->qin_dst_off[i] += out->conn_off[k];
		}
	}
	free(link);
	if (counts)
		for (int k = 0; k < GCL_TCPRXOC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* The rule of gcl_tcp_rx_states (gclassify.h) on the CPU: gcl_tcp_rx_ooo_host's
 * threading and walk, every connection's live state beside its queue, composed
 * of the pieces of gcl_tcprxs.h as the GPU walk composes them. */
int gcl_tcp_rx_states_host(const struct gcl_batch *b, const struct gcl_tcprxs_in *sin,
                           const struct gcl_tcprx_out *out, struct gcl_tcp_conn_ext *out_ext,
                           const struct gcl_tcprxo_out *oo, const struct gcl_tcprxs_out *so, uint64_t *counts)
{
	uint64_t c[GCL_TCPRXSC_NR] = {0}, at = 0;

	if (!b || !sin || !out || !oo || !so || sin->size != sizeof(*sin))
		return -EINVAL;
	const struct gcl_tcprx_in rin = {sizeof(rin), sin->align, sin->order, sin->m, sin->sock, sin->l4_status,
	                                 sin->conn, sin->nconn, sin->blocks};
	const struct gcl_tcprx_in *in = &rin;
	const uint32_t nq = sin->nq;

	if (!gcl_pay_align_ok(in->align) ||
	    (!in->order && in->m != b->n) || in->m > (1ull << 31) || in->nconn > GCL_TCPRX_MAX_CONN ||
	    in->blocks > GCL_TCPRX_MAX_BLOCKS || !in->sock || !out->conn_off || nq > (1u << 31) || !oo->qout_off ||
	    !oo->totals)
		return -EINVAL;
	if (in->nconn && (!in->conn || !out->out_conn || !out_ext || !so->state_out))
		return -EINVAL;
	if (in->m && (!out->verdict || !out->sflags || !out->rcv_nxt_after || !out->copy_len || !out->dst_off ||
	              !oo->oflags || !oo->skip || !so->ev || !so->rst_seq || !so->state_after))
		return -EINVAL;
	if (nq && (!sin->q || !oo->qin_state || !oo->qin_skip || !oo->qin_len || !oo->qin_dst_off))
		return -EINVAL;
	if (sin->q_out_cap && !oo->qout)
		return -EINVAL;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->conn & 15) ||
	    ((uintptr_t)out->rcv_nxt_after & 3) || ((uintptr_t)out->copy_len & 1) || ((uintptr_t)out->dst_off & 7) ||
	    ((uintptr_t)out->out_conn & 15) || ((uintptr_t)out->conn_off & 7) || ((uintptr_t)counts & 7) ||
	    ((uintptr_t)out_ext & 15) || ((uintptr_t)sin->q_off & 3) || ((uintptr_t)sin->q & 15) ||
	    ((uintptr_t)oo->skip & 1) || ((uintptr_t)oo->qin_skip & 1) || ((uintptr_t)oo->qin_len & 1) ||
	    ((uintptr_t)oo->qin_dst_off & 7) || ((uintptr_t)oo->qout_off & 3) || ((uintptr_t)oo->qout & 15) ||
	    ((uintptr_t)oo->totals & 7) || ((uintptr_t)so->rst_seq & 3))
		return -EINVAL;
	if (in->m && (!b->frames || b->frames_len == UINT64_MAX || b->n > (1ull << 40) ||
	              (!b->offs && (b->stride < 16 || (b->stride & 15) || b->stride > (1u << 20))) ||
	              !b->pkt_len || ((uintptr_t)b->pkt_len & 1)))
		return -EINVAL;
	const uint32_t amask = in->align ? in->align - 1 : 0;
	/* first[k], last[k] and next[j]: connection k's segments in list order */
	uint32_t *link = malloc(4 * ((size_t)in->m + 2 * (size_t)in->nconn) + 4);

	if (!link)
		return -ENOMEM;
	uint32_t *first = link, *last = link + in->nconn, *next = link + 2 * (size_t)in->nconn;

	for (uint32_t k = 0; k < in->nconn; k++)
		first[k] = last[k] = GCL_TCPRX_NONE;
	for (uint32_t i = 0; i < nq; i++) {
		oo->qin_state[i] = GCL_OOOQ_UNTOUCHED;
		oo->qin_skip[i] = 0;
		oo->qin_len[i] = 0;
		oo->qin_dst_off[i] = 0;
	}
	for (uint64_t j = 0; j < in->m; j++) {
		struct gcl_tcprx_seg s = {0, 0, 0, 0, 0};
		const uint32_t k = tcprx_entry(b, in, j, &s);
		const uint32_t verdict = k == GCL_TCPRX_NONE ? GCL_TCPRX_NA : k >= in->nconn ? GCL_TCPRX_NOCONN :
		                         s.len > in->conn[k].rcv_mss ? GCL_TCPRX_DROP : GCL_TCPRX_FAST;

		out->verdict[j] = (uint8_t)verdict;
		out->sflags[j] = 0;
		out->rcv_nxt_after[j] = 0;
		out->copy_len[j] = 0;
		out->dst_off[j] = 0;
		oo->oflags[j] = 0;
		oo->skip[j] = 0;
		so->ev[j] = 0;
		so->rst_seq[j] = 0;
		so->state_after[j] = 0;
		next[j] = GCL_TCPRX_NONE;
		if (verdict != GCL_TCPRX_FAST) {
			c[verdict]++;
			continue;
		}
		if (first[k] == GCL_TCPRX_NONE)
			first[k] = (uint32_t)j;
		else
			next[last[k]] = (uint32_t)j;
		last[k] = (uint32_t)j;
	}
	for (uint32_t k = 0; k < in->nconn; k++) {
		const struct gcl_tcp_conn cn = in->conn[k];
		struct gcl_tcp_conn_out *o = &out->out_conn[k];
		struct gcl_tcp_conn_ext *e = &out_ext[k];
		struct gcl_tcprxf_live x = {gcl_tcprx_live_of(&cn), sin->rep_acks ? sin->rep_acks[k] : 0, 0, 0};
		struct tcprxo_ent Q[GCL_TCPOOO_CAP];
		struct tcprxo_cnt n = {0, 0, 0, 0, 0, 0};
		uint32_t qs = 0, qe = 0, qn = 0, nfast = 0, nslow = 0, nacks = 0, nrule2 = 0, ndropped = 0;
		uint32_t first_slow = GCL_TCPRX_NONE;
		uint32_t st = gcl_tcprxs_state_of(sin->state, k, cn.flags);
		int dead = 0;

		if (sin->q_off) {
			qs = sin->q_off[k] < nq ? sin->q_off[k] : nq;
			qe = sin->q_off[k + 1] < nq ? sin->q_off[k + 1] : nq;
			if (qe < qs)
				qe = qs;
		}
		const int taken = gcl_tcprxs_state_ok(st) && qe - qs <= GCL_TCPOOO_CAP;

		if (taken) {
			for (uint32_t i = qs; i < qe; i++)
				Q[i - qs] = (struct tcprxo_ent){sin->q[i].seq, sin->q[i].end, sin->q[i].flags, i};
			qn = qe - qs;
		} else if (qe != qs) {
			x.xflags |= GCL_TCPX_QSKIP;
		}
		for (uint32_t j = first[k]; j != GCL_TCPRX_NONE; j = next[j]) {
			struct gcl_tcprx_seg s = {0, 0, 0, 0, 0};
			struct gcl_tcprxs_mid mid;
			uint32_t sf = 0, len = 0, head = 0, of = 0;
			const uint32_t rel = x.l.rcv_nxt - in->conn[k].rcv_nxt; /* where an in-order piece lands */
			int stop = (x.l.flags & GCL_TCPO_STOPPED) != 0 || !taken || dead;

			(void)tcprx_entry(b, in, j, &s);
			if (!stop && qn == GCL_TCPOOO_CAP) { /* would it be the 65th insert?  asked on copies: nothing moves */
				struct gcl_tcprxf_live xt = x;
				uint32_t stt = st, lt;

				if (gcl_tcprxs_head(&cn, &xt, &stt, &s, qn, &mid, &lt) == GCL_TCPRXO_TEXT &&
				    !gcl_tcprxo_in_order(&xt.l, s.seq))
					stop = tcprxo_find(Q, qn, s.seq, s.seq + mid.slen) != GCL_TCPRXO_REJECT;
			}
			if (!stop) {
				const uint32_t t0 = gcl_tcprxs_head(&cn, &x, &st, &s, qn, &mid, &len);

				if (t0 == GCL_TCPRXO_FASTED) {
					sf = mid.o.sf;
				} else {
					if (t0 == GCL_TCPRXO_TEXT) {
						const uint32_t end = s.seq + mid.slen;
						int used = 1, wake = 0;

						if (gcl_tcprxo_in_order(&x.l, s.seq)) {
							wake = gcl_tcprxs_in_order_wake(&x.l, s.flags);
							if (wake && (s.flags & GCL_TCPRX_FIN))
								mid.fin = 1;
							gcl_tcprxs_append(&x.l, s.seq, end, (s.flags & GCL_TCPRX_FIN) != 0, &head, &len);
							if (head) {
								of |= GCL_OOOF_HEADCLIP;
								n.headclip++;
							}
						} else {
							const uint32_t pos = tcprxo_find(Q, qn, s.seq, end);

							of |= GCL_OOOF_OOO;
							n.ooo++;
							if (pos == GCL_TCPRXO_REJECT) {
								used = 0;
							} else {
								memmove(&Q[pos + 1], &Q[pos], (qn - pos) * sizeof(Q[0]));
								Q[pos] = (struct tcprxo_ent){s.seq, end, s.flags | 1u << 16, j};
								qn++;
								of |= GCL_OOOF_QUEUED;
								n.queued++;
							}
						}
						while (used && qn) {
							const uint32_t t = gcl_tcprxo_drain_test(Q[0].seq, Q[0].end, x.l.rcv_nxt);
							uint32_t h = 0, ln = 0;
							const uint32_t r = x.l.rcv_nxt - in->conn[k].rcv_nxt;

							if (t == GCL_TCPRXO_BREAK)
								break;
							if (t == GCL_TCPRXO_APPEND) {
								wake = 1;
								if (Q[0].fl & GCL_TCPRX_FIN)
									mid.fin = 1;
								gcl_tcprxs_append(&x.l, Q[0].seq, Q[0].end, (Q[0].fl & GCL_TCPRX_FIN) != 0, &h, &ln);
								n.headclip += h != 0;
								n.drained++;
							} else {
								n.freed++;
							}
							tcprxo_fate(out, oo, &Q[0], t, h, ln, r);
							memmove(&Q[0], &Q[1], (qn - 1) * sizeof(Q[0]));
							qn--;
						}
						gcl_tcprxo_text_tail(&x.l, &mid.o, used, wake, qn);
						gcl_tcprxs_fin(&x, &st, &mid);
					}
					sf = gcl_tcprxo_done(&x.l, &mid.o);
				}
			}
			if (stop) {
				if (!(x.l.flags & GCL_TCPO_STOPPED))
					first_slow = j;
				x.l.flags |= GCL_TCPO_STOPPED;
				nslow++;
				out->verdict[j] = GCL_TCPRX_SLOW;
				c[GCL_TCPRX_SLOW]++;
				continue;
			}
			dead = gcl_tcprxs_ends(mid.ev);
			nfast++;
			nacks += (sf & GCL_TCPRX_SF_ACK_NOW) != 0;
			nrule2 += (sf & GCL_TCPRX_SF_RULE2) != 0;
			ndropped += (sf & GCL_TCPRX_SF_DROPPED) != 0;
			c[GCL_TCPRX_FAST]++;
			c[GCL_TCPRXC_WAKES] += (sf & GCL_TCPRX_SF_WAKE) != 0;
			c[GCL_TCPRXFC_TXWAKES] += (sf & GCL_TCPRX_SF_TXWAKE) != 0;
			c[GCL_TCPRXFC_FASTRTX] += (sf & GCL_TCPRX_SF_FASTRTX) != 0;
			c[GCL_TCPRXFC_DUPACKS] += (sf & GCL_TCPRXF_EV_DUPACK) != 0;
			c[GCL_TCPRXSC_RSTS] += (mid.ev & (GCL_TCPS_RST | GCL_TCPS_RST_ACK)) != 0;
			c[GCL_TCPRXSC_FAILS] += (mid.ev & GCL_TCPS_FAIL) != 0;
			c[GCL_TCPRXSC_FINS] += (mid.ev & GCL_TCPS_FIN) != 0;
			c[GCL_TCPRXSC_STATE_CHANGES] += (mid.ev & GCL_TCPS_STATE) != 0;
			out->sflags[j] = (uint8_t)sf;
			out->rcv_nxt_after[j] = x.l.rcv_nxt;
			so->ev[j] = (uint8_t)mid.ev;
			so->rst_seq[j] = mid.rst_seq;
			so->state_after[j] = (uint8_t)st;
			if (!(of & GCL_OOOF_QUEUED)) { /* a queued entry gets these with its fate */
				out->copy_len[j] = (uint16_t)len;
				out->dst_off[j] = len ? rel : 0;
				oo->oflags[j] = (uint8_t)of;
				oo->skip[j] = (uint16_t)head;
			}
		}
		for (uint32_t i = 0; i < qn; i++) {
			if (Q[i].fl >> 16) {
				oo->oflags[Q[i].idx] = GCL_OOOF_OOO | GCL_OOOF_QUEUED | GCL_OOOF_HELD;
				n.held++;
			} else {
				oo->qin_state[Q[i].idx] = GCL_OOOQ_KEPT;
			}
			if (at + i < sin->q_out_cap)
				oo->qout[at + i] = (struct gcl_tcp_ooo_ent){Q[i].seq, Q[i].end,
				                                            Q[i].fl >> 16 ? Q[i].idx : sin->q[Q[i].idx].ref,
				                                            (uint16_t)Q[i].fl, (uint16_t)(Q[i].fl >> 16)};
		}
		oo->qout_off[k] = (uint32_t)at;
		at += qn;
		memset(o, 0, sizeof(*o));
		o->snd_una = x.l.snd_una;
		o->snd_wnd = x.l.snd_wnd;
		o->snd_wl1 = x.l.snd_wl1;
		o->snd_wl2 = x.l.snd_wl2;
		o->rcv_nxt = x.l.rcv_nxt;
		o->rcv_wnd = x.l.rcv_wnd;
		o->nfast = nfast;
		o->nslow = nslow;
		o->nacks = nacks;
		o->first_slow = first_slow;
		o->acks_delayed_cnt = (uint8_t)x.l.cnt;
		o->flags = (uint8_t)x.l.flags;
		memset(e, 0, sizeof(*e));
		e->nrule2 = nrule2;
		e->ndropped = ndropped;
		e->fast_rtx_ack = x.fast_rtx_ack;
		e->rep_acks = (uint8_t)x.rep_acks;
		e->xflags = (uint8_t)x.xflags;
		so->state_out[k] = (uint8_t)st;
		c[GCL_TCPRXC_BYTES] += (uint32_t)(x.l.rcv_nxt - in->conn[k].rcv_nxt);
		c[GCL_TCPRXC_ACKS] += nacks;
		c[GCL_TCPRXFC_RULE2] += nrule2;
		c[GCL_TCPRXFC_DROPPED] += ndropped;
		c[GCL_TCPRXOC_OOO] += n.ooo;
		c[GCL_TCPRXOC_QUEUED] += n.queued;
		c[GCL_TCPRXOC_DRAINED] += n.drained;
		c[GCL_TCPRXOC_FREED] += n.freed;
		c[GCL_TCPRXOC_HEADCLIP] += n.headclip;
		c[GCL_TCPRXOC_HELD] += n.held;
	}
	oo->qout_off[in->nconn] = (uint32_t)at;
	oo->totals[0] = at;
	at = 0;
	for (uint32_t k = 0; k < in->nconn; k++) {
		out->conn_off[k] = at;
		at += gcl_tcprx_pad((uint32_t)(out->out_conn[k].rcv_nxt - in->conn[k].rcv_nxt), amask);
	}
	out->conn_off[in->nconn] = at;
	/* the layout: every accepted piece moves by its connection's offset */
	for (uint32_t k = 0; k < in->nconn; k++) {
		for (uint32_t j = first[k]; j != GCL_TCPRX_NONE; j = next[j])
			if (out->copy_len[j])
				out->dst_off[j] += out->conn_off[k];
		if (sin->q_off && gcl_tcprxs_state_ok(gcl_tcprxs_state_of(sin->state, k, in->conn[k].flags))) {
			const uint32_t qs = sin->q_off[k] < nq ? sin->q_off[k] : nq;
			const uint32_t qe = sin->q_off[k + 1] < nq ? sin->q_off[k + 1] : nq;

			for (uint32_t i = qs; i < qe && qe - qs <= GCL_TCPOOO_CAP; i++)
				if (oo->qin_state[i] == GCL_OOOQ_DRAINED && oo->qin_len[i])
					oo->qin_dst_off[i] += out->conn_off[k];
		}
	}
	free(link);
	if (counts)
		for (int k = 0; k < GCL_TCPRXSC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* what gcl_tcp_tick and gcl_tcp_rx_acks both refuse of the fields they share */
static int ctl_refused(uint32_t nconn, uint32_t blocks, uint64_t seg_cap, uint32_t frame_stride, uint64_t items,
                       const struct gcl_ctlseg_out *o, const uint64_t *counts)
{
	if (nconn > GCL_TICK_MAX_CONN || blocks > GCL_TICK_MAX_BLOCKS || seg_cap > (1ull << 31) ||
	    frame_stride < GCL_CTL_MIN_STRIDE || !o->totals)
		return 1;
	if (items && seg_cap && (!o->desc || !o->frame_off || !o->seg_conn || !o->seg_kind || !o->seg_src))
		return 1;
	return ((uintptr_t)o->desc & 15) || ((uintptr_t)o->frame_off & 7) || ((uintptr_t)o->seg_conn & 3) ||
	       ((uintptr_t)o->seg_src & 3) || ((uintptr_t)o->totals & 7) || ((uintptr_t)counts & 7);
}

/* segment @at of a call, when it lies below @seg_cap; returns whether it was written */
static int ctl_emit(const struct gcl_ctlseg_out *o, uint64_t at, uint64_t seg_cap, uint64_t frame_base,
                    uint32_t frame_stride, const struct gcl_tcp_conn *cn, const struct gcl_tcp_addr *ad, uint32_t c,
                    uint32_t kind, uint32_t src, uint32_t ack, uint32_t rcv_wnd)
{
	uint32_t a[4], d[8];

	if (at >= seg_cap)
		return 0;
	memcpy(a, ad, sizeof(a)); /* little-endian host */
	gcl_ctl_desc(a, gcl_ctl_seq(kind, cn->snd_una, cn->snd_nxt), ack, rcv_wnd, d);
	memcpy(&o->desc[at], d, sizeof(o->desc[at]));
	o->frame_off[at] = frame_base + at * frame_stride;
	o->seg_conn[at] = c;
	o->seg_kind[at] = (uint8_t)kind;
	o->seg_src[at] = src;
	return 1;
}

/* The rule of gcl_tcp_tick (gclassify.h) on the CPU: gcl_tmr_sweep of
 * gcl_tcptmr.h for every connection in turn, the segment count running. */
int gcl_tcp_tick_host(const struct gcl_tick_in *in, const struct gcl_tick_out *out, uint64_t *counts)
{
	uint64_t c[GCL_TICKC_NR] = {0}, at = 0;

	if (!in || !out || in->size != sizeof(*in) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->nconn, &out->seg, counts))
		return -EINVAL;
	if (in->nconn && (!in->tmr || !in->conn || !in->addr || !out->out_tmr))
		return -EINVAL;
	if (((uintptr_t)in->tmr & 15) || ((uintptr_t)in->conn & 15) || ((uintptr_t)in->addr & 15) ||
	    ((uintptr_t)out->out_tmr & 15))
		return -EINVAL;
	for (uint32_t k = 0; k < in->nconn; k++) {
		struct gcl_tcp_tmr_out o;
		uint32_t action = gcl_tmr_sweep(&in->tmr[k], in->now, &o);
		const uint32_t sg = gcl_tmr_segs(action);
		const struct gcl_tcp_conn *cn = &in->conn[k];
		int lost = 0;

		for (uint32_t kind = GCL_CTL_ACK; kind <= GCL_CTL_PROBE; kind++)
			if (sg & (1u << kind)) {
				lost |= !ctl_emit(&out->seg, at, in->seg_cap, in->frame_base, in->frame_stride, cn,
				                  &in->addr[k], k, kind, k, cn->rcv_nxt, cn->rcv_wnd);
				at++;
			}
		if (lost) {
			action |= GCL_TMRA_NOSPACE;
			o.action = (uint8_t)action;
		}
		out->out_tmr[k] = o;
		for (int x = 0; x <= GCL_TICKC_NOSPACE; x++)
			c[x] += (action >> x) & 1u;
	}
	out->seg.totals[0] = at;
	out->seg.totals[1] = c[GCL_TICKC_SEGS] = at < in->seg_cap ? at : in->seg_cap;
	if (counts)
		for (int k = 0; k < GCL_TICKC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* The rule of gcl_tcp_rx_acks (gclassify.h) on the CPU: one walk over the list. */
int gcl_tcp_rx_acks_host(const struct gcl_rxack_in *in, const struct gcl_ctlseg_out *out, uint64_t *counts)
{
	uint64_t at = 0, skipped = 0;

	if (!in || !out || in->size != sizeof(*in) || in->m > (1ull << 31) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->m, out, counts))
		return -EINVAL;
	if (in->m && (!in->sock || !in->verdict || !in->sflags || !in->rcv_nxt_after))
		return -EINVAL;
	if (in->m && in->nconn && (!in->conn || !in->addr))
		return -EINVAL;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->rcv_nxt_after & 3) ||
	    ((uintptr_t)in->conn & 15) || ((uintptr_t)in->addr & 15))
		return -EINVAL;
	for (uint64_t j = 0; j < in->m; j++) {
		if (!gcl_rxack_asked(in->verdict[j], in->sflags[j]))
			continue;
		const uint64_t i = in->order ? in->order[j] : j;
		const uint32_t k = i < in->n ? in->sock[i] : UINT32_MAX;

		if (k >= in->nconn) {
			skipped++;
			continue;
		}
		const struct gcl_tcp_conn *cn = &in->conn[k];
		const uint32_t after = in->rcv_nxt_after[j];
		(void)ctl_emit(out, at, in->seg_cap, in->frame_base, in->frame_stride, cn, &in->addr[k], k, GCL_CTL_ACK,
		               (uint32_t)j, after, gcl_rxack_wnd(cn->rcv_wnd, cn->rcv_nxt, after));
		at++;
	}
	out->totals[0] = at;
	out->totals[1] = at < in->seg_cap ? at : in->seg_cap;
	if (counts) {
		counts[GCL_RXACKC_WANTED] += at;
		counts[GCL_RXACKC_WRITTEN] += out->totals[1];
		counts[GCL_RXACKC_SKIPPED] += skipped;
	}
	return 0;
}

/* The rule of gcl_tcp_rx_ctl (gclassify.h) on the CPU: gcl_tcp_rx_acks_host's
 * walk with gcl_rxctl_kind of gcl_tcptmr.h saying which segment an entry asks for. */
int gcl_tcp_rx_ctl_host(const struct gcl_rxctl_in *in, const struct gcl_ctlseg_out *out, uint64_t *counts)
{
	uint64_t at = 0, skipped = 0;

	if (!in || !out || in->size != sizeof(*in) || in->m > (1ull << 31) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->m, out, counts))
		return -EINVAL;
	if (in->m && (!in->sock || !in->verdict || !in->sflags || !in->rcv_nxt_after || !in->ev || !in->rst_seq))
		return -EINVAL;
	if (in->m && in->nconn && (!in->conn || !in->addr))
		return -EINVAL;
	if (((uintptr_t)in->order & 3) || ((uintptr_t)in->sock & 3) || ((uintptr_t)in->rcv_nxt_after & 3) ||
	    ((uintptr_t)in->conn & 15) || ((uintptr_t)in->addr & 15) || ((uintptr_t)in->rst_seq & 3))
		return -EINVAL;
	for (uint64_t j = 0; j < in->m; j++) {
		const uint32_t kind = gcl_rxctl_kind(in->verdict[j], in->sflags[j], in->ev[j]);

		if (kind == GCL_RXCTL_NONE)
			continue;
		const uint64_t i = in->order ? in->order[j] : j;
		const uint32_t k = i < in->n ? in->sock[i] : UINT32_MAX;

		if (k >= in->nconn) {
			skipped++;
			continue;
		}
		const struct gcl_tcp_conn *cn = &in->conn[k];

		if (kind == GCL_CTL_ACK) {
			const uint32_t after = in->rcv_nxt_after[j];
			(void)ctl_emit(out, at, in->seg_cap, in->frame_base, in->frame_stride, cn, &in->addr[k], k, GCL_CTL_ACK,
			               (uint32_t)j, after, gcl_rxack_wnd(cn->rcv_wnd, cn->rcv_nxt, after));
		} else if (at < in->seg_cap) {
			uint32_t a[4], d[8];

			memcpy(a, &in->addr[k], sizeof(a)); /* little-endian host */
			gcl_ctl_rst_desc(a, kind, in->rst_seq[j], d);
			memcpy(&out->desc[at], d, sizeof(out->desc[at]));
			out->frame_off[at] = in->frame_base + at * in->frame_stride;
			out->seg_conn[at] = k;
			out->seg_kind[at] = (uint8_t)kind;
			out->seg_src[at] = (uint32_t)j;
		}
		at++;
	}
	out->totals[0] = at;
	out->totals[1] = at < in->seg_cap ? at : in->seg_cap;
	if (counts) {
		counts[GCL_RXACKC_WANTED] += at;
		counts[GCL_RXACKC_WRITTEN] += out->totals[1];
		counts[GCL_RXACKC_SKIPPED] += skipped;
	}
	return 0;
}

/* The rule of gcl_tcp_rx_open (gclassify.h) on the CPU, taken literally: one
 * walk over the list in order with the running backlog in backlog_out and the
 * tuples accepted so far in an open-addressed table, gcl_open_head and
 * gcl_open_walk of gcl_tcpopen.h for every entry. */
int gcl_tcp_rx_open_host(const struct gcl_batch *b, const struct gcl_tcpopen_in *in,
                         const struct gcl_tcpopen_out *out, const struct gcl_ctlseg_out *seg, uint64_t *counts)
{
	uint64_t c[GCL_OPENC_NR] = {0}, at = 0, nopen = 0;

	if (gcl_open_refused(b, in, out, seg, counts))
		return -EINVAL;
	if (in->m == 0)
		return 0;
	const uint64_t lim = gcl_open_seg_lim(in->seg_cap, in->frame_base, in->frame_stride, in->tx_frames_len);
	const uint64_t slots = in->hash_slots ? in->hash_slots : gcl_open_slots(in->m);
	struct open_acc { uint32_t lip, rip, ports, listener, k; } *tbl = malloc(slots * sizeof(*tbl));

	if (!tbl)
		return -ENOMEM;
	for (uint64_t x = 0; x < slots; x++)
		tbl[x].k = GCL_OPEN_NONE;
	for (uint32_t l = 0; l < in->nlisten; l++)
		out->backlog_out[l] = in->listen[l].backlog;
	for (uint64_t j = 0; j < in->m; j++) {
		const uint64_t i = in->order ? in->order[j] : j;
		struct gcl_open_ent e = {GCL_OPEN_OOR, 0, 0, 0, 0, 0, 0};
		struct gcl_open_opts op = {0, 0, 0, 0};
		uint32_t verdict, later = GCL_OPEN_NONE, l4[4] = {0, 0, 0, 0};
		uint64_t o = 0, avail = 0;

		if (i < b->n) {
			const uint64_t raw = b->offs ? b->offs[i] : i * b->stride;
			uint8_t h[56] = {0};
			uint32_t d[11];

			o = raw < b->frames_len ? raw : b->frames_len;
			avail = b->frames_len - o;
			const uint64_t L = b->pkt_len[i] < avail ? b->pkt_len[i] : avail;
			if (avail)
				memcpy(h, b->frames + o, avail < sizeof(h) ? avail : sizeof(h));
			for (int x = 0; x < 11; x++)
				d[x] = h[12 + 4 * x] | (uint32_t)h[13 + 4 * x] << 8 | (uint32_t)h[14 + 4 * x] << 16 |
				       (uint32_t)h[15 + 4 * x] << 24;
			e = gcl_open_head(d, L, in->l4_status != NULL, in->l4_status ? in->l4_status[i] : 0, in->sock[i],
			                  in->listen_base, in->nlisten);
		}
		verdict = e.cls;
		if (gcl_open_listener_route(e.cls)) {
			uint64_t s = gcl_open_hash(e.lip, e.rip, e.ports, e.listener) & (slots - 1);

			memcpy(l4, &in->listen[e.listener], sizeof(l4)); /* little-endian host */
			while (tbl[s].k != GCL_OPEN_NONE && !(tbl[s].lip == e.lip && tbl[s].rip == e.rip &&
			                                      tbl[s].ports == e.ports && tbl[s].listener == e.listener))
				s = (s + 1) & (slots - 1); /* ACCEPTs <= m <= slots / 2: an empty slot exists */
			later = tbl[s].k;
			/* the running backlog is backlog minus the ACCEPTs so far: "before" = those */
			verdict = gcl_open_final(e.cls, later != GCL_OPEN_NONE, gcl_open_l_flags(l4), gcl_open_l_backlog(l4),
			                         gcl_open_l_backlog(l4) - out->backlog_out[e.listener]);
			if (verdict == GCL_OPEN_ACCEPT) {
				uint8_t ob[GCL_OPEN_MAX_OPT] = {0};
				uint32_t w[10];

				for (uint32_t x = 0; x < e.optlen; x++)
					ob[x] = 54 + x < avail ? b->frames[o + 54 + x] : 0;
				for (int x = 0; x < 10; x++)
					w[x] = ob[4 * x] | (uint32_t)ob[4 * x + 1] << 8 | (uint32_t)ob[4 * x + 2] << 16 |
					       (uint32_t)ob[4 * x + 3] << 24;
				op = gcl_open_walk(w, e.optlen);
				if (op.bad)
					verdict = GCL_OPEN_BADOPT;
			}
			if (verdict == GCL_OPEN_ACCEPT) {
				out->backlog_out[e.listener]--;
				tbl[s].lip = e.lip;
				tbl[s].rip = e.rip;
				tbl[s].ports = e.ports;
				tbl[s].listener = e.listener;
				tbl[s].k = (uint32_t)j;
			}
		}
		out->verdict[j] = (uint8_t)verdict;
		out->later_of[j] = verdict == GCL_OPEN_LATER ? later : GCL_OPEN_NONE;
		out->rst_seq[j] = verdict == GCL_OPEN_RST || verdict == GCL_OPEN_CLOSED_RST ||
		                  verdict == GCL_OPEN_CLOSED_RST_ACK ? e.val : 0;
		c[verdict]++;
		if (verdict == GCL_OPEN_ACCEPT) {
			uint32_t r[16], dd[8];

			gcl_open_record(&e, &op, (uint32_t)j, in->iss[j], l4, r);
			if (nopen < in->open_cap)
				memcpy(&out->open[nopen], r, sizeof(out->open[nopen]));
			else
				c[GCL_OPENC_NOSPACE]++;
			if (at < lim) {
				uint8_t ob[8];
				const uint32_t nb = gcl_open_optbytes(r, l4, ob);
				const uint64_t fo = in->frame_base + at * in->frame_stride;

				gcl_open_synack_desc(r, dd);
				memcpy(&seg->desc[at], dd, sizeof(seg->desc[at]));
				seg->frame_off[at] = fo;
				seg->seg_conn[at] = (uint32_t)nopen;
				seg->seg_kind[at] = GCL_CTL_SYNACK;
				seg->seg_src[at] = (uint32_t)j;
				for (uint32_t x = 0; x < nb; x++)
					in->tx_frames[fo + 54 + x] = ob[x];
			}
			nopen++;
			at++;
		} else if (verdict == GCL_OPEN_RST || verdict == GCL_OPEN_CLOSED_RST || verdict == GCL_OPEN_CLOSED_RST_ACK) {
			if (at < lim) {
				const uint32_t a[4] = {e.lip, e.rip, e.ports, 0};
				const uint32_t kind = verdict == GCL_OPEN_CLOSED_RST_ACK ? GCL_CTL_RST_ACK : GCL_CTL_RST;
				uint32_t dd[8];

				gcl_ctl_rst_desc(a, kind, e.val, dd);
				memcpy(&seg->desc[at], dd, sizeof(seg->desc[at]));
				seg->frame_off[at] = in->frame_base + at * in->frame_stride;
				seg->seg_conn[at] = GCL_OPEN_NONE;
				seg->seg_kind[at] = (uint8_t)kind;
				seg->seg_src[at] = (uint32_t)j;
			}
			at++;
		}
	}
	free(tbl);
	out->totals[0] = nopen;
	out->totals[1] = nopen < in->open_cap ? nopen : in->open_cap;
	seg->totals[0] = at;
	seg->totals[1] = at < lim ? at : lim;
	c[GCL_OPENC_SEGS] = seg->totals[1];
	c[GCL_OPENC_SEGSKIP] = at - seg->totals[1];
	if (counts)
		for (int k = 0; k < GCL_OPENC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* One list entry of gcl_udp_rx: the frame's bytes [12, 48) as dwords, gcl_pay_rule's
 * word on them and gcl_udprx_class.  Returns the verdict so far (NA, NOSOCK, or
 * QUEUED for a datagram of socket *s). */
static uint32_t udprx_entry(const struct gcl_batch *b, const struct gcl_udprx_in *in, uint64_t j,
                            struct gcl_pay_desc *r, uint32_t *s)
{
	const uint64_t i = in->order ? in->order[j] : j;

	*s = GCL_UDPRX_NONE;
	if (i >= b->n)
		return GCL_UDPRX_NA;
	const uint64_t raw = b->offs ? b->offs[i] : i * b->stride;
	const uint64_t o = raw < b->frames_len ? raw : b->frames_len;
	const uint64_t avail = b->frames_len - o;
	const uint64_t L = b->pkt_len[i] < avail ? b->pkt_len[i] : avail;
	uint8_t h[48] = {0};
	uint32_t d[9];

	if (avail)
		memcpy(h, b->frames + o, avail < sizeof(h) ? avail : sizeof(h));
	for (int x = 0; x < 9; x++)
		d[x] = h[12 + 4 * x] | (uint32_t)h[13 + 4 * x] << 8 | (uint32_t)h[14 + 4 * x] << 16 |
		       (uint32_t)h[15 + 4 * x] << 24;
	*r = gcl_pay_rule(d, o, L, in->l4_status != NULL, in->l4_status ? in->l4_status[i] : 0, 1, in->sock[i]);
	return gcl_udprx_class(r, in->sock[i], in->sock_base, in->nsock, s);
}

/* The rule of gcl_udp_rx (gclassify.h) on the CPU, taken literally: one walk
 * over the list in order with every socket's running inq_len kept in out_sock,
 * gcl_udprx_step of gcl_udprx.h for every datagram as udp_conn_recv does it
 * under the lock (not the closed form the kernels use); then the layout, and a
 * second walk for dst_off, rec_idx and the records. */
int gcl_udp_rx_host(const struct gcl_batch *b, const struct gcl_udprx_in *in,
                    const struct gcl_udprx_out *out, uint64_t *counts)
{
	uint64_t c[GCL_UDPRXC_NR] = {0}, at = 0;
	uint32_t nrec = 0;

	if (gcl_udprx_refused(b, in, out, counts))
		return -EINVAL;
	const uint32_t amask = in->align ? in->align - 1 : 0;

	for (uint32_t s = 0; s < in->nsock; s++) {
		memset(&out->out_sock[s], 0, sizeof(out->out_sock[s]));
		out->out_sock[s].inq_len = in->usock[s].inq_len;
		out->sock_off[s] = 0;
	}
	for (uint64_t j = 0; j < in->m; j++) {
		struct gcl_pay_desc r;
		uint32_t s, sf = 0, len = 0, idx = GCL_UDPRX_NONE;
		uint32_t verdict = udprx_entry(b, in, j, &r, &s);
		uint64_t off = 0;

		if (verdict == GCL_UDPRX_QUEUED) {
			struct gcl_udp_sock_out *o = &out->out_sock[s];
			int32_t run = o->inq_len;

			verdict = gcl_udprx_step(&run, in->usock[s].inq_cap, in->usock[s].flags, &sf);
			o->inq_len = run;
			o->flags |= (uint8_t)sf;
			if (gcl_udprx_taken(verdict)) {
				len = r.len;
				/* for now the record and the offset inside the socket's region */
				idx = o->ntaken++;
				off = out->sock_off[s];
				out->sock_off[s] += gcl_pay_pad(len, amask);
				c[GCL_UDPRXC_BYTES] += len;
				c[GCL_UDPRXC_POLLINS] += (sf & GCL_UDPRX_SF_POLLIN) != 0;
			} else {
				o->ndropped++;
			}
		}
		out->verdict[j] = (uint8_t)verdict;
		out->sflags[j] = (uint8_t)sf;
		out->copy_len[j] = (uint16_t)len;
		out->dst_off[j] = off;
		out->rec_idx[j] = idx;
		c[verdict]++;
	}
	for (uint32_t s = 0; s < in->nsock; s++) {
		const uint64_t bytes = out->sock_off[s];

		out->rec_off[s] = nrec;
		out->sock_off[s] = at;
		nrec += out->out_sock[s].ntaken;
		at += bytes;
	}
	out->rec_off[in->nsock] = nrec;
	out->sock_off[in->nsock] = at;
	for (uint64_t j = 0; j < in->m; j++)
		if (gcl_udprx_taken(out->verdict[j])) {
			struct gcl_pay_desc r;
			struct gcl_udp_rec *rec;
			uint32_t s;

			(void)udprx_entry(b, in, j, &r, &s);
			out->dst_off[j] += out->sock_off[s];
			out->rec_idx[j] += out->rec_off[s];
			rec = &out->rec[out->rec_idx[j]];
			rec->dst_off = out->dst_off[j];
			rec->rip = r.meta[0];
			rec->rport = (uint16_t)gcl_udprx_rport(&r);
			rec->len = (uint16_t)r.len;
		}
	if (counts)
		for (int k = 0; k < GCL_UDPRXC_NR; k++)
			counts[k] += c[k];
	return 0;
}

/* The rule of gcl_tcp_txq (gclassify.h) on the CPU: gcl_txq_conn of gcl_txq.h
 * for every connection in turn, first for its count alone, as the GPU's decide
 * launch runs it, then with the room its position leaves it. */
int gcl_tcp_txq_host(const struct gcl_txq_in *in, const struct gcl_txq_out *out, uint64_t *counts)
{
	uint64_t c[GCL_TXQC_NR] = {0}, at = 0;

	if (!in || !out || in->size != sizeof(*in) || in->nconn > GCL_TXQ_MAX_CONN ||
	    in->blocks > GCL_TXQ_MAX_BLOCKS || in->nent > (1ull << 31) || in->seg_cap > (1ull << 31) ||
	    in->frame_stride < GCL_CTL_MIN_STRIDE || !out->totals)
		return -EINVAL;
	if (in->nconn && (!in->qoff || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if (in->nent && (!in->ent || !in->cold || !out->state))
		return -EINVAL;
	if (in->nconn && in->seg_cap && (!out->desc || !out->frame_off || !out->src_off || !out->len ||
	                                 !out->dst_off || !out->seg_conn || !out->seg_ent))
		return -EINVAL;
	if (((uintptr_t)in->qoff & 3) || ((uintptr_t)in->ent & 15) || ((uintptr_t)in->cold & 15) ||
	    ((uintptr_t)in->conn & 15) || ((uintptr_t)in->addr & 15) || ((uintptr_t)out->out_conn & 15) ||
	    ((uintptr_t)out->desc & 15) || ((uintptr_t)out->frame_off & 7) || ((uintptr_t)out->src_off & 7) ||
	    ((uintptr_t)out->len & 1) || ((uintptr_t)out->dst_off & 7) || ((uintptr_t)out->seg_conn & 3) ||
	    ((uintptr_t)out->seg_ent & 3) || ((uintptr_t)out->totals & 7) || ((uintptr_t)counts & 7))
		return -EINVAL;
	const struct gcl_txq_call k = {out, in->now, in->frame_base, in->frame_stride};

	for (uint32_t j = 0; j < in->nconn; j++) {
		const struct gcl_tcp_conn *cn = &in->conn[j];
		struct gcl_txq_cx x;
		struct gcl_txq_res r;
		uint32_t ad[4], e0, bad;
		const uint32_t n = gcl_txq_range(in->qoff[j], in->qoff[j + 1], in->nent, &e0, &bad);
		const uint64_t first = at < in->seg_cap ? at : in->seg_cap;

		memcpy(ad, &in->addr[j], sizeof(ad)); /* little-endian host */
		gcl_txq_cx_fill(&x, j, cn->snd_una, cn->rcv_nxt, cn->rcv_wnd, ad, in->want ? in->want[j] : 0);
		gcl_txq_conn(&k, &x, in->ent, in->cold, e0, n, 0, GCL_TXQ_NOROOM, 0, &r);
		at += r.nretx;
		if (r.nretx)
			gcl_txq_conn(&k, &x, in->ent, in->cold, e0, n, first, in->seg_cap - first, 1, &r);
		gcl_txq_conn_out(&out->out_conn[j], &r, bad, first);
		c[GCL_TXQC_ACKED] += r.nacked;
		c[GCL_TXQC_RETX] += r.nretx;
		c[GCL_TXQC_COPIED] += r.copied;
		c[GCL_TXQC_TRIMMED] += r.trimmed;
		c[GCL_TXQC_REFUSED] += r.refused;
		c[GCL_TXQC_NOSPACE] += (r.flags & GCL_TXQO_NOSPACE) ? 1 : 0;
		c[GCL_TXQC_DEFERRED] += (r.flags & GCL_TXQO_DEFERRED) ? 1 : 0;
		c[GCL_TXQC_BYTES] += r.bytes;
	}
	out->totals[0] = at;
	out->totals[1] = at < in->seg_cap ? at : in->seg_cap;
	out->totals[2] = c[GCL_TXQC_BYTES];
	if (counts)
		for (int i = 0; i < GCL_TXQC_NR; i++)
			counts[i] += c[i];
	return 0;
}

/* The rule of gcl_tcp_read (gclassify.h) on the CPU, one connection after the
 * other: the walks of gcl_tcpread.h, then copy_into_iov's two cursors over the
 * entries and the vectors for the items. */
int gcl_tcp_read_host(const struct gcl_rd_in *in, const struct gcl_rd_out *out, uint64_t *counts)
{
	uint64_t c[GCL_RDC_NR] = {0}, items = 0, segs = 0, bytes = 0, retsum = 0;

	if (!in || !out || in->size != sizeof(*in) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->nconn, &out->seg, counts))
		return -EINVAL;
	const uint64_t nvec = in->voff ? in->nvec : 0;
	if (in->nent > (1ull << 31) || nvec > (1ull << 31) || in->item_cap > (1ull << 31) || !out->totals)
		return -EINVAL;
	if (in->nconn && (!in->qoff || !in->rd || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if ((in->nent && !in->ent) || (nvec && !in->iov))
		return -EINVAL;
	if (in->nconn && in->item_cap && (!out->src_off || !out->len || !out->dst_off || !out->item_conn ||
	                                  !out->item_ent))
		return -EINVAL;
	if (((uintptr_t)in->qoff & 3) || ((uintptr_t)in->voff & 3) || ((uintptr_t)in->ent & 15) ||
	    ((uintptr_t)in->iov & 15) || ((uintptr_t)in->rd & 15) || ((uintptr_t)in->conn & 15) ||
	    ((uintptr_t)in->addr & 15) || ((uintptr_t)out->out_conn & 15) || ((uintptr_t)out->src_off & 7) ||
	    ((uintptr_t)out->len & 1) || ((uintptr_t)out->dst_off & 7) || ((uintptr_t)out->item_conn & 3) ||
	    ((uintptr_t)out->item_ent & 3) || ((uintptr_t)out->totals & 7))
		return -EINVAL;

	for (uint32_t j = 0; j < in->nconn; j++) {
		const struct gcl_tcp_rd *rd = &in->rd[j];
		const struct gcl_tcp_conn *cn = &in->conn[j];
		const struct gcl_rd_iov one = {rd->dst_off, rd->len, {0}};
		const struct gcl_rd_iov *iov = &one;
		struct gcl_rd_res r;
		uint32_t e0, v0 = 0, nv = 1, bad = 0, w[8], flags, written = 0;
		const uint32_t n = gcl_rd_range(in->qoff[j], in->qoff[j + 1], in->nent, &e0, &bad);
		const uint64_t first = items < in->item_cap ? items : in->item_cap;
		uint64_t len = rd->len;

		if (in->voff) {
			nv = gcl_rd_range(in->voff[j], in->voff[j + 1], nvec, &v0, &bad);
			iov = in->iov + v0;
			len = 0;
			for (uint32_t i = 0; i < nv; i++) /* iov_len() */
				len += iov[i].len;
		}
		if (bad)
			nv = 0;
		if (gcl_rd_wait(rd->flags, n, rd->err, bad, cn->rcv_wnd, &r)) {
			if (rd->flags & GCL_RD_PEEK) {
				gcl_rd_peek_done(&r, gcl_rd_peek_walk(in->ent, e0, n, len));
			} else {
				uint32_t npop, pull;
				int closed;
				const uint64_t readlen = gcl_rd_walk(in->ent, e0, n, len, &npop, &pull, &closed);

				gcl_rd_read_done(&r, readlen, npop, pull, closed, n, cn->rcv_nxt, rd->tx_last_ack,
				                 rd->tx_last_win, rd->winmax);
			}
		}
		flags = r.flags;
		if (r.status == GCL_RDS_DONE && r.ret > 0) { /* a CLOSED connection's -err is no length */
			/* copy_into_iov (tcp.c:1144-1181): entry i from @ea, vector v from @vb, the stream at @at */
			const uint64_t ret = (uint64_t)r.ret;
			uint64_t at = 0, ea = 0, vb = 0;
			uint32_t i = 0, v = 0;

			for (;;) {
				const struct gcl_rdq_ent *m = &in->ent[e0 + i];
				const uint64_t ee = ea + m->len < ret ? ea + m->len : ret;
				const uint64_t ve = vb + iov[v].len < ret ? vb + iov[v].len : ret;
				const uint64_t to = ee < ve ? ee : ve;
				const uint64_t k = items + r.nitems;

				if (k < in->item_cap) {
					gcl_rd_item_store(out, k, j, e0 + i, m->off, ea, iov[v].off, vb, at, to);
					written++;
					bytes += to - at;
				}
				r.nitems++;
				at = to;
				/* the one that ends here goes on; at a tie the entry first; neither past the byte @ret */
				if (ea + m->len <= vb + iov[v].len && ea + m->len < ret) {
					ea += m->len;
					i++;
				} else if (vb + iov[v].len < ret) {
					vb += iov[v].len;
					v++;
				} else {
					break;
				}
			}
			if (written < r.nitems)
				flags |= GCL_RDO_ITEM_NOSPACE;
			retsum += ret;
		}
		if (flags & GCL_RDO_ACK) {
			if (ctl_emit(&out->seg, segs, in->seg_cap, in->frame_base, in->frame_stride, cn, &in->addr[j], j,
			             GCL_CTL_ACK, j, cn->rcv_nxt, r.rcv_wnd))
				c[GCL_RDC_ACKS]++;
			else
				flags |= GCL_RDO_SEG_NOSPACE;
			segs++;
		}
		items += r.nitems;
		gcl_rd_conn_words(&r, (uint32_t)first, written, flags, w);
		memcpy(&out->out_conn[j], w, sizeof(w)); /* little-endian host */
		c[GCL_RDC_DONE] += r.status == GCL_RDS_DONE;
		c[GCL_RDC_AGAIN] += r.status == GCL_RDS_AGAIN;
		c[GCL_RDC_BLOCK] += r.status == GCL_RDS_BLOCK;
		c[GCL_RDC_CLOSED] += r.status == GCL_RDS_CLOSED;
		c[GCL_RDC_PEEKS] += r.status == GCL_RDS_DONE && (rd->flags & GCL_RD_PEEK);
		c[GCL_RDC_POPPED] += r.npop;
		c[GCL_RDC_PARTIAL] += (flags & GCL_RDO_PARTIAL) ? 1 : 0;
		c[GCL_RDC_RX_CLOSED] += (flags & GCL_RDO_RX_CLOSED) ? 1 : 0;
		c[GCL_RDC_ITEMS] += written;
		c[GCL_RDC_NOSPACE] += (flags & (GCL_RDO_SEG_NOSPACE | GCL_RDO_ITEM_NOSPACE)) ? 1 : 0;
	}
	c[GCL_RDC_BYTES] = bytes;
	out->totals[0] = items;
	out->totals[1] = items < in->item_cap ? items : in->item_cap;
	out->totals[2] = bytes;
	out->totals[3] = retsum;
	out->seg.totals[0] = segs;
	out->seg.totals[1] = segs < in->seg_cap ? segs : in->seg_cap;
	if (counts)
		for (int i = 0; i < GCL_RDC_NR; i++)
			counts[i] += c[i];
	return 0;
}

/* the mbuf tcp_tx_send works on, and c->tx_pending */
struct wr_mbuf {
	uint64_t frame_off;
	uint32_t seg_seq, fill;
	int live;
};

/* one connection's write as it runs */
struct wr_run {
	struct wr_mbuf pend;
	uint32_t snd_nxt, mss;
	uint32_t segs, items, slots, shorts, pushes;
};

/* tcp_tx_send (tcp_out.c:313-386) over @len bytes at @src for connection @c, whose segments, items and
 * slots start at @S, @I and @K of the call; with @emit it writes them */
static void wr_tx_send(const struct gcl_wr_in *in, const struct gcl_wr_out *out, int emit, struct wr_run *r,
                       uint32_t c, uint64_t S, uint64_t I, uint64_t K, uint64_t src, uint32_t len, int push)
{
	const struct gcl_tcp_conn *cn = &in->conn[c];
	uint32_t pos = 0;

	do {
		struct wr_mbuf m;
		uint32_t seglen;

		if (r->pend.live) { /* :331 */
			m = r->pend;
			r->pend.live = 0;
			seglen = len - pos < r->mss - m.fill ? len - pos : r->mss - m.fill;
		} else {
			seglen = len - pos < r->mss ? len - pos : r->mss;
			m.seg_seq = r->snd_nxt;
			m.fill = 0;
			m.frame_off = in->frame_base + (K + r->slots) * in->frame_stride;
			m.live = 1;
			r->slots++;
		}
		if (emit) { /* memcpy(mbuf_put(m, seglen), pos, seglen) */
			const uint64_t k = I + r->items;
			out->src_off[k] = src + pos;
			out->len[k] = (uint16_t)seglen;
			out->dst_off[k] = m.frame_off + GCL_WR_HDR + m.fill;
			out->item_conn[k] = c;
			out->item_seg[k] = (uint32_t)(S + r->segs);
		}
		r->items++;
		m.fill += seglen;
		r->snd_nxt += seglen;
		pos += seglen;
		if (!push && pos == len && (size_t)m.fill - GCL_WR_TCPHDR < r->mss) { /* :359: mbuf_length has no header yet */
			r->pend = m;
			break;
		}
		if (!push && pos == len)
			r->shorts++;
		if (emit) {
			const uint64_t k = S + r->segs;
			uint32_t a[4], d[16];

			memcpy(a, &in->addr[c], sizeof(a));
			gcl_wr_seg_words(a, in->wr[c].ecn, GCL_WR_TCP_ACK | (push && pos == len ? GCL_WR_TCP_PUSH : 0), m.seg_seq,
			                 cn->rcv_nxt, cn->rcv_wnd, m.fill, m.frame_off, in->now, d);
			memcpy(&out->desc[k], d, 32); /* little-endian host */
			memcpy(&out->txq_ent[k], d + 8, 16);
			memcpy(&out->txq_cold[k], d + 12, 16);
			out->frame_off[k] = m.frame_off;
			out->seg_conn[k] = c;
		}
		r->segs++;
		r->pushes += push && pos == len;
	} while (pos < len);
}

/* tcp_write3's or tcp_writev2's sends (tcp.c:1374, :1405-1416) for connection @c */
static void wr_run_conn(const struct gcl_wr_in *in, const struct gcl_wr_out *out, int emit, struct wr_run *r,
                        uint32_t c, uint64_t S, uint64_t I, uint64_t K, uint32_t v0, uint32_t nv, uint32_t winlen)
{
	const struct gcl_tcp_wr *wr = &in->wr[c];

	memset(r, 0, sizeof(*r));
	r->snd_nxt = in->conn[c].snd_nxt;
	r->mss = wr->snd_mss;
	if (wr->pend_len) {
		r->pend.live = 1;
		r->pend.fill = wr->pend_len;
		r->pend.seg_seq = r->snd_nxt - wr->pend_len;
		r->pend.frame_off = wr->pend_frame_off;
	}
	if (!(wr->flags & GCL_WR_VEC)) {
		wr_tx_send(in, out, emit, r, c, S, I, K, wr->src_off, wr->len < winlen ? wr->len : winlen, 1);
		return;
	}
	for (uint32_t i = 0; i < nv; i++) {
		const struct gcl_rd_iov *v = &in->iov[v0 + i];

		if (winlen == 0)
			break;
		if (!v->len)
			continue;
		const uint32_t x = v->len < winlen ? v->len : winlen;
		wr_tx_send(in, out, emit, r, c, S, I, K, v->off, x, i == nv - 1 && v->len <= winlen);
		winlen -= x;
	}
}

/* The rule of gcl_tcp_write (gclassify.h) on the CPU, one connection after the
 * other: the wait of gcl_tcpwrite.h, then the reference's loops, run once to
 * count and, when everything fits, once more to write. */
int gcl_tcp_write_host(const struct gcl_wr_in *in, const struct gcl_wr_out *out, uint64_t *counts)
{
	uint64_t cnt[GCL_WRC_NR] = {0}, S = 0, I = 0, K = 0, named = 0, tot[6] = {0};

	if (!in || !out || in->size != sizeof(*in) || in->nconn > GCL_WR_MAX_CONN || in->blocks > GCL_WR_MAX_BLOCKS ||
	    in->seg_cap > (1ull << 31) || in->item_cap > (1ull << 31) || in->frame_stride < GCL_WR_HDR ||
	    in->frame_stride > GCL_WR_MAX_STRIDE || !out->totals)
		return -EINVAL;
	const uint64_t nvec = in->voff ? in->nvec : 0;
	if (nvec > (1ull << 31))
		return -EINVAL;
	if (in->nconn && (!in->wr || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if (nvec && !in->iov)
		return -EINVAL;
	if (in->nconn && in->seg_cap && (!out->desc || !out->frame_off || !out->seg_conn || !out->txq_ent || !out->txq_cold))
		return -EINVAL;
	if (in->nconn && in->item_cap && (!out->src_off || !out->len || !out->dst_off || !out->item_conn || !out->item_seg))
		return -EINVAL;
	if (((uintptr_t)in->voff & 3) || ((uintptr_t)in->iov & 15) || ((uintptr_t)in->wr & 15) ||
	    ((uintptr_t)in->conn & 15) || ((uintptr_t)in->addr & 15) || ((uintptr_t)out->out_conn & 15) ||
	    ((uintptr_t)out->desc & 15) || ((uintptr_t)out->frame_off & 7) || ((uintptr_t)out->seg_conn & 3) ||
	    ((uintptr_t)out->txq_ent & 15) || ((uintptr_t)out->txq_cold & 15) || ((uintptr_t)out->src_off & 7) ||
	    ((uintptr_t)out->len & 1) || ((uintptr_t)out->dst_off & 7) || ((uintptr_t)out->item_conn & 3) ||
	    ((uintptr_t)out->item_seg & 3) || ((uintptr_t)out->totals & 7) || ((uintptr_t)counts & 7))
		return -EINVAL;
	const uint64_t slot_cap = gcl_wr_slot_cap(in->frames_len, in->frame_base, in->frame_stride);

	for (uint32_t c = 0; c < in->nconn; c++) {
		const struct gcl_tcp_wr *wr = &in->wr[c];
		const struct gcl_tcp_conn *cn = &in->conn[c];
		const uint32_t fseg = (uint32_t)(S < in->seg_cap ? S : in->seg_cap);
		const uint32_t fitem = (uint32_t)(I < in->item_cap ? I : in->item_cap);
		uint32_t w[12], o[12], v0 = 0, nv = 0, bad = 0;
		struct gcl_wr_res r;

		memcpy(w, wr, sizeof(w)); /* little-endian host */
		if (wr->flags & GCL_WR_VEC) {
			nv = gcl_wr_range(in->voff, c, nvec, &v0, &bad);
			if (named + nv > nvec) /* the rows the kernels' walk would take */
				bad = 1;
		}
		named += gcl_wr_named(w, in->voff, c, nvec);
		if (!gcl_wr_wait(w, bad, cn->snd_una, cn->snd_wnd, cn->snd_nxt, in->frame_stride, &r)) {
			gcl_wr_conn_words(r.ret, cn->snd_nxt, fseg, 0, fitem, 0, wr->pend_len, wr->pend_frame_off, r.status,
			                  r.flags, o);
		} else {
			struct wr_run run;

			wr_run_conn(in, out, 0, &run, c, S, I, K, v0, nv, r.winlen);
			if (gcl_wr_fits(S, run.segs, in->seg_cap, I, run.items, in->item_cap, K, run.slots, slot_cap)) {
				const uint32_t taken = run.snd_nxt - cn->snd_nxt;

				wr_run_conn(in, out, 1, &run, c, S, I, K, v0, nv, r.winlen);
				if (run.pend.live) /* the items of the segment that stays held */
					for (uint64_t k = I + run.items; k > I && out->item_seg[k - 1] == (uint32_t)(S + run.segs); k--)
						out->item_seg[k - 1] = GCL_WR_SEG_HELD;
				gcl_wr_conn_words(taken, run.snd_nxt, fseg, run.segs, fitem, run.items,
				                  run.pend.live ? run.pend.fill : 0, run.pend.live ? run.pend.frame_off : 0, GCL_WRS_DONE,
				                  gcl_wr_finish_flags(r.flags, run.segs, cn->rcv_nxt, wr->tx_last_ack, cn->snd_una,
				                                      cn->snd_wnd, run.snd_nxt), o);
				cnt[GCL_WRC_SEGS] += run.segs;
				cnt[GCL_WRC_PUSH] += run.pushes;
				cnt[GCL_WRC_HELD] += run.pend.live;
				cnt[GCL_WRC_SHORT] += run.shorts;
				cnt[GCL_WRC_ITEMS] += run.items;
				cnt[GCL_WRC_BYTES] += taken;
				tot[1] += run.segs;
				tot[3] += run.items;
				tot[4] += run.slots;
				tot[5] += taken;
			} else {
				r.status = GCL_WRS_NOSPACE;
				gcl_wr_conn_words(-GCL_WR_ENOBUFS, cn->snd_nxt, fseg, 0, fitem, 0, wr->pend_len, wr->pend_frame_off,
				                  r.status, 0, o);
			}
			S += run.segs;
			I += run.items;
			K += run.slots;
		}
		memcpy(&out->out_conn[c], o, sizeof(o));
		cnt[o[10] & 0xFFu]++;
	}
	tot[0] = S;
	tot[2] = I;
	memcpy(out->totals, tot, sizeof(tot));
	if (counts)
		for (int i = 0; i < GCL_WRC_NR; i++)
			counts[i] += cnt[i];
	return 0;
}

/* The rule of gcl_tcp_shut (gclassify.h) on the CPU: gcl_shut_rule of
 * gcl_tcpshut.h for every connection in turn, the count of wanted segments
 * running. */
int gcl_tcp_shut_host(const struct gcl_shut_in *in, const struct gcl_shut_out *out, uint64_t *counts)
{
	uint64_t cnt[GCL_SHUTC_NR] = {0}, W = 0;

	if (!in || !out || in->size != sizeof(*in) ||
	    ctl_refused(in->nconn, in->blocks, in->seg_cap, in->frame_stride, in->nconn, &out->seg, counts))
		return -EINVAL;
	if (in->nconn && (!in->shut || !in->tmr || !in->conn || !in->addr || !out->out_conn))
		return -EINVAL;
	if (in->nconn && in->seg_cap && (!out->txq_ent || !out->txq_cold))
		return -EINVAL;
	if (((uintptr_t)in->shut & 15) || ((uintptr_t)in->tmr & 15) || ((uintptr_t)in->conn & 15) ||
	    ((uintptr_t)in->addr & 15) || ((uintptr_t)out->out_conn & 15) || ((uintptr_t)out->txq_ent & 15) ||
	    ((uintptr_t)out->txq_cold & 15))
		return -EINVAL;
	const uint64_t cap = gcl_shut_cap(in->seg_cap, in->frames_len, in->frame_base, in->frame_stride);

	for (uint32_t c = 0; c < in->nconn; c++) {
		const struct gcl_tcp_conn *cn = &in->conn[c];
		struct gcl_shut_one t;
		struct gcl_shut_res r;
		uint32_t m[16], s[4], o[12], first = 0, nseg = 0;

		memcpy(m, &in->tmr[c], sizeof(m)); /* little-endian host */
		memcpy(s, &in->shut[c], sizeof(s));
		gcl_shut_load(m, s, cn->snd_nxt, &t);
		gcl_shut_rule(&t, in->now, &r);
		if (r.want != GCL_SHUT_WANT_NONE) {
			if (W >= cap) {
				gcl_shut_nospace(&t, &r);
			} else {
				const uint64_t off = in->frame_base + W * in->frame_stride;
				uint32_t a[4], d[16];

				memcpy(a, &in->addr[c], sizeof(a));
				gcl_shut_seg_words(a, r.want, cn->snd_nxt, cn->rcv_nxt, cn->rcv_wnd, off, in->now, d);
				memcpy(&out->seg.desc[W], d, 32);
				memcpy(&out->txq_ent[W], d + 8, 16);
				memcpy(&out->txq_cold[W], d + 12, 16);
				out->seg.frame_off[W] = off;
				out->seg.seg_conn[W] = c;
				out->seg.seg_src[W] = c;
				out->seg.seg_kind[W] = r.want == GCL_SHUT_WANT_FIN ? GCL_CTL_FIN : GCL_CTL_RST;
				first = (uint32_t)W;
				nseg = 1;
				cnt[r.want == GCL_SHUT_WANT_FIN ? GCL_SHUTC_FIN : GCL_SHUTC_RST]++;
			}
			W++;
		}
		gcl_shut_conn_words(&r, first, nseg, o);
		memcpy(&out->out_conn[c], o, sizeof(o));
		cnt[r.status]++;
		cnt[GCL_SHUTC_FAIL] += r.err != 0;
		cnt[GCL_SHUTC_PUT] += r.nput;
		cnt[GCL_SHUTC_WARN] += (r.flags & GCL_SHO_WARN) != 0;
	}
	out->seg.totals[0] = W;
	out->seg.totals[1] = W < cap ? W : cap;
	if (counts)
		for (int i = 0; i < GCL_SHUTC_NR; i++)
			counts[i] += cnt[i];
	return 0;
}

/* rx_send_to_runtime (rx.c:50-73) for the flow_tbl slot @slot of runtime @p
 * (hash % thread_count: every DELIVER or WAKE verdict carries it), or, when
 * @slot < 0, the slot of @hash.  The flow_tbl and the active count are read
 * here, at delivery time, like rx.c:55-72: a sched_add_core earlier in the
 * same batch that re-steered @p (or took its last core) is seen. */
static bool send_to_runtime(struct gcl_host_proc *p, uint32_t hash, int slot,
                            uint64_t cmd, unsigned long payload,
                            const struct gcl_host_ops *ops)
{
	int th;

	/* verdicts come from device memory: a flow_tbl slot outside the
	 * runtime's thread_count (a stale or corrupted verdict) is refused
	 * like a full ring, never used as an index */
	if (p->thread_count == 0 || p->thread_count > GCL_NCPU)
		return false;
	if (slot < 0)
		slot = (int)(hash % p->thread_count);
	else if (slot >= p->thread_count)
		return false;
	if (p->active_thread_count > 0) {
		th = p->flow_tbl[slot];
	} else {
		if (ops && ops->sched_add_core)
			ops->sched_add_core(ops->arg, p);
		if (p->active_thread_count == 0)
			th = p->idle_top;
		else
			th = p->flow_tbl[slot];
	}
	if (th < 0 || th >= p->thread_count || !p->rxq[th])
		return false;
	if (ops && ops->enable_poll)
		ops->enable_poll(ops->arg, p, (unsigned int)th);
	return gcl_lrpc_send(p->rxq[th], cmd, payload);
}

/* One packet of the post-pass, rx_one_pkt's exits after classification
 * (rx.c:171-233): the verdict's fields, the broadcast @hash, the ready
 * message {@cmd, @payload}, and the packet index @i the callbacks see.
 * Returns 1 when the packet was handed to a runtime. */
static uint64_t deliver_one(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                            struct gcl_host_proc *const *clients, int nr_clients,
                            uint16_t uniqid, uint8_t thread, uint8_t act, uint32_t hash,
                            uint64_t cmd, unsigned long payload,
                            const struct gcl_host_ops *ops, uint64_t i, uint64_t *stats)
{
	struct gcl_host_proc *p = NULL;

	if (act == GCL_ACT_DELIVER || act == GCL_ACT_WAKE) {
		if (uniqid < max_runtimes)
			p = clients_by_id[uniqid];
		if (p && send_to_runtime(p, hash, (int)thread, cmd, payload, ops)) {
			if (ops && ops->owned)
				ops->owned(ops->arg, p, i);
			return 1;
		}
		stats[GCL_RX_UNICAST_FAIL]++; /* rx.c:140-142, :213-215 */
	} else if (act == GCL_ACT_BROADCAST) {
		int n_sent = 0;
		for (int c = 0; c < nr_clients; c++) {
			if (send_to_runtime(clients[c], hash, -1, cmd, payload, ops)) {
				n_sent++;
				if (ops && ops->owned)
					ops->owned(ops->arg, clients[c], i);
			} else {
				stats[GCL_RX_BROADCAST_FAIL]++;
			}
		}
		if (n_sent == 0) {
			if (ops && ops->free_pkt)
				ops->free_pkt(ops->arg, i);
			return 0;
		}
		if (ops && ops->refcnt_update)
			ops->refcnt_update(ops->arg, i, n_sent - 1);
		return 1; /* rx.c:185-189: no RX_UNHANDLED */
	} else if (act == GCL_ACT_ARP_RESPOND) {
		if (ops && ops->arp_respond && ops->arp_respond(ops->arg, i))
			return 0;
		stats[GCL_RX_UNREGISTERED_MAC]++; /* rx.c:205 */
	} else {
		/* DROP_*: the device already counted them */
		if (ops && ops->free_pkt)
			ops->free_pkt(ops->arg, i);
		return 0;
	}
	/* fail_free, rx.c:225-232 */
	if (ops && ops->free_pkt)
		ops->free_pkt(ops->arg, i);
	stats[GCL_RX_UNHANDLED]++;
	return 0;
}

/* One verdict stream, either format: @v8 (gcl_verdict) or @v4 (gcl_verdict4,
 * whose broadcast hashes come from @bcast_hash).  Callbacks see packet
 * index @base + i. */
static uint64_t deliver(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                        struct gcl_host_proc *const *clients, int nr_clients,
                        const struct gcl_verdict *v8, const struct gcl_verdict4 *v4,
                        const uint32_t *bcast_hash, const uint16_t *pkt_len,
                        const uint8_t *olflags, uint8_t default_olflags,
                        const uint64_t *shmptr, uint64_t n,
                        const struct gcl_host_ops *ops, uint64_t base, uint64_t *stats)
{
	uint64_t delivered = 0;

	for (uint64_t i = 0; i < n; i++) {
		const uint16_t uniqid = v8 ? v8[i].uniqid : v4[i].uniqid;
		const uint8_t thread = v8 ? v8[i].thread : v4[i].thread;
		const uint8_t act = (v8 ? v8[i].action : v4[i].action) & GCL_ACT_MASK;
		const uint32_t hash = v8 ? v8[i].hash : (bcast_hash ? bcast_hash[i] : 0);
		uint8_t fl = olflags ? olflags[i] : default_olflags;

		delivered += deliver_one(clients_by_id, max_runtimes, clients, nr_clients, uniqid, thread,
		                         act, hash, gcl_rx_make_cmd(pkt_len ? pkt_len[i] : 0, fl),
		                         shmptr ? shmptr[i] : 0, ops, base + i, stats);
	}
	return delivered;
}

uint64_t gcl_host_deliver(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                          struct gcl_host_proc *const *clients, int nr_clients,
                          const struct gcl_verdict *v, const uint16_t *pkt_len,
                          const uint8_t *olflags, uint8_t default_olflags,
                          const uint64_t *shmptr, uint64_t n,
                          const struct gcl_host_ops *ops, uint64_t *stats)
{
	return deliver(clients_by_id, max_runtimes, clients, nr_clients, v, NULL, NULL, pkt_len,
	               olflags, default_olflags, shmptr, n, ops, 0, stats);
}

struct gcl_verdict4 gcl_verdict2_to4(uint16_t v, uint8_t thread_bits)
{
	struct gcl_verdict4 o;
	const uint16_t kind = v & GCL_V2_KIND, q = v & GCL_V2_Q_MASK;

	if (kind == GCL_V2_DELIVER || kind == GCL_V2_WAKE) {
		o.uniqid = (uint16_t)(q >> thread_bits);
		o.thread = (uint8_t)(q & ((1u << thread_bits) - 1));
		o.action = kind == GCL_V2_WAKE ? GCL_ACT_WAKE : GCL_ACT_DELIVER;
	} else {
		o.uniqid = GCL_NO_RUNTIME;
		o.thread = GCL_NO_THREAD;
		o.action = (uint8_t)(v & GCL_ACT_MASK);
	}
	return o;
}

struct gcl_verdict4 gcl_verdict1_to4(uint8_t v, uint8_t thread_bits)
{
	struct gcl_verdict4 o;

	if (!(v & GCL_V1_OTHER)) {
		o.uniqid = (uint16_t)((v & GCL_V1_Q_MASK) >> thread_bits);
		o.thread = (uint8_t)(v & ((1u << thread_bits) - 1));
		o.action = GCL_ACT_DELIVER;
	} else {
		o.uniqid = GCL_NO_RUNTIME;
		o.thread = GCL_NO_THREAD;
		o.action = (uint8_t)(v & GCL_ACT_MASK);
	}
	return o;
}

/* the packed records of a list (gcl_plan_pack), as deliver_compact takes them */
struct packed_recs {
	const uint64_t *cmd, *payload; /* [m], in list order */
	uint64_t n;                    /* packets in the batch */
};

/* deliver() for compact verdicts, with the common case inlined: a DELIVER
 * verdict for a runtime that still has an active kthread goes straight into
 * the ring of flow_tbl[slot] as it stands now (rx.c:55-59, then :76-92),
 * with the two per-delivery callbacks of the reference,
 * thread_enable_sched_poll and the ownership record.  Everything else (WAKE,
 * a runtime whose last core a scheduler side effect of this batch took,
 * broadcast, drops, a full ring) takes deliver_one() for that one packet, in
 * order, so the outcome is the same packet by packet.  A write prefetch of
 * the ring slot 8-32 packets ahead made it slower (profiles/archive/r01_deliver.txt).
 * Verdicts are @v2 (2-byte, of a context with @thread_bits), @v1 (1-byte) or
 * @v4; always inlined with constant NULLs for the two absent forms.  @idx,
 * when not NULL, lists the packets to take (gcl_host_deliver_idx): packet j
 * of the pass is idx[j], which indexes every per-packet array and is what
 * the callbacks see.  @pk, when not NULL, holds the list's packed records
 * (gcl_host_deliver_packed): verdict (@v4) and message of packet j of the
 * pass are read at position j, idx[j] only names the packet to the
 * callbacks and indexes @bcast_hash, and an idx[j] outside the batch is
 * skipped. */
static inline __attribute__((always_inline)) uint64_t
deliver_compact(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                struct gcl_host_proc *const *clients, int nr_clients,
                const struct gcl_verdict4 *v4, const uint16_t *v2, const uint8_t *v1,
                uint8_t thread_bits,
                const uint32_t *bcast_hash, const uint16_t *pkt_len, const uint8_t *olflags,
                uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                const struct gcl_host_ops *ops, uint64_t *stats, size_t vstride,
                const uint32_t *idx, const struct packed_recs *pk)
{
	const uint64_t csum_def = (default_olflags & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD;
	void (*const enable_poll)(void *, struct gcl_host_proc *, unsigned int) =
		ops ? ops->enable_poll : NULL;
	void (*const owned)(void *, struct gcl_host_proc *, uint64_t) = ops ? ops->owned : NULL;
	const uint32_t tmask = (1u << thread_bits) - 1;
	uint64_t delivered = 0;

	for (uint64_t j = 0; j < n; j++) {
		/* packet j of the pass: j itself, or the plan list's entry */
		const uint64_t i = idx ? idx[j] : j;
		struct gcl_host_proc *p;
		struct gcl_lrpc_chan_out *chan;
		uint32_t uniqid, slot, th;
		bool fast;

		if (pk && i >= pk->n)
			continue; /* names no packet: no callback, no counter */
		/* verdict i sits @vstride bytes after verdict i - 1: packed
		 * arrays, or the rx loop's 16-B records read in place; a list's
		 * packed records hold the verdict of idx[j] at j */
		const uint64_t vi = pk ? j : i;
		const uint16_t *v2i = v2 ? (const uint16_t *)((const char *)v2 + vi * vstride) : NULL;
		const uint8_t *v1i = v1 ? (const uint8_t *)v1 + vi * vstride : NULL;
		const struct gcl_verdict4 *v4i =
			v4 ? (const struct gcl_verdict4 *)((const char *)v4 + vi * vstride) : NULL;
		if (v1) { /* no WAKE mark: the active count below decides, as rx.c:59 */
			const uint8_t x = *v1i;
			uniqid = (x & GCL_V1_Q_MASK) >> thread_bits;
			slot = x & tmask;
			fast = !(x & GCL_V1_OTHER);
		} else if (v2) {
			const uint16_t x = *v2i;
			uniqid = (x & GCL_V2_Q_MASK) >> thread_bits;
			slot = x & tmask;
			fast = (x & GCL_V2_KIND) == GCL_V2_DELIVER;
		} else {
			const struct gcl_verdict4 x = *v4i;
			uniqid = x.uniqid;
			slot = x.thread;
			fast = (x.action & GCL_ACT_MASK) == GCL_ACT_DELIVER;
		}
		if (!fast || uniqid >= max_runtimes || !(p = clients_by_id[uniqid]) ||
		    slot >= p->thread_count || p->active_thread_count == 0 ||
		    (th = p->flow_tbl[slot]) >= p->thread_count || !(chan = p->rxq[th]) ||
		    chan->send_head - chan->send_tail >= chan->size) {
			const struct gcl_verdict4 w = v1 ? gcl_verdict1_to4(*v1i, thread_bits)
			                            : v2 ? gcl_verdict2_to4(*v2i, thread_bits) : *v4i;
			const uint64_t cmd = pk ? pk->cmd[j] :
				gcl_rx_make_cmd(pkt_len ? pkt_len[i] : 0, olflags ? olflags[i] : default_olflags);
			delivered += deliver_one(clients_by_id, max_runtimes, clients, nr_clients, w.uniqid,
			                         w.thread, w.action & GCL_ACT_MASK,
			                         bcast_hash ? bcast_hash[i] : 0, cmd,
			                         pk ? pk->payload[j] : shmptr ? shmptr[i] : 0, ops, i, stats);
			continue;
		}
		if (enable_poll)
			enable_poll(ops->arg, p, th);
		uint64_t cmd;
		if (pk) {
			cmd = pk->cmd[j];
		} else {
			const uint64_t csum = olflags ?
				(olflags[i] & GCL_F_IP_CKSUM_MASK) == GCL_F_IP_CKSUM_GOOD : csum_def;
			cmd = (uint64_t)(pkt_len ? pkt_len[i] : 0) << 16 | csum << 48;
		}
		const uint32_t h = chan->send_head++;
		struct gcl_lrpc_msg *dst = &chan->tbl[h & (chan->size - 1)];
		dst->payload = pk ? pk->payload[j] : shmptr ? shmptr[i] : 0;
		__atomic_store_n(&dst->cmd, cmd | ((h & chan->size) ? 0 : GCL_LRPC_DONE_PARITY),
		                 __ATOMIC_RELEASE);
		if (owned)
			owned(ops->arg, p, i);
		delivered++;
	}
	return delivered;
}

uint64_t gcl_host_deliver4(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                           struct gcl_host_proc *const *clients, int nr_clients,
                           const struct gcl_verdict4 *v, const uint32_t *bcast_hash,
                           const uint16_t *pkt_len, const uint8_t *olflags,
                           uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                           const struct gcl_host_ops *ops, uint64_t *stats)
{
	return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients, v, NULL, NULL, 0,
	                       bcast_hash, pkt_len, olflags, default_olflags, shmptr, n, ops, stats,
	                       sizeof(*v), NULL, NULL);
}

uint64_t gcl_host_deliver2(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                           struct gcl_host_proc *const *clients, int nr_clients,
                           const uint16_t *v, uint8_t thread_bits, const uint32_t *bcast_hash,
                           const uint16_t *pkt_len, const uint8_t *olflags,
                           uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                           const struct gcl_host_ops *ops, uint64_t *stats)
{
	if (thread_bits > 8 || !v)
		return 0;
	return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients, NULL, v, NULL,
	                       thread_bits, bcast_hash, pkt_len, olflags, default_olflags, shmptr,
	                       n, ops, stats, sizeof(*v), NULL, NULL);
}

uint64_t gcl_host_deliver1(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                           struct gcl_host_proc *const *clients, int nr_clients,
                           const uint8_t *v, uint8_t thread_bits, const uint32_t *bcast_hash,
                           const uint16_t *pkt_len, const uint8_t *olflags,
                           uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                           const struct gcl_host_ops *ops, uint64_t *stats)
{
	if (thread_bits > 7 || !v)
		return 0;
	return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients, NULL, NULL, v,
	                       thread_bits, bcast_hash, pkt_len, olflags, default_olflags, shmptr,
	                       n, ops, stats, sizeof(*v), NULL, NULL);
}

void gcl_host_prefetch_rxq(struct gcl_host_proc *const *clients, int nr_clients)
{
	for (int c = 0; c < nr_clients; c++) {
		const struct gcl_host_proc *p = clients[c];
		if (!p)
			continue;
		const unsigned int nt = p->thread_count <= GCL_NCPU ? p->thread_count : GCL_NCPU;
		for (unsigned int t = 0; t < nt; t++) {
			struct gcl_lrpc_chan_out *ch = p->rxq[t];
			if (!ch || !ch->tbl || !ch->size)
				continue;
			__builtin_prefetch(ch, 1, 3);
			__builtin_prefetch(&ch->tbl[ch->send_head & (ch->size - 1)], 1, 3);
		}
	}
}

uint64_t gcl_host_deliver_recs(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                               struct gcl_host_proc *const *clients, int nr_clients,
                               const struct gcl_loop_rec *recs, uint8_t vbytes,
                               uint8_t thread_bits, const uint32_t *bcast_hash,
                               const uint16_t *pkt_len, const uint8_t *olflags,
                               uint8_t default_olflags, const uint64_t *shmptr, uint64_t n,
                               const struct gcl_host_ops *ops, uint64_t *stats)
{
	uint64_t delivered = 0;

	if (!recs || thread_bits > 8)
		return 0;
	if (vbytes == 4)
		return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients,
		                       (const struct gcl_verdict4 *)&recs[0].verdict, NULL, NULL, 0,
		                       bcast_hash, pkt_len, olflags, default_olflags, shmptr, n, ops, stats,
		                       sizeof(*recs), NULL, NULL);
	if (vbytes == 2)
		return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients, NULL,
		                       (const uint16_t *)&recs[0].verdict, NULL, thread_bits, bcast_hash,
		                       pkt_len, olflags, default_olflags, shmptr, n, ops, stats,
		                       sizeof(*recs), NULL, NULL);
	if (vbytes == 1)
		return thread_bits > 7 ? 0
		                       : deliver_compact(clients_by_id, max_runtimes, clients, nr_clients,
		                                         NULL, NULL, (const uint8_t *)&recs[0].verdict,
		                                         thread_bits, bcast_hash, pkt_len, olflags,
		                                         default_olflags, shmptr, n, ops, stats,
		                                         sizeof(*recs), NULL, NULL);
	if (vbytes != 8)
		return 0;
	/* 8-byte contexts: a record's first 8 bytes are the struct gcl_verdict */
	for (uint64_t i = 0; i < n; i++) {
		struct gcl_verdict v;
		memcpy(&v, &recs[i], sizeof(v));
		delivered += deliver(clients_by_id, max_runtimes, clients, nr_clients, &v, NULL, NULL,
		                     pkt_len ? pkt_len + i : NULL, olflags ? olflags + i : NULL,
		                     default_olflags, shmptr ? shmptr + i : NULL, 1, ops, i, stats);
	}
	return delivered;
}

/* The post-pass over a delivery plan's list (gcl_plan): the packets
 * @idx[0..m) in list order, each through the same per-packet body as the
 * in-order passes above (deliver_compact, or deliver for 8-byte verdicts). */
uint64_t gcl_host_deliver_idx(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                              struct gcl_host_proc *const *clients, int nr_clients,
                              const void *v, uint8_t vbytes, uint8_t thread_bits,
                              const uint32_t *bcast_hash, const uint16_t *pkt_len,
                              const uint8_t *olflags, uint8_t default_olflags,
                              const uint64_t *shmptr, const uint32_t *idx, uint64_t m,
                              const struct gcl_host_ops *ops, uint64_t *stats)
{
	uint64_t delivered = 0;

	if (!v || !idx || thread_bits > 8)
		return 0;
	if (vbytes == 4)
		return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients, v, NULL, NULL, 0,
		                       bcast_hash, pkt_len, olflags, default_olflags, shmptr, m, ops, stats,
		                       sizeof(struct gcl_verdict4), idx, NULL);
	if (vbytes == 2)
		return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients, NULL, v, NULL,
		                       thread_bits, bcast_hash, pkt_len, olflags, default_olflags, shmptr,
		                       m, ops, stats, sizeof(uint16_t), idx, NULL);
	if (vbytes == 1)
		return thread_bits > 7 ? 0
		                       : deliver_compact(clients_by_id, max_runtimes, clients, nr_clients,
		                                         NULL, NULL, v, thread_bits, bcast_hash, pkt_len,
		                                         olflags, default_olflags, shmptr, m, ops, stats,
		                                         sizeof(uint8_t), idx, NULL);
	if (vbytes != 8)
		return 0;
	for (uint64_t j = 0; j < m; j++) {
		const uint64_t i = idx[j];
		delivered += deliver(clients_by_id, max_runtimes, clients, nr_clients,
		                     (const struct gcl_verdict *)v + i, NULL, NULL,
		                     pkt_len ? pkt_len + i : NULL, olflags ? olflags + i : NULL,
		                     default_olflags, shmptr ? shmptr + i : NULL, 1, ops, i, stats);
	}
	return delivered;
}

/* The post-pass over a list's packed records (gcl_plan_pack): deliver_compact
 * with the verdicts @v4 and the messages read at the list position. */
uint64_t gcl_host_deliver_packed(struct gcl_host_proc *const *clients_by_id, uint32_t max_runtimes,
                                 struct gcl_host_proc *const *clients, int nr_clients,
                                 const uint64_t *cmd, const uint64_t *payload,
                                 const struct gcl_verdict4 *v4, const uint32_t *idx,
                                 uint64_t m, uint64_t n, const uint32_t *bcast_hash,
                                 const struct gcl_host_ops *ops, uint64_t *stats)
{
	const struct packed_recs pk = { cmd, payload, n };

	if (!cmd || !payload || !v4 || !idx)
		return 0;
	return deliver_compact(clients_by_id, max_runtimes, clients, nr_clients, v4, NULL, NULL, 0,
	                       bcast_hash, NULL, NULL, 0, NULL, m, ops, stats, sizeof(*v4), idx, &pk);
}
