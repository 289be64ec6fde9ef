/*
 * ref_tcpin.c - test infrastructure (oracle/_ref only, never linked into the
 * product): the reference's own tcp_rx_conn, __tcp_rx_conn, is_acceptable,
 * tcp_rx_text and tcp_rx_append_text (runtime/net/tcp_in.c), compiled where
 * they lie, behind one driver that feeds a connection its segments and writes
 * down what the reference did with each.
 *
 * oracle/Makefile passes the reference file's path as REF_TCP_IN_C and this
 * file #includes it unmodified, against the reference's own headers.  After
 * --gc-sections the link asks for 24 symbols of the runtime; each is defined
 * here and either records that it was called or does nothing:
 *   tcp_conn_ack, tcp_tx_ack, tcp_timer_update (called only at done: in
 *     __tcp_rx_conn, so it marks that the slow path ran) and
 *     tcp_tx_fast_retransmit_start count their calls;
 *   tcp_conn_fail, tcp_conn_set_state, tcp_tx_raw_rst and tcp_tx_raw_rst_ack
 *     record their argument;
 *   thread_ready, preempt, sfree, tcp_tx_fast_retransmit_finish, tcp_tx_ctl and
 *     tcp_conn_alloc / _attach / _destroy / _release_ref (only tcp_rx_listener
 *     reaches those four, and the driver never calls it) do nothing;
 *   logk_bug aborts;
 *   ks, cycles_per_us and start_tsc are plain definitions;
 *   __perthread_preempt_cnt and __perthread_thread_id are plain definitions in
 *     section .perthread of this file, so that the %gs-relative accesses of
 *     spin_lock_np and STAT() resolve to them in a plain process.
 * Wakes are seen through c->poll_src.set_fn (POLLIN: the receive wake of
 * tcp_in.c:272-273 and :565-566; POLLOUT: the tx wake of :503) and frees
 * through m->release.  The driver applies no rule of the product: no stop, no
 * cap, no flag filter.  Asserts are as the reference's headers decide.
 */
#include <stdlib.h>

#include REF_TCP_IN_C

/* ---------------------------------------------------------------- what the link asks for */
struct ref_events {
	uint32_t slow, conn_ack, tx_ack, pollin, pollout, fastrtx, frees;
	uint32_t fail_err, new_state, rst_kind, rst_seq, rst_ack;
};
static struct ref_events ev;

struct kthread ks[NCPU];
int cycles_per_us = 1;
uint64_t start_tsc;
unsigned int __perthread_preempt_cnt __attribute__((section(".perthread")));
unsigned int __perthread_thread_id __attribute__((section(".perthread")));

void logk_bug(bool fatal, const char *expr, const char *file, int line, const char *func)
{
	abort();
}

void thread_ready(thread_t *thread) {}
void preempt(void) {}
void sfree(void *item) {}

void tcp_conn_ack(tcpconn_t *c, struct list_head *freeq) { ev.conn_ack++; }
int tcp_tx_ack(tcpconn_t *c) { ev.tx_ack++; return 0; }
void tcp_timer_update(tcpconn_t *c) { ev.slow++; }
struct mbuf *tcp_tx_fast_retransmit_start(tcpconn_t *c) { ev.fastrtx++; return NULL; }
void tcp_tx_fast_retransmit_finish(tcpconn_t *c, struct mbuf *m) {}
void tcp_conn_fail(tcpconn_t *c, int err) { ev.fail_err = (uint32_t)err; }
void tcp_conn_set_state(tcpconn_t *c, int new_state)
{
	ev.new_state = (uint32_t)new_state + 1;
	c->pcb.state = new_state;
}
int tcp_tx_raw_rst(struct netaddr laddr, struct netaddr raddr, tcp_seq seq)
{
	ev.rst_kind = 1;
	ev.rst_seq = seq;
	return 0;
}
int tcp_tx_raw_rst_ack(struct netaddr laddr, struct netaddr raddr, tcp_seq seq, tcp_seq ack)
{
	ev.rst_kind = 2;
	ev.rst_seq = seq;
	ev.rst_ack = ack;
	return 0;
}
int tcp_tx_ctl(tcpconn_t *c, uint8_t flags, const struct tcp_options *opts) { return 0; }
tcpconn_t *tcp_conn_alloc(void) { return NULL; }
int tcp_conn_attach(tcpconn_t *c, struct netaddr laddr, struct netaddr raddr, bind_token_t *token) { return 0; }
void tcp_conn_destroy(tcpconn_t *c) {}
void tcp_conn_release_ref(struct kref *r) {}

/* ---------------------------------------------------------------- the driver */
#define REF_EXPORT __attribute__((visibility("default")))

/* one mbuf of the driver: the reference's, and where it came from */
struct ref_mbuf {
	struct mbuf m;
	unsigned char *text;   /* m.data when the text began: behind the TCP header and options */
	int32_t id;            /* segment k: k; input queue entry i: -1 - i; the dummy of rxq: INT32_MIN */
	uint32_t freed;
};

static int32_t *freed_out;
static uint32_t freed_cap, freed_n;

static void ref_release(struct mbuf *m)
{
	struct ref_mbuf *r = container_of(m, struct ref_mbuf, m);

	ev.frees++;
	r->freed++;
	if (freed_n < freed_cap)
		freed_out[freed_n] = r->id;
	freed_n++;
}

static void ref_poll_set(unsigned long pdata, unsigned int event_mask)
{
	if (event_mask & POLLIN)
		ev.pollin++;
	if (event_mask & POLLOUT)
		ev.pollout++;
}

/* the u32 words of @conn */
enum { RC_SND_UNA, RC_SND_NXT, RC_SND_WND, RC_SND_WL1, RC_SND_WL2, RC_RCV_NXT, RC_RCV_WND, RC_RCV_MSS,
       RC_SND_WSCALE, RC_ACKS_DELAYED_CNT, RC_ACK_DELAYED, RC_REP_ACKS, RC_STATE, RC_RXQ, RC_NR };
/* the u32 words of one trace record */
enum { RT_PRE_RCV_NXT, RT_PRE_RCV_WND, RT_PRE_OOO_LEN,
       RT_SND_UNA, RT_SND_WND, RT_SND_WL1, RT_SND_WL2, RT_RCV_NXT, RT_RCV_WND, RT_ACKS_DELAYED_CNT,
       RT_ACK_DELAYED, RT_REP_ACKS, RT_STATE, RT_OOO_LEN, RT_ACK_TS,
       RT_SLOW, RT_CONN_ACK, RT_TX_ACK, RT_POLLIN, RT_POLLOUT, RT_FASTRTX, RT_FREES,
       RT_FAIL_ERR, RT_NEW_STATE, RT_RST_KIND, RT_RST_SEQ, RT_RST_ACK,
       RT_FREED_AT, RT_FREED_N, RT_LINKED_AT, RT_LINKED_N, RT_Q_AT, RT_Q_N, RT_NR };

#define REF_ACK_TS_UNSET UINT64_MAX

REF_EXPORT uint32_t ref_tcpin_conn_words(void) { return RC_NR; }
REF_EXPORT uint32_t ref_tcpin_trace_words(void) { return RT_NR; }

/*
 * One tcpconn_t with the PCB words @conn (tx_exclusive = 0), an rxq that holds
 * a dummy mbuf when conn[RC_RXQ], and an rxq_ooo of the @nq entries @q (seq,
 * end, flags each; no bytes behind them: m.len is end - seq, at most 65535).
 * Frame k is the @len[k] bytes at @base + @ip_off[k], an IPv4 header first;
 * its mbuf has the network offset marked there and data at the TCP header.
 * tcp_rx_conn(&c.e, m) runs once per frame, in order, and trace record k
 * (RT_NR words at @trace) says what it did; the ids of the mbufs it freed go
 * to @freed from record k's RT_FREED_AT on, RT_FREED_N of them, and the mbufs
 * newly linked at the tail of c->rxq to @linked as (id, bytes pulled from the
 * front of the text, length) from RT_LINKED_AT on, and the ids of rxq_ooo as it
 * stands after the call, in list order, to @qsnap from RT_Q_AT on, RT_Q_N of
 * them.  After the last frame @qfinal gets rxq_ooo as (seq, end, id) in list
 * order, at most @qfinal_cap entries.  Returns the length of that list, or -1
 * when out of memory or when @freed (capacity @freed_cap_), @linked
 * (@linked_cap triples) or @qsnap (@qsnap_cap) is too small.
 */
REF_EXPORT int64_t ref_tcpin_run(const uint32_t *conn, const uint32_t *q, uint32_t nq, const uint8_t *base,
                                 const uint64_t *ip_off, const uint32_t *len, uint32_t n, uint32_t *trace,
                                 int32_t *freed, uint32_t freed_cap_, int32_t *linked, uint32_t linked_cap,
                                 int32_t *qsnap, uint32_t qsnap_cap, uint32_t *qfinal, uint32_t qfinal_cap)
{
	static unsigned char nothing[65536];
	struct ref_mbuf *mb, dummy;
	struct mbuf *pos;
	tcpconn_t c;
	uint32_t k, linked_n = 0, qsnap_n = 0, rxq_len = 0, at;
	int64_t ret;

	mb = calloc((size_t)nq + n + 1, sizeof(*mb));
	if (!mb)
		return -1;
	memset(&c, 0, sizeof(c));
	memset(&dummy, 0, sizeof(dummy));
	c.pcb.state = (int)conn[RC_STATE];
	c.pcb.snd_una = conn[RC_SND_UNA];
	c.pcb.snd_nxt = conn[RC_SND_NXT];
	c.pcb.snd_wnd = conn[RC_SND_WND];
	c.pcb.snd_wl1 = conn[RC_SND_WL1];
	c.pcb.snd_wl2 = conn[RC_SND_WL2];
	c.pcb.rcv_nxt = conn[RC_RCV_NXT];
	c.pcb.rcv_wnd = conn[RC_RCV_WND];
	c.pcb.rcv_mss = conn[RC_RCV_MSS];
	c.pcb.snd_wscale = conn[RC_SND_WSCALE];
	c.acks_delayed_cnt = (int)conn[RC_ACKS_DELAYED_CNT];
	c.ack_delayed = conn[RC_ACK_DELAYED] != 0;
	c.rep_acks = (int)conn[RC_REP_ACKS];
	c.tx_exclusive = false;
	c.next_timeout = UINT64_MAX;
	spin_lock_init(&c.lock);
	c.poll_src.set_fn = ref_poll_set;
	waitq_init(&c.rx_wq);
	waitq_init(&c.tx_wq);
	list_head_init(&c.rxq_ooo);
	list_head_init(&c.rxq);
	list_head_init(&c.txq);
	if (conn[RC_RXQ]) {
		dummy.id = INT32_MIN;
		dummy.m.release = ref_release;
		list_add_tail(&c.rxq, &dummy.m.link);
		rxq_len = 1;
	}
	for (k = 0; k < nq; k++) {
		struct ref_mbuf *r = &mb[k];
		uint32_t l = q[3 * k + 1] - q[3 * k];

		r->id = -1 - (int32_t)k;
		r->m.head = r->m.data = r->text = nothing;
		r->m.head_len = 65535;
		r->m.len = l > 65535 ? 65535 : l;
		r->m.seg_seq = q[3 * k];
		r->m.seg_end = q[3 * k + 1];
		r->m.flags = (uint8_t)q[3 * k + 2];
		r->m.release = ref_release;
		list_add_tail(&c.rxq_ooo, &r->m.link);
		c.rxq_ooo_len++;
	}
	freed_out = freed;
	freed_cap = freed_cap_;
	freed_n = 0;
	for (k = 0; k < n; k++) {
		struct ref_mbuf *r = &mb[nq + k];
		uint32_t *t = trace + (size_t)k * RT_NR;
		const struct ip_hdr *ip = (const struct ip_hdr *)(base + ip_off[k]);
		const struct tcp_hdr *tcp = (const struct tcp_hdr *)(ip + 1);

		r->id = (int32_t)k;
		r->m.head = (unsigned char *)(uintptr_t)ip;
		r->m.head_len = len[k] > 65535 ? 65535 : len[k];
		r->m.data = r->m.head;
		r->m.len = r->m.head_len;
		r->m.release = ref_release;
		mbuf_mark_network_offset(&r->m);
		mbuf_pull(&r->m, sizeof(*ip));
		/* where the text begins once tcp_rx_conn has pulled the header and the options */
		r->text = r->m.data + (len[k] >= sizeof(*ip) + sizeof(*tcp) ? tcp->off * 4 : 0);

		memset(&ev, 0, sizeof(ev));
		memset(t, 0, RT_NR * sizeof(*t));
		t[RT_PRE_RCV_NXT] = c.pcb.rcv_nxt;
		t[RT_PRE_RCV_WND] = c.pcb.rcv_wnd;
		t[RT_PRE_OOO_LEN] = c.rxq_ooo_len;
		t[RT_FREED_AT] = freed_n;
		t[RT_LINKED_AT] = linked_n;
		c.ack_ts = REF_ACK_TS_UNSET;

		tcp_rx_conn(&c.e, &r->m);

		t[RT_SND_UNA] = c.pcb.snd_una;
		t[RT_SND_WND] = c.pcb.snd_wnd;
		t[RT_SND_WL1] = c.pcb.snd_wl1;
		t[RT_SND_WL2] = c.pcb.snd_wl2;
		t[RT_RCV_NXT] = c.pcb.rcv_nxt;
		t[RT_RCV_WND] = c.pcb.rcv_wnd;
		t[RT_ACKS_DELAYED_CNT] = (uint32_t)c.acks_delayed_cnt;
		t[RT_ACK_DELAYED] = c.ack_delayed;
		t[RT_REP_ACKS] = (uint32_t)c.rep_acks;
		t[RT_STATE] = (uint32_t)c.pcb.state;
		t[RT_OOO_LEN] = c.rxq_ooo_len;
		t[RT_ACK_TS] = c.ack_ts != REF_ACK_TS_UNSET;
		t[RT_SLOW] = ev.slow;
		t[RT_CONN_ACK] = ev.conn_ack;
		t[RT_TX_ACK] = ev.tx_ack;
		t[RT_POLLIN] = ev.pollin;
		t[RT_POLLOUT] = ev.pollout;
		t[RT_FASTRTX] = ev.fastrtx;
		t[RT_FREES] = ev.frees;
		t[RT_FAIL_ERR] = ev.fail_err;
		t[RT_NEW_STATE] = ev.new_state;
		t[RT_RST_KIND] = ev.rst_kind;
		t[RT_RST_SEQ] = ev.rst_seq;
		t[RT_RST_ACK] = ev.rst_ack;
		t[RT_FREED_N] = freed_n - t[RT_FREED_AT];
		at = 0;
		list_for_each(&c.rxq, pos, link) {
			struct ref_mbuf *p = container_of(pos, struct ref_mbuf, m);

			if (at++ < rxq_len)
				continue;
			if (linked_n < linked_cap) {
				linked[3 * linked_n] = p->id;
				linked[3 * linked_n + 1] = (int32_t)(p->m.data - p->text);
				linked[3 * linked_n + 2] = p->m.len;
			}
			linked_n++;
		}
		rxq_len = at;
		t[RT_LINKED_N] = linked_n - t[RT_LINKED_AT];
		t[RT_Q_AT] = qsnap_n;
		list_for_each(&c.rxq_ooo, pos, link) {
			if (qsnap_n < qsnap_cap)
				qsnap[qsnap_n] = container_of(pos, struct ref_mbuf, m)->id;
			qsnap_n++;
		}
		t[RT_Q_N] = qsnap_n - t[RT_Q_AT];
	}
	ret = 0;
	list_for_each(&c.rxq_ooo, pos, link) {
		if (ret < qfinal_cap) {
			qfinal[3 * ret] = pos->seg_seq;
			qfinal[3 * ret + 1] = pos->seg_end;
			qfinal[3 * ret + 2] = (uint32_t)container_of(pos, struct ref_mbuf, m)->id;
		}
		ret++;
	}
	if (freed_n > freed_cap || linked_n > linked_cap || qsnap_n > qsnap_cap)
		ret = -1;
	free(mb);
	return ret;
}
