"""Python binding of libgclassify.so (ctypes), for tests and bench.py.

The product boundary is the C ABI in include/gclassify.h; the dataplane side
that consumes verdicts is C (include/gcl_host.h).  This module is a thin
mirror of that ABI with the reference's names and error behaviour: every call
that returns -errno raises OSError(errno) here, the way the reference's init
paths fail (rx_init, dp_clients_init return -1/-errno).

There is no CPU fallback: if the shared library is missing, importing the
binding raises, and classify() needs device (HBM) buffers.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libgclassify.so")

GCL_MAX_PROC = 4096
GCL_NCPU = 256
GCL_RX_BURST_SIZE = 64

HASH_NIC, HASH_JENKINS, HASH_TOEPLITZ = 0, 1, 2
HASH_MODES = {"nic": HASH_NIC, "jenkins": HASH_JENKINS, "toeplitz": HASH_TOEPLITZ}

CFG_AZURE_ARP, CFG_HASH16, CFG_PROFILE, CFG_TRANS_HASH, CFG_VERDICT4 = 0x1, 0x2, 0x4, 0x8, 0x10
CFG_VERDICT2, CFG_VERDICT1 = 0x20, 0x40
# GCL_CFG_VERDICT2: u16 q = uniqid << thread_bits | flow_tbl slot; kind in the top two bits
V2_Q_MASK, V2_KIND, V2_DELIVER, V2_WAKE, V2_OTHER, V2_QUEUES = 0x3FFF, 0xC000, 0, 0x4000, 0xC000, 0x4000
# GCL_CFG_VERDICT1: u8 q (DELIVER or WAKE, unmarked) or V1_OTHER | action
V1_Q_MASK, V1_OTHER, V1_QUEUES = 0x7F, 0x80, 0x80
PAIR_NEW_READS, PAIR_NEW_WRITES, PAIR_TRIES, PAIR_RUN = 0x1, 0x2, 24, 2
PAIR_QUIET, PAIR_VERBOSE = 0x10000, 0x20000
PROBE_MIN = 0x100  # gcl_access_probe: the layout's minimal-request probe

F_RSS_HASH, F_FDIR_ID = 0x01, 0x02
F_IP_CKSUM_MASK, F_IP_CKSUM_UNKNOWN, F_IP_CKSUM_BAD = 0x0C, 0x00, 0x04
F_IP_CKSUM_GOOD, F_IP_CKSUM_NONE = 0x08, 0x0C

ACT_DELIVER, ACT_WAKE, ACT_DROP_ETHERTYPE, ACT_DROP_UNREG = 0, 1, 2, 3
ACT_BROADCAST, ACT_ARP_RESPOND = 4, 5
ACT_MASK, ACT_F_FDIR, ACT_F_TRANS = 0x3F, 0x80, 0x40
NO_RUNTIME, NO_THREAD = 0xFFFF, 0xFF

(RX_UNREGISTERED_MAC, RX_UNICAST_FAIL, RX_BROADCAST_FAIL, RX_FLOW_TAG_MATCH,
 RX_UNHANDLED, RX_HASH_MISSING, RX_PULLED) = range(7)
NR_STATS = 8
# gcl_rx_csum's counter slots
CSUM_CHECKED, CSUM_GOOD, CSUM_BAD, CSUM_SKIPPED, CSUM_NR = 0, 1, 2, 3, 4
# its launch (csrc/gcl_csum.hip): packets a block takes per pass, and the grid's cap
CSUM_BLOCK_PKTS, CSUM_BLOCKS_PER_CU = 256, 7
# gcl_copy_batch's counter slots
COPY_COPIED, COPY_REFUSED, COPY_BYTES, COPY_NR = 0, 1, 2, 4
# its launch (csrc/gcl_copy.hip): lanes per block, and the grid's cap
COPY_THREADS, COPY_BLOCKS_PER_CU = 256, 6
# gcl_l4_csum: modes, the status byte, the counter slots
L4_VERIFY, L4_FILL = 0, 1
L4_NA, L4_GOOD, L4_BAD, L4_NONE, L4_FILLED_IP, L4_FILLED_L4 = 0, 1, 2, 3, 0x10, 0x20
(L4C_GOOD, L4C_BAD, L4C_NONE, L4C_NA, L4C_FILLED_IP, L4C_FILLED_L4, L4C_BYTES) = range(7)
L4C_NR = 8
# its launch (csrc/gcl_l4.hip): lanes per block, and the grid's cap
L4_THREADS, L4_BLOCKS_PER_CU = 256, 7
# gcl_l4_payload: the kind byte, the counter slots, the cap on blocks, struct gcl_pay_meta
PAY_NA, PAY_UDP, PAY_TCP, PAY_NOSOCK, PAY_BADCSUM, PAY_OOR = range(6)
(PAYC_UDP, PAYC_TCP, PAYC_NA, PAYC_NOSOCK, PAYC_BADCSUM, PAYC_OOR, PAYC_BYTES) = range(7)
PAYC_NR, PAY_MAX_BLOCKS = 8, 1024
# its launches (csrc/gcl_payload.hip): entries per tile, and the library's ranges per CU
PAY_TILE, PAY_BLOCKS_PER_CU = 256, 4
PAY_META_DTYPE = np.dtype([("rip", "<u4"), ("rport", "<u2"), ("proto", "u1"), ("tcp_flags", "u1"),
                           ("seq", "<u4"), ("ack", "<u4")])
# gcl_sock_lookup: entry kinds, the answers that are not cookies, the counter slots
SOCK_MATCH_3TUPLE, SOCK_MATCH_5TUPLE, SOCK_MAX_ENTRIES = 3, 5, 1 << 20
SOCK_NA, SOCK_MISS, SOCK_MULTI, SOCK_COOKIE_MAX = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFEF
SOCK_HIT5, SOCK_HIT3, SOCK_HIT3_ANY, SOCK_N_MULTI, SOCK_N_MISS, SOCK_N_NA, SOCK_NR = 0, 1, 2, 3, 4, 5, 8
# its launch (csrc/gcl_sock.hip): packets a block takes per pass, and the grid's cap
SOCK_BLOCK_PKTS, SOCK_BLOCKS_PER_CU = 256, 4
# struct gcl_sock_entry as a numpy record
SOCK_ENTRY_DTYPE = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"),
                             ("proto", "u1"), ("match", "u1"), ("pad", "<u2"), ("cookie", "<u4")])
# gcl_tx_hdr: the status byte, the counter slots, gcl_txh_net.flags, the txpkt olflags it writes
TXH_OK, TXH_SELF, TXH_NONEIGH, TXH_REFUSED = range(4)
(TXHC_OK, TXHC_SELF, TXHC_NONEIGH, TXHC_REFUSED, TXHC_LOCAL, TXHC_BYTES) = range(6)
TXHC_NR, TXH_IP_CSUM, NEIGH_MAX_ENTRIES = 8, 0x01, 1 << 16
OLFLAG_IP_CHKSUM, OLFLAG_TCP_CHKSUM, OLFLAG_IPV4, TXFLAG_LOCAL, TXFLAG_LOCAL_HINT = 0x01, 0x02, 0x04, 0x10, 0x40
# its launch (csrc/gcl_txhdr.hip): entries a block takes per pass, and the grid's cap
TXH_BLOCK_PKTS, TXH_BLOCKS_PER_CU = 256, 4
# struct gcl_txh_desc and struct gcl_neigh_entry as numpy records
TXH_DESC_DTYPE = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"),
                           ("proto", "u1"), ("tcp_flags", "u1"), ("tcp_off", "u1"), ("ecn", "u1"),
                           ("seq", "<u4"), ("ack", "<u4"), ("win", "<u2"), ("paylen", "<u2"),
                           ("pad", "<u4")])
NEIGH_ENTRY_DTYPE = np.dtype([("ip", "<u4"), ("mac", "u1", (6,)), ("pad", "<u2")])
# gcl_tx_seg: the status byte, the counter slots, the cap on blocks, struct gcl_seg_send
SEG_OK, SEG_REFUSED, SEG_NOSPACE = range(3)
(SEGC_OK, SEGC_REFUSED, SEGC_NOSPACE, SEGC_SEGS, SEGC_BYTES, SEGC_PUSH) = range(6)
SEGC_NR, SEG_MAX_BLOCKS = 8, 1024
# its launches (csrc/gcl_seg.hip): writes or segments per tile
SEG_TILE = 256
SEG_SEND_DTYPE = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"),
                           ("proto", "u1"), ("ecn", "u1"), ("mss", "<u2"), ("snd_nxt", "<u4"),
                           ("ack", "<u4"), ("win", "<u2"), ("pad", "<u2"), ("len", "<u4"),
                           ("winlen", "<u4"), ("pad2", "<u4"), ("src_off", "<u8")])
# gcl_tcp_rx: the verdict byte (also the first counter slots), the counters, sflags, the connection
# flags, the caps, struct gcl_tcp_conn and struct gcl_tcp_conn_out
TCPRX_FAST, TCPRX_SLOW, TCPRX_DROP, TCPRX_NOCONN, TCPRX_NA = range(5)
TCPRXC_BYTES, TCPRXC_ACKS, TCPRXC_WAKES, TCPRXC_NR = 5, 6, 7, 8
TCPRX_SF_WAKE, TCPRX_SF_ACK_NOW, TCPRX_SF_ACKED, TCPRX_SF_WND = 0x01, 0x02, 0x04, 0x08
TCPC_ELIGIBLE, TCPC_RXQ, TCPC_ACK_DELAYED = 0x01, 0x02, 0x04
TCPO_STOPPED, TCPO_WOKEN, TCPO_TIMER_ARMED, TCPO_REP_ACKS_RESET = 0x08, 0x10, 0x20, 0x40
TCPRX_MAX_BLOCKS, TCPRX_MAX_CONN, TCPRX_NONE = 1024, 1 << 20, 0xFFFFFFFF
# its grouping (csrc/gcl_tcprx.hip): the connections one counting-sort pass serves
TCPRX_PASS_CONN = 2048
TCP_CONN_DTYPE = np.dtype([("snd_una", "<u4"), ("snd_nxt", "<u4"), ("snd_wnd", "<u4"), ("snd_wl1", "<u4"),
                           ("snd_wl2", "<u4"), ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("rcv_mss", "<u2"),
                           ("snd_wscale", "u1"), ("flags", "u1"), ("acks_delayed_cnt", "u1"),
                           ("pad", "u1", (15,))])
TCP_CONN_OUT_DTYPE = np.dtype([("snd_una", "<u4"), ("snd_wnd", "<u4"), ("snd_wl1", "<u4"), ("snd_wl2", "<u4"),
                               ("rcv_nxt", "<u4"), ("rcv_wnd", "<u4"), ("nfast", "<u4"), ("nslow", "<u4"),
                               ("nacks", "<u4"), ("first_slow", "<u4"), ("acks_delayed_cnt", "u1"),
                               ("flags", "u1"), ("pad", "u1", (6,))])
# gcl_tcp_rx_full: the sflags it adds, gcl_tcp_conn_ext.xflags, the counters behind gcl_tcp_rx's
# eight and struct gcl_tcp_conn_ext
TCPRX_SF_RULE2, TCPRX_SF_TXWAKE, TCPRX_SF_FASTRTX, TCPRX_SF_DROPPED = 0x10, 0x20, 0x40, 0x80
TCPX_TXWAKE, TCPX_FASTRTX = 0x01, 0x02
TCPRXFC_RULE2, TCPRXFC_TXWAKES, TCPRXFC_FASTRTX, TCPRXFC_DUPACKS, TCPRXFC_DROPPED, TCPRXFC_NR = 8, 9, 10, 11, 12, 13
TCP_CONN_EXT_DTYPE = np.dtype([("nrule2", "<u4"), ("ndropped", "<u4"), ("fast_rtx_ack", "<u4"),
                               ("rep_acks", "u1"), ("xflags", "u1"), ("pad", "u1", (2,))])
# gcl_tcp_rx_ooo: the queue cap, the flag bits it adds, oflags, qin_state, the counters behind
# gcl_tcp_rx_full's thirteen and struct gcl_tcp_ooo_ent
TCPOOO_CAP, TCPC_ESTABLISHED, TCPX_QSKIP = 64, 0x80, 0x04
OOOF_OOO, OOOF_QUEUED, OOOF_HEADCLIP, OOOF_LATE_DRAINED, OOOF_LATE_FREED, OOOF_HELD = 1, 2, 4, 8, 0x10, 0x20
OOOQ_UNTOUCHED, OOOQ_KEPT, OOOQ_FREED, OOOQ_DRAINED = 0, 1, 2, 3
(TCPRXOC_OOO, TCPRXOC_QUEUED, TCPRXOC_DRAINED, TCPRXOC_FREED, TCPRXOC_HEADCLIP, TCPRXOC_HELD,
 TCPRXOC_NR) = 13, 14, 15, 16, 17, 18, 19
TCP_OOO_ENT_DTYPE = np.dtype([("seq", "<u4"), ("end", "<u4"), ("ref", "<u4"), ("flags", "<u2"), ("src", "<u2")])
# gcl_tcp_rx_states: enum tcp state, ev[j], the xflags it adds and the counters behind gcl_tcp_rx_ooo's nineteen
(TCP_STATE_SYN_SENT, TCP_STATE_SYN_RECEIVED, TCP_STATE_ESTABLISHED, TCP_STATE_FIN_WAIT1, TCP_STATE_FIN_WAIT2,
 TCP_STATE_CLOSE_WAIT, TCP_STATE_CLOSING, TCP_STATE_LAST_ACK, TCP_STATE_TIME_WAIT, TCP_STATE_CLOSED) = range(10)
TCPS_NOSTATE = 0xFF
TCPS_RST, TCPS_RST_ACK, TCPS_FAIL, TCPS_STATE, TCPS_FIN, TCPS_PUT = 1, 2, 4, 8, 0x10, 0x20
TCPX_FAILED, TCPX_PUT, TCPX_TIMEWAIT, TCPX_OPENED = 0x08, 0x10, 0x20, 0x40
CTL_RST, CTL_RST_ACK = 2, 3      # seg_kind of gcl_tcp_rx_ctl beside CTL_ACK and CTL_PROBE
TCPRXSC_RSTS, TCPRXSC_FAILS, TCPRXSC_FINS, TCPRXSC_STATE_CHANGES, TCPRXSC_NR = 19, 20, 21, 22, 23
# gcl_tcp_tick / gcl_tcp_rx_acks: the timer flags, the action bits (bits 0..6 are also the first
# counter slots), the segment kinds, the counters, the caps, the TCP states the sweep tests,
# struct gcl_tcp_tmr, struct gcl_tcp_tmr_out and struct gcl_tcp_addr
TMR_LIVE, TMR_ACK_DELAYED, TMR_ZERO_WND, TMR_TX_EXCLUSIVE, TMR_TXQ, TMR_OOO = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
(TMRA_FIRED, TMRA_ACK, TMRA_PROBE, TMRA_RETRANSMIT, TMRA_FAIL, TMRA_CLOSE,
 TMRA_NOSPACE) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
CTL_ACK, CTL_PROBE, CTL_MIN_STRIDE = 0, 1, 54
(TICKC_FIRED, TICKC_ACK, TICKC_PROBE, TICKC_RETRANSMIT, TICKC_FAIL, TICKC_CLOSE, TICKC_NOSPACE,
 TICKC_SEGS) = range(8)
TICKC_NR, TICK_MAX_BLOCKS, TICK_MAX_CONN = 8, 1024, 1 << 20
RXACKC_WANTED, RXACKC_WRITTEN, RXACKC_SKIPPED = range(3)
TCP_STATE_ESTABLISHED, TCP_STATE_TIME_WAIT, TCP_STATE_CLOSED = 2, 8, 9
# its launches (csrc/gcl_tcptmr.hip): connections or list entries per tile
TICK_TILE = 256
TCP_TMR_DTYPE = np.dtype([("next_timeout", "<u8"), ("attach_ts", "<u8"), ("time_wait_ts", "<u8"),
                          ("ack_ts", "<u8"), ("zero_wnd_ts", "<u8"), ("txq_ts", "<u8"), ("state", "u1"),
                          ("flags", "u1"), ("pad", "u1", (14,))])
TCP_TMR_OUT_DTYPE = np.dtype([("next_timeout", "<u8"), ("zero_wnd_ts", "<u8"), ("state", "u1"), ("flags", "u1"),
                              ("action", "u1"), ("pad", "u1", (13,))])
TCP_ADDR_DTYPE = np.dtype([("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"), ("rport", "<u2"),
                           ("rcv_wscale", "u1"), ("pad", "u1", (3,))])
# gcl_tcp_rx_open: the verdicts (also their counter slots), the counters behind them, the caps, the
# new segment kind, the listener flag, the option bits, struct gcl_tcp_listen and struct gcl_tcp_open
(OPEN_NA, OPEN_OOR, OPEN_SHORT, OPEN_CLOSED_DROP, OPEN_CLOSED_RST, OPEN_CLOSED_RST_ACK, OPEN_LATER, OPEN_FULL,
 OPEN_DROP, OPEN_RST, OPEN_BADOPT, OPEN_ACCEPT) = range(12)
OPEN_NR_VERDICTS = 12
OPENC_SEGS, OPENC_SEGSKIP, OPENC_NOSPACE, OPENC_NR = 12, 13, 14, 16
OPEN_MAX_LISTEN, OPEN_MAX_BLOCKS, OPEN_NONE = 4096, 1024, 0xFFFFFFFF
CTL_SYNACK = 4
LISTEN_SHUTDOWN = 0x01
OPEN_OPT_MSS, OPEN_OPT_WSCALE = 0x01, 0x02
TCP_LISTEN_DTYPE = np.dtype([("backlog", "<u4"), ("winmax", "<u4"), ("rcv_mss", "<u2"), ("rcv_wscale", "u1"),
                             ("flags", "u1"), ("pad", "<u4")])
TCP_OPEN_DTYPE = np.dtype([("src", "<u4"), ("listener", "<u4"), ("lip", "<u4"), ("rip", "<u4"), ("lport", "<u2"),
                           ("rport", "<u2"), ("irs", "<u4"), ("rcv_nxt", "<u4"), ("iss", "<u4"),
                           ("snd_una", "<u4"), ("snd_nxt", "<u4"), ("rcv_wnd", "<u4"), ("winmax", "<u4"),
                           ("snd_mss", "<u2"), ("snd_wscale", "u1"), ("rcv_wscale", "u1"), ("opt_en", "u1"),
                           ("state", "u1"), ("pad", "u1", (10,))])
# gcl_tcp_txq: the want bits, the entry flag, the state byte, the connection flags, the counters,
# the caps, struct gcl_txq_ent, struct gcl_txq_cold and struct gcl_txq_conn_out
TXQ_W_RTO, TXQ_W_FAST, TXQ_W_EXCL = 0x01, 0x02, 0x04
# gcl_udp_rx: the verdict byte (also the first counter slots), the counters, sflags, the socket flags,
# the caps, struct gcl_udp_sock, struct gcl_udp_sock_out and struct gcl_udp_rec
UDPRX_QUEUED, UDPRX_SPAWN, UDPRX_FULL, UDPRX_CLOSED, UDPRX_NOSOCK, UDPRX_NA = range(6)
UDPRX_NR_VERDICTS, UDPRXC_BYTES, UDPRXC_POLLINS, UDPRXC_NR = 6, 6, 7, 8
UDPRX_SF_POLLIN = 0x01
UDPS_SHUTDOWN, UDPS_ERR, UDPS_SPAWNER = 0x01, 0x02, 0x04
UDPRX_MAX_BLOCKS, UDPRX_MAX_SOCK, UDPRX_NONE = 1024, 1 << 20, 0xFFFFFFFF
# its grouping (csrc/gcl_udprx.hip): the sockets one counting-sort pass serves
UDPRX_PASS_SOCK = 2048
UDP_SOCK_DTYPE = np.dtype([("inq_len", "<i4"), ("inq_cap", "<i4"), ("flags", "u1"), ("pad", "u1", (7,))])
UDP_SOCK_OUT_DTYPE = np.dtype([("inq_len", "<i4"), ("ntaken", "<u4"), ("ndropped", "<u4"), ("flags", "u1"),
                               ("pad", "u1", (3,))])
UDP_REC_DTYPE = np.dtype([("dst_off", "<u8"), ("rip", "<u4"), ("rport", "<u2"), ("len", "<u2")])
TXQE_INFLIGHT = 0x01
TXQS_KEPT, TXQS_ACKED, TXQS_RETX, TXQS_RETX_COPY, TXQS_NOSPACE, TXQS_REFUSED = range(6)
TXQS_TRIMMED = 0x80
TXQO_EMPTY, TXQO_DEFERRED, TXQO_NOSPACE, TXQO_BATCH, TXQO_BADRANGE = 0x01, 0x02, 0x04, 0x08, 0x10
(TXQC_ACKED, TXQC_RETX, TXQC_COPIED, TXQC_TRIMMED, TXQC_REFUSED, TXQC_NOSPACE, TXQC_DEFERRED,
 TXQC_BYTES) = range(8)
TXQC_NR, TXQ_MAX_BLOCKS, TXQ_MAX_CONN = 8, 1024, 1 << 20
# its launches (csrc/gcl_txq.hip): connections per tile, and the queue length from which the
# whole wave walks a queue
TXQ_TILE, TXQ_LONG = 256, 64
# gcl_tcp_read: the read's flags, the entry flag, the status byte, the connection flags, the
# counters, the caps, its launches' tile, and struct gcl_tcp_rd, gcl_rdq_ent, gcl_rd_iov and
# gcl_rd_conn_out
RD_WANT, RD_PEEK, RD_NONBLOCK, RD_RX_CLOSED, RD_RX_EXCL = 0x01, 0x02, 0x04, 0x08, 0x10
RDQE_FIN = 0x01
RDS_NONE, RDS_DONE, RDS_AGAIN, RDS_BLOCK, RDS_CLOSED, RDS_BADRANGE = range(6)
(RDO_RXWAKE, RDO_EXCL_LEFT, RDO_RX_CLOSED, RDO_PARTIAL, RDO_ACK, RDO_POLLIN_CLEAR, RDO_SEG_NOSPACE,
 RDO_ITEM_NOSPACE) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
(RDC_DONE, RDC_AGAIN, RDC_BLOCK, RDC_CLOSED, RDC_PEEKS, RDC_POPPED, RDC_PARTIAL, RDC_RX_CLOSED, RDC_ACKS,
 RDC_ITEMS, RDC_BYTES, RDC_NOSPACE) = range(12)
RDC_NR, RD_MAX_BLOCKS, RD_MAX_CONN, RD_TILE = 12, 1024, 1 << 20, 256
TCP_RD_DTYPE = np.dtype([("dst_off", "<u8"), ("len", "<u4"), ("tx_last_ack", "<u4"), ("tx_last_win", "<u4"),
                         ("winmax", "<u4"), ("err", "<i4"), ("flags", "u1"), ("pad", "u1", (3,))])
RDQ_ENT_DTYPE = np.dtype([("off", "<u8"), ("len", "<u2"), ("flags", "u1"), ("pad", "u1", (5,))])
RD_IOV_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("pad", "u1", (4,))])
RD_CONN_OUT_DTYPE = np.dtype([("ret", "<i8"), ("npop", "<u4"), ("pull", "<u4"), ("rcv_wnd", "<u4"),
                              ("first_item", "<u4"), ("nitems", "<u4"), ("status", "u1"), ("flags", "u1"),
                              ("pad", "u1", (2,))])
# gcl_tcp_write: the write's flags, the status byte (also the first counter slots), the connection
# flags, the other counters, the caps, its launches' tile, and struct gcl_tcp_wr and gcl_wr_conn_out
(WR_WANT, WR_VEC, WR_NONBLOCK, WR_NO_PARTIAL, WR_TX_CLOSED, WR_TX_EXCL, WR_ZERO_WND,
 WR_BELOW_EST) = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
WRS_NONE, WRS_DONE, WRS_AGAIN, WRS_BLOCK, WRS_CLOSED, WRS_NOSPC, WRS_REFUSED, WRS_NOSPACE = range(8)
WRO_ZWND_ARM, WRO_ZWND_CLEAR, WRO_ACKS_RESET, WRO_TXWAKE, WRO_ACK_TS, WRO_POLLOUT_CLEAR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20
WRC_SEGS, WRC_PUSH, WRC_HELD, WRC_SHORT, WRC_ITEMS, WRC_BYTES = range(8, 14)
WRC_NR, WR_MAX_IOV, WR_MAX_BLOCKS, WR_MAX_CONN, WR_TILE, WR_SEG_HELD = 14, 1024, 1024, 1 << 20, 256, 0xFFFFFFFF
TCP_WR_DTYPE = np.dtype([("src_off", "<u8"), ("len", "<u4"), ("tx_last_ack", "<u4"), ("pend_frame_off", "<u8"),
                         ("pend_len", "<u4"), ("err", "<i4"), ("snd_mss", "<u2"), ("ecn", "u1"), ("flags", "u1"),
                         ("pad", "u1", (12,))])
WR_CONN_OUT_DTYPE = np.dtype([("ret", "<i8"), ("snd_nxt", "<u4"), ("first_seg", "<u4"), ("nseg", "<u4"),
                              ("first_item", "<u4"), ("nitems", "<u4"), ("pend_len", "<u4"),
                              ("pend_frame_off", "<u8"), ("status", "u1"), ("flags", "u1"), ("pad", "u1", (6,))])
TXQ_ENT_DTYPE = np.dtype([("seg_seq", "<u4"), ("seg_end", "<u4"), ("ts", "<u8")])
TXQ_COLD_DTYPE = np.dtype([("frame_off", "<u8"), ("tcp_flags", "u1"), ("tcp_off", "u1"), ("flags", "u1"),
                           ("pad", "u1", (5,))])
TXQ_CONN_OUT_DTYPE = np.dtype([("head_ts", "<u8"), ("nacked", "<u4"), ("nretx", "<u4"), ("first", "<u4"),
                               ("flags", "u1"), ("pad", "u1", (11,))])
# gcl_tcp_shut: the ops, the request's flags, the status byte (also the first counter slots), the
# connection flags, the other counters, the caps, and struct gcl_tcp_shut and gcl_shut_conn_out
SHUT_OP_NONE, SHUT_OP_SHUTDOWN, SHUT_OP_CLOSE, SHUT_OP_ABORT = range(4)
SHUT_TX_CLOSED, SHUT_RX_CLOSED, SHUT_RX_EXCL = 0x01, 0x02, 0x04
SHUTS_NONE, SHUTS_DONE, SHUTS_BLOCK, SHUTS_ABORT_WAIT, SHUTS_EINVAL, SHUTS_REFUSED, SHUTS_NOSPACE = range(7)
(SHO_POLLHUP, SHO_TX_CLOSED_SET, SHO_TXWAKE, SHO_POLLRDHUP_IN, SHO_RX_CLOSED_SET, SHO_RXWAKE, SHO_DETACH_POLL,
 SHO_FREE_TXQ, SHO_FREE_PEND, SHO_FREE_RXQ, SHO_FREE_OOO, SHO_WARN, SHO_POLLOUT) = (1 << i for i in range(13))
SHUTC_FIN, SHUTC_RST, SHUTC_FAIL, SHUTC_PUT, SHUTC_WARN = range(7, 12)
SHUTS_NR, SHUTC_NR, SHUT_MAX_BLOCKS, SHUT_MAX_CONN, SHUT_TILE, CTL_FIN = 7, 12, 1024, 1 << 20, 256, 5
TCP_SHUT_DTYPE = np.dtype([("how", "<i4"), ("op", "u1"), ("flags", "u1"), ("pad", "u1", (10,))])
SHUT_CONN_OUT_DTYPE = np.dtype([("next_timeout", "<u8"), ("txq_ts", "<u8"), ("ret", "<i4"), ("err", "<i4"),
                                ("snd_nxt", "<u4"), ("first_seg", "<u4"), ("flags", "<u4"), ("status", "u1"),
                                ("state", "u1"), ("tmr_flags", "u1"), ("nseg", "u1"), ("nput", "u1"),
                                ("pad", "u1", (7,))])
STAT_NAMES = ["RX_UNREGISTERED_MAC", "RX_UNICAST_FAIL", "RX_BROADCAST_FAIL",
              "RX_FLOW_TAG_MATCH", "RX_UNHANDLED", "RX_HASH_MISSING", "RX_PULLED"]

WL_UDP64, WL_TCP1500_ZIPF, WL_MIXED = 0, 1, 2

# Fixed 40-B Toeplitz key of the reference (iokernel/directpath/core.c:35-39)
CALADAN_RSS_KEY = bytes([
    0x82, 0x19, 0xFA, 0x80, 0xA4, 0x31, 0x06, 0x59, 0x3E, 0x3F, 0x9A,
    0xAC, 0x3D, 0xAE, 0xD6, 0xD9, 0xF5, 0xFC, 0x0C, 0x63, 0x94, 0xBF,
    0x8F, 0xDE, 0xD2, 0xC5, 0xE2, 0x04, 0xB1, 0xCF, 0xB1, 0xB1, 0xA1,
    0x0D, 0x6D, 0x86, 0xBA, 0x61, 0x78, 0xEB])

VERDICT_DTYPE = np.dtype([("hash", "<u4"), ("uniqid", "<u2"), ("thread", "u1"), ("action", "u1")])
# every DELIVER / WAKE verdict carries the flow_tbl slot (hash % thread_count) in `thread`:
# the host post-pass reads flow_tbl[slot] at delivery time (rx.c:55-72)
VERDICT4_DTYPE = np.dtype([("uniqid", "<u2"), ("thread", "u1"), ("action", "u1")])
TRANS_DTYPE = np.dtype([("h5", "<u4"), ("h3", "<u4")])
# struct gcl_loop_rec: one persistent-loop verdict record (gcl_rxloop_peek)
LOOP_REC_DTYPE = np.dtype([("hash", "<u4"), ("verdict", "<u4"), ("ticket", "<u8")])


class GclCfg(ctypes.Structure):
    _fields_ = [("max_runtimes", ctypes.c_uint32), ("hash_mode", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("default_olflags", ctypes.c_uint8),
                ("rss_key", ctypes.c_uint8 * 40), ("thread_bits", ctypes.c_uint8),
                ("pad", ctypes.c_uint8 * 2)]


class GclBatch(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_void_p), ("frames_len", ctypes.c_uint64),
                ("stride", ctypes.c_uint64), ("offs", ctypes.c_void_p),
                ("olflags", ctypes.c_void_p), ("rss", ctypes.c_void_p),
                ("fdir_hi", ctypes.c_void_p), ("pkt_len", ctypes.c_void_p),
                ("n", ctypes.c_uint64), ("dst_hint", ctypes.c_void_p)]


class GclGenParams(ctypes.Structure):
    _fields_ = [("workload", ctypes.c_uint32), ("nruntimes", ctypes.c_uint32),
                ("seed", ctypes.c_uint64), ("n", ctypes.c_uint64), ("stride", ctypes.c_uint64),
                ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32),
                ("shard_block", ctypes.c_uint64), ("zipf_cdf", ctypes.c_void_p),
                ("nflows", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("pkt_len", ctypes.c_void_p)]


class GclOut(ctypes.Structure):
    _fields_ = [("verdicts", ctypes.c_void_p), ("runtime_counts", ctypes.c_void_p),
                ("stats", ctypes.c_void_p), ("trans", ctypes.c_void_p)]


class GclSockEntry(ctypes.Structure):
    _fields_ = [("lip", ctypes.c_uint32), ("rip", ctypes.c_uint32), ("lport", ctypes.c_uint16),
                ("rport", ctypes.c_uint16), ("proto", ctypes.c_uint8), ("match", ctypes.c_uint8),
                ("pad", ctypes.c_uint16), ("cookie", ctypes.c_uint32)]


class GclTrans(ctypes.Structure):
    _fields_ = [("h5", ctypes.c_uint32), ("h3", ctypes.c_uint32)]


class GclTrace(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_void_p), ("frames_len", ctypes.c_uint64),
                ("alloc_len", ctypes.c_uint64), ("offs", ctypes.c_void_p),
                ("pkt_len", ctypes.c_void_p), ("orig_len", ctypes.c_void_p),
                ("ts_ns", ctypes.c_void_p), ("n", ctypes.c_uint64), ("skipped", ctypes.c_uint64)]


class GclE2eOpts(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_uint32), ("nstreams", ctypes.c_uint32), ("chunk", ctypes.c_uint64)]


E2E_COPY, E2E_ZEROCOPY = 0, 1


class GclPairInfo(ctypes.Structure):
    _fields_ = [("chosen_us", ctypes.c_double), ("worst_us", ctypes.c_double),
                ("candidates", ctypes.c_uint32), ("classes", ctypes.c_uint32),
                ("spacer_bytes", ctypes.c_uint64), ("probe_write_bytes", ctypes.c_uint64)]


class GclRxloopCfg(ctypes.Structure):
    _fields_ = [("slots", ctypes.c_uint32), ("max_burst", ctypes.c_uint32),
                ("workers", ctypes.c_uint32), ("lifetime_ms", ctypes.c_uint32),
                ("region", ctypes.c_void_p), ("region_len", ctypes.c_uint64),
                ("counts", ctypes.c_void_p), ("stats", ctypes.c_void_p),
                ("flags", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


LOOP_INLINE_HDRS = 0x1
LOOP_HDR_RECORDS = 0x2
LOOP_STAMPS = 0x4


class GclTune(ctypes.Structure):
    """struct gcl_tune: test / A-B overrides of the library's defaults
    (GCL_TUNE_AUTO = -1 everywhere: the library's own choice)."""
    _fields_ = [("size", ctypes.c_uint32), ("tables", ctypes.c_int32), ("depth", ctypes.c_int32),
                ("threads", ctypes.c_int32), ("grid", ctypes.c_int32), ("blocks_per_cu", ctypes.c_int32),
                ("defer", ctypes.c_int32), ("pair_lean", ctypes.c_int32),
                ("tile_lean", ctypes.c_int32), ("loop64", ctypes.c_int32),
                ("loop_lean", ctypes.c_int32), ("loop_spec", ctypes.c_int32),
                ("loop_phase_max", ctypes.c_int32), ("loop_phase_up", ctypes.c_int32),
                ("loop_phase_down", ctypes.c_int32), ("loop_prefetch", ctypes.c_int32),
                ("debug", ctypes.c_uint32), ("rec_prefetch", ctypes.c_int32),
                ("slot_prefetch", ctypes.c_int32), ("vstage", ctypes.c_int32), ("pair_i32", ctypes.c_int32),
                ("tile_order", ctypes.c_int32), ("loop_t0", ctypes.c_uint64)]


TUNE_AUTO = -1


class GclVerdict(ctypes.Structure):
    _fields_ = [("hash", ctypes.c_uint32), ("uniqid", ctypes.c_uint16),
                ("thread", ctypes.c_uint8), ("action", ctypes.c_uint8)]


assert ctypes.sizeof(GclVerdict) == 8 and VERDICT_DTYPE.itemsize == 8


class GclLrpcMsg(ctypes.Structure):
    _fields_ = [("cmd", ctypes.c_uint64), ("payload", ctypes.c_ulong)]


class GclLrpcChanOut(ctypes.Structure):
    _fields_ = [("send_head", ctypes.c_uint32), ("send_tail", ctypes.c_uint32),
                ("tbl", ctypes.POINTER(GclLrpcMsg)), ("recv_head_wb", ctypes.POINTER(ctypes.c_uint32)),
                ("size", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class GclHostProc(ctypes.Structure):
    _fields_ = [("uniqid", ctypes.c_uint16), ("thread_count", ctypes.c_uint16),
                ("active_thread_count", ctypes.c_uint16), ("idle_top", ctypes.c_int16),
                ("flow_tbl", ctypes.c_uint16 * GCL_NCPU),
                ("rxq", ctypes.POINTER(GclLrpcChanOut) * GCL_NCPU)]


SCHED_ADD_CORE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(GclHostProc))
ENABLE_POLL_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(GclHostProc), ctypes.c_uint)
FREE_PKT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64)
OWNED_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(GclHostProc), ctypes.c_uint64)
REFCNT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int)
ARP_RESPOND_FN = ctypes.CFUNCTYPE(ctypes.c_bool, ctypes.c_void_p, ctypes.c_uint64)


class GclHostOps(ctypes.Structure):
    _fields_ = [("arg", ctypes.c_void_p), ("sched_add_core", SCHED_ADD_CORE_FN),
                ("enable_poll", ENABLE_POLL_FN), ("free_pkt", FREE_PKT_FN),
                ("owned", OWNED_FN), ("refcnt_update", REFCNT_FN),
                ("arp_respond", ARP_RESPOND_FN)]


PLAN_BY_RUNTIME = 0  # a packet-index list per runtime (every verdict width)
PLAN_BY_QUEUE = 1    # ... per flow-table queue (1- and 2-byte verdicts)


class GclPlanCfg(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("key", ctypes.c_uint32), ("blocks", ctypes.c_uint32),
                ("pad", ctypes.c_uint32)]


class GclPlanOut(ctypes.Structure):
    _fields_ = [("order", ctypes.c_void_p), ("bucket_off", ctypes.c_void_p)]


class GclPackIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("verdicts", ctypes.c_void_p),
                ("n", ctypes.c_uint64), ("order", ctypes.c_void_p), ("m", ctypes.c_uint64),
                ("pkt_len", ctypes.c_void_p), ("olflags", ctypes.c_void_p), ("offs", ctypes.c_void_p),
                ("stride", ctypes.c_uint64), ("shm_base", ctypes.c_uint64)]


class GclPackOut(ctypes.Structure):
    _fields_ = [("cmd", ctypes.c_void_p), ("payload", ctypes.c_void_p), ("v4", ctypes.c_void_p)]


class GclCopyIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("group", ctypes.c_uint32), ("src", ctypes.c_void_p),
                ("src_len", ctypes.c_uint64), ("src_off", ctypes.c_void_p), ("len", ctypes.c_void_p),
                ("tx_olflags", ctypes.c_void_p), ("hash", ctypes.c_void_p), ("n", ctypes.c_uint64),
                ("len_hint", ctypes.c_uint32), ("dst_cap", ctypes.c_uint32)]


class GclCopyOut(ctypes.Structure):
    _fields_ = [("dst", ctypes.c_void_p), ("dst_len", ctypes.c_uint64), ("dst_off", ctypes.c_void_p),
                ("dst_stride", ctypes.c_uint64), ("pkt_len", ctypes.c_void_p),
                ("olflags", ctypes.c_void_p), ("rss", ctypes.c_void_p)]


class GclL4In(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("group", ctypes.c_uint32),
                ("len_hint", ctypes.c_uint32), ("tx_olflags", ctypes.c_void_p)]


class GclPayIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("align", ctypes.c_uint32), ("order", ctypes.c_void_p),
                ("m", ctypes.c_uint64), ("sock", ctypes.c_void_p), ("l4_status", ctypes.c_void_p),
                ("seg_off", ctypes.c_void_p), ("nseg", ctypes.c_uint32), ("blocks", ctypes.c_uint32)]


class GclPayOut(ctypes.Structure):
    _fields_ = [("src_off", ctypes.c_void_p), ("len", ctypes.c_void_p), ("dst_off", ctypes.c_void_p),
                ("kind", ctypes.c_void_p), ("meta", ctypes.c_void_p), ("seg_bytes", ctypes.c_void_p),
                ("total", ctypes.c_void_p)]


class GclTxhNet(ctypes.Structure):
    _fields_ = [("addr", ctypes.c_uint32), ("netmask", ctypes.c_uint32), ("gateway", ctypes.c_uint32),
                ("mac", ctypes.c_uint8 * 6), ("min_pkt_size", ctypes.c_uint8), ("flags", ctypes.c_uint8)]


class GclTxhIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("desc", ctypes.c_void_p),
                ("frame_off", ctypes.c_void_p), ("m", ctypes.c_uint64), ("frames", ctypes.c_void_p),
                ("frames_len", ctypes.c_uint64), ("shm_base", ctypes.c_uint64), ("cap", ctypes.c_uint32),
                ("pad2", ctypes.c_uint32), ("net", GclTxhNet)]


class GclTxhOut(ctypes.Structure):
    _fields_ = [("cmd", ctypes.c_void_p), ("payload", ctypes.c_void_p), ("pkt_len", ctypes.c_void_p),
                ("tx_olflags", ctypes.c_void_p), ("hash", ctypes.c_void_p), ("status", ctypes.c_void_p)]


class GclSegIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("send", ctypes.c_void_p),
                ("m", ctypes.c_uint64), ("seg_cap", ctypes.c_uint64), ("frame_base", ctypes.c_uint64),
                ("frames_len", ctypes.c_uint64), ("stride", ctypes.c_uint32), ("lead", ctypes.c_uint32),
                ("udp_max", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


SEG_WRITE_FIELDS = ("status", "sent", "snd_nxt_out", "seg_first", "nseg")
SEG_SEG_FIELDS = ("desc", "frame_off", "src_off", "len", "dst_off", "send_idx")
SEG_OUT_FIELDS = SEG_WRITE_FIELDS + SEG_SEG_FIELDS + ("total_segs", "total_bytes")


class GclSegOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in SEG_OUT_FIELDS]


class GclTcprxIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("align", ctypes.c_uint32), ("order", ctypes.c_void_p),
                ("m", ctypes.c_uint64), ("sock", ctypes.c_void_p), ("l4_status", ctypes.c_void_p),
                ("conn", ctypes.c_void_p), ("nconn", ctypes.c_uint32), ("blocks", ctypes.c_uint32)]


class GclTcprxfIn(ctypes.Structure):
    _fields_ = GclTcprxIn._fields_ + [("rep_acks", ctypes.c_void_p)]


class GclTcprxoIn(ctypes.Structure):
    _fields_ = GclTcprxfIn._fields_ + [("q_off", ctypes.c_void_p), ("q", ctypes.c_void_p),
                                       ("nq", ctypes.c_uint32), ("q_out_cap", ctypes.c_uint32)]


# struct gcl_tcprxo_out: (field, bytes per element, which count it is sized by)
TCPRXO_OUT_FIELDS = (("oflags", 1, "m"), ("skip", 2, "m"), ("qin_state", 1, "nq"), ("qin_skip", 2, "nq"),
                     ("qin_len", 2, "nq"), ("qin_dst_off", 8, "nq"), ("qout_off", 4, "nconn1"),
                     ("qout", 16, "cap"), ("totals", 8, "one"))


class GclTcprxoOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f, _, _ in TCPRXO_OUT_FIELDS]


class GclTcprxsIn(ctypes.Structure):
    _fields_ = GclTcprxoIn._fields_ + [("state", ctypes.c_void_p)]


# struct gcl_tcprxs_out: (field, bytes per element, which count it is sized by)
TCPRXS_OUT_FIELDS = (("ev", 1, "m"), ("rst_seq", 4, "m"), ("state_after", 1, "m"), ("state_out", 1, "nconn"))


class GclTcprxsOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f, _, _ in TCPRXS_OUT_FIELDS]


TCPRX_ENTRY_FIELDS = ("verdict", "sflags", "rcv_nxt_after", "copy_len", "dst_off")
TCPRX_OUT_FIELDS = TCPRX_ENTRY_FIELDS + ("out_conn", "conn_off")


class GclTcprxOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in TCPRX_OUT_FIELDS]


CTLSEG_SEG_FIELDS = ("desc", "frame_off", "seg_conn", "seg_kind", "seg_src")
CTLSEG_OUT_FIELDS = CTLSEG_SEG_FIELDS + ("totals",)
TICK_OUT_FIELDS = ("out_tmr",) + CTLSEG_OUT_FIELDS


class GclCtlsegOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in CTLSEG_OUT_FIELDS]


class GclTickIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("now", ctypes.c_uint64),
                ("tmr", ctypes.c_void_p), ("conn", ctypes.c_void_p), ("addr", ctypes.c_void_p),
                ("nconn", ctypes.c_uint32), ("frame_stride", ctypes.c_uint32), ("seg_cap", ctypes.c_uint64),
                ("frame_base", ctypes.c_uint64)]


class GclTickOut(ctypes.Structure):
    _fields_ = [("out_tmr", ctypes.c_void_p), ("seg", GclCtlsegOut)]


class GclRxackIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("order", ctypes.c_void_p),
                ("m", ctypes.c_uint64), ("n", ctypes.c_uint64), ("sock", ctypes.c_void_p),
                ("verdict", ctypes.c_void_p), ("sflags", ctypes.c_void_p), ("rcv_nxt_after", ctypes.c_void_p),
                ("conn", ctypes.c_void_p), ("addr", ctypes.c_void_p), ("nconn", ctypes.c_uint32),
                ("frame_stride", ctypes.c_uint32), ("seg_cap", ctypes.c_uint64), ("frame_base", ctypes.c_uint64)]


class GclRxctlIn(ctypes.Structure):
    _fields_ = GclRxackIn._fields_ + [("ev", ctypes.c_void_p), ("rst_seq", ctypes.c_void_p)]


class GclTcpopenIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("order", ctypes.c_void_p),
                ("m", ctypes.c_uint64), ("sock", ctypes.c_void_p), ("l4_status", ctypes.c_void_p),
                ("hash_slots", ctypes.c_uint32), ("listen_base", ctypes.c_uint32), ("nlisten", ctypes.c_uint32),
                ("frame_stride", ctypes.c_uint32), ("listen", ctypes.c_void_p), ("iss", ctypes.c_void_p),
                ("seg_cap", ctypes.c_uint64), ("frame_base", ctypes.c_uint64), ("open_cap", ctypes.c_uint64),
                ("tx_frames", ctypes.c_void_p), ("tx_frames_len", ctypes.c_uint64)]


TCPOPEN_OUT_FIELDS = ("verdict", "later_of", "rst_seq", "open", "backlog_out", "totals")


class GclTcpopenOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in TCPOPEN_OUT_FIELDS]


class GclUdprxIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("align", ctypes.c_uint32), ("order", ctypes.c_void_p),
                ("m", ctypes.c_uint64), ("sock", ctypes.c_void_p), ("l4_status", ctypes.c_void_p),
                ("usock", ctypes.c_void_p), ("nsock", ctypes.c_uint32), ("sock_base", ctypes.c_uint32),
                ("blocks", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


UDPRX_ENTRY_FIELDS = ("verdict", "sflags", "copy_len", "dst_off", "rec_idx")
UDPRX_OUT_FIELDS = UDPRX_ENTRY_FIELDS + ("rec", "out_sock", "rec_off", "sock_off")


class GclUdprxOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in UDPRX_OUT_FIELDS]


class GclTxqIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("now", ctypes.c_uint64),
                ("qoff", ctypes.c_void_p), ("ent", ctypes.c_void_p), ("cold", ctypes.c_void_p),
                ("nent", ctypes.c_uint64), ("conn", ctypes.c_void_p), ("addr", ctypes.c_void_p),
                ("want", ctypes.c_void_p), ("nconn", ctypes.c_uint32), ("frame_stride", ctypes.c_uint32),
                ("seg_cap", ctypes.c_uint64), ("frame_base", ctypes.c_uint64)]


TXQ_SEG_FIELDS = ("desc", "frame_off", "src_off", "len", "dst_off", "seg_conn", "seg_ent")
TXQ_OUT_FIELDS = ("out_conn", "state") + TXQ_SEG_FIELDS + ("totals",)


class GclTxqOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in TXQ_OUT_FIELDS]


class GclRdIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("qoff", ctypes.c_void_p),
                ("ent", ctypes.c_void_p), ("nent", ctypes.c_uint64), ("voff", ctypes.c_void_p),
                ("iov", ctypes.c_void_p), ("nvec", ctypes.c_uint64), ("rd", ctypes.c_void_p),
                ("conn", ctypes.c_void_p), ("addr", ctypes.c_void_p), ("nconn", ctypes.c_uint32),
                ("frame_stride", ctypes.c_uint32), ("item_cap", ctypes.c_uint64), ("seg_cap", ctypes.c_uint64),
                ("frame_base", ctypes.c_uint64)]


RD_ITEM_FIELDS = ("src_off", "len", "dst_off", "item_conn", "item_ent")
# the control segments' fields of a Classifier.tcp_read `out` dict: gcl_rd_out.seg
RD_SEG_FIELDS = CTLSEG_SEG_FIELDS + ("seg_totals",)
RD_OUT_FIELDS = ("out_conn",) + RD_ITEM_FIELDS + ("totals",) + RD_SEG_FIELDS


class GclRdOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in ("out_conn",) + RD_ITEM_FIELDS + ("totals",)] + [("seg", GclCtlsegOut)]


class GclWrIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("now", ctypes.c_uint64),
                ("voff", ctypes.c_void_p), ("iov", ctypes.c_void_p), ("nvec", ctypes.c_uint64),
                ("wr", ctypes.c_void_p), ("conn", ctypes.c_void_p), ("addr", ctypes.c_void_p),
                ("nconn", ctypes.c_uint32), ("frame_stride", ctypes.c_uint32), ("seg_cap", ctypes.c_uint64),
                ("item_cap", ctypes.c_uint64), ("frame_base", ctypes.c_uint64), ("frames_len", ctypes.c_uint64)]


WR_SEG_FIELDS = ("desc", "frame_off", "seg_conn", "txq_ent", "txq_cold")
WR_ITEM_FIELDS = ("src_off", "len", "dst_off", "item_conn", "item_seg")
WR_OUT_FIELDS = ("out_conn",) + WR_SEG_FIELDS + WR_ITEM_FIELDS + ("totals",)


class GclWrOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_void_p) for f in WR_OUT_FIELDS]


class GclShutIn(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("now", ctypes.c_uint64),
                ("shut", ctypes.c_void_p), ("tmr", ctypes.c_void_p), ("conn", ctypes.c_void_p),
                ("addr", ctypes.c_void_p), ("nconn", ctypes.c_uint32), ("frame_stride", ctypes.c_uint32),
                ("seg_cap", ctypes.c_uint64), ("frame_base", ctypes.c_uint64), ("frames_len", ctypes.c_uint64)]


SHUT_SEG_FIELDS = CTLSEG_SEG_FIELDS + ("txq_ent", "txq_cold")
SHUT_OUT_FIELDS = ("out_conn",) + SHUT_SEG_FIELDS + ("totals",)


class GclShutOut(ctypes.Structure):
    _fields_ = [("out_conn", ctypes.c_void_p), ("seg", GclCtlsegOut), ("txq_ent", ctypes.c_void_p),
                ("txq_cold", ctypes.c_void_p)]


assert ctypes.sizeof(GclShutIn) == 80 and ctypes.sizeof(GclShutOut) == 72
assert TCP_SHUT_DTYPE.itemsize == 16 and SHUT_CONN_OUT_DTYPE.itemsize == 48
assert ctypes.sizeof(GclWrIn) == 104 and ctypes.sizeof(GclWrOut) == 96
assert TCP_WR_DTYPE.itemsize == 48 and WR_CONN_OUT_DTYPE.itemsize == 48
assert ctypes.sizeof(GclRdIn) == 112 and ctypes.sizeof(GclRdOut) == 104
assert TCP_RD_DTYPE.itemsize == 32 and RDQ_ENT_DTYPE.itemsize == 16 and RD_IOV_DTYPE.itemsize == 16
assert RD_CONN_OUT_DTYPE.itemsize == 32
assert ctypes.sizeof(GclTxqIn) == 96 and ctypes.sizeof(GclTxqOut) == 80
assert ctypes.sizeof(GclUdprxIn) == 64 and ctypes.sizeof(GclUdprxOut) == 72
assert UDP_SOCK_DTYPE.itemsize == 16 and UDP_SOCK_OUT_DTYPE.itemsize == 16 and UDP_REC_DTYPE.itemsize == 16
assert TXQ_ENT_DTYPE.itemsize == 16 and TXQ_COLD_DTYPE.itemsize == 16 and TXQ_CONN_OUT_DTYPE.itemsize == 32
assert ctypes.sizeof(GclTickIn) == 64 and ctypes.sizeof(GclTickOut) == 56 and ctypes.sizeof(GclRxackIn) == 104
assert ctypes.sizeof(GclCtlsegOut) == 48 and TCP_TMR_DTYPE.itemsize == 64 and TCP_TMR_OUT_DTYPE.itemsize == 32
assert TCP_ADDR_DTYPE.itemsize == 16
assert ctypes.sizeof(GclTcprxIn) == 56 and ctypes.sizeof(GclTcprxOut) == 56
assert ctypes.sizeof(GclTcprxfIn) == 64 and TCP_CONN_EXT_DTYPE.itemsize == 16
assert ctypes.sizeof(GclTcprxoIn) == 88 and ctypes.sizeof(GclTcprxoOut) == 72 and TCP_OOO_ENT_DTYPE.itemsize == 16
assert ctypes.sizeof(GclRxctlIn) == 120
assert ctypes.sizeof(GclTcpopenIn) == 112 and ctypes.sizeof(GclTcpopenOut) == 48
assert TCP_LISTEN_DTYPE.itemsize == 16 and TCP_OPEN_DTYPE.itemsize == 64
assert ctypes.sizeof(GclTcprxsIn) == 96 and ctypes.sizeof(GclTcprxsOut) == 32
assert TCP_CONN_DTYPE.itemsize == 48 and TCP_CONN_OUT_DTYPE.itemsize == 48
assert ctypes.sizeof(GclSegIn) == 64 and ctypes.sizeof(GclSegOut) == 104 and SEG_SEND_DTYPE.itemsize == 48
assert ctypes.sizeof(GclTxhIn) == 88 and ctypes.sizeof(GclTxhNet) == 20 and TXH_DESC_DTYPE.itemsize == 32
assert NEIGH_ENTRY_DTYPE.itemsize == 12
assert ctypes.sizeof(GclPayIn) == 56 and ctypes.sizeof(GclPayOut) == 56 and PAY_META_DTYPE.itemsize == 16


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: run `python caladan_amd/build.py` "
                          "(the classifier has no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    vp, u16, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    sig = {
        "gcl_open": (i32, [i32, ctypes.POINTER(GclCfg), ctypes.POINTER(vp)]),
        "gcl_close": (None, [vp]),
        "gcl_runtime_set": (i32, [vp, u16, u32, u16, u16, ctypes.POINTER(u16)]),
        "gcl_runtime_del": (i32, [vp, u16]),
        "gcl_steer_flows": (i32, [u16, ctypes.POINTER(u16), u16, ctypes.POINTER(u16)]),
        "gcl_classify": (i32, [vp, ctypes.POINTER(GclBatch), vp, vp, vp, vp]),
        "gcl_classify_ex": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclOut), vp]),
        "gcl_access_probe": (i32, [vp, ctypes.POINTER(GclBatch), vp, u32, vp]),
        "gcl_runtime_set_trans_seed": (i32, [vp, u16, u32]),
        "gcl_crc32c_u64": (u32, [u32, u64]),
        "gcl_trans_hash": (None, [u32, ctypes.c_uint8, u32, u16, u32, u16, ctypes.POINTER(GclTrans)]),
        "gcl_sync": (i32, [vp]),
        "gcl_kernel_time": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64), i32]),
        "gcl_profile_sample": (i32, [vp, u32]),
        "gcl_generate": (i32, [ctypes.POINTER(GclGenParams), vp, vp, vp, vp]),
        "gcl_runtime_ip": (u32, [u32]),
        "gcl_loopback_olflags": (ctypes.c_uint8, [ctypes.c_uint8]),
        "gcl_txpkt_rss": (u32, [u64]),
        "gcl_zipf_cdf": (i32, [u32, ctypes.c_double, vp]),
        "gcl_jenkins_hash": (u32, [ctypes.c_char_p, ctypes.c_size_t]),
        "gcl_toeplitz": (u32, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]),
        "gcl_version": (ctypes.c_char_p, []),
        "gcl_lrpc_init_out": (i32, [ctypes.POINTER(GclLrpcChanOut), ctypes.POINTER(GclLrpcMsg), ctypes.c_uint, ctypes.POINTER(u32)]),
        "gcl_lrpc_send": (ctypes.c_bool, [ctypes.POINTER(GclLrpcChanOut), u64, ctypes.c_ulong]),
        "gcl_rx_make_cmd": (u64, [u16, ctypes.c_uint8]),
        "gcl_classify_host": (i32, [vp, ctypes.POINTER(GclBatch), vp, vp, vp, ctypes.POINTER(GclE2eOpts)]),
        "gcl_host_register": (i32, [vp, ctypes.c_size_t]),
        "gcl_dev_alloc": (i32, [i32, ctypes.c_size_t, ctypes.POINTER(vp)]),
        "gcl_dev_free": (i32, [vp]),
        "gcl_rxloop_start": (i32, [vp, ctypes.POINTER(GclRxloopCfg), ctypes.POINTER(vp)]),
        "gcl_rxloop_submit": (ctypes.c_int64, [vp, u32, vp, vp, vp, vp, vp]),
        "gcl_rxloop_wait": (i32, [vp, ctypes.c_int64, vp, u64]),
        "gcl_rxloop_stop": (i32, [vp]),
        "gcl_rxloop_drive": (i32, [vp, u32, vp, u32, u32, vp, ctypes.POINTER(u64)]),
        "gcl_dev_alloc_paired": (i32, [i32, ctypes.c_size_t, vp, ctypes.c_size_t, u32,
                                       ctypes.POINTER(vp), ctypes.POINTER(GclPairInfo)]),
        "gcl_host_unregister": (i32, [vp]),
        "gcl_pcap_write": (i32, [ctypes.c_char_p, vp, u64, vp, vp, vp, u64, u32]),
        "gcl_pcap_load": (i32, [ctypes.c_char_p, ctypes.POINTER(GclTrace), u64]),
        "gcl_pcap_free": (None, [ctypes.POINTER(GclTrace)]),
        "gcl_host_deliver": (u64, [vp, u32, vp, i32, vp, vp, vp, ctypes.c_uint8, vp, u64,
                                   ctypes.POINTER(GclHostOps), vp]),
        "gcl_host_deliver4": (u64, [vp, u32, vp, i32, vp, vp, vp, vp, ctypes.c_uint8, vp, u64,
                                    ctypes.POINTER(GclHostOps), vp]),
        "gcl_host_deliver2": (u64, [vp, u32, vp, i32, vp, ctypes.c_uint8, vp, vp, vp,
                                    ctypes.c_uint8, vp, u64, ctypes.POINTER(GclHostOps), vp]),
        "gcl_verdict2_to4": (ctypes.c_uint32, [ctypes.c_uint16, ctypes.c_uint8]),
        "gcl_host_deliver1": (u64, [vp, u32, vp, i32, vp, ctypes.c_uint8, vp, vp, vp,
                                    ctypes.c_uint8, vp, u64, ctypes.POINTER(GclHostOps), vp]),
        "gcl_verdict1_to4": (ctypes.c_uint32, [ctypes.c_uint8, ctypes.c_uint8]),
        "gcl_host_deliver_recs": (u64, [vp, u32, vp, i32, vp, ctypes.c_uint8, ctypes.c_uint8, vp, vp,
                                        vp, ctypes.c_uint8, vp, u64, ctypes.POINTER(GclHostOps), vp]),
        "gcl_host_prefetch_rxq": (None, [vp, i32]),
        "gcl_host_deliver_idx": (u64, [vp, u32, vp, i32, vp, ctypes.c_uint8, ctypes.c_uint8, vp, vp,
                                       vp, ctypes.c_uint8, vp, vp, u64, ctypes.POINTER(GclHostOps), vp]),
        "gcl_plan_buckets": (i32, [vp, u32, ctypes.POINTER(u32)]),
        "gcl_plan_workspace": (i32, [vp, ctypes.POINTER(GclPlanCfg), u64,
                                     ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_plan": (i32, [vp, ctypes.POINTER(GclPlanCfg), vp, u64, ctypes.POINTER(GclPlanOut), vp,
                           ctypes.c_size_t, vp]),
        "gcl_plan_pack": (i32, [vp, ctypes.POINTER(GclPackIn), ctypes.POINTER(GclPackOut), vp]),
        "gcl_rx_csum": (i32, [vp, ctypes.POINTER(GclBatch), vp, vp, vp]),
        "gcl_rx_csum_flags": (ctypes.c_uint8, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint8]),
        "gcl_l4_csum": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclL4In), vp, vp, vp]),
        "gcl_l4_csum_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclL4In), vp, vp]),
        "gcl_l4_payload_workspace": (i32, [u64, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_l4_payload": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclPayIn),
                                 ctypes.POINTER(GclPayOut), vp, vp, ctypes.c_size_t, vp]),
        "gcl_l4_payload_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclPayIn),
                                      ctypes.POINTER(GclPayOut), vp]),
        "gcl_sock_set": (i32, [vp, ctypes.c_uint16, vp, u32]),
        "gcl_sock_lookup": (i32, [vp, ctypes.POINTER(GclBatch), vp, vp, vp, vp]),
        "gcl_sock_tbl_new": (vp, []),
        "gcl_sock_tbl_free": (None, [vp]),
        "gcl_sock_tbl_set": (i32, [vp, ctypes.c_uint16, vp, u32]),
        "gcl_sock_tbl_del": (i32, [vp, ctypes.c_uint16]),
        "gcl_sock_tbl_hash_bits": (i32, [vp, u32]),
        "gcl_sock_tbl_lookup_host": (i32, [vp, ctypes.c_uint8, ctypes.c_uint8, u32,
                                           ctypes.POINTER(GclBatch), vp, vp, vp]),
        "gcl_neigh_set": (i32, [vp, vp, u32]),
        "gcl_tx_hdr": (i32, [vp, ctypes.POINTER(GclTxhIn), ctypes.POINTER(GclTxhOut), vp, vp]),
        "gcl_tx_hdr_host": (i32, [vp, ctypes.c_char_p, ctypes.POINTER(GclTxhIn), ctypes.POINTER(GclTxhOut),
                                  vp]),
        "gcl_tx_seg_workspace": (i32, [u64, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tx_seg": (i32, [vp, ctypes.POINTER(GclSegIn), ctypes.POINTER(GclSegOut), vp, vp,
                             ctypes.c_size_t, vp]),
        "gcl_tx_seg_host": (i32, [ctypes.POINTER(GclSegIn), ctypes.POINTER(GclSegOut), vp]),
        "gcl_tcp_rx_workspace": (i32, [u64, u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_rx": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxIn),
                             ctypes.POINTER(GclTcprxOut), vp, vp, ctypes.c_size_t, vp]),
        "gcl_tcp_rx_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxIn),
                                  ctypes.POINTER(GclTcprxOut), vp]),
        "gcl_tcp_rx_full_workspace": (i32, [u64, u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_rx_full": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxfIn),
                                  ctypes.POINTER(GclTcprxOut), vp, vp, vp, ctypes.c_size_t, vp]),
        "gcl_tcp_rx_full_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxfIn),
                                       ctypes.POINTER(GclTcprxOut), vp, vp]),
        "gcl_tcp_rx_ooo_workspace": (i32, [u64, u32, u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_rx_ooo": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxoIn),
                                 ctypes.POINTER(GclTcprxOut), vp, ctypes.POINTER(GclTcprxoOut), vp, vp,
                                 ctypes.c_size_t, vp]),
        "gcl_tcp_rx_ooo_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxoIn),
                                      ctypes.POINTER(GclTcprxOut), vp, ctypes.POINTER(GclTcprxoOut), vp]),
        "gcl_tcp_rx_states_workspace": (i32, [u64, u32, u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_rx_states": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxsIn),
                                    ctypes.POINTER(GclTcprxOut), vp, ctypes.POINTER(GclTcprxoOut),
                                    ctypes.POINTER(GclTcprxsOut), vp, vp, ctypes.c_size_t, vp]),
        "gcl_tcp_rx_states_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcprxsIn),
                                         ctypes.POINTER(GclTcprxOut), vp, ctypes.POINTER(GclTcprxoOut),
                                         ctypes.POINTER(GclTcprxsOut), vp]),
        "gcl_tcp_tick_workspace": (i32, [u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_tick": (i32, [vp, ctypes.POINTER(GclTickIn), ctypes.POINTER(GclTickOut), vp, vp,
                               ctypes.c_size_t, vp]),
        "gcl_tcp_tick_host": (i32, [ctypes.POINTER(GclTickIn), ctypes.POINTER(GclTickOut), vp]),
        "gcl_tcp_rx_ctl_workspace": (i32, [u64, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_rx_ctl": (i32, [vp, ctypes.POINTER(GclRxctlIn), ctypes.POINTER(GclCtlsegOut), vp, vp,
                                 ctypes.c_size_t, vp]),
        "gcl_tcp_rx_ctl_host": (i32, [ctypes.POINTER(GclRxctlIn), ctypes.POINTER(GclCtlsegOut), vp]),
        "gcl_tcp_rx_acks_workspace": (i32, [u64, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_rx_acks": (i32, [vp, ctypes.POINTER(GclRxackIn), ctypes.POINTER(GclCtlsegOut), vp, vp,
                                  ctypes.c_size_t, vp]),
        "gcl_tcp_rx_acks_host": (i32, [ctypes.POINTER(GclRxackIn), ctypes.POINTER(GclCtlsegOut), vp]),
        "gcl_tcp_rx_open_workspace": (i32, [u64, u32, u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_rx_open": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcpopenIn),
                                  ctypes.POINTER(GclTcpopenOut), ctypes.POINTER(GclCtlsegOut), vp, vp,
                                  ctypes.c_size_t, vp]),
        "gcl_tcp_rx_open_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclTcpopenIn),
                                       ctypes.POINTER(GclTcpopenOut), ctypes.POINTER(GclCtlsegOut), vp]),
        "gcl_udp_rx_workspace": (i32, [u64, u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_udp_rx": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(GclUdprxIn),
                             ctypes.POINTER(GclUdprxOut), vp, vp, ctypes.c_size_t, vp]),
        "gcl_udp_rx_host": (i32, [ctypes.POINTER(GclBatch), ctypes.POINTER(GclUdprxIn),
                                  ctypes.POINTER(GclUdprxOut), vp]),
        "gcl_tcp_txq_workspace": (i32, [u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_txq": (i32, [vp, ctypes.POINTER(GclTxqIn), ctypes.POINTER(GclTxqOut), vp, vp,
                              ctypes.c_size_t, vp]),
        "gcl_tcp_txq_host": (i32, [ctypes.POINTER(GclTxqIn), ctypes.POINTER(GclTxqOut), vp]),
        "gcl_tcp_read_workspace": (i32, [u32, u64, u64, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_read": (i32, [vp, ctypes.POINTER(GclRdIn), ctypes.POINTER(GclRdOut), vp, vp,
                               ctypes.c_size_t, vp]),
        "gcl_tcp_read_host": (i32, [ctypes.POINTER(GclRdIn), ctypes.POINTER(GclRdOut), vp]),
        "gcl_tcp_write_workspace": (i32, [u32, u64, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_write": (i32, [vp, ctypes.POINTER(GclWrIn), ctypes.POINTER(GclWrOut), vp, vp,
                                ctypes.c_size_t, vp]),
        "gcl_tcp_write_host": (i32, [ctypes.POINTER(GclWrIn), ctypes.POINTER(GclWrOut), vp]),
        "gcl_tcp_shut_workspace": (i32, [u32, u32, ctypes.POINTER(ctypes.c_size_t)]),
        "gcl_tcp_shut": (i32, [vp, ctypes.POINTER(GclShutIn), ctypes.POINTER(GclShutOut), vp, vp,
                               ctypes.c_size_t, vp]),
        "gcl_tcp_shut_host": (i32, [ctypes.POINTER(GclShutIn), ctypes.POINTER(GclShutOut), vp]),
        "gcl_neigh_tbl_new": (vp, []),
        "gcl_neigh_tbl_free": (None, [vp]),
        "gcl_neigh_tbl_set": (i32, [vp, vp, u32]),
        "gcl_neigh_tbl_hash_bits": (i32, [vp, u32]),
        "gcl_neigh_tbl_count": (u32, [vp]),
        "gcl_neigh_tbl_lookup": (i32, [vp, u32, ctypes.POINTER(ctypes.c_uint8 * 6)]),
        "gcl_copy_batch": (i32, [vp, ctypes.POINTER(GclCopyIn), ctypes.POINTER(GclCopyOut), vp, vp]),
        "gcl_copy_batch_host": (i32, [ctypes.POINTER(GclCopyIn), ctypes.POINTER(GclCopyOut), vp]),
        "gcl_host_deliver_packed": (u64, [vp, u32, vp, i32, vp, vp, vp, vp, u64, u64, vp,
                                          ctypes.POINTER(GclHostOps), vp]),
        "gcl_rxloop_peek": (i32, [vp, ctypes.c_int64, u64, ctypes.POINTER(vp), ctypes.POINTER(u32)]),
        "gcl_rxloop_release": (i32, [vp, ctypes.c_int64]),
        "gcl_rxloop_poll_stats": (i32, [vp, vp]),
        "gcl_rxloop_lean_bursts": (i32, [vp, vp]),
        "gcl_rxloop_trans": (i32, [vp, ctypes.c_int64, vp]),
        "gcl_tune_init": (None, [ctypes.POINTER(GclTune)]),
        "gcl_ctx_tune": (i32, [vp, ctypes.POINTER(GclTune)]),
        "gcl_abi_version": (i32, []),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


lib = _load()


def _check(ret, what):
    if ret < 0:
        raise OSError(-ret, f"{what}: {os.strerror(-ret)}")
    return ret


def _ptr(x):
    """Device/host address of a torch tensor or numpy array (None -> NULL)."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return int(x)


def _nbytes(x):
    if hasattr(x, "numel"):
        return x.numel() * x.element_size()
    if isinstance(x, int):  # raw device address: caller vouches for the size
        return 1 << 62
    return x.nbytes


def _frames_len(frames, frames_len):
    """The readable length the kernel is given: the whole buffer, or a
    caller's shorter limit -- never more than the buffer holds (the kernel
    trusts it as the bound of every frame read)."""
    size = _nbytes(frames)
    if frames_len is None:
        return size
    if frames_len < 0 or frames_len > size:
        raise ValueError(f"frames_len {frames_len} exceeds the {size}-byte frame buffer")
    return frames_len


def make_tune(**kw):
    """A struct gcl_tune with the library's defaults (gcl_tune_init) and the
    fields in @kw set; loop_phase=(max, up, down) sets the three phase fields
    together (0 as max: off)."""
    t = GclTune()
    lib.gcl_tune_init(ctypes.byref(t))
    ph = kw.pop("loop_phase", None)
    if ph is not None:
        ph = tuple(ph) if not isinstance(ph, int) else (ph,)
        t.loop_phase_max = ph[0]
        t.loop_phase_up = ph[1] if len(ph) > 1 else 16
        t.loop_phase_down = ph[2] if len(ph) > 2 else 1
    for k, v in kw.items():
        if not hasattr(t, k) or k in ("size", "pad"):
            raise AttributeError(f"struct gcl_tune has no field {k}")
        setattr(t, k, int(v))
    return t


def jenkins_hash(key: bytes) -> int:
    return lib.gcl_jenkins_hash(key, len(key))


def toeplitz(key: bytes, data: bytes) -> int:
    return lib.gcl_toeplitz(key, len(key), data, len(data))


def crc32c_u64(crc, val):
    return lib.gcl_crc32c_u64(crc, val)


def trans_hash(seed, proto, lip, lport, rip, rport):
    t = GclTrans()
    lib.gcl_trans_hash(seed, proto, lip, lport, rip, rport, ctypes.byref(t))
    return t.h5, t.h3


def rx_csum_flags(frame: bytes, olflags: int) -> int:
    """gcl_rx_csum_flags: the rule of Classifier.rx_csum for one frame on the CPU."""
    frame = bytes(frame)
    return lib.gcl_rx_csum_flags(frame, len(frame), olflags)


def _copy_structs(src, src_len, src_off, length, tx_olflags, hash, n, len_hint, dst_cap, group,
                  dst, dst_len, dst_off, dst_stride, pkt_len, olflags, rss):
    """The two structs of gcl_copy_batch / gcl_copy_batch_host, sizes checked."""
    for arr, w in ((src_off, 8), (length, 2), (tx_olflags, 1), (hash, 4), (dst_off, 8),
                   (pkt_len, 2), (olflags, 1), (rss, 4)):
        if arr is not None and _nbytes(arr) < w * n:
            raise ValueError("per-packet array too small")
    cin = GclCopyIn(size=ctypes.sizeof(GclCopyIn), group=group, src=_ptr(src),
                    src_len=_frames_len(src, src_len), src_off=_ptr(src_off), len=_ptr(length),
                    tx_olflags=_ptr(tx_olflags), hash=_ptr(hash), n=n, len_hint=len_hint,
                    dst_cap=dst_cap)
    cout = GclCopyOut(dst=_ptr(dst), dst_len=_frames_len(dst, dst_len), dst_off=_ptr(dst_off),
                      dst_stride=dst_stride, pkt_len=_ptr(pkt_len), olflags=_ptr(olflags),
                      rss=_ptr(rss))
    return cin, cout


def copy_batch_host(src, src_off, length, dst, dst_off=None, dst_stride=0, tx_olflags=None,
                    hash=None, n=None, src_len=None, dst_len=None, dst_cap=0, counts=None,
                    pkt_len=None, olflags=None, rss=None):
    """gcl_copy_batch_host: the rule of Classifier.copy_batch on the CPU over
    numpy arrays (@dst is written in place).  @pkt_len, @olflags and @rss are
    allocated when None; False leaves olflags or rss out.  @counts is a
    u64[COPY_NR], accumulated.  Returns (pkt_len, olflags, rss)."""
    n = len(length) if n is None else n
    if pkt_len is None:
        pkt_len = np.zeros(max(n, 1), dtype=np.uint16)
    olflags = None if olflags is False else np.zeros(max(n, 1), dtype=np.uint8) if olflags is None else olflags
    rss = None if rss is False else np.zeros(max(n, 1), dtype=np.uint32) if rss is None else rss
    if counts is not None and _nbytes(counts) < 8 * COPY_NR:
        raise ValueError("counts buffer too small")
    cin, cout = _copy_structs(src, src_len, src_off, length, tx_olflags, hash, n, 0, dst_cap, 0,
                              dst, dst_len, dst_off, dst_stride, pkt_len, olflags, rss)
    _check(lib.gcl_copy_batch_host(ctypes.byref(cin), ctypes.byref(cout), _ptr(counts)),
           "gcl_copy_batch_host")
    return pkt_len, olflags, rss


def _l4_structs(frames, n, stride, offs, pkt_len, frames_len, mode, tx_olflags, group, len_hint,
                status, counts):
    """The two structs of gcl_l4_csum / gcl_l4_csum_host, sizes checked."""
    for arr, w in ((offs, 8), (pkt_len, 2), (tx_olflags, 1), (status, 1)):
        if arr is not None and _nbytes(arr) < w * n:
            raise ValueError("per-packet array too small")
    if counts is not None and _nbytes(counts) < 8 * L4C_NR:
        raise ValueError("counts buffer too small")
    b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), stride=stride,
                 offs=_ptr(offs), olflags=None, rss=None, fdir_hi=None, pkt_len=_ptr(pkt_len), n=n,
                 dst_hint=None)
    lin = GclL4In(size=ctypes.sizeof(GclL4In), mode=mode, group=group, len_hint=len_hint,
                  tx_olflags=_ptr(tx_olflags))
    return b, lin


def l4_csum_host(frames, pkt_len, mode=L4_VERIFY, stride=0, offs=None, n=None, frames_len=None,
                 tx_olflags=None, status=None, counts=None):
    """gcl_l4_csum_host: the rule of Classifier.l4_csum on the CPU over numpy
    arrays (L4_FILL writes the checksum fields into @frames in place).
    @status (uint8[n]) is allocated when None; @counts is a u64[L4C_NR],
    accumulated.  Returns @status."""
    n = len(pkt_len) if n is None else n
    if status is None:
        status = np.zeros(max(n, 1), dtype=np.uint8)
    b, lin = _l4_structs(frames, n, stride, offs, pkt_len, frames_len, mode, tx_olflags, 0, 0, status,
                         counts)
    _check(lib.gcl_l4_csum_host(ctypes.byref(b), ctypes.byref(lin), _ptr(status), _ptr(counts)),
           "gcl_l4_csum_host")
    return status


PAY_OUT_FIELDS = ("src_off", "len", "dst_off", "kind", "meta", "seg_bytes", "total")


def _pay_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status, seg_off,
                 nseg, align, blocks, out, counts):
    """The three structs of gcl_l4_payload / gcl_l4_payload_host, sizes
    checked; @out maps PAY_OUT_FIELDS to buffers (meta and seg_bytes may be
    None)."""
    for arr, w in ((offs, 8), (pkt_len, 2), (sock, 4), (l4_status, 1)):
        if arr is not None and _nbytes(arr) < w * n:
            raise ValueError("per-packet array too small")
    for arr, w in ((order, 4), (out["src_off"], 8), (out["len"], 2), (out["dst_off"], 8),
                   (out["kind"], 1), (out["meta"], 16)):
        if arr is not None and _nbytes(arr) < w * m:
            raise ValueError("per-entry array too small")
    if seg_off is not None and _nbytes(seg_off) < 4 * (nseg + 1):
        raise ValueError("seg_off too small")
    if out["seg_bytes"] is not None and _nbytes(out["seg_bytes"]) < 8 * (nseg + 1):
        raise ValueError("seg_bytes too small")
    if out["total"] is not None and _nbytes(out["total"]) < 8:
        raise ValueError("total too small")
    if counts is not None and _nbytes(counts) < 8 * PAYC_NR:
        raise ValueError("counts buffer too small")
    b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), stride=stride,
                 offs=_ptr(offs), olflags=None, rss=None, fdir_hi=None, pkt_len=_ptr(pkt_len), n=n,
                 dst_hint=None)
    pin = GclPayIn(size=ctypes.sizeof(GclPayIn), align=align, order=_ptr(order), m=m, sock=_ptr(sock),
                   l4_status=_ptr(l4_status), seg_off=_ptr(seg_off), nseg=nseg, blocks=blocks)
    pout = GclPayOut(**{f: _ptr(out[f]) for f in PAY_OUT_FIELDS})
    return b, pin, pout


def _pay_m(n, m, order):
    if m is not None:
        return m
    if order is None:
        return n
    if not (hasattr(order, "numel") or isinstance(order, np.ndarray)):
        raise ValueError("m is required when order is a raw address")
    return order.numel() if hasattr(order, "numel") else len(order)


def l4_payload_host(frames, pkt_len, stride=0, offs=None, n=None, frames_len=None, order=None, m=None,
                    sock=None, l4_status=None, seg_off=None, nseg=None, align=0, blocks=0, out=None,
                    counts=None):
    """gcl_l4_payload_host: the rule of Classifier.l4_payload on the CPU over
    numpy arrays.  @out maps PAY_OUT_FIELDS to arrays (u64, u16, u64, u8,
    PAY_META_DTYPE, u64[nseg + 1], u64[1]); the ones left out are allocated
    (meta too; seg_bytes only with @seg_off).  @counts is a u64[PAYC_NR],
    accumulated.  Returns the dict."""
    n = len(pkt_len) if n is None else n
    m = _pay_m(n, m, order)
    nseg = (len(seg_off) - 1 if seg_off is not None else 0) if nseg is None else nseg
    out = dict(out or {})
    for f, dt, k in (("src_off", np.uint64, m), ("len", np.uint16, m), ("dst_off", np.uint64, m),
                     ("kind", np.uint8, m), ("meta", PAY_META_DTYPE, m), ("total", np.uint64, 1)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    if "seg_bytes" not in out:
        out["seg_bytes"] = np.zeros(nseg + 1, dtype=np.uint64) if seg_off is not None else None
    b, pin, pout = _pay_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                seg_off, nseg, align, blocks, out, counts)
    _check(lib.gcl_l4_payload_host(ctypes.byref(b), ctypes.byref(pin), ctypes.byref(pout), _ptr(counts)),
           "gcl_l4_payload_host")
    return out


def l4_payload_workspace(m, blocks=0):
    """gcl_l4_payload_workspace: bytes of device scratch a call over @m entries takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_l4_payload_workspace(m, blocks, ctypes.byref(need)), "gcl_l4_payload_workspace")
    return need.value


def sock_entries(entries):
    """struct gcl_sock_entry[n] as a numpy record array (SOCK_ENTRY_DTYPE):
    @entries is such an array already, or a sequence of GclSockEntry, of dicts
    or of (lip, lport, proto, match, cookie[, rip, rport]) tuples."""
    if isinstance(entries, np.ndarray):
        if entries.dtype != SOCK_ENTRY_DTYPE:
            raise ValueError("entries: not SOCK_ENTRY_DTYPE")
        return np.ascontiguousarray(entries)
    out = np.zeros(len(entries), dtype=SOCK_ENTRY_DTYPE)
    for i, e in enumerate(entries):
        if isinstance(e, GclSockEntry):
            e = {f: getattr(e, f) for f, _ in GclSockEntry._fields_}
        elif not isinstance(e, dict):
            e = dict(zip(("lip", "lport", "proto", "match", "cookie", "rip", "rport"), e))
        for f, v in e.items():
            out[f][i] = v
    return out


class SockTable:
    """The host-only socket table (gcl_sock_tbl_*, include/gcl_host.h): the
    table of Classifier.sock_set / sock_lookup without a GPU."""

    def __init__(self, hash_bits=None):
        self._tbl = ctypes.c_void_p(lib.gcl_sock_tbl_new())
        if not self._tbl:
            raise MemoryError("gcl_sock_tbl_new")
        if hash_bits is not None:
            self.hash_bits(hash_bits)

    def close(self):
        if self._tbl:
            lib.gcl_sock_tbl_free(self._tbl)
            self._tbl = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hash_bits(self, bits):
        """The test knob: only the low @bits of the internal hash, from the next set on."""
        return _check(lib.gcl_sock_tbl_hash_bits(self._tbl, bits), "gcl_sock_tbl_hash_bits")

    def set(self, uniqid, entries):
        e = sock_entries(entries)
        return _check(lib.gcl_sock_tbl_set(self._tbl, uniqid, e.ctypes.data if len(e) else None, len(e)),
                      "gcl_sock_tbl_set")

    def delete(self, uniqid):
        return _check(lib.gcl_sock_tbl_del(self._tbl, uniqid), "gcl_sock_tbl_del")

    def lookup(self, frames, n, verdicts, vbytes, thread_bits=0, max_runtimes=GCL_MAX_PROC, stride=0,
               offs=None, frames_len=None, sock=None, counts=None):
        """gcl_sock_tbl_lookup_host over numpy arrays; returns (sock u32[n],
        counts u64[SOCK_NR]), @counts accumulated when given."""
        if _nbytes(verdicts) < vbytes * n or (offs is not None and _nbytes(offs) < 8 * n):
            raise ValueError("per-packet array too small")
        sock = np.empty(max(n, 1), dtype=np.uint32) if sock is None else sock
        counts = np.zeros(SOCK_NR, dtype=np.uint64) if counts is None else counts
        if _nbytes(sock) < 4 * n or _nbytes(counts) < 8 * SOCK_NR:
            raise ValueError("output buffer too small")
        b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), stride=stride,
                     offs=_ptr(offs), n=n)
        _check(lib.gcl_sock_tbl_lookup_host(self._tbl, vbytes, thread_bits, max_runtimes, ctypes.byref(b),
                                            _ptr(verdicts), _ptr(sock), _ptr(counts)),
               "gcl_sock_tbl_lookup_host")
        return sock[:n], counts


def neigh_entries(entries):
    """struct gcl_neigh_entry[n] as a numpy record array (NEIGH_ENTRY_DTYPE):
    @entries is such an array already, or a sequence of (ip, mac) pairs, mac
    six bytes."""
    if isinstance(entries, np.ndarray):
        if entries.dtype != NEIGH_ENTRY_DTYPE:
            raise ValueError("entries: not NEIGH_ENTRY_DTYPE")
        return np.ascontiguousarray(entries)
    out = np.zeros(len(entries), dtype=NEIGH_ENTRY_DTYPE)
    for i, (ip, mac) in enumerate(entries):
        out["ip"][i] = ip
        out["mac"][i] = np.frombuffer(bytes(mac), dtype=np.uint8)
    return out


class NeighTable:
    """The host-only neighbour table (gcl_neigh_tbl_*, include/gcl_host.h):
    the table of Classifier.neigh_set / tx_hdr without a GPU."""

    def __init__(self, hash_bits=None):
        self._tbl = ctypes.c_void_p(lib.gcl_neigh_tbl_new())
        if not self._tbl:
            raise MemoryError("gcl_neigh_tbl_new")
        if hash_bits is not None:
            self.hash_bits(hash_bits)

    def close(self):
        if self._tbl:
            lib.gcl_neigh_tbl_free(self._tbl)
            self._tbl = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hash_bits(self, bits):
        """The test knob: only the low @bits of the internal hash, from the next set on."""
        return _check(lib.gcl_neigh_tbl_hash_bits(self._tbl, bits), "gcl_neigh_tbl_hash_bits")

    def set(self, entries):
        e = neigh_entries(entries)
        return _check(lib.gcl_neigh_tbl_set(self._tbl, e.ctypes.data if len(e) else None, len(e)),
                      "gcl_neigh_tbl_set")

    def __len__(self):
        return lib.gcl_neigh_tbl_count(self._tbl)

    def lookup(self, ip):
        """The mac (six bytes) that answers for @ip, or None."""
        mac = (ctypes.c_uint8 * 6)()
        return bytes(mac) if _check(lib.gcl_neigh_tbl_lookup(self._tbl, ip, ctypes.byref(mac)),
                                    "gcl_neigh_tbl_lookup") else None


TXH_OUT_FIELDS = ("cmd", "payload", "pkt_len", "tx_olflags", "hash", "status")


def txh_net(addr, netmask, gateway, mac, min_pkt_size=0, flags=0):
    """struct gcl_txh_net: one runtime's netcfg (addresses in host order, @mac six bytes)."""
    return GclTxhNet(addr=addr, netmask=netmask, gateway=gateway, mac=(ctypes.c_uint8 * 6)(*bytes(mac)),
                     min_pkt_size=min_pkt_size, flags=flags)


def _txh_structs(desc, frame_off, m, frames, frames_len, shm_base, cap, net, out, counts):
    """The two structs of gcl_tx_hdr / gcl_tx_hdr_host, sizes checked; @out
    maps TXH_OUT_FIELDS to buffers (hash may be None)."""
    for arr, w in ((desc, 32), (frame_off, 8), (out["cmd"], 8), (out["payload"], 8), (out["pkt_len"], 2),
                   (out["tx_olflags"], 1), (out["hash"], 4), (out["status"], 1)):
        if arr is not None and _nbytes(arr) < w * m:
            raise ValueError("per-entry array too small")
    if counts is not None and _nbytes(counts) < 8 * TXHC_NR:
        raise ValueError("counts buffer too small")
    tin = GclTxhIn(size=ctypes.sizeof(GclTxhIn), desc=_ptr(desc), frame_off=_ptr(frame_off), m=m,
                   frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), shm_base=shm_base,
                   cap=cap, net=net)
    tout = GclTxhOut(**{f: _ptr(out[f]) for f in TXH_OUT_FIELDS})
    return tin, tout


def tx_hdr_host(desc, frame_off, frames, net, table=None, rss_key=None, m=None, frames_len=None,
                shm_base=0, cap=0, out=None, counts=None):
    """gcl_tx_hdr_host: the rule of Classifier.tx_hdr on the CPU over numpy
    arrays.  @desc is TXH_DESC_DTYPE[m], @frame_off u64[m], @frames a writable
    uint8 array, @net a txh_net(), @table a NeighTable (None: empty), @rss_key
    the 40-byte Toeplitz key (None: CALADAN_RSS_KEY).  @out maps
    TXH_OUT_FIELDS to arrays (u64, u64, u16, u8, u32, u8); the ones left out
    are allocated; hash=None in @out leaves it out.  @counts is a
    u64[TXHC_NR], accumulated.  Returns the dict."""
    m = len(desc) if m is None else m
    out = dict(out or {})
    for f, dt in (("cmd", np.uint64), ("payload", np.uint64), ("pkt_len", np.uint16),
                  ("tx_olflags", np.uint8), ("hash", np.uint32), ("status", np.uint8)):
        if f not in out:
            out[f] = np.zeros(max(m, 1), dtype=dt)
    tin, tout = _txh_structs(desc, frame_off, m, frames, frames_len, shm_base, cap, net, out, counts)
    key = CALADAN_RSS_KEY if rss_key is None else bytes(rss_key)
    if len(key) != 40:
        raise ValueError("rss_key: 40 bytes")
    _check(lib.gcl_tx_hdr_host(table._tbl if table is not None else None, key, ctypes.byref(tin),
                               ctypes.byref(tout), _ptr(counts)), "gcl_tx_hdr_host")
    return out


SEG_OUT_WIDTH = {"status": 1, "sent": 4, "snd_nxt_out": 4, "seg_first": 4, "nseg": 4, "desc": 32,
                 "frame_off": 8, "src_off": 8, "len": 2, "dst_off": 8, "send_idx": 4}


def _seg_structs(send, m, seg_cap, stride, lead, frame_base, frames_len, udp_max, blocks, out, counts):
    """The two structs of gcl_tx_seg / gcl_tx_seg_host, sizes checked; @out
    maps SEG_OUT_FIELDS to buffers (send_idx may be None)."""
    if send is not None and _nbytes(send) < 48 * m:
        raise ValueError("send array too small")
    for f in SEG_WRITE_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < SEG_OUT_WIDTH[f] * m:
            raise ValueError(f"{f}: per-write array too small")
    for f in SEG_SEG_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < SEG_OUT_WIDTH[f] * seg_cap:
            raise ValueError(f"{f}: per-segment array shorter than seg_cap")
    for f in ("total_segs", "total_bytes"):
        if out[f] is not None and _nbytes(out[f]) < 8:
            raise ValueError(f"{f} too small")
    if counts is not None and _nbytes(counts) < 8 * SEGC_NR:
        raise ValueError("counts buffer too small")
    sin = GclSegIn(size=ctypes.sizeof(GclSegIn), blocks=blocks, send=_ptr(send), m=m, seg_cap=seg_cap,
                   frame_base=frame_base, frames_len=frames_len, stride=stride, lead=lead, udp_max=udp_max)
    sout = GclSegOut(**{f: _ptr(out[f]) for f in SEG_OUT_FIELDS})
    return sin, sout


def tx_seg_host(send, seg_cap, stride=0, lead=0, frame_base=0, frames_len=0, udp_max=1472, m=None,
                blocks=0, out=None, counts=None):
    """gcl_tx_seg_host: the rule of Classifier.tx_seg on the CPU over numpy
    arrays.  @send is SEG_SEND_DTYPE[m]; @out maps SEG_OUT_FIELDS to arrays
    (per write u8, u32 x 4; per segment TXH_DESC_DTYPE, u64, u64, u16, u64,
    u32, each @seg_cap long; the totals u64[1]); the ones left out are
    allocated; send_idx=None in @out leaves it out.  @counts is a
    u64[SEGC_NR], accumulated.  Returns the dict."""
    m = len(send) if m is None else m
    out = dict(out or {})
    for f, dt, k in (("status", np.uint8, m), ("sent", np.uint32, m), ("snd_nxt_out", np.uint32, m),
                     ("seg_first", np.uint32, m), ("nseg", np.uint32, m), ("desc", TXH_DESC_DTYPE, seg_cap),
                     ("frame_off", np.uint64, seg_cap), ("src_off", np.uint64, seg_cap),
                     ("len", np.uint16, seg_cap), ("dst_off", np.uint64, seg_cap),
                     ("send_idx", np.uint32, seg_cap), ("total_segs", np.uint64, 1),
                     ("total_bytes", np.uint64, 1)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    sin, sout = _seg_structs(send, m, seg_cap, stride, lead, frame_base, frames_len, udp_max, blocks, out,
                             counts)
    _check(lib.gcl_tx_seg_host(ctypes.byref(sin), ctypes.byref(sout), _ptr(counts)), "gcl_tx_seg_host")
    return out


def tx_seg_workspace(m, blocks=0):
    """gcl_tx_seg_workspace: bytes of device scratch a call over @m writes takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tx_seg_workspace(m, blocks, ctypes.byref(need)), "gcl_tx_seg_workspace")
    return need.value


def _tcprx_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status, conn, nconn,
                   align, blocks, out, counts):
    """The three structs of gcl_tcp_rx / gcl_tcp_rx_host, sizes checked; @out
    maps TCPRX_OUT_FIELDS to buffers."""
    if sock is None:
        raise ValueError("sock is required")
    for arr, w in ((offs, 8), (pkt_len, 2), (sock, 4), (l4_status, 1)):
        if arr is not None and _nbytes(arr) < w * n:
            raise ValueError("per-packet array too small")
    for arr, w in ((order, 4), (out["verdict"], 1), (out["sflags"], 1), (out["rcv_nxt_after"], 4),
                   (out["copy_len"], 2), (out["dst_off"], 8)):
        if arr is not None and _nbytes(arr) < w * m:
            raise ValueError("per-entry array too small")
    for arr, w in ((conn, 48), (out["out_conn"], 48)):
        if arr is not None and _nbytes(arr) < w * nconn:
            raise ValueError("per-connection array too small")
    if out["conn_off"] is not None and _nbytes(out["conn_off"]) < 8 * (nconn + 1):
        raise ValueError("conn_off too small")
    if counts is not None and _nbytes(counts) < 8 * TCPRXC_NR:
        raise ValueError("counts buffer too small")
    b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), stride=stride,
                 offs=_ptr(offs), olflags=None, rss=None, fdir_hi=None, pkt_len=_ptr(pkt_len), n=n,
                 dst_hint=None)
    rin = GclTcprxIn(size=ctypes.sizeof(GclTcprxIn), align=align, order=_ptr(order), m=m, sock=_ptr(sock),
                     l4_status=_ptr(l4_status), conn=_ptr(conn), nconn=nconn, blocks=blocks)
    rout = GclTcprxOut(**{f: _ptr(out[f]) for f in TCPRX_OUT_FIELDS})
    return b, rin, rout


def tcp_rx_host(frames, pkt_len, sock, conn, stride=0, offs=None, n=None, frames_len=None, order=None,
                m=None, l4_status=None, nconn=None, align=0, blocks=0, out=None, counts=None):
    """gcl_tcp_rx_host: the rule of Classifier.tcp_rx on the CPU over numpy
    arrays.  @conn is a TCP_CONN_DTYPE array indexed by cookie.  @out maps
    TCPRX_OUT_FIELDS to arrays (u8, u8, u32, u16, u64, TCP_CONN_OUT_DTYPE,
    u64[nconn + 1]); the ones left out are allocated.  @counts is a
    u64[TCPRXC_NR], accumulated.  Returns the dict."""
    n = len(pkt_len) if n is None else n
    m = _pay_m(n, m, order)
    nconn = len(conn) if nconn is None else nconn
    out = dict(out or {})
    for f, dt, k in (("verdict", np.uint8, m), ("sflags", np.uint8, m), ("rcv_nxt_after", np.uint32, m),
                     ("copy_len", np.uint16, m), ("dst_off", np.uint64, m),
                     ("out_conn", TCP_CONN_OUT_DTYPE, nconn), ("conn_off", np.uint64, nconn + 1)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    b, rin, rout = _tcprx_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                  conn, nconn, align, blocks, out, counts)
    _check(lib.gcl_tcp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), _ptr(counts)),
           "gcl_tcp_rx_host")
    return out


def tcp_rx_workspace(m, nconn, blocks=0):
    """gcl_tcp_rx_workspace: bytes of device scratch a call over @m entries and @nconn connections takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_rx_workspace(m, nconn, blocks, ctypes.byref(need)), "gcl_tcp_rx_workspace")
    return need.value


def _tcprxf_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status, conn, nconn,
                    align, blocks, out, counts, rep_acks):
    """The three structs of gcl_tcp_rx_full / gcl_tcp_rx_full_host, sizes
    checked; @out maps TCPRX_OUT_FIELDS and "out_ext" to buffers."""
    if counts is not None and _nbytes(counts) < 8 * TCPRXFC_NR:
        raise ValueError("counts buffer too small")
    if rep_acks is not None and _nbytes(rep_acks) < nconn:
        raise ValueError("rep_acks too small")
    if out["out_ext"] is not None and _nbytes(out["out_ext"]) < 16 * nconn:
        raise ValueError("out_ext too small")
    b, rin, rout = _tcprx_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                  conn, nconn, align, blocks, out, None)
    fin = GclTcprxfIn(size=ctypes.sizeof(GclTcprxfIn), align=align, order=rin.order, m=m, sock=rin.sock,
                      l4_status=rin.l4_status, conn=rin.conn, nconn=nconn, blocks=blocks,
                      rep_acks=_ptr(rep_acks))
    return b, fin, rout


def tcp_rx_full_host(frames, pkt_len, sock, conn, stride=0, offs=None, n=None, frames_len=None, order=None,
                     m=None, l4_status=None, nconn=None, align=0, blocks=0, rep_acks=None, out=None,
                     counts=None):
    """gcl_tcp_rx_full_host: the rule of Classifier.tcp_rx_full on the CPU over
    numpy arrays: tcp_rx_host's arguments, @rep_acks (u8[nconn], None: zeros)
    and in @out also "out_ext" (TCP_CONN_EXT_DTYPE[nconn]).  @counts is a
    u64[TCPRXFC_NR], accumulated.  Returns the dict."""
    n = len(pkt_len) if n is None else n
    m = _pay_m(n, m, order)
    nconn = len(conn) if nconn is None else nconn
    out = dict(out or {})
    for f, dt, k in (("verdict", np.uint8, m), ("sflags", np.uint8, m), ("rcv_nxt_after", np.uint32, m),
                     ("copy_len", np.uint16, m), ("dst_off", np.uint64, m),
                     ("out_conn", TCP_CONN_OUT_DTYPE, nconn), ("conn_off", np.uint64, nconn + 1),
                     ("out_ext", TCP_CONN_EXT_DTYPE, nconn)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    b, fin, rout = _tcprxf_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                   conn, nconn, align, blocks, out, counts, rep_acks)
    _check(lib.gcl_tcp_rx_full_host(ctypes.byref(b), ctypes.byref(fin), ctypes.byref(rout), _ptr(out["out_ext"]),
                                    _ptr(counts)), "gcl_tcp_rx_full_host")
    return out


def tcp_rx_full_workspace(m, nconn, blocks=0):
    """gcl_tcp_rx_full_workspace: bytes of device scratch a call over @m entries and @nconn connections takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_rx_full_workspace(m, nconn, blocks, ctypes.byref(need)), "gcl_tcp_rx_full_workspace")
    return need.value


def _tcprxo_sizes(m, nconn, nq, q_out_cap):
    return {"m": m, "nq": nq, "nconn1": nconn + 1, "cap": q_out_cap, "one": 1}


def _tcprxo_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status, conn, nconn,
                    align, blocks, out, counts, rep_acks, q_off, q, nq, q_out_cap):
    """The four structs of gcl_tcp_rx_ooo / gcl_tcp_rx_ooo_host, sizes checked;
    @out maps TCPRX_OUT_FIELDS, "out_ext" and TCPRXO_OUT_FIELDS to buffers."""
    if counts is not None and _nbytes(counts) < 8 * TCPRXOC_NR:
        raise ValueError("counts buffer too small")
    if q_off is not None and _nbytes(q_off) < 4 * (nconn + 1):
        raise ValueError("q_off too small")
    if q is not None and _nbytes(q) < 16 * nq:
        raise ValueError("q too small")
    size = _tcprxo_sizes(m, nconn, nq, q_out_cap)
    for f, w, by in TCPRXO_OUT_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < w * size[by]:
            raise ValueError(f"{f} too small")
    b, fin, rout = _tcprxf_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                   conn, nconn, align, blocks, out, None, rep_acks)
    oin = GclTcprxoIn(size=ctypes.sizeof(GclTcprxoIn), align=align, order=fin.order, m=m, sock=fin.sock,
                      l4_status=fin.l4_status, conn=fin.conn, nconn=nconn, blocks=blocks, rep_acks=fin.rep_acks,
                      q_off=_ptr(q_off), q=_ptr(q), nq=nq, q_out_cap=q_out_cap)
    oout = GclTcprxoOut(**{f: _ptr(out[f]) for f, _, _ in TCPRXO_OUT_FIELDS})
    return b, oin, rout, oout


def tcp_rx_ooo_host(frames, pkt_len, sock, conn, stride=0, offs=None, n=None, frames_len=None, order=None,
                    m=None, l4_status=None, nconn=None, align=0, blocks=0, rep_acks=None, q_off=None, q=None,
                    nq=None, q_out_cap=0, out=None, counts=None):
    """gcl_tcp_rx_ooo_host: the rule of Classifier.tcp_rx_ooo on the CPU over
    numpy arrays: tcp_rx_full_host's arguments, the input queues (@q_off
    u32[nconn + 1] or None, @q TCP_OOO_ENT_DTYPE[nq]) and @q_out_cap; in @out
    also the fields of TCPRXO_OUT_FIELDS.  @counts is a u64[TCPRXOC_NR],
    accumulated.  Returns the dict."""
    n = len(pkt_len) if n is None else n
    m = _pay_m(n, m, order)
    nconn = len(conn) if nconn is None else nconn
    nq = (0 if q is None else len(q)) if nq is None else nq
    out = dict(out or {})
    size = _tcprxo_sizes(m, nconn, nq, q_out_cap)
    for f, dt, k in (("verdict", np.uint8, m), ("sflags", np.uint8, m), ("rcv_nxt_after", np.uint32, m),
                     ("copy_len", np.uint16, m), ("dst_off", np.uint64, m),
                     ("out_conn", TCP_CONN_OUT_DTYPE, nconn), ("conn_off", np.uint64, nconn + 1),
                     ("out_ext", TCP_CONN_EXT_DTYPE, nconn)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    for f, w, by in TCPRXO_OUT_FIELDS:
        if f not in out:
            out[f] = np.zeros(max(size[by], 1), dtype=TCP_OOO_ENT_DTYPE if f == "qout" else f"<u{w}")
    b, oin, rout, oout = _tcprxo_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                         conn, nconn, align, blocks, out, counts, rep_acks, q_off, q, nq,
                                         q_out_cap)
    _check(lib.gcl_tcp_rx_ooo_host(ctypes.byref(b), ctypes.byref(oin), ctypes.byref(rout), _ptr(out["out_ext"]),
                                   ctypes.byref(oout), _ptr(counts)), "gcl_tcp_rx_ooo_host")
    return out


def tcp_rx_ooo_workspace(m, nconn, blocks=0, nq=0):
    """gcl_tcp_rx_ooo_workspace: bytes of device scratch a call over @m entries, @nconn connections and @nq input queue entries takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_rx_ooo_workspace(m, nconn, blocks, nq, ctypes.byref(need)), "gcl_tcp_rx_ooo_workspace")
    return need.value


def _tcprxs_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status, conn, nconn,
                    align, blocks, out, counts, rep_acks, q_off, q, nq, q_out_cap, state):
    """The five structs of gcl_tcp_rx_states / gcl_tcp_rx_states_host, sizes
    checked; @out maps TCPRX_OUT_FIELDS, "out_ext", TCPRXO_OUT_FIELDS and
    TCPRXS_OUT_FIELDS to buffers."""
    if counts is not None and _nbytes(counts) < 8 * TCPRXSC_NR:
        raise ValueError("counts buffer too small")
    if state is not None and _nbytes(state) < nconn:
        raise ValueError("state too small")
    size = {"m": m, "nconn": nconn}
    for f, w, by in TCPRXS_OUT_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < w * size[by]:
            raise ValueError(f"{f} too small")
    b, oin, rout, oout = _tcprxo_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                         conn, nconn, align, blocks, out, None, rep_acks, q_off, q, nq, q_out_cap)
    sin = GclTcprxsIn(size=ctypes.sizeof(GclTcprxsIn), align=align, order=oin.order, m=m, sock=oin.sock,
                      l4_status=oin.l4_status, conn=oin.conn, nconn=nconn, blocks=blocks, rep_acks=oin.rep_acks,
                      q_off=oin.q_off, q=oin.q, nq=nq, q_out_cap=q_out_cap, state=_ptr(state))
    sout = GclTcprxsOut(**{f: _ptr(out[f]) for f, _, _ in TCPRXS_OUT_FIELDS})
    return b, sin, rout, oout, sout


def tcp_rx_states_host(frames, pkt_len, sock, conn, stride=0, offs=None, n=None, frames_len=None, order=None,
                       m=None, l4_status=None, nconn=None, align=0, blocks=0, rep_acks=None, q_off=None, q=None,
                       nq=None, q_out_cap=0, state=None, out=None, counts=None):
    """gcl_tcp_rx_states_host: the rule of Classifier.tcp_rx_states on the CPU
    over numpy arrays: tcp_rx_ooo_host's arguments and @state (u8[nconn] of
    TCP_STATE_*, None: the connections' flags decide); in @out also the fields
    of TCPRXS_OUT_FIELDS.  @counts is a u64[TCPRXSC_NR], accumulated.  Returns
    the dict."""
    n = len(pkt_len) if n is None else n
    m = _pay_m(n, m, order)
    nconn = len(conn) if nconn is None else nconn
    nq = (0 if q is None else len(q)) if nq is None else nq
    out = dict(out or {})
    size = _tcprxo_sizes(m, nconn, nq, q_out_cap)
    size["nconn"] = nconn
    for f, dt, k in (("verdict", np.uint8, m), ("sflags", np.uint8, m), ("rcv_nxt_after", np.uint32, m),
                     ("copy_len", np.uint16, m), ("dst_off", np.uint64, m),
                     ("out_conn", TCP_CONN_OUT_DTYPE, nconn), ("conn_off", np.uint64, nconn + 1),
                     ("out_ext", TCP_CONN_EXT_DTYPE, nconn)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    for f, w, by in TCPRXO_OUT_FIELDS + TCPRXS_OUT_FIELDS:
        if f not in out:
            out[f] = np.zeros(max(size[by], 1), dtype=TCP_OOO_ENT_DTYPE if f == "qout" else f"<u{w}")
    b, sin, rout, oout, sout = _tcprxs_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                               l4_status, conn, nconn, align, blocks, out, counts, rep_acks, q_off,
                                               q, nq, q_out_cap, state)
    _check(lib.gcl_tcp_rx_states_host(ctypes.byref(b), ctypes.byref(sin), ctypes.byref(rout), _ptr(out["out_ext"]),
                                      ctypes.byref(oout), ctypes.byref(sout), _ptr(counts)),
           "gcl_tcp_rx_states_host")
    return out


def tcp_rx_states_workspace(m, nconn, blocks=0, nq=0):
    """gcl_tcp_rx_states_workspace: bytes of device scratch a call over @m entries, @nconn connections and @nq input queue entries takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_rx_states_workspace(m, nconn, blocks, nq, ctypes.byref(need)), "gcl_tcp_rx_states_workspace")
    return need.value


CTLSEG_OUT_WIDTH = {"desc": 32, "frame_off": 8, "seg_conn": 4, "seg_kind": 1, "seg_src": 4}


def _ctlseg_struct(seg_cap, out, counts):
    """struct gcl_ctlseg_out of @out (CTLSEG_OUT_FIELDS to buffers), sizes checked"""
    for f in CTLSEG_SEG_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < CTLSEG_OUT_WIDTH[f] * seg_cap:
            raise ValueError(f"{f}: per-segment array shorter than seg_cap")
    if out["totals"] is not None and _nbytes(out["totals"]) < 16:
        raise ValueError("totals too small")
    if counts is not None and _nbytes(counts) < 8 * TICKC_NR:
        raise ValueError("counts buffer too small")
    return GclCtlsegOut(**{f: _ptr(out[f]) for f in CTLSEG_OUT_FIELDS})


def _tick_structs(now, tmr, conn, addr, nconn, seg_cap, frame_base, frame_stride, blocks, out, counts):
    """The two structs of gcl_tcp_tick / gcl_tcp_tick_host, sizes checked; @out
    maps TICK_OUT_FIELDS to buffers."""
    for arr, w in ((tmr, 64), (conn, 48), (addr, 16), (out["out_tmr"], 32)):
        if arr is not None and _nbytes(arr) < w * nconn:
            raise ValueError("per-connection array too small")
    tin = GclTickIn(size=ctypes.sizeof(GclTickIn), blocks=blocks, now=now, tmr=_ptr(tmr), conn=_ptr(conn),
                    addr=_ptr(addr), nconn=nconn, frame_stride=frame_stride, seg_cap=seg_cap,
                    frame_base=frame_base)
    tout = GclTickOut(out_tmr=_ptr(out["out_tmr"]), seg=_ctlseg_struct(seg_cap, out, counts))
    return tin, tout


def _rxack_structs(verdict, sflags, rcv_nxt_after, sock, conn, addr, m, n, nconn, order, seg_cap, frame_base,
                   frame_stride, blocks, out, counts):
    """The two structs of gcl_tcp_rx_acks / gcl_tcp_rx_acks_host, sizes checked;
    @out maps CTLSEG_OUT_FIELDS to buffers."""
    for arr, w in ((order, 4), (verdict, 1), (sflags, 1), (rcv_nxt_after, 4)):
        if arr is not None and _nbytes(arr) < w * m:
            raise ValueError("per-entry array too small")
    if sock is not None and _nbytes(sock) < 4 * n:
        raise ValueError("sock too small")
    for arr, w in ((conn, 48), (addr, 16)):
        if arr is not None and _nbytes(arr) < w * nconn:
            raise ValueError("per-connection array too small")
    rin = GclRxackIn(size=ctypes.sizeof(GclRxackIn), blocks=blocks, order=_ptr(order), m=m, n=n, sock=_ptr(sock),
                     verdict=_ptr(verdict), sflags=_ptr(sflags), rcv_nxt_after=_ptr(rcv_nxt_after),
                     conn=_ptr(conn), addr=_ptr(addr), nconn=nconn, frame_stride=frame_stride, seg_cap=seg_cap,
                     frame_base=frame_base)
    return rin, _ctlseg_struct(seg_cap, out, counts)


def _ctlseg_host_arrays(out, seg_cap):
    for f, dt in (("desc", TXH_DESC_DTYPE), ("frame_off", np.uint64), ("seg_conn", np.uint32),
                  ("seg_kind", np.uint8), ("seg_src", np.uint32)):
        if f not in out:
            out[f] = np.zeros(max(seg_cap, 1), dtype=dt)
    if "totals" not in out:
        out["totals"] = np.zeros(2, dtype=np.uint64)


def tcp_tick_host(now, tmr, conn, addr, seg_cap, frame_stride=64, frame_base=0, nconn=None, blocks=0, out=None,
                  counts=None):
    """gcl_tcp_tick_host: the rule of Classifier.tcp_tick on the CPU over
    numpy arrays.  @tmr, @conn and @addr are TCP_TMR_DTYPE, TCP_CONN_DTYPE and
    TCP_ADDR_DTYPE arrays indexed by cookie.  @out maps TICK_OUT_FIELDS to
    arrays (TCP_TMR_OUT_DTYPE[nconn]; per segment TXH_DESC_DTYPE, u64, u32, u8,
    u32, each @seg_cap long; totals u64[2]); the ones left out are allocated.
    @counts is a u64[TICKC_NR], accumulated.  Returns the dict."""
    nconn = len(tmr) if nconn is None else nconn
    out = dict(out or {})
    if "out_tmr" not in out:
        out["out_tmr"] = np.zeros(max(nconn, 1), dtype=TCP_TMR_OUT_DTYPE)
    _ctlseg_host_arrays(out, seg_cap)
    tin, tout = _tick_structs(now, tmr, conn, addr, nconn, seg_cap, frame_base, frame_stride, blocks, out, counts)
    _check(lib.gcl_tcp_tick_host(ctypes.byref(tin), ctypes.byref(tout), _ptr(counts)), "gcl_tcp_tick_host")
    return out


def tcp_rx_acks_host(verdict, sflags, rcv_nxt_after, sock, conn, addr, seg_cap, frame_stride=64, frame_base=0,
                     order=None, m=None, n=None, nconn=None, blocks=0, out=None, counts=None):
    """gcl_tcp_rx_acks_host: the rule of Classifier.tcp_rx_acks on the CPU over
    numpy arrays: @verdict, @sflags and @rcv_nxt_after as tcp_rx_host wrote
    them, @sock, @order, @conn as it was given them.  @out maps
    CTLSEG_OUT_FIELDS to arrays; the ones left out are allocated.  @counts is a
    u64[TICKC_NR], accumulated (RXACKC_* slots).  Returns the dict."""
    m = len(verdict) if m is None else m
    n = len(sock) if n is None else n
    nconn = len(conn) if nconn is None else nconn
    out = dict(out or {})
    _ctlseg_host_arrays(out, seg_cap)
    rin, rout = _rxack_structs(verdict, sflags, rcv_nxt_after, sock, conn, addr, m, n, nconn, order, seg_cap,
                               frame_base, frame_stride, blocks, out, counts)
    _check(lib.gcl_tcp_rx_acks_host(ctypes.byref(rin), ctypes.byref(rout), _ptr(counts)), "gcl_tcp_rx_acks_host")
    return out


def _rxctl_structs(verdict, sflags, rcv_nxt_after, ev, rst_seq, sock, conn, addr, m, n, nconn, order, seg_cap,
                   frame_base, frame_stride, blocks, out, counts):
    """The two structs of gcl_tcp_rx_ctl / gcl_tcp_rx_ctl_host, sizes checked"""
    for arr, w in ((ev, 1), (rst_seq, 4)):
        if arr is not None and _nbytes(arr) < w * m:
            raise ValueError("per-entry array too small")
    rin, rout = _rxack_structs(verdict, sflags, rcv_nxt_after, sock, conn, addr, m, n, nconn, order, seg_cap,
                               frame_base, frame_stride, blocks, out, counts)
    cin = GclRxctlIn(**{f: getattr(rin, f) for f, _ in GclRxackIn._fields_})
    cin.size, cin.ev, cin.rst_seq = ctypes.sizeof(GclRxctlIn), _ptr(ev), _ptr(rst_seq)
    return cin, rout


def tcp_rx_ctl_host(verdict, sflags, rcv_nxt_after, ev, rst_seq, sock, conn, addr, seg_cap, frame_stride=64,
                    frame_base=0, order=None, m=None, n=None, nconn=None, blocks=0, out=None, counts=None):
    """gcl_tcp_rx_ctl_host: the rule of Classifier.tcp_rx_ctl on the CPU over
    numpy arrays: tcp_rx_acks_host's arguments and @ev and @rst_seq as
    tcp_rx_states_host wrote them.  Returns the dict; seg_kind also holds
    CTL_RST and CTL_RST_ACK."""
    m = len(verdict) if m is None else m
    n = len(sock) if n is None else n
    nconn = len(conn) if nconn is None else nconn
    out = dict(out or {})
    _ctlseg_host_arrays(out, seg_cap)
    cin, rout = _rxctl_structs(verdict, sflags, rcv_nxt_after, ev, rst_seq, sock, conn, addr, m, n, nconn, order,
                               seg_cap, frame_base, frame_stride, blocks, out, counts)
    _check(lib.gcl_tcp_rx_ctl_host(ctypes.byref(cin), ctypes.byref(rout), _ptr(counts)), "gcl_tcp_rx_ctl_host")
    return out


def tcp_rx_ctl_workspace(m, blocks=0):
    """gcl_tcp_rx_ctl_workspace: bytes of device scratch a call over @m list entries takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_rx_ctl_workspace(m, blocks, ctypes.byref(need)), "gcl_tcp_rx_ctl_workspace")
    return need.value


def _tcpopen_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status, listen, nlisten,
                     listen_base, iss, seg_cap, open_cap, frame_base, frame_stride, tx_frames, tx_frames_len,
                     blocks, hash_slots, out, counts):
    """The four structs of gcl_tcp_rx_open / gcl_tcp_rx_open_host, sizes
    checked; @out maps TCPOPEN_OUT_FIELDS and CTLSEG_SEG_FIELDS to buffers and
    "seg_totals" to the segments' totals."""
    for arr, w in ((order, 4), (iss, 4), (out["verdict"], 1), (out["later_of"], 4), (out["rst_seq"], 4)):
        if arr is not None and _nbytes(arr) < w * m:
            raise ValueError("per-entry array too small")
    for arr, w in ((sock, 4), (l4_status, 1), (pkt_len, 2)):
        if arr is not None and _nbytes(arr) < w * n:
            raise ValueError("per-packet array too small")
    for arr, w in ((listen, 16), (out["backlog_out"], 4)):
        if arr is not None and _nbytes(arr) < w * nlisten:
            raise ValueError("per-listener array too small")
    if out["open"] is not None and _nbytes(out["open"]) < 64 * open_cap:
        raise ValueError("open shorter than open_cap")
    for f in CTLSEG_SEG_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < CTLSEG_OUT_WIDTH[f] * seg_cap:
            raise ValueError(f"{f}: per-segment array shorter than seg_cap")
    for f in ("totals", "seg_totals"):
        if out[f] is not None and _nbytes(out[f]) < 16:
            raise ValueError("totals too small")
    if counts is not None and _nbytes(counts) < 8 * OPENC_NR:
        raise ValueError("counts buffer too small")
    tx_frames_len = (0 if tx_frames is None else _nbytes(tx_frames)) if tx_frames_len is None else tx_frames_len
    if tx_frames is not None and _nbytes(tx_frames) < tx_frames_len:
        raise ValueError("tx_frames shorter than tx_frames_len")
    b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), stride=stride,
                 offs=_ptr(offs), olflags=None, rss=None, fdir_hi=None, pkt_len=_ptr(pkt_len), n=n,
                 dst_hint=None)
    oin = GclTcpopenIn(size=ctypes.sizeof(GclTcpopenIn), blocks=blocks, order=_ptr(order), m=m, sock=_ptr(sock),
                       l4_status=_ptr(l4_status), hash_slots=hash_slots, listen_base=listen_base, nlisten=nlisten,
                       frame_stride=frame_stride, listen=_ptr(listen), iss=_ptr(iss), seg_cap=seg_cap,
                       frame_base=frame_base, open_cap=open_cap, tx_frames=_ptr(tx_frames),
                       tx_frames_len=tx_frames_len)
    oout = GclTcpopenOut(**{f: _ptr(out[f]) for f in TCPOPEN_OUT_FIELDS})
    seg = GclCtlsegOut(**{f: _ptr(out[f]) for f in CTLSEG_SEG_FIELDS}, totals=_ptr(out["seg_totals"]))
    return b, oin, oout, seg


def tcp_rx_open_host(frames, pkt_len, sock, listen, iss, seg_cap, open_cap, tx_frames, stride=0, offs=None, n=None,
                     frames_len=None, order=None, m=None, l4_status=None, nlisten=None, listen_base=0,
                     frame_stride=64, frame_base=0, tx_frames_len=None, blocks=0, hash_slots=0, out=None,
                     counts=None):
    """gcl_tcp_rx_open_host: the rule of Classifier.tcp_rx_open on the CPU over
    numpy arrays.  @listen is a TCP_LISTEN_DTYPE array, cookie listen_base + l
    naming listen[l]; @iss a u32[m]; @tx_frames the uint8 tx region, written in
    place (the option bytes of the SYN|ACKs).  @out maps TCPOPEN_OUT_FIELDS
    (u8[m], u32[m], u32[m], TCP_OPEN_DTYPE[open_cap], u32[nlisten], u64[2]),
    CTLSEG_SEG_FIELDS (each @seg_cap long) and "seg_totals" (u64[2]) to arrays;
    the ones left out are allocated.  @counts is a u64[OPENC_NR], accumulated.
    Returns the dict."""
    n = len(pkt_len) if n is None else n
    m = _pay_m(n, m, order)
    nlisten = len(listen) if nlisten is None else nlisten
    out = dict(out or {})
    for f, dt, k in (("verdict", np.uint8, m), ("later_of", np.uint32, m), ("rst_seq", np.uint32, m),
                     ("open", TCP_OPEN_DTYPE, open_cap), ("backlog_out", np.uint32, nlisten),
                     ("totals", np.uint64, 2), ("seg_totals", np.uint64, 2), ("desc", TXH_DESC_DTYPE, seg_cap),
                     ("frame_off", np.uint64, seg_cap), ("seg_conn", np.uint32, seg_cap),
                     ("seg_kind", np.uint8, seg_cap), ("seg_src", np.uint32, seg_cap)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    b, oin, oout, seg = _tcpopen_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                         listen, nlisten, listen_base, iss, seg_cap, open_cap, frame_base,
                                         frame_stride, tx_frames, tx_frames_len, blocks, hash_slots, out, counts)
    _check(lib.gcl_tcp_rx_open_host(ctypes.byref(b), ctypes.byref(oin), ctypes.byref(oout), ctypes.byref(seg),
                                    _ptr(counts)), "gcl_tcp_rx_open_host")
    return out


def tcp_rx_open_workspace(m, nlisten, blocks=0, hash_slots=0):
    """gcl_tcp_rx_open_workspace: bytes of device scratch a call over @m list entries and @nlisten listeners takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_rx_open_workspace(m, nlisten, blocks, hash_slots, ctypes.byref(need)),
           "gcl_tcp_rx_open_workspace")
    return need.value


def _udprx_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status, usock, nsock,
                   sock_base, align, blocks, out, counts):
    """The three structs of gcl_udp_rx / gcl_udp_rx_host, sizes checked; @out
    maps UDPRX_OUT_FIELDS to buffers."""
    if sock is None:
        raise ValueError("sock is required")
    for arr, w in ((offs, 8), (pkt_len, 2), (sock, 4), (l4_status, 1)):
        if arr is not None and _nbytes(arr) < w * n:
            raise ValueError("per-packet array too small")
    for arr, w in ((order, 4), (out["verdict"], 1), (out["sflags"], 1), (out["copy_len"], 2),
                   (out["dst_off"], 8), (out["rec_idx"], 4), (out["rec"], 16)):
        if arr is not None and _nbytes(arr) < w * m:
            raise ValueError("per-entry array too small")
    for arr, w in ((usock, 16), (out["out_sock"], 16)):
        if arr is not None and _nbytes(arr) < w * nsock:
            raise ValueError("per-socket array too small")
    for f, w in (("rec_off", 4), ("sock_off", 8)):
        if out[f] is not None and _nbytes(out[f]) < w * (nsock + 1):
            raise ValueError(f + " too small")
    if counts is not None and _nbytes(counts) < 8 * UDPRXC_NR:
        raise ValueError("counts buffer too small")
    b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), stride=stride,
                 offs=_ptr(offs), olflags=None, rss=None, fdir_hi=None, pkt_len=_ptr(pkt_len), n=n,
                 dst_hint=None)
    rin = GclUdprxIn(size=ctypes.sizeof(GclUdprxIn), align=align, order=_ptr(order), m=m, sock=_ptr(sock),
                     l4_status=_ptr(l4_status), usock=_ptr(usock), nsock=nsock, sock_base=sock_base,
                     blocks=blocks, pad=0)
    rout = GclUdprxOut(**{f: _ptr(out[f]) for f in UDPRX_OUT_FIELDS})
    return b, rin, rout


def udp_rx_host(frames, pkt_len, sock, usock, stride=0, offs=None, n=None, frames_len=None, order=None,
                m=None, l4_status=None, nsock=None, sock_base=0, align=0, blocks=0, out=None, counts=None):
    """gcl_udp_rx_host: the rule of Classifier.udp_rx on the CPU over numpy
    arrays.  @usock is a UDP_SOCK_DTYPE array; cookie c names
    usock[c - sock_base].  @out maps UDPRX_OUT_FIELDS to arrays (u8, u8, u16,
    u64, u32, UDP_REC_DTYPE[m], UDP_SOCK_OUT_DTYPE[nsock], u32[nsock + 1],
    u64[nsock + 1]); the ones left out are allocated.  @counts is a
    u64[UDPRXC_NR], accumulated.  Returns the dict."""
    n = len(pkt_len) if n is None else n
    m = _pay_m(n, m, order)
    nsock = len(usock) if nsock is None else nsock
    out = dict(out or {})
    for f, dt, k in (("verdict", np.uint8, m), ("sflags", np.uint8, m), ("copy_len", np.uint16, m),
                     ("dst_off", np.uint64, m), ("rec_idx", np.uint32, m), ("rec", UDP_REC_DTYPE, m),
                     ("out_sock", UDP_SOCK_OUT_DTYPE, nsock), ("rec_off", np.uint32, nsock + 1),
                     ("sock_off", np.uint64, nsock + 1)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    b, rin, rout = _udprx_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock, l4_status,
                                  usock, nsock, sock_base, align, blocks, out, counts)
    _check(lib.gcl_udp_rx_host(ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), _ptr(counts)),
           "gcl_udp_rx_host")
    return out


def udp_rx_workspace(m, nsock, blocks=0):
    """gcl_udp_rx_workspace: bytes of device scratch a call over @m entries and @nsock sockets takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_udp_rx_workspace(m, nsock, blocks, ctypes.byref(need)), "gcl_udp_rx_workspace")
    return need.value


def tcp_tick_workspace(nconn, blocks=0):
    """gcl_tcp_tick_workspace: bytes of device scratch a sweep of @nconn connections takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_tick_workspace(nconn, blocks, ctypes.byref(need)), "gcl_tcp_tick_workspace")
    return need.value


def tcp_rx_acks_workspace(m, blocks=0):
    """gcl_tcp_rx_acks_workspace: bytes of device scratch a call over @m list entries takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_rx_acks_workspace(m, blocks, ctypes.byref(need)), "gcl_tcp_rx_acks_workspace")
    return need.value


TXQ_OUT_WIDTH = {"desc": 32, "frame_off": 8, "src_off": 8, "len": 2, "dst_off": 8, "seg_conn": 4, "seg_ent": 4}


def _txq_structs(now, qoff, ent, cold, nent, conn, addr, want, nconn, seg_cap, frame_base, frame_stride, blocks,
                 out, counts):
    """The two structs of gcl_tcp_txq / gcl_tcp_txq_host, sizes checked; @out
    maps TXQ_OUT_FIELDS to buffers."""
    if qoff is not None and _nbytes(qoff) < 4 * (nconn + 1):
        raise ValueError("qoff shorter than nconn + 1")
    for arr, w in ((conn, 48), (addr, 16), (want, 1), (out["out_conn"], 32)):
        if arr is not None and _nbytes(arr) < w * nconn:
            raise ValueError("per-connection array too small")
    for arr, w in ((ent, 16), (cold, 16), (out["state"], 1)):
        if arr is not None and _nbytes(arr) < w * nent:
            raise ValueError("per-entry array too small")
    for f in TXQ_SEG_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < TXQ_OUT_WIDTH[f] * seg_cap:
            raise ValueError(f"{f}: per-segment array shorter than seg_cap")
    if out["totals"] is not None and _nbytes(out["totals"]) < 24:
        raise ValueError("totals too small")
    if counts is not None and _nbytes(counts) < 8 * TXQC_NR:
        raise ValueError("counts buffer too small")
    qin = GclTxqIn(size=ctypes.sizeof(GclTxqIn), blocks=blocks, now=now, qoff=_ptr(qoff), ent=_ptr(ent),
                   cold=_ptr(cold), nent=nent, conn=_ptr(conn), addr=_ptr(addr), want=_ptr(want), nconn=nconn,
                   frame_stride=frame_stride, seg_cap=seg_cap, frame_base=frame_base)
    return qin, GclTxqOut(**{f: _ptr(out[f]) for f in TXQ_OUT_FIELDS})


def tcp_txq_host(now, qoff, ent, cold, conn, addr, seg_cap, want=None, frame_stride=64, frame_base=0, nconn=None,
                 nent=None, blocks=0, out=None, counts=None):
    """gcl_tcp_txq_host: the rule of Classifier.tcp_txq on the CPU over numpy
    arrays.  @qoff is a u32[nconn + 1] CSR over the TXQ_ENT_DTYPE / TXQ_COLD_DTYPE
    arrays @ent and @cold; @conn and @addr are TCP_CONN_DTYPE and TCP_ADDR_DTYPE
    arrays indexed by cookie, @want an optional u8[nconn] of TXQ_W_* bits.  @out
    maps TXQ_OUT_FIELDS to arrays (TXQ_CONN_OUT_DTYPE[nconn], u8[nent]; per
    segment TXH_DESC_DTYPE, u64, u64, u16, u64, u32, u32, each @seg_cap long;
    totals u64[3]); the ones left out are allocated.  @counts is a
    u64[TXQC_NR], accumulated.  Returns the dict."""
    nconn = len(conn) if nconn is None else nconn
    nent = len(ent) if nent is None else nent
    out = dict(out or {})
    for f, dt, k in (("out_conn", TXQ_CONN_OUT_DTYPE, nconn), ("state", np.uint8, nent),
                     ("desc", TXH_DESC_DTYPE, seg_cap), ("frame_off", np.uint64, seg_cap),
                     ("src_off", np.uint64, seg_cap), ("len", np.uint16, seg_cap), ("dst_off", np.uint64, seg_cap),
                     ("seg_conn", np.uint32, seg_cap), ("seg_ent", np.uint32, seg_cap), ("totals", np.uint64, 3)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    qin, qout = _txq_structs(now, qoff, ent, cold, nent, conn, addr, want, nconn, seg_cap, frame_base, frame_stride,
                             blocks, out, counts)
    _check(lib.gcl_tcp_txq_host(ctypes.byref(qin), ctypes.byref(qout), _ptr(counts)), "gcl_tcp_txq_host")
    return out


def tcp_txq_workspace(nconn, blocks=0):
    """gcl_tcp_txq_workspace: bytes of device scratch a call over @nconn connections takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_txq_workspace(nconn, blocks, ctypes.byref(need)), "gcl_tcp_txq_workspace")
    return need.value


RD_OUT_WIDTH = {"src_off": 8, "len": 2, "dst_off": 8, "item_conn": 4, "item_ent": 4}


def _rd_structs(qoff, ent, nent, voff, iov, nvec, rd, conn, addr, nconn, item_cap, seg_cap, frame_base,
                frame_stride, blocks, out, counts):
    """The two structs of gcl_tcp_read / gcl_tcp_read_host, sizes checked; @out
    maps RD_OUT_FIELDS to buffers."""
    for arr in (qoff, voff):
        if arr is not None and _nbytes(arr) < 4 * (nconn + 1):
            raise ValueError("qoff or voff shorter than nconn + 1")
    for arr, w in ((rd, 32), (conn, 48), (addr, 16), (out["out_conn"], 32)):
        if arr is not None and _nbytes(arr) < w * nconn:
            raise ValueError("per-connection array too small")
    if ent is not None and _nbytes(ent) < 16 * nent:
        raise ValueError("ent shorter than nent")
    if voff is not None and iov is not None and _nbytes(iov) < 16 * nvec:
        raise ValueError("iov shorter than nvec")
    for f in RD_ITEM_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < RD_OUT_WIDTH[f] * item_cap:
            raise ValueError(f"{f}: per-item array shorter than item_cap")
    for f in CTLSEG_SEG_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < CTLSEG_OUT_WIDTH[f] * seg_cap:
            raise ValueError(f"{f}: per-segment array shorter than seg_cap")
    if out["totals"] is not None and _nbytes(out["totals"]) < 32:
        raise ValueError("totals too small")
    if out["seg_totals"] is not None and _nbytes(out["seg_totals"]) < 16:
        raise ValueError("seg_totals too small")
    if counts is not None and _nbytes(counts) < 8 * RDC_NR:
        raise ValueError("counts buffer too small")
    rin = GclRdIn(size=ctypes.sizeof(GclRdIn), blocks=blocks, qoff=_ptr(qoff), ent=_ptr(ent), nent=nent,
                  voff=_ptr(voff), iov=_ptr(iov), nvec=nvec, rd=_ptr(rd), conn=_ptr(conn), addr=_ptr(addr),
                  nconn=nconn, frame_stride=frame_stride, item_cap=item_cap, seg_cap=seg_cap,
                  frame_base=frame_base)
    seg = GclCtlsegOut(**{f: _ptr(out[f]) for f in CTLSEG_SEG_FIELDS}, totals=_ptr(out["seg_totals"]))
    return rin, GclRdOut(**{f: _ptr(out[f]) for f in ("out_conn",) + RD_ITEM_FIELDS + ("totals",)}, seg=seg)


def tcp_read_host(qoff, ent, rd, conn, addr, item_cap, seg_cap, voff=None, iov=None, frame_stride=64,
                  frame_base=0, nconn=None, nent=None, nvec=None, blocks=0, out=None, counts=None):
    """gcl_tcp_read_host: the rule of Classifier.tcp_read on the CPU over numpy
    arrays.  @qoff is a u32[nconn + 1] CSR over the RDQ_ENT_DTYPE array @ent,
    @voff an optional one over the RD_IOV_DTYPE array @iov; @rd, @conn and
    @addr are TCP_RD_DTYPE, TCP_CONN_DTYPE and TCP_ADDR_DTYPE arrays indexed by
    cookie.  @out maps RD_OUT_FIELDS to arrays (RD_CONN_OUT_DTYPE[nconn]; per
    item u64, u16, u64, u32, u32, each @item_cap long; totals u64[4]; per
    segment TXH_DESC_DTYPE, u64, u32, u8, u32, each @seg_cap long; seg_totals
    u64[2]); the ones left out are allocated.  @counts is a u64[RDC_NR],
    accumulated.  Returns the dict."""
    nconn = len(rd) if nconn is None else nconn
    nent = len(ent) if nent is None else nent
    nvec = (len(iov) if iov is not None else 0) if nvec is None else nvec
    out = dict(out or {})
    for f, dt, k in (("out_conn", RD_CONN_OUT_DTYPE, nconn), ("src_off", np.uint64, item_cap),
                     ("len", np.uint16, item_cap), ("dst_off", np.uint64, item_cap),
                     ("item_conn", np.uint32, item_cap), ("item_ent", np.uint32, item_cap), ("totals", np.uint64, 4),
                     ("desc", TXH_DESC_DTYPE, seg_cap), ("frame_off", np.uint64, seg_cap),
                     ("seg_conn", np.uint32, seg_cap), ("seg_kind", np.uint8, seg_cap),
                     ("seg_src", np.uint32, seg_cap), ("seg_totals", np.uint64, 2)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    rin, rout = _rd_structs(qoff, ent, nent, voff, iov, nvec, rd, conn, addr, nconn, item_cap, seg_cap, frame_base,
                            frame_stride, blocks, out, counts)
    _check(lib.gcl_tcp_read_host(ctypes.byref(rin), ctypes.byref(rout), _ptr(counts)), "gcl_tcp_read_host")
    return out


def tcp_read_workspace(nconn, nent, nvec=0, blocks=0):
    """gcl_tcp_read_workspace: bytes of device scratch a call over @nconn connections, @nent queue
    entries and @nvec vectors takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_read_workspace(nconn, nent, nvec, blocks, ctypes.byref(need)), "gcl_tcp_read_workspace")
    return need.value


WR_OUT_WIDTH = {"desc": 32, "frame_off": 8, "seg_conn": 4, "txq_ent": 16, "txq_cold": 16, "src_off": 8, "len": 2,
                "dst_off": 8, "item_conn": 4, "item_seg": 4}


def _wr_structs(now, voff, iov, nvec, wr, conn, addr, nconn, seg_cap, item_cap, frame_base, frame_stride, frames_len,
                blocks, out, counts):
    """The two structs of gcl_tcp_write / gcl_tcp_write_host, sizes checked;
    @out maps WR_OUT_FIELDS to buffers."""
    if voff is not None and _nbytes(voff) < 4 * (nconn + 1):
        raise ValueError("voff shorter than nconn + 1")
    for arr, w in ((wr, 48), (conn, 48), (addr, 16), (out["out_conn"], 48)):
        if arr is not None and _nbytes(arr) < w * nconn:
            raise ValueError("per-connection array too small")
    if voff is not None and iov is not None and _nbytes(iov) < 16 * nvec:
        raise ValueError("iov shorter than nvec")
    for f in WR_SEG_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < WR_OUT_WIDTH[f] * seg_cap:
            raise ValueError(f"{f}: per-segment array shorter than seg_cap")
    for f in WR_ITEM_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < WR_OUT_WIDTH[f] * item_cap:
            raise ValueError(f"{f}: per-item array shorter than item_cap")
    if out["totals"] is not None and _nbytes(out["totals"]) < 48:
        raise ValueError("totals too small")
    if counts is not None and _nbytes(counts) < 8 * WRC_NR:
        raise ValueError("counts buffer too small")
    win = GclWrIn(size=ctypes.sizeof(GclWrIn), blocks=blocks, now=now, voff=_ptr(voff), iov=_ptr(iov), nvec=nvec,
                  wr=_ptr(wr), conn=_ptr(conn), addr=_ptr(addr), nconn=nconn, frame_stride=frame_stride,
                  seg_cap=seg_cap, item_cap=item_cap, frame_base=frame_base, frames_len=frames_len)
    return win, GclWrOut(**{f: _ptr(out[f]) for f in WR_OUT_FIELDS})


def tcp_write_host(now, wr, conn, addr, seg_cap, item_cap, voff=None, iov=None, frame_stride=2048, frame_base=0,
                   frames_len=0, nconn=None, nvec=None, blocks=0, out=None, counts=None):
    """gcl_tcp_write_host: the rule of Classifier.tcp_write on the CPU over
    numpy arrays.  @wr, @conn and @addr are TCP_WR_DTYPE, TCP_CONN_DTYPE and
    TCP_ADDR_DTYPE arrays indexed by cookie; @voff an optional u32[nconn + 1]
    CSR over the RD_IOV_DTYPE array @iov.  @out maps WR_OUT_FIELDS to arrays
    (WR_CONN_OUT_DTYPE[nconn]; per segment TXH_DESC_DTYPE, u64, u32,
    TXQ_ENT_DTYPE, TXQ_COLD_DTYPE, each @seg_cap long; per item u64, u16, u64,
    u32, u32, each @item_cap long; totals u64[6]); the ones left out are
    allocated.  @counts is a u64[WRC_NR], accumulated.  Returns the dict."""
    nconn = len(wr) if nconn is None else nconn
    nvec = (len(iov) if iov is not None else 0) if nvec is None else nvec
    out = dict(out or {})
    for f, dt, k in (("out_conn", WR_CONN_OUT_DTYPE, nconn), ("desc", TXH_DESC_DTYPE, seg_cap),
                     ("frame_off", np.uint64, seg_cap), ("seg_conn", np.uint32, seg_cap),
                     ("txq_ent", TXQ_ENT_DTYPE, seg_cap), ("txq_cold", TXQ_COLD_DTYPE, seg_cap),
                     ("src_off", np.uint64, item_cap), ("len", np.uint16, item_cap), ("dst_off", np.uint64, item_cap),
                     ("item_conn", np.uint32, item_cap), ("item_seg", np.uint32, item_cap), ("totals", np.uint64, 6)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    win, wout = _wr_structs(now, voff, iov, nvec, wr, conn, addr, nconn, seg_cap, item_cap, frame_base, frame_stride,
                            frames_len, blocks, out, counts)
    _check(lib.gcl_tcp_write_host(ctypes.byref(win), ctypes.byref(wout), _ptr(counts)), "gcl_tcp_write_host")
    return out


SHUT_OUT_WIDTH = dict(CTLSEG_OUT_WIDTH, txq_ent=16, txq_cold=16)


def _shut_structs(now, shut, tmr, conn, addr, nconn, seg_cap, frame_base, frame_stride, frames_len, blocks, out,
                  counts):
    """The two structs of gcl_tcp_shut / gcl_tcp_shut_host, sizes checked; @out
    maps SHUT_OUT_FIELDS to buffers."""
    for arr, w in ((shut, 16), (tmr, 64), (conn, 48), (addr, 16), (out["out_conn"], 48)):
        if arr is not None and _nbytes(arr) < w * nconn:
            raise ValueError("per-connection array too small")
    for f in SHUT_SEG_FIELDS:
        if out[f] is not None and _nbytes(out[f]) < SHUT_OUT_WIDTH[f] * seg_cap:
            raise ValueError(f"{f}: per-segment array shorter than seg_cap")
    if out["totals"] is not None and _nbytes(out["totals"]) < 16:
        raise ValueError("totals too small")
    if counts is not None and _nbytes(counts) < 8 * SHUTC_NR:
        raise ValueError("counts buffer too small")
    sin = GclShutIn(size=ctypes.sizeof(GclShutIn), blocks=blocks, now=now, shut=_ptr(shut), tmr=_ptr(tmr),
                    conn=_ptr(conn), addr=_ptr(addr), nconn=nconn, frame_stride=frame_stride, seg_cap=seg_cap,
                    frame_base=frame_base, frames_len=frames_len)
    seg = GclCtlsegOut(**{f: _ptr(out[f]) for f in CTLSEG_OUT_FIELDS})
    return sin, GclShutOut(out_conn=_ptr(out["out_conn"]), seg=seg, txq_ent=_ptr(out["txq_ent"]),
                           txq_cold=_ptr(out["txq_cold"]))


def tcp_shut_host(now, shut, tmr, conn, addr, seg_cap, frame_stride=64, frame_base=0, frames_len=0, nconn=None,
                  blocks=0, out=None, counts=None):
    """gcl_tcp_shut_host: the rule of Classifier.tcp_shut on the CPU over numpy
    arrays.  @shut, @tmr, @conn and @addr are TCP_SHUT_DTYPE, TCP_TMR_DTYPE,
    TCP_CONN_DTYPE and TCP_ADDR_DTYPE arrays indexed by cookie.  @out maps
    SHUT_OUT_FIELDS to arrays (SHUT_CONN_OUT_DTYPE[nconn]; per segment
    TXH_DESC_DTYPE, u64, u32, u8, u32, TXQ_ENT_DTYPE, TXQ_COLD_DTYPE, each
    @seg_cap long; totals u64[2]); the ones left out are allocated.  @counts is
    a u64[SHUTC_NR], accumulated.  Returns the dict."""
    nconn = len(shut) if nconn is None else nconn
    out = dict(out or {})
    for f, dt, k in (("out_conn", SHUT_CONN_OUT_DTYPE, nconn), ("txq_ent", TXQ_ENT_DTYPE, seg_cap),
                     ("txq_cold", TXQ_COLD_DTYPE, seg_cap)):
        if f not in out:
            out[f] = np.zeros(max(k, 1), dtype=dt)
    _ctlseg_host_arrays(out, seg_cap)
    sin, sout = _shut_structs(now, shut, tmr, conn, addr, nconn, seg_cap, frame_base, frame_stride, frames_len,
                              blocks, out, counts)
    _check(lib.gcl_tcp_shut_host(ctypes.byref(sin), ctypes.byref(sout), _ptr(counts)), "gcl_tcp_shut_host")
    return out


def tcp_shut_workspace(nconn, blocks=0):
    """gcl_tcp_shut_workspace: bytes of device scratch a call over @nconn connections takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_shut_workspace(nconn, blocks, ctypes.byref(need)), "gcl_tcp_shut_workspace")
    return need.value


def tcp_write_workspace(nconn, nvec=0, blocks=0):
    """gcl_tcp_write_workspace: bytes of device scratch a call over @nconn connections and @nvec
    vectors takes."""
    need = ctypes.c_size_t()
    _check(lib.gcl_tcp_write_workspace(nconn, nvec, blocks, ctypes.byref(need)), "gcl_tcp_write_workspace")
    return need.value


def runtime_ip(r: int) -> int:
    return lib.gcl_runtime_ip(r)


def steer_flows(thread_count, active_idx):
    """sched_steer_flows (iokernel/sched.c:122-147); returns the flow table."""
    n = len(active_idx)
    act = (ctypes.c_uint16 * max(n, 1))(*active_idx)
    out = (ctypes.c_uint16 * thread_count)(*([0] * thread_count))
    _check(lib.gcl_steer_flows(thread_count, act, n, out), "gcl_steer_flows")
    return list(out)


class DeviceBuffer:
    """hipMalloc'd device memory owned by the library (gcl_dev_alloc): a raw
    address with the duck-typed interface the binding accepts (data_ptr,
    numel, element_size)."""

    def __init__(self, nbytes, device=0, partner=None, new_reads=True, vbytes=4):
        """partner: another buffer (data_ptr/numel); the new one is then placed
        by gcl_dev_alloc_paired so that reading the frame side while writing
        the verdict side does not hit the same-placement-class slowdown.
        new_reads: the new buffer is the frame (read) side.
        vbytes: the verdict width the classifier will write (1, 2, 4 or 8)."""
        p = ctypes.c_void_p()
        self.probe_us = None
        self.pair_info = None
        if partner is None:
            _check(lib.gcl_dev_alloc(device, nbytes, ctypes.byref(p)), "gcl_dev_alloc")
        else:
            info = GclPairInfo()
            _check(lib.gcl_dev_alloc_paired(device, nbytes, _ptr(partner), _nbytes(partner),
                                            (PAIR_NEW_READS if new_reads else PAIR_NEW_WRITES) |
                                            vbytes << 8,
                                            ctypes.byref(p), ctypes.byref(info)), "gcl_dev_alloc_paired")
            self.probe_us = (info.chosen_us, info.worst_us)
            self.pair_info = {"probe_us_chosen": round(info.chosen_us, 2),
                              "probe_us_worst": round(info.worst_us, 2),
                              "candidates": info.candidates, "classes_seen": info.classes,
                              "spacer_MiB": info.spacer_bytes >> 20,
                              "probe_write_bytes": info.probe_write_bytes}
        self.ptr, self.nbytes = p.value, nbytes

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1

    def free(self):
        if self.ptr:
            lib.gcl_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Trace:
    """A pcap trace loaded by gcl_pcap_load: packed 16-B-aligned frames in
    host memory with numpy views of offsets, lengths and timestamps."""

    def __init__(self, path, max_pkts=0):
        self.t = GclTrace()
        _check(lib.gcl_pcap_load(os.fsencode(path), ctypes.byref(self.t), max_pkts), "gcl_pcap_load")
        n = self.t.n
        self.n = n
        self.skipped = self.t.skipped  # records longer than 65535 bytes, not loaded

        def view(ptr, ctype, count, dtype):
            if not count:
                return np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array((ctype * count).from_address(ptr)).view(dtype)
        self.frames = view(self.t.frames, ctypes.c_uint8, self.t.alloc_len, np.uint8)
        self.frames_len = self.t.frames_len
        self.offs = view(self.t.offs, ctypes.c_uint64, n, np.uint64)
        self.pkt_len = view(self.t.pkt_len, ctypes.c_uint16, n, np.uint16)
        self.orig_len = view(self.t.orig_len, ctypes.c_uint32, n, np.uint32)
        self.ts_ns = view(self.t.ts_ns, ctypes.c_uint64, n, np.uint64)

    def close(self):
        if self.t.frames:
            lib.gcl_pcap_free(ctypes.byref(self.t))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_register(arr):
    """Pin + map a host numpy array for ZEROCOPY (gcl_host_register)."""
    _check(lib.gcl_host_register(arr.ctypes.data, arr.nbytes), "gcl_host_register")


def host_unregister(arr):
    return lib.gcl_host_unregister(arr.ctypes.data)


def pcap_write(path, frames, pkt_len, stride=0, offs=None, ts_ns=None, snaplen=0):
    n = len(pkt_len)
    pl = np.ascontiguousarray(pkt_len, dtype=np.uint16)
    o = None if offs is None else np.ascontiguousarray(offs, dtype=np.uint64)
    ts = None if ts_ns is None else np.ascontiguousarray(ts_ns, dtype=np.uint64)
    _check(lib.gcl_pcap_write(os.fsencode(path), _ptr(frames), stride, _ptr(o), _ptr(pl),
                              _ptr(ts), n, snaplen), "gcl_pcap_write")


# The reference's ingress mbuf pool (iokernel/defs.h:70, :503-523; rx.c:398-415):
# 2 MiB pages of 9408-B elements, 222 per page; an element is a 64-B mempool
# object header, the 128-B rte_mbuf, 24 B of rx_priv_data and 128 B of
# headroom before the frame, so frame data sits at element + 344 (8-B aligned).
RX_ELT_SIZE = 9408
RX_ELT_PER_PAGE = (2 << 20) // RX_ELT_SIZE
RX_DATA_OFF = 64 + 128 + 24 + 128
IOKERNEL_NUM_MBUFS = 8192 * 16


def mbuf_data_offsets(nmbufs=IOKERNEL_NUM_MBUFS):
    """Offset of mbuf i's frame data from the ingress region base
    (rte_pktmbuf_mtod(m) - dp.ingress_mbuf_region.base, rx.c:82), u64[nmbufs]."""
    i = np.arange(nmbufs, dtype=np.uint64)
    return ((i // RX_ELT_PER_PAGE) * np.uint64(2 << 20) + (i % RX_ELT_PER_PAGE) * np.uint64(RX_ELT_SIZE)
            + np.uint64(RX_DATA_OFF))


def mbuf_region_bytes(nmbufs=IOKERNEL_NUM_MBUFS):
    """Bytes of ingress region holding @nmbufs elements (whole 2 MiB pages)."""
    return -(-nmbufs // RX_ELT_PER_PAGE) * (2 << 20)


def zipf_cdf(nflows, s=0.99):
    cdf = np.empty(nflows, dtype=np.uint64)
    _check(lib.gcl_zipf_cdf(nflows, s, cdf.ctypes.data), "gcl_zipf_cdf")
    return cdf


def generate(workload, n, stride, nruntimes, frames, olflags=None, rss=None, seed=0xCA1ADA4,
             rank=0, world=1, shard_block=0, zipf_cdf_dev=None, nflows=0, stream=None,
             pkt_len=None):
    """Fill device buffers with synthetic rx traffic (gcl_generate)."""
    if _nbytes(frames) < n * stride:
        raise ValueError("frames buffer too small")
    if pkt_len is not None and _nbytes(pkt_len) < 2 * n:
        raise ValueError("pkt_len buffer too small")
    p = GclGenParams(workload=workload, nruntimes=nruntimes, seed=seed, n=n, stride=stride,
                     rank=rank, world=world, shard_block=shard_block,
                     zipf_cdf=_ptr(zipf_cdf_dev), nflows=nflows, pkt_len=_ptr(pkt_len))
    _check(lib.gcl_generate(ctypes.byref(p), _ptr(frames), _ptr(olflags), _ptr(rss), stream),
           "gcl_generate")


def verdict_bytes(flags):
    return 1 if flags & CFG_VERDICT1 else 2 if flags & CFG_VERDICT2 else 4 if flags & CFG_VERDICT4 else 8


def verdict_dtype(vbytes):
    return {1: np.dtype("u1"), 2: np.dtype("<u2"), 4: VERDICT4_DTYPE, 8: VERDICT_DTYPE}[vbytes]


def thread_bits_for(max_runtimes, max_threads):
    """Smallest GclCfg.thread_bits that holds @max_threads kthreads per runtime;
    None when max_runtimes << thread_bits would exceed the 2-byte verdict."""
    tb = max(0, (int(max_threads) - 1).bit_length())
    return tb if tb <= 8 and (max_runtimes << tb) <= V2_QUEUES else None


class Classifier:
    """One gcl_ctx: the GPU side of one dataplane (iokernel/dpdk.c:276-280)."""

    def __init__(self, device=0, max_runtimes=16, hash_mode=HASH_JENKINS, flags=0,
                 default_olflags=F_RSS_HASH | F_IP_CKSUM_GOOD, rss_key=CALADAN_RSS_KEY,
                 thread_bits=0, tune=None):
        if isinstance(hash_mode, str):
            hash_mode = HASH_MODES[hash_mode]
        cfg = GclCfg(max_runtimes=max_runtimes, hash_mode=hash_mode, flags=flags,
                     default_olflags=default_olflags, thread_bits=thread_bits)
        key = bytes(rss_key)[:40].ljust(40, b"\0")
        for i in range(40):
            cfg.rss_key[i] = key[i]
        self.cfg = cfg
        self.max_runtimes = max_runtimes
        self.vbytes = verdict_bytes(flags)  # bytes per verdict
        self.thread_bits = thread_bits
        self._ctx = ctypes.c_void_p()
        _check(lib.gcl_open(device, ctypes.byref(cfg), ctypes.byref(self._ctx)), "gcl_open")
        if tune:
            self.tune(**tune)

    def tune(self, **kw):
        """gcl_ctx_tune: the library's defaults with the fields in @kw
        overridden (make_tune); no arguments: back to the defaults.  Batch
        fields apply from the next classify, loop fields from the next rxloop."""
        t = make_tune(**kw)
        return _check(lib.gcl_ctx_tune(self._ctx, ctypes.byref(t)), "gcl_ctx_tune")

    def close(self):
        loop = getattr(self, "_loop", None)
        if loop is not None:
            loop.stop()  # gcl_close would free it under the RxLoop object
        if self._ctx:
            lib.gcl_close(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def runtime_set(self, uniqid, ip, thread_count, active_count, flow_tbl=None):
        tbl = None
        if flow_tbl is not None:
            tbl = (ctypes.c_uint16 * max(len(flow_tbl), 1))(*flow_tbl)
        return _check(lib.gcl_runtime_set(self._ctx, uniqid, ip, thread_count, active_count, tbl),
                      "gcl_runtime_set")

    def runtime_del(self, uniqid):
        return _check(lib.gcl_runtime_del(self._ctx, uniqid), "gcl_runtime_del")

    def set_trans_seed(self, uniqid, seed):
        return _check(lib.gcl_runtime_set_trans_seed(self._ctx, uniqid, seed),
                      "gcl_runtime_set_trans_seed")

    def classify(self, frames, n, stride=0, verdicts=None, counts=None, stats=None, offs=None,
                 olflags=None, rss=None, fdir_hi=None, frames_len=None, stream=None,
                 dst_hint=None, trans=None):
        """Launch the classify kernel on device buffers (asynchronous)."""
        if verdicts is not None and _nbytes(verdicts) < self.vbytes * n:
            raise ValueError("verdict buffer too small")
        if counts is not None and _nbytes(counts) < 8 * self.max_runtimes:
            raise ValueError("counts buffer too small")
        if stats is not None and _nbytes(stats) < 8 * NR_STATS:
            raise ValueError("stats buffer too small")
        for arr, w in ((offs, 8), (olflags, 1), (rss, 4), (fdir_hi, 4), (dst_hint, 4)):
            if arr is not None and _nbytes(arr) < w * n:
                raise ValueError("per-packet array too small")
        b = GclBatch(frames=_ptr(frames),
                     frames_len=_frames_len(frames, frames_len),
                     stride=stride, offs=_ptr(offs), olflags=_ptr(olflags), rss=_ptr(rss),
                     fdir_hi=_ptr(fdir_hi), pkt_len=None, n=n, dst_hint=_ptr(dst_hint))
        if trans is not None and _nbytes(trans) < 8 * n:
            raise ValueError("trans buffer too small")
        o = GclOut(verdicts=_ptr(verdicts), runtime_counts=_ptr(counts), stats=_ptr(stats),
                   trans=_ptr(trans))
        return _check(lib.gcl_classify_ex(self._ctx, ctypes.byref(b), ctypes.byref(o), stream),
                      "gcl_classify_ex")

    def access_probe(self, frames, n, stride=0, out=None, vbytes=None, offs=None, olflags=None,
                     rss=None, frames_len=None, stream=None, minimal=False):
        """gcl_access_probe: at the context's verdict width, the classify
        launch itself (tile or pair kernel) with rx_one_pkt folded away (the
        kernel's own ceiling); at another width, or with @minimal, the fewest
        requests the frame layout allows (the layout's ceiling).  Asynchronous."""
        vbytes = self.vbytes if vbytes is None else vbytes
        if out is None or _nbytes(out) < vbytes * n:
            raise ValueError("probe output buffer too small")
        if minimal:
            vbytes |= PROBE_MIN
        b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len),
                     stride=stride, offs=_ptr(offs), olflags=_ptr(olflags), rss=_ptr(rss),
                     fdir_hi=None, pkt_len=None, n=n, dst_hint=None)
        return _check(lib.gcl_access_probe(self._ctx, ctypes.byref(b), _ptr(out), vbytes, stream),
                      "gcl_access_probe")

    def classify_host(self, frames, n, stride=0, verdicts=None, counts=None, stats=None,
                      olflags=None, rss=None, fdir_hi=None, offs=None, frames_len=None,
                      mode=E2E_COPY, nstreams=2, chunk=1 << 20, dst_hint=None):
        """End-to-end: host (pinned) frames in, host verdicts out (synchronous)."""
        if verdicts is not None and _nbytes(verdicts) < self.vbytes * n:
            raise ValueError("verdict buffer too small")
        b = GclBatch(frames=_ptr(frames),
                     frames_len=_frames_len(frames, frames_len),
                     stride=stride, offs=_ptr(offs), olflags=_ptr(olflags), rss=_ptr(rss),
                     fdir_hi=_ptr(fdir_hi), pkt_len=None, n=n, dst_hint=_ptr(dst_hint))
        o = GclE2eOpts(mode=mode, nstreams=nstreams, chunk=chunk)
        return _check(lib.gcl_classify_host(self._ctx, ctypes.byref(b), _ptr(verdicts), _ptr(counts),
                                            _ptr(stats), ctypes.byref(o)), "gcl_classify_host")

    def plan_buckets(self, key=PLAN_BY_RUNTIME):
        """gcl_plan_buckets: the plan's bucket count, the host bucket included."""
        nb = ctypes.c_uint32()
        _check(lib.gcl_plan_buckets(self._ctx, key, ctypes.byref(nb)), "gcl_plan_buckets")
        return nb.value

    def plan(self, verdicts, n, key=PLAN_BY_RUNTIME, order=None, bucket_off=None, blocks=0,
             stream=None):
        """gcl_plan: the stable partition of @n classified packets by runtime
        (or queue), asynchronous.  Returns (order, bucket_off): u32[n] packet
        indices and u32[nbuckets + 1] list starts (given as int32 tensors when
        allocated here).  The scratch is a torch tensor kept on the classifier
        and reused while it is large enough."""
        import torch
        nb = self.plan_buckets(key)
        if _nbytes(verdicts) < self.vbytes * n:
            raise ValueError("verdict buffer too small")
        dev = verdicts.device if hasattr(verdicts, "device") else None
        if order is None:
            order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if bucket_off is None:
            bucket_off = torch.empty(nb + 1, dtype=torch.int32, device=dev)
        if _nbytes(order) < 4 * n or _nbytes(bucket_off) < 4 * (nb + 1):
            raise ValueError("plan output buffer too small")
        cfg = GclPlanCfg(size=ctypes.sizeof(GclPlanCfg), key=key, blocks=blocks)
        need = ctypes.c_size_t()
        _check(lib.gcl_plan_workspace(self._ctx, ctypes.byref(cfg), n, ctypes.byref(need)),
               "gcl_plan_workspace")
        ws = getattr(self, "_plan_ws", None)
        if ws is None or ws.numel() < need.value or ws.device != order.device:
            ws = self._plan_ws = torch.empty(max(need.value, 16), dtype=torch.uint8,
                                             device=order.device)
        out = GclPlanOut(order=_ptr(order), bucket_off=_ptr(bucket_off))
        _check(lib.gcl_plan(self._ctx, ctypes.byref(cfg), _ptr(verdicts), n, ctypes.byref(out),
                            _ptr(ws), ws.numel(), stream), "gcl_plan")
        return order, bucket_off

    def plan_pack(self, verdicts, n, order, m=None, pkt_len=None, olflags=None, offs=None, stride=0,
                  shm_base=0, out=None, stream=None):
        """gcl_plan_pack: the ready-to-send records of the list @order[0..m)
        (a plan's order, or one bucket's slice of it; @m defaults to the whole
        of @order), asynchronous.  Returns (cmd, payload, v4): u64[m] lrpc
        commands, u64[m] shm pointers and gcl_verdict4[m], given as int64,
        int64 and int32 tensors when allocated here; @out is such a triple."""
        import torch
        if m is None:
            if not hasattr(order, "numel"):
                raise ValueError("m is required when order is a raw address")
            m = order.numel()
        if _nbytes(verdicts) < self.vbytes * n:
            raise ValueError("verdict buffer too small")
        if _nbytes(order) < 4 * m:
            raise ValueError("order buffer too small")
        for arr, w in ((pkt_len, 2), (olflags, 1), (offs, 8)):
            if arr is not None and _nbytes(arr) < w * n:
                raise ValueError("per-packet array too small")
        if out is None:
            dev = verdicts.device if hasattr(verdicts, "device") else None
            out = (torch.empty(max(m, 1), dtype=torch.int64, device=dev),
                   torch.empty(max(m, 1), dtype=torch.int64, device=dev),
                   torch.empty(max(m, 1), dtype=torch.int32, device=dev))
        cmd, payload, v4 = out
        if _nbytes(cmd) < 8 * m or _nbytes(payload) < 8 * m or _nbytes(v4) < 4 * m:
            raise ValueError("pack output buffer too small")
        pin = GclPackIn(size=ctypes.sizeof(GclPackIn), verdicts=_ptr(verdicts), n=n, order=_ptr(order),
                        m=m, pkt_len=_ptr(pkt_len), olflags=_ptr(olflags), offs=_ptr(offs),
                        stride=stride, shm_base=shm_base)
        pout = GclPackOut(cmd=_ptr(cmd), payload=_ptr(payload), v4=_ptr(v4))
        _check(lib.gcl_plan_pack(self._ctx, ctypes.byref(pin), ctypes.byref(pout), stream),
               "gcl_plan_pack")
        return cmd, payload, v4

    def rx_csum(self, frames, n, stride=0, olflags_out=None, counts=None, offs=None, olflags=None,
                rss=None, fdir_hi=None, frames_len=None, stream=None, dst_hint=None):
        """gcl_rx_csum: the batch's ol_flags with the IPv4 header checksum of
        every packet that is not already IP_CKSUM_GOOD resolved on the GPU
        (asynchronous).  The batch arguments are classify's (rss, fdir_hi and
        dst_hint are ignored); @olflags_out may be @olflags (in place) and is
        allocated as a uint8 tensor when not given; @counts is a device
        u64[CSUM_NR], accumulated.  Returns the output array."""
        for arr, w in ((offs, 8), (olflags, 1)):
            if arr is not None and _nbytes(arr) < w * n:
                raise ValueError("per-packet array too small")
        if counts is not None and _nbytes(counts) < 8 * CSUM_NR:
            raise ValueError("counts buffer too small")
        if olflags_out is None:
            import torch
            dev = frames.device if hasattr(frames, "device") else None
            olflags_out = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        if _nbytes(olflags_out) < n:
            raise ValueError("olflags_out buffer too small")
        b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len),
                     stride=stride, offs=_ptr(offs), olflags=_ptr(olflags), rss=None,
                     fdir_hi=None, pkt_len=None, n=n, dst_hint=None)
        _check(lib.gcl_rx_csum(self._ctx, ctypes.byref(b), _ptr(olflags_out), _ptr(counts), stream),
               "gcl_rx_csum")
        return olflags_out

    def l4_csum(self, frames, n, pkt_len, mode=L4_VERIFY, stride=0, offs=None, frames_len=None,
                tx_olflags=None, status=None, counts=None, len_hint=0, group=0, stream=None):
        """gcl_l4_csum: the TCP/UDP checksum of every eligible packet of the
        batch checked (L4_VERIFY) or, with the IPv4 header checksum, written
        into @frames (L4_FILL) on the GPU (asynchronous).  @pkt_len (int16,
        u16[n]) is required; @tx_olflags (uint8) says per packet which fields
        FILL writes (None: both); @status (uint8) is allocated on @frames'
        device when None; @counts is a device u64[L4C_NR], accumulated.
        Returns @status."""
        if pkt_len is None:
            raise ValueError("pkt_len is required")
        if status is None:
            import torch
            dev = frames.device if hasattr(frames, "device") else None
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        b, lin = _l4_structs(frames, n, stride, offs, pkt_len, frames_len, mode, tx_olflags, group,
                             len_hint, status, counts)
        _check(lib.gcl_l4_csum(self._ctx, ctypes.byref(b), ctypes.byref(lin), _ptr(status),
                               _ptr(counts), stream), "gcl_l4_csum")
        return status

    def l4_payload(self, frames, n, pkt_len, stride=0, offs=None, frames_len=None, order=None, m=None,
                   sock=None, l4_status=None, seg_off=None, nseg=None, align=0, blocks=0, out=None,
                   counts=None, workspace=None, stream=None):
        """gcl_l4_payload: the payload descriptors and the packed receive
        layout of the list @order[0..m) (None: every packet in turn) on the
        GPU, asynchronous.  @pkt_len is required; @sock and @l4_status are
        what sock_lookup and l4_csum(L4_VERIFY) wrote; @seg_off (int32,
        u32[nseg + 1]) is e.g. a plan's bucket_off.  @out maps PAY_OUT_FIELDS
        to device buffers; the ones left out are allocated on @frames' device
        (src_off, dst_off, seg_bytes and total int64, len int16, kind uint8,
        meta uint8[m, 16]; seg_bytes only with @seg_off).  @counts is a device
        u64[PAYC_NR], accumulated.  The scratch is @workspace, or a torch
        tensor kept on the classifier.  Returns the dict: src_off, len and
        dst_off are copy_batch's src_off, length and dst_off."""
        import torch
        if pkt_len is None:
            raise ValueError("pkt_len is required")
        m = _pay_m(n, m, order)
        nseg = (seg_off.numel() - 1 if seg_off is not None else 0) if nseg is None else nseg
        dev = frames.device if hasattr(frames, "device") else None
        out = dict(out or {})
        for f, dt, shape in (("src_off", torch.int64, (max(m, 1),)), ("len", torch.int16, (max(m, 1),)),
                             ("dst_off", torch.int64, (max(m, 1),)), ("kind", torch.uint8, (max(m, 1),)),
                             ("meta", torch.uint8, (max(m, 1), 16)), ("total", torch.int64, (1,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        if "seg_bytes" not in out:
            out["seg_bytes"] = torch.empty(nseg + 1, dtype=torch.int64, device=dev) \
                if seg_off is not None else None
        b, pin, pout = _pay_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                    l4_status, seg_off, nseg, align, blocks, out, counts)
        ws = workspace
        if ws is None:
            need = l4_payload_workspace(m, blocks)
            ws = getattr(self, "_pay_ws", None)
            if ws is None or ws.numel() < need or ws.device != out["total"].device:
                ws = self._pay_ws = torch.empty(need, dtype=torch.uint8, device=out["total"].device)
        _check(lib.gcl_l4_payload(self._ctx, ctypes.byref(b), ctypes.byref(pin), ctypes.byref(pout),
                                  _ptr(counts), _ptr(ws), _nbytes(ws), stream), "gcl_l4_payload")
        return out

    def sock_set(self, uniqid, entries):
        """gcl_sock_set: replace runtime @uniqid's socket entries (sock_entries
        says what @entries may be; an empty sequence clears them)."""
        e = sock_entries(entries)
        return _check(lib.gcl_sock_set(self._ctx, uniqid, e.ctypes.data if len(e) else None, len(e)),
                      "gcl_sock_set")

    def sock_lookup(self, frames, n, stride=0, verdicts=None, sock=None, counts=None, offs=None,
                    frames_len=None, stream=None):
        """gcl_sock_lookup: the socket demux of a classified batch on the GPU
        (asynchronous).  @verdicts is the device array classify wrote, in the
        context's width; @sock (int32, u32[n]) is allocated when not given;
        @counts is a device u64[SOCK_NR], accumulated.  Returns @sock."""
        if verdicts is None or _nbytes(verdicts) < self.vbytes * n:
            raise ValueError("verdict buffer too small")
        if offs is not None and _nbytes(offs) < 8 * n:
            raise ValueError("per-packet array too small")
        if counts is not None and _nbytes(counts) < 8 * SOCK_NR:
            raise ValueError("counts buffer too small")
        if sock is None:
            import torch
            dev = frames.device if hasattr(frames, "device") else None
            sock = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if _nbytes(sock) < 4 * n:
            raise ValueError("sock buffer too small")
        b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len),
                     stride=stride, offs=_ptr(offs), olflags=None, rss=None,
                     fdir_hi=None, pkt_len=None, n=n, dst_hint=None)
        _check(lib.gcl_sock_lookup(self._ctx, ctypes.byref(b), _ptr(verdicts), _ptr(sock), _ptr(counts),
                                   stream), "gcl_sock_lookup")
        return sock

    def neigh_set(self, entries):
        """gcl_neigh_set: replace the context's neighbour table (neigh_entries
        says what @entries may be; an empty sequence clears it)."""
        e = neigh_entries(entries)
        return _check(lib.gcl_neigh_set(self._ctx, e.ctypes.data if len(e) else None, len(e)),
                      "gcl_neigh_set")

    def tx_hdr(self, desc, frame_off, m, frames, net, frames_len=None, shm_base=0, cap=0, out=None,
               counts=None, stream=None):
        """gcl_tx_hdr: the Ethernet, IPv4 and UDP or TCP headers, the next hop
        and the txpkt command of @m segments of one runtime on the GPU,
        asynchronous.  @desc is a device uint8[m, 32] holding TXH_DESC_DTYPE
        records (16-B aligned), @frame_off a device int64[m], @frames the
        device tx region, @net a txh_net().  @out maps TXH_OUT_FIELDS to
        device buffers; the ones left out are allocated on @frames' device
        (cmd and payload int64, pkt_len int16, tx_olflags and status uint8,
        hash int32); hash=None in @out leaves it out.  @counts is a device
        u64[TXHC_NR], accumulated.  Returns the dict: frame_off, pkt_len,
        tx_olflags and hash are l4_csum's and copy_batch's inputs."""
        import torch
        dev = frames.device if hasattr(frames, "device") else None
        out = dict(out or {})
        for f, dt in (("cmd", torch.int64), ("payload", torch.int64), ("pkt_len", torch.int16),
                      ("tx_olflags", torch.uint8), ("hash", torch.int32), ("status", torch.uint8)):
            if f not in out:
                out[f] = torch.empty(max(m, 1), dtype=dt, device=dev)
        tin, tout = _txh_structs(desc, frame_off, m, frames, frames_len, shm_base, cap, net, out, counts)
        _check(lib.gcl_tx_hdr(self._ctx, ctypes.byref(tin), ctypes.byref(tout), _ptr(counts), stream),
               "gcl_tx_hdr")
        return out

    def tx_seg(self, send, m, seg_cap, stride=0, lead=0, frame_base=0, frames_len=0, udp_max=1472,
               blocks=0, out=None, counts=None, workspace=None, stream=None):
        """gcl_tx_seg: cut @m socket writes of one runtime into tx segments on
        the GPU, asynchronous.  @send is a device uint8[m, 48] holding
        SEG_SEND_DTYPE records (16-B aligned).  @out maps SEG_OUT_FIELDS to
        device buffers; the ones left out are allocated on @send's device
        (status uint8, sent, snd_nxt_out, seg_first, nseg and send_idx int32,
        desc uint8[seg_cap, 32], frame_off, src_off, dst_off and the totals
        int64, len int16); send_idx=None in @out leaves it out.  @counts is a
        device u64[SEGC_NR], accumulated.  The scratch is @workspace, or a
        torch tensor kept on the classifier.  Returns the dict: src_off, len
        and dst_off are copy_batch's src_off, length and dst_off, desc and
        frame_off are tx_hdr's, and total_segs is their m."""
        import torch
        dev = send.device if hasattr(send, "device") else None
        out = dict(out or {})
        mm, cc = max(m, 1), max(seg_cap, 1)
        for f, dt, shape in (("status", torch.uint8, (mm,)), ("sent", torch.int32, (mm,)),
                             ("snd_nxt_out", torch.int32, (mm,)), ("seg_first", torch.int32, (mm,)),
                             ("nseg", torch.int32, (mm,)), ("desc", torch.uint8, (cc, 32)),
                             ("frame_off", torch.int64, (cc,)), ("src_off", torch.int64, (cc,)),
                             ("len", torch.int16, (cc,)), ("dst_off", torch.int64, (cc,)),
                             ("send_idx", torch.int32, (cc,)), ("total_segs", torch.int64, (1,)),
                             ("total_bytes", torch.int64, (1,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        sin, sout = _seg_structs(send, m, seg_cap, stride, lead, frame_base, frames_len, udp_max, blocks,
                                 out, counts)
        ws = workspace
        if ws is None:
            need = tx_seg_workspace(m, blocks)
            ws = getattr(self, "_seg_ws", None)
            if ws is None or ws.numel() < need or ws.device != out["total_segs"].device:
                ws = self._seg_ws = torch.empty(need, dtype=torch.uint8, device=out["total_segs"].device)
        _check(lib.gcl_tx_seg(self._ctx, ctypes.byref(sin), ctypes.byref(sout), _ptr(counts), _ptr(ws),
                              _nbytes(ws), stream), "gcl_tx_seg")
        return out

    def tcp_rx(self, frames, n, pkt_len, sock, conn, nconn, stride=0, offs=None, frames_len=None,
               order=None, m=None, l4_status=None, align=0, blocks=0, out=None, counts=None,
               workspace=None, stream=None):
        """gcl_tcp_rx: tcp_rx_conn's established fast path for one runtime's
        list @order[0..m) (None: every packet in turn) on the GPU,
        asynchronous.  @sock is what sock_lookup wrote, @l4_status what
        l4_csum(L4_VERIFY) wrote, @conn a device uint8[nconn, 48] holding
        TCP_CONN_DTYPE records indexed by cookie (16-B aligned).  @out maps
        TCPRX_OUT_FIELDS to device buffers; the ones left out are allocated on
        @frames' device (verdict and sflags uint8, rcv_nxt_after int32,
        copy_len int16, dst_off and conn_off int64, out_conn uint8[nconn, 48]).
        @counts is a device u64[TCPRXC_NR], accumulated.  The scratch is
        @workspace, or a torch tensor kept on the classifier.  Returns the
        dict: with l4_payload's src_off, copy_len and dst_off are copy_batch's
        length and dst_off."""
        import torch
        m = _pay_m(n, m, order)
        dev = frames.device if hasattr(frames, "device") else None
        out = dict(out or {})
        mm = max(m, 1)
        for f, dt, shape in (("verdict", torch.uint8, (mm,)), ("sflags", torch.uint8, (mm,)),
                             ("rcv_nxt_after", torch.int32, (mm,)), ("copy_len", torch.int16, (mm,)),
                             ("dst_off", torch.int64, (mm,)), ("out_conn", torch.uint8, (max(nconn, 1), 48)),
                             ("conn_off", torch.int64, (nconn + 1,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        b, rin, rout = _tcprx_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                      l4_status, conn, nconn, align, blocks, out, counts)
        ws = workspace
        if ws is None:
            need = tcp_rx_workspace(m, nconn, blocks)
            ws = getattr(self, "_tcprx_ws", None)
            if ws is None or ws.numel() < need or ws.device != out["conn_off"].device:
                ws = self._tcprx_ws = torch.empty(need, dtype=torch.uint8, device=out["conn_off"].device)
        _check(lib.gcl_tcp_rx(self._ctx, ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout),
                              _ptr(counts), _ptr(ws), _nbytes(ws), stream), "gcl_tcp_rx")
        return out

    def tcp_rx_full(self, frames, n, pkt_len, sock, conn, nconn, stride=0, offs=None, frames_len=None,
                    order=None, m=None, l4_status=None, align=0, blocks=0, rep_acks=None, out=None,
                    counts=None, workspace=None, stream=None):
        """gcl_tcp_rx_full: tcp_rx_conn with the established part of its slow
        path for one runtime's list on the GPU, asynchronous.  The arguments
        are tcp_rx's; @rep_acks is a device uint8[nconn] (None: zeros), @out
        also holds "out_ext" (uint8[nconn, 16], TCP_CONN_EXT_DTYPE records) and
        @counts is a device u64[TCPRXFC_NR], accumulated.  Returns the dict:
        verdict, sflags and rcv_nxt_after are tcp_rx_acks' inputs, copy_len and
        dst_off copy_batch's, out_conn's snd_una and out_ext's xflags what
        tcp_txq's conn and want are made of."""
        import torch
        m = _pay_m(n, m, order)
        dev = frames.device if hasattr(frames, "device") else None
        out = dict(out or {})
        mm = max(m, 1)
        for f, dt, shape in (("verdict", torch.uint8, (mm,)), ("sflags", torch.uint8, (mm,)),
                             ("rcv_nxt_after", torch.int32, (mm,)), ("copy_len", torch.int16, (mm,)),
                             ("dst_off", torch.int64, (mm,)), ("out_conn", torch.uint8, (max(nconn, 1), 48)),
                             ("conn_off", torch.int64, (nconn + 1,)),
                             ("out_ext", torch.uint8, (max(nconn, 1), 16))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        b, fin, rout = _tcprxf_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                       l4_status, conn, nconn, align, blocks, out, counts, rep_acks)
        ws = workspace
        if ws is None:
            need = tcp_rx_full_workspace(m, nconn, blocks)
            ws = getattr(self, "_tcprx_ws", None)
            if ws is None or ws.numel() < need or ws.device != out["conn_off"].device:
                ws = self._tcprx_ws = torch.empty(need, dtype=torch.uint8, device=out["conn_off"].device)
        _check(lib.gcl_tcp_rx_full(self._ctx, ctypes.byref(b), ctypes.byref(fin), ctypes.byref(rout),
                                   _ptr(out["out_ext"]), _ptr(counts), _ptr(ws), _nbytes(ws), stream),
               "gcl_tcp_rx_full")
        return out

    def tcp_rx_ooo(self, frames, n, pkt_len, sock, conn, nconn, stride=0, offs=None, frames_len=None,
                   order=None, m=None, l4_status=None, align=0, blocks=0, rep_acks=None, q_off=None, q=None,
                   nq=0, q_out_cap=0, out=None, counts=None, workspace=None, stream=None):
        """gcl_tcp_rx_ooo: tcp_rx_conn with its established slow path and the
        out-of-order queue for one runtime's list on the GPU, asynchronous.
        The arguments are tcp_rx_full's; @q_off is a device int32[nconn + 1]
        (None: every queue is empty), @q a device uint8[nq, 16] of
        TCP_OOO_ENT_DTYPE records, @q_out_cap the entries out["qout"] holds.
        @out also holds the fields of TCPRXO_OUT_FIELDS and @counts is a device
        u64[TCPRXOC_NR], accumulated.  Returns the dict: copy_batch takes
        src_off + skip, copy_len and dst_off; qout_off and qout are the queues
        to relink, totals[0] the entries wanted."""
        import torch
        m = _pay_m(n, m, order)
        dev = frames.device if hasattr(frames, "device") else None
        out = dict(out or {})
        mm = max(m, 1)
        size = _tcprxo_sizes(m, nconn, nq, q_out_cap)
        for f, dt, shape in (("verdict", torch.uint8, (mm,)), ("sflags", torch.uint8, (mm,)),
                             ("rcv_nxt_after", torch.int32, (mm,)), ("copy_len", torch.int16, (mm,)),
                             ("dst_off", torch.int64, (mm,)), ("out_conn", torch.uint8, (max(nconn, 1), 48)),
                             ("conn_off", torch.int64, (nconn + 1,)),
                             ("out_ext", torch.uint8, (max(nconn, 1), 16))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        for f, w, by in TCPRXO_OUT_FIELDS:
            if f not in out:
                out[f] = torch.empty((max(size[by], 1), w), dtype=torch.uint8, device=dev)
        b, oin, rout, oout = _tcprxo_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                             l4_status, conn, nconn, align, blocks, out, counts, rep_acks, q_off,
                                             q, nq, q_out_cap)
        ws = workspace
        if ws is None:
            need = tcp_rx_ooo_workspace(m, nconn, blocks, nq)
            ws = getattr(self, "_tcprx_ws", None)
            if ws is None or ws.numel() < need or ws.device != out["conn_off"].device:
                ws = self._tcprx_ws = torch.empty(need, dtype=torch.uint8, device=out["conn_off"].device)
        _check(lib.gcl_tcp_rx_ooo(self._ctx, ctypes.byref(b), ctypes.byref(oin), ctypes.byref(rout),
                                  _ptr(out["out_ext"]), ctypes.byref(oout), _ptr(counts), _ptr(ws), _nbytes(ws),
                                  stream), "gcl_tcp_rx_ooo")
        return out

    def tcp_rx_states(self, frames, n, pkt_len, sock, conn, nconn, stride=0, offs=None, frames_len=None,
                      order=None, m=None, l4_status=None, align=0, blocks=0, rep_acks=None, q_off=None, q=None,
                      nq=0, q_out_cap=0, state=None, out=None, counts=None, workspace=None, stream=None):
        """gcl_tcp_rx_states: tcp_rx_conn with all of __tcp_rx_conn (FIN, RST,
        SYN, URG and every state but SYN_SENT) for one runtime's list on the
        GPU, asynchronous.  The arguments are tcp_rx_ooo's and @state, a device
        uint8[nconn] of TCP_STATE_* (None: the connections' flags decide).
        @out also holds the fields of TCPRXS_OUT_FIELDS (ev, state_after and
        state_out uint8, rst_seq int32) and @counts is a device
        u64[TCPRXSC_NR], accumulated.  Returns the dict: ev and rst_seq say
        which RST to send, out_ext's xflags what the runtime still owes."""
        import torch
        m = _pay_m(n, m, order)
        dev = frames.device if hasattr(frames, "device") else None
        out = dict(out or {})
        mm = max(m, 1)
        size = _tcprxo_sizes(m, nconn, nq, q_out_cap)
        size["nconn"] = nconn
        for f, dt, shape in (("verdict", torch.uint8, (mm,)), ("sflags", torch.uint8, (mm,)),
                             ("rcv_nxt_after", torch.int32, (mm,)), ("copy_len", torch.int16, (mm,)),
                             ("dst_off", torch.int64, (mm,)), ("out_conn", torch.uint8, (max(nconn, 1), 48)),
                             ("conn_off", torch.int64, (nconn + 1,)),
                             ("out_ext", torch.uint8, (max(nconn, 1), 16))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        for f, w, by in TCPRXO_OUT_FIELDS + TCPRXS_OUT_FIELDS:
            if f not in out:
                out[f] = torch.empty((max(size[by], 1), w), dtype=torch.uint8, device=dev)
        b, sin, rout, oout, sout = _tcprxs_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                                   l4_status, conn, nconn, align, blocks, out, counts, rep_acks,
                                                   q_off, q, nq, q_out_cap, state)
        ws = workspace
        if ws is None:
            need = tcp_rx_states_workspace(m, nconn, blocks, nq)
            ws = getattr(self, "_tcprx_ws", None)
            if ws is None or ws.numel() < need or ws.device != out["conn_off"].device:
                ws = self._tcprx_ws = torch.empty(need, dtype=torch.uint8, device=out["conn_off"].device)
        _check(lib.gcl_tcp_rx_states(self._ctx, ctypes.byref(b), ctypes.byref(sin), ctypes.byref(rout),
                                     _ptr(out["out_ext"]), ctypes.byref(oout), ctypes.byref(sout), _ptr(counts),
                                     _ptr(ws), _nbytes(ws), stream), "gcl_tcp_rx_states")
        return out

    def _ctlseg_device_arrays(self, out, seg_cap, dev):
        import torch
        cc = max(seg_cap, 1)
        for f, dt, shape in (("desc", torch.uint8, (cc, 32)), ("frame_off", torch.int64, (cc,)),
                             ("seg_conn", torch.int32, (cc,)), ("seg_kind", torch.uint8, (cc,)),
                             ("seg_src", torch.int32, (cc,)), ("totals", torch.int64, (2,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)

    def _tick_ws(self, need, dev):
        import torch
        ws = getattr(self, "_tick_ws_buf", None)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self._tick_ws_buf = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    def tcp_tick(self, now, tmr, conn, addr, nconn, seg_cap, frame_stride=64, frame_base=0, blocks=0,
                 out=None, counts=None, workspace=None, stream=None):
        """gcl_tcp_tick: the TCP timer sweep of one runtime's @nconn
        connections at the clock reading @now (us) on the GPU, asynchronous:
        tcp_worker's loop with tcp_handle_timeouts and tcp_timer_update, and
        the ACK and window-probe segments it sends.  @tmr, @conn and @addr are
        device uint8[nconn, 64 / 48 / 16] holding TCP_TMR_DTYPE, TCP_CONN_DTYPE
        and TCP_ADDR_DTYPE records indexed by cookie (16-B aligned).  @out maps
        TICK_OUT_FIELDS to device buffers; the ones left out are allocated on
        @tmr's device (out_tmr uint8[nconn, 32]; desc uint8[seg_cap, 32],
        frame_off int64, seg_conn and seg_src int32, seg_kind uint8; totals
        int64[2]).  @counts is a device u64[TICKC_NR], accumulated.  The
        scratch is @workspace, or a torch tensor kept on the classifier.
        Returns the dict: desc and frame_off are tx_hdr's, totals[1] its m."""
        import torch
        dev = tmr.device if hasattr(tmr, "device") else None
        out = dict(out or {})
        if "out_tmr" not in out:
            out["out_tmr"] = torch.empty((max(nconn, 1), 32), dtype=torch.uint8, device=dev)
        self._ctlseg_device_arrays(out, seg_cap, dev)
        tin, tout = _tick_structs(now, tmr, conn, addr, nconn, seg_cap, frame_base, frame_stride, blocks, out,
                                  counts)
        ws = workspace if workspace is not None else self._tick_ws(tcp_tick_workspace(nconn, blocks),
                                                                   out["totals"].device)
        _check(lib.gcl_tcp_tick(self._ctx, ctypes.byref(tin), ctypes.byref(tout), _ptr(counts), _ptr(ws),
                                _nbytes(ws), stream), "gcl_tcp_tick")
        return out

    def tcp_rx_acks(self, verdict, sflags, rcv_nxt_after, m, sock, n, conn, addr, nconn, seg_cap, order=None,
                    frame_stride=64, frame_base=0, blocks=0, out=None, counts=None, workspace=None,
                    stream=None):
        """gcl_tcp_rx_acks: the ACK segments of one tcp_rx call on the GPU,
        asynchronous: one per FAST entry with TCPRX_SF_ACK_NOW, in list order.
        @verdict, @sflags and @rcv_nxt_after are tcp_rx's outputs, @sock,
        @order, @conn and @nconn what it was given; @addr is a device
        uint8[nconn, 16] of TCP_ADDR_DTYPE records.  @out maps
        CTLSEG_OUT_FIELDS to device buffers; the ones left out are allocated on
        @verdict's device.  @counts is a device u64[TICKC_NR], accumulated
        (RXACKC_* slots).  Returns the dict: desc and frame_off are tx_hdr's,
        totals[1] its m, seg_src the list position of each ACK."""
        dev = verdict.device if hasattr(verdict, "device") else None
        out = dict(out or {})
        self._ctlseg_device_arrays(out, seg_cap, dev)
        rin, rout = _rxack_structs(verdict, sflags, rcv_nxt_after, sock, conn, addr, m, n, nconn, order, seg_cap,
                                   frame_base, frame_stride, blocks, out, counts)
        ws = workspace if workspace is not None else self._tick_ws(tcp_rx_acks_workspace(m, blocks),
                                                                   out["totals"].device)
        _check(lib.gcl_tcp_rx_acks(self._ctx, ctypes.byref(rin), ctypes.byref(rout), _ptr(counts), _ptr(ws),
                                   _nbytes(ws), stream), "gcl_tcp_rx_acks")
        return out

    def tcp_rx_ctl(self, verdict, sflags, rcv_nxt_after, ev, rst_seq, m, sock, n, conn, addr, nconn, seg_cap,
                   order=None, frame_stride=64, frame_base=0, blocks=0, out=None, counts=None, workspace=None,
                   stream=None):
        """gcl_tcp_rx_ctl: the control segments of one tcp_rx_states call on
        the GPU, asynchronous: tcp_rx_acks' ACKs and, in list order among
        them, the RST and RST|ACK segments that @ev and @rst_seq name.  The
        other arguments and the returned dict are tcp_rx_acks'; seg_kind also
        holds CTL_RST and CTL_RST_ACK."""
        dev = verdict.device if hasattr(verdict, "device") else None
        out = dict(out or {})
        self._ctlseg_device_arrays(out, seg_cap, dev)
        cin, rout = _rxctl_structs(verdict, sflags, rcv_nxt_after, ev, rst_seq, sock, conn, addr, m, n, nconn,
                                   order, seg_cap, frame_base, frame_stride, blocks, out, counts)
        ws = workspace if workspace is not None else self._tick_ws(tcp_rx_ctl_workspace(m, blocks),
                                                                   out["totals"].device)
        _check(lib.gcl_tcp_rx_ctl(self._ctx, ctypes.byref(cin), ctypes.byref(rout), _ptr(counts), _ptr(ws),
                                  _nbytes(ws), stream), "gcl_tcp_rx_ctl")
        return out

    def tcp_rx_open(self, frames, n, pkt_len, sock, m, listen, nlisten, iss, seg_cap, open_cap, tx_frames,
                    stride=0, offs=None, frames_len=None, order=None, l4_status=None, listen_base=0,
                    frame_stride=64, frame_base=0, tx_frames_len=None, blocks=0, hash_slots=0, out=None,
                    counts=None, workspace=None, stream=None):
        """gcl_tcp_rx_open: the passive open of one runtime's list on the GPU,
        asynchronous: tcp_rx_listener for the packets of listeners (cookies
        listen_base .. listen_base + nlisten) and tcp_rx_closed for
        SOCK_MISS, with the new connections, their SYN|ACKs and the RSTs.
        @listen is a device uint8[nlisten, 16] of TCP_LISTEN_DTYPE records,
        @iss a device int32[m], @tx_frames the device tx region (the option
        bytes of the SYN|ACKs are written into it).  @out maps
        TCPOPEN_OUT_FIELDS, CTLSEG_SEG_FIELDS and "seg_totals" to device
        buffers; the ones left out are allocated on @sock's device (open
        uint8[open_cap, 64]).  @counts is a device u64[OPENC_NR], accumulated.
        Returns the dict: desc and frame_off are tx_hdr's, seg_totals[1] its
        m; open[0:totals[1]] are the connections to install."""
        import torch
        dev = sock.device
        out = dict(out or {})
        sc, oc = max(seg_cap, 1), max(open_cap, 1)
        for f, dt, shape in (("verdict", torch.uint8, (max(m, 1),)), ("later_of", torch.int32, (max(m, 1),)),
                             ("rst_seq", torch.int32, (max(m, 1),)), ("open", torch.uint8, (oc, 64)),
                             ("backlog_out", torch.int32, (max(nlisten, 1),)), ("totals", torch.int64, (2,)),
                             ("seg_totals", torch.int64, (2,)), ("desc", torch.uint8, (sc, 32)),
                             ("frame_off", torch.int64, (sc,)), ("seg_conn", torch.int32, (sc,)),
                             ("seg_kind", torch.uint8, (sc,)), ("seg_src", torch.int32, (sc,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        b, oin, oout, seg = _tcpopen_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                             l4_status, listen, nlisten, listen_base, iss, seg_cap, open_cap,
                                             frame_base, frame_stride, tx_frames, tx_frames_len, blocks,
                                             hash_slots, out, counts)
        if workspace is None:
            need = tcp_rx_open_workspace(m, nlisten, blocks, hash_slots)
            ws = getattr(self, "_open_ws_buf", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._open_ws_buf = torch.empty(need, dtype=torch.uint8, device=dev)
            workspace = ws
        _check(lib.gcl_tcp_rx_open(self._ctx, ctypes.byref(b), ctypes.byref(oin), ctypes.byref(oout),
                                   ctypes.byref(seg), _ptr(counts), _ptr(workspace), _nbytes(workspace), stream),
               "gcl_tcp_rx_open")
        return out

    def udp_rx(self, frames, n, pkt_len, sock, usock, nsock, stride=0, offs=None, frames_len=None,
               order=None, m=None, l4_status=None, sock_base=0, align=0, blocks=0, out=None, counts=None,
               workspace=None, stream=None):
        """gcl_udp_rx: udp_conn_recv and udp_par_recv for one runtime's list
        @order[0..m) (None: every packet in turn) on the GPU, asynchronous.
        @sock is what sock_lookup wrote, @l4_status what l4_csum(L4_VERIFY)
        wrote, @usock a device uint8[nsock, 16] holding UDP_SOCK_DTYPE records
        (16-B aligned); cookie c names usock[c - sock_base].  @out maps
        UDPRX_OUT_FIELDS to device buffers; the ones left out are allocated on
        @frames' device (verdict and sflags uint8, copy_len int16, dst_off and
        sock_off int64, rec_idx and rec_off int32, rec uint8[m, 16], out_sock
        uint8[nsock, 16]).  @counts is a device u64[UDPRXC_NR], accumulated.
        The scratch is @workspace, or a torch tensor kept on the classifier.
        Returns the dict: with l4_payload's src_off, copy_len and dst_off are
        copy_batch's length and dst_off."""
        import torch
        m = _pay_m(n, m, order)
        dev = frames.device if hasattr(frames, "device") else None
        out = dict(out or {})
        mm = max(m, 1)
        for f, dt, shape in (("verdict", torch.uint8, (mm,)), ("sflags", torch.uint8, (mm,)),
                             ("copy_len", torch.int16, (mm,)), ("dst_off", torch.int64, (mm,)),
                             ("rec_idx", torch.int32, (mm,)), ("rec", torch.uint8, (mm, 16)),
                             ("out_sock", torch.uint8, (max(nsock, 1), 16)),
                             ("rec_off", torch.int32, (nsock + 1,)), ("sock_off", torch.int64, (nsock + 1,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        b, rin, rout = _udprx_structs(frames, n, stride, offs, pkt_len, frames_len, m, order, sock,
                                      l4_status, usock, nsock, sock_base, align, blocks, out, counts)
        ws = workspace
        if ws is None:
            need = udp_rx_workspace(m, nsock, blocks)
            ws = getattr(self, "_udprx_ws", None)
            if ws is None or ws.numel() < need or ws.device != out["sock_off"].device:
                ws = self._udprx_ws = torch.empty(need, dtype=torch.uint8, device=out["sock_off"].device)
        _check(lib.gcl_udp_rx(self._ctx, ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout),
                              _ptr(counts), _ptr(ws), _nbytes(ws), stream), "gcl_udp_rx")
        return out

    def tcp_txq(self, now, qoff, ent, cold, nent, conn, addr, nconn, seg_cap, want=None, frame_stride=64,
                frame_base=0, blocks=0, out=None, counts=None, workspace=None, stream=None):
        """gcl_tcp_txq: the retransmit queues of one runtime's @nconn
        connections at the clock reading @now (us) on the GPU, asynchronous:
        tcp_conn_ack's pops, tcp_tx_retransmit's walk and
        tcp_tx_fast_retransmit_start, and the retransmitted segments.  @qoff is
        a device int32[nconn + 1] CSR over @ent and @cold, device uint8[nent,
        16] of TXQ_ENT_DTYPE and TXQ_COLD_DTYPE records; @conn and @addr are
        device uint8[nconn, 48 / 16] (16-B aligned), @want an optional device
        uint8[nconn] of TXQ_W_* bits.  @out maps TXQ_OUT_FIELDS to device
        buffers; the ones left out are allocated on @qoff's device (out_conn
        uint8[nconn, 32], state uint8[nent]; desc uint8[seg_cap, 32],
        frame_off, src_off and dst_off int64, len int16, seg_conn and seg_ent
        int32; totals int64[3]).  @counts is a device u64[TXQC_NR],
        accumulated.  The scratch is @workspace, or a torch tensor the
        classifier keeps for this call alone (tcp_tick's is another one; two
        tcp_txq calls in flight on different streams need a @workspace each).
        Returns the dict: src_off, len and dst_off are
        copy_batch's, desc and frame_off tx_hdr's, totals[1] their m."""
        import torch
        dev = qoff.device if hasattr(qoff, "device") else None
        out = dict(out or {})
        cc = max(seg_cap, 1)
        for f, dt, shape in (("out_conn", torch.uint8, (max(nconn, 1), 32)), ("state", torch.uint8, (max(nent, 1),)),
                             ("desc", torch.uint8, (cc, 32)), ("frame_off", torch.int64, (cc,)),
                             ("src_off", torch.int64, (cc,)), ("len", torch.int16, (cc,)),
                             ("dst_off", torch.int64, (cc,)), ("seg_conn", torch.int32, (cc,)),
                             ("seg_ent", torch.int32, (cc,)), ("totals", torch.int64, (3,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        qin, qout = _txq_structs(now, qoff, ent, cold, nent, conn, addr, want, nconn, seg_cap, frame_base,
                                 frame_stride, blocks, out, counts)
        ws = workspace
        if ws is None:      # its own scratch: a sweep in flight on another stream keeps tcp_tick's
            need, ws = tcp_txq_workspace(nconn, blocks), getattr(self, "_txq_ws_buf", None)
            if ws is None or ws.numel() < need or ws.device != out["totals"].device:
                ws = self._txq_ws_buf = torch.empty(need, dtype=torch.uint8, device=out["totals"].device)
        _check(lib.gcl_tcp_txq(self._ctx, ctypes.byref(qin), ctypes.byref(qout), _ptr(counts), _ptr(ws),
                               _nbytes(ws), stream), "gcl_tcp_txq")
        return out

    def tcp_read(self, qoff, ent, nent, rd, conn, addr, nconn, item_cap, seg_cap, voff=None, iov=None, nvec=0,
                 frame_stride=64, frame_base=0, blocks=0, out=None, counts=None, workspace=None, stream=None):
        """gcl_tcp_read: tcp_read / tcp_readv on one runtime's @nconn
        connections on the GPU, asynchronous: what each read returns, what it
        takes off the receive queue, the copy items into the application's
        buffers and the window-update ACKs.  @qoff is a device int32[nconn + 1]
        CSR over @ent, device uint8[nent, 16] of RDQ_ENT_DTYPE records; @voff
        and @iov (uint8[nvec, 16], RD_IOV_DTYPE) the optional vectors; @rd,
        @conn and @addr are device uint8[nconn, 32 / 48 / 16] (16-B aligned).
        @out maps RD_OUT_FIELDS to device buffers; the ones left out are
        allocated on @qoff's device (out_conn uint8[nconn, 32]; src_off and
        dst_off int64, len int16, item_conn and item_ent int32, item_cap long;
        totals int64[4]; desc uint8[seg_cap, 32], frame_off int64, seg_conn and
        seg_src int32, seg_kind uint8; seg_totals int64[2]).  @counts is a
        device u64[RDC_NR], accumulated.  The scratch is @workspace, or a torch
        tensor the classifier keeps for this call alone.  Returns the dict:
        src_off, len and dst_off are copy_batch's with totals[1] their n, desc
        and frame_off tx_hdr's with seg_totals[1] their m."""
        import torch
        dev = qoff.device if hasattr(qoff, "device") else None
        out = dict(out or {})
        ic, sc = max(item_cap, 1), max(seg_cap, 1)
        for f, dt, shape in (("out_conn", torch.uint8, (max(nconn, 1), 32)), ("src_off", torch.int64, (ic,)),
                             ("len", torch.int16, (ic,)), ("dst_off", torch.int64, (ic,)),
                             ("item_conn", torch.int32, (ic,)), ("item_ent", torch.int32, (ic,)),
                             ("totals", torch.int64, (4,)), ("desc", torch.uint8, (sc, 32)),
                             ("frame_off", torch.int64, (sc,)), ("seg_conn", torch.int32, (sc,)),
                             ("seg_kind", torch.uint8, (sc,)), ("seg_src", torch.int32, (sc,)),
                             ("seg_totals", torch.int64, (2,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        nvec = nvec if voff is not None else 0
        rin, rout = _rd_structs(qoff, ent, nent, voff, iov, nvec, rd, conn, addr, nconn, item_cap, seg_cap,
                                frame_base, frame_stride, blocks, out, counts)
        ws = workspace
        if ws is None:
            need, ws = tcp_read_workspace(nconn, nent, nvec, blocks), getattr(self, "_rd_ws_buf", None)
            if ws is None or ws.numel() < need or ws.device != out["totals"].device:
                ws = self._rd_ws_buf = torch.empty(need, dtype=torch.uint8, device=out["totals"].device)
        _check(lib.gcl_tcp_read(self._ctx, ctypes.byref(rin), ctypes.byref(rout), _ptr(counts), _ptr(ws),
                                _nbytes(ws), stream), "gcl_tcp_read")
        return out

    def tcp_write(self, now, wr, conn, addr, nconn, seg_cap, item_cap, voff=None, iov=None, nvec=0,
                  frame_stride=2048, frame_base=0, frames_len=0, blocks=0, out=None, counts=None, workspace=None,
                  stream=None):
        """gcl_tcp_write: tcp_write / tcp_writev on one runtime's @nconn
        connections at the clock reading @now (us) on the GPU, asynchronous:
        whether each write goes ahead and what it returns, the segments it
        sends with their retransmit-queue records, the copy items out of the
        application's buffers and the tail it holds.  @wr, @conn and @addr are
        device uint8[nconn, 48 / 48 / 16] (16-B aligned) of TCP_WR_DTYPE,
        TCP_CONN_DTYPE and TCP_ADDR_DTYPE records; @voff (int32[nconn + 1]) and
        @iov (uint8[nvec, 16], RD_IOV_DTYPE) the optional vectors.  @out maps
        WR_OUT_FIELDS to device buffers; the ones left out are allocated on
        @wr's device (out_conn uint8[nconn, 48]; desc uint8[seg_cap, 32],
        frame_off int64, seg_conn int32, txq_ent and txq_cold uint8[seg_cap,
        16]; src_off and dst_off int64, len int16, item_conn and item_seg
        int32, item_cap long; totals int64[6]).  @counts is a device
        u64[WRC_NR], accumulated.  The scratch is @workspace, or a torch tensor
        the classifier keeps for this call alone.  Returns the dict: src_off,
        len and dst_off are copy_batch's with totals[3] their n, desc and
        frame_off tx_hdr's with totals[1] their m."""
        import torch
        dev = wr.device if hasattr(wr, "device") else None
        out = dict(out or {})
        sc, ic = max(seg_cap, 1), max(item_cap, 1)
        for f, dt, shape in (("out_conn", torch.uint8, (max(nconn, 1), 48)), ("desc", torch.uint8, (sc, 32)),
                             ("frame_off", torch.int64, (sc,)), ("seg_conn", torch.int32, (sc,)),
                             ("txq_ent", torch.uint8, (sc, 16)), ("txq_cold", torch.uint8, (sc, 16)),
                             ("src_off", torch.int64, (ic,)), ("len", torch.int16, (ic,)),
                             ("dst_off", torch.int64, (ic,)), ("item_conn", torch.int32, (ic,)),
                             ("item_seg", torch.int32, (ic,)), ("totals", torch.int64, (6,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        nvec = nvec if voff is not None else 0
        win, wout = _wr_structs(now, voff, iov, nvec, wr, conn, addr, nconn, seg_cap, item_cap, frame_base,
                                frame_stride, frames_len, blocks, out, counts)
        ws = workspace
        if ws is None:
            need, ws = tcp_write_workspace(nconn, nvec, blocks), getattr(self, "_wr_ws_buf", None)
            if ws is None or ws.numel() < need or ws.device != out["totals"].device:
                ws = self._wr_ws_buf = torch.empty(max(need, 16), dtype=torch.uint8, device=out["totals"].device)
        _check(lib.gcl_tcp_write(self._ctx, ctypes.byref(win), ctypes.byref(wout), _ptr(counts), _ptr(ws),
                                 _nbytes(ws), stream), "gcl_tcp_write")
        return out

    def tcp_shut(self, now, shut, tmr, conn, addr, nconn, seg_cap, frame_stride=64, frame_base=0, frames_len=0,
                 blocks=0, out=None, counts=None, workspace=None, stream=None):
        """gcl_tcp_shut: tcp_shutdown / tcp_close / tcp_abort on one runtime's
        @nconn connections at the clock reading @now (us) on the GPU,
        asynchronous: the state, timer words and flags each request leaves, and
        the FIN and RST segments with the FINs' retransmit-queue records.
        @shut, @tmr, @conn and @addr are device uint8[nconn, 16 / 64 / 48 / 16]
        (16-B aligned) of TCP_SHUT_DTYPE, TCP_TMR_DTYPE, TCP_CONN_DTYPE and
        TCP_ADDR_DTYPE records.  @out maps SHUT_OUT_FIELDS to device buffers;
        the ones left out are allocated on @shut's device (out_conn
        uint8[nconn, 48]; desc uint8[seg_cap, 32], frame_off int64, seg_conn
        int32, seg_kind uint8, seg_src int32, txq_ent and txq_cold
        uint8[seg_cap, 16]; totals int64[2]).  @counts is a device
        u64[SHUTC_NR], accumulated.  The scratch is @workspace, or a torch
        tensor the classifier keeps for this call alone.  Returns the dict:
        desc and frame_off are tx_hdr's with totals[1] their m."""
        import torch
        dev = shut.device if hasattr(shut, "device") else None
        out = dict(out or {})
        sc = max(seg_cap, 1)
        for f, dt, shape in (("out_conn", torch.uint8, (max(nconn, 1), 48)), ("desc", torch.uint8, (sc, 32)),
                             ("frame_off", torch.int64, (sc,)), ("seg_conn", torch.int32, (sc,)),
                             ("seg_kind", torch.uint8, (sc,)), ("seg_src", torch.int32, (sc,)),
                             ("txq_ent", torch.uint8, (sc, 16)), ("txq_cold", torch.uint8, (sc, 16)),
                             ("totals", torch.int64, (2,))):
            if f not in out:
                out[f] = torch.empty(shape, dtype=dt, device=dev)
        sin, sout = _shut_structs(now, shut, tmr, conn, addr, nconn, seg_cap, frame_base, frame_stride, frames_len,
                                  blocks, out, counts)
        ws = workspace
        if ws is None:
            need, ws = tcp_shut_workspace(nconn, blocks), getattr(self, "_shut_ws_buf", None)
            if ws is None or ws.numel() < need or ws.device != out["totals"].device:
                ws = self._shut_ws_buf = torch.empty(max(need, 16), dtype=torch.uint8, device=out["totals"].device)
        _check(lib.gcl_tcp_shut(self._ctx, ctypes.byref(sin), ctypes.byref(sout), _ptr(counts), _ptr(ws),
                                _nbytes(ws), stream), "gcl_tcp_shut")
        return out

    def copy_batch(self, src, src_off, length, n, dst, dst_off=None, dst_stride=0, tx_olflags=None,
                   hash=None, src_len=None, dst_len=None, dst_cap=0, len_hint=0, group=0,
                   counts=None, pkt_len=None, olflags=None, rss=None, stream=None):
        """gcl_copy_batch: the loopback frame copy of copy_batch on the GPU
        (asynchronous): frame i, @length[i] bytes at @src + @src_off[i], into
        @dst at @dst_off[i] (or i * @dst_stride), refused when it does not fit.
        @src is a device tensor or a host_register'ed numpy array; @pkt_len
        (int16), @olflags (uint8) and @rss (int32) are allocated on @dst's
        device when None; False leaves olflags or rss out.  @counts is a
        device u64[COPY_NR], accumulated.  Returns (pkt_len, olflags, rss)."""
        import torch
        dev = dst.device if hasattr(dst, "device") else None
        if pkt_len is None:
            pkt_len = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
        olflags = None if olflags is False else \
            torch.empty(max(n, 1), dtype=torch.uint8, device=dev) if olflags is None else olflags
        rss = None if rss is False else \
            torch.empty(max(n, 1), dtype=torch.int32, device=dev) if rss is None else rss
        if counts is not None and _nbytes(counts) < 8 * COPY_NR:
            raise ValueError("counts buffer too small")
        cin, cout = _copy_structs(src, src_len, src_off, length, tx_olflags, hash, n, len_hint,
                                  dst_cap, group, dst, dst_len, dst_off, dst_stride, pkt_len,
                                  olflags, rss)
        _check(lib.gcl_copy_batch(self._ctx, ctypes.byref(cin), ctypes.byref(cout), _ptr(counts),
                                  stream), "gcl_copy_batch")
        return pkt_len, olflags, rss

    def rxloop(self, region, slots=64, max_burst=GCL_RX_BURST_SIZE, workers=1, lifetime_ms=20000,
               counts=None, stats=None, region_len=None, flags=0):
        """Start the persistent rx loop over a registered host region."""
        return RxLoop(self, region, slots, max_burst, workers, lifetime_ms, counts, stats,
                      region_len, flags)

    def sync(self):
        return _check(lib.gcl_sync(self._ctx), "gcl_sync")

    def profile_sample(self, every):
        """Time one launch in `every` (GCL_CFG_PROFILE); see gcl_profile_sample."""
        return _check(lib.gcl_profile_sample(self._ctx, int(every)), "gcl_profile_sample")

    def kernel_time(self, reset=False):
        ms = ctypes.c_double()
        nl = ctypes.c_uint64()
        _check(lib.gcl_kernel_time(self._ctx, ctypes.byref(ms), ctypes.byref(nl), int(reset)),
               "gcl_kernel_time")
        return ms.value, nl.value


def version():
    return lib.gcl_version().decode()


# ------------------------------------------------------------- multi-GPU group
GROUP_LIB_PATH = os.path.join(HERE, "libgclgroup.so")
GROUP_BLOCK = 64 << 10
XCHG_RCCL, XCHG_HOST = 0, 1
GROUP_FAULT_EXCHANGE = 0x1


class GclGroupCfg(ctypes.Structure):
    """struct gcl_group_cfg (GCL_GROUP_ABI 2): `size` is filled in here."""
    _fields_ = [("block", ctypes.c_uint64), ("exchange", ctypes.c_uint32),
                ("nstreams", ctypes.c_uint32), ("init_timeout_ms", ctypes.c_uint32),
                ("size", ctypes.c_uint32)]

    def __init__(self, **kw):
        kw.setdefault("size", ctypes.sizeof(GclGroupCfg))
        super().__init__(**kw)


_glib = None


def group_lib():
    """libgclgroup.so (include/gcl_group.h), loaded on first use: the
    single-GPU binding never pulls in RCCL."""
    global _glib
    if _glib is not None:
        return _glib
    if not os.path.exists(GROUP_LIB_PATH):
        raise ImportError(f"{GROUP_LIB_PATH} missing: run `python caladan_amd/build.py`")
    gl = ctypes.CDLL(GROUP_LIB_PATH)
    vp, u16, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint16, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    sig = {
        "gcl_group_open_v2": (i32, [i32, ctypes.POINTER(i32), ctypes.POINTER(GclCfg),
                                    ctypes.POINTER(GclGroupCfg), ctypes.POINTER(vp)]),
        # the ABI-1 symbol (16-B struct gcl_group_cfg_v1), kept for old binaries
        "gcl_group_open": (i32, [i32, ctypes.POINTER(i32), ctypes.POINTER(GclCfg),
                                 vp, ctypes.POINTER(vp)]),
        "gcl_group_close": (None, [vp]),
        "gcl_group_size": (i32, [vp]),
        "gcl_group_ctx": (vp, [vp, i32]),
        "gcl_group_stream": (vp, [vp, i32]),
        "gcl_group_runtime_set": (i32, [vp, u16, u32, u16, u16, ctypes.POINTER(u16)]),
        "gcl_group_runtime_del": (i32, [vp, u16]),
        "gcl_group_runtime_set_trans_seed": (i32, [vp, u16, u32]),
        "gcl_shard_count": (u64, [u64, u32, u32, u64]),
        "gcl_shard_global": (u64, [u64, u32, u32, u64]),
        "gcl_group_classify": (i32, [vp, ctypes.POINTER(GclBatch), ctypes.POINTER(vp)]),
        "gcl_group_classify_host": (i32, [vp, ctypes.POINTER(GclBatch), vp, ctypes.POINTER(GclE2eOpts)]),
        "gcl_group_exchange": (i32, [vp]),
        "gcl_group_read": (i32, [vp, vp, vp, vp]),
        "gcl_group_reset": (i32, [vp]),
        "gcl_group_sync": (i32, [vp]),
        "gcl_group_test_fault": (i32, [vp, u32]),
        "gcl_group_rccl_ranks": (i32, [vp, ctypes.POINTER(i32)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(gl, name)
        f.restype = res
        f.argtypes = args
    _glib = gl
    return gl


def shard_count(n, world, rank, block=GROUP_BLOCK):
    return group_lib().gcl_shard_count(n, world, rank, block)


def shard_global(j, world, rank, block=GROUP_BLOCK):
    return group_lib().gcl_shard_global(j, world, rank, block)


class Group:
    """gcl_group: one dataplane driving several GPUs (include/gcl_group.h) --
    a gcl_ctx per GPU, round-robin block shards, RCCL all-gather of the
    per-runtime counts and rx counters."""

    def __init__(self, devices, max_runtimes=16, hash_mode=HASH_JENKINS, flags=0,
                 default_olflags=F_RSS_HASH | F_IP_CKSUM_GOOD, rss_key=CALADAN_RSS_KEY,
                 thread_bits=0, block=GROUP_BLOCK, exchange=XCHG_RCCL, nstreams=2,
                 init_timeout_ms=0):
        gl = group_lib()
        if isinstance(hash_mode, str):
            hash_mode = HASH_MODES[hash_mode]
        cfg = GclCfg(max_runtimes=max_runtimes, hash_mode=hash_mode, flags=flags,
                     default_olflags=default_olflags, thread_bits=thread_bits)
        key = bytes(rss_key)[:40].ljust(40, b"\0")
        for i in range(40):
            cfg.rss_key[i] = key[i]
        self.devices = list(devices)
        self.n = len(self.devices)
        self.max_runtimes = max_runtimes
        self.vbytes = verdict_bytes(flags)
        self.block = block
        devs = (ctypes.c_int * self.n)(*self.devices)
        gc = GclGroupCfg(block=block, exchange=exchange, nstreams=nstreams,
                         init_timeout_ms=init_timeout_ms)
        self._g = ctypes.c_void_p()
        _check(gl.gcl_group_open_v2(self.n, devs, ctypes.byref(cfg), ctypes.byref(gc), ctypes.byref(self._g)),
               "gcl_group_open_v2")

    def close(self):
        if self._g:
            group_lib().gcl_group_close(self._g)
            self._g = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stream(self, i=0):
        return group_lib().gcl_group_stream(self._g, i)

    def runtime_set(self, uniqid, ip, thread_count, active_count, flow_tbl=None):
        tbl = None
        if flow_tbl is not None:
            tbl = (ctypes.c_uint16 * max(len(flow_tbl), 1))(*flow_tbl)
        return _check(group_lib().gcl_group_runtime_set(self._g, uniqid, ip, thread_count, active_count, tbl),
                      "gcl_group_runtime_set")

    def runtime_del(self, uniqid):
        return _check(group_lib().gcl_group_runtime_del(self._g, uniqid), "gcl_group_runtime_del")

    def classify(self, shards, verdicts):
        """shards: one dict per GPU (frames, n, stride, and optional offs,
        olflags, rss, fdir_hi, dst_hint, frames_len) of device buffers on that
        GPU; verdicts: one device buffer per GPU.  Asynchronous."""
        if len(shards) != self.n or len(verdicts) != self.n:
            raise ValueError("one shard and one verdict buffer per GPU")
        bs = (GclBatch * self.n)()
        vs = (ctypes.c_void_p * self.n)()
        for i, (s, v) in enumerate(zip(shards, verdicts)):
            if _nbytes(v) < self.vbytes * s["n"]:
                raise ValueError("verdict buffer too small")
            bs[i] = GclBatch(frames=_ptr(s["frames"]), frames_len=_frames_len(s["frames"], s.get("frames_len")),
                             stride=s.get("stride", 0), offs=_ptr(s.get("offs")),
                             olflags=_ptr(s.get("olflags")), rss=_ptr(s.get("rss")),
                             fdir_hi=_ptr(s.get("fdir_hi")), pkt_len=None, n=s["n"],
                             dst_hint=_ptr(s.get("dst_hint")))
            vs[i] = _ptr(v)
        return _check(group_lib().gcl_group_classify(self._g, bs, vs), "gcl_group_classify")

    def classify_host(self, frames, n, stride=0, verdicts=None, offs=None, olflags=None, rss=None,
                      fdir_hi=None, dst_hint=None, frames_len=None, mode=E2E_ZEROCOPY, nstreams=0):
        """One host batch split round-robin over the GPUs (synchronous)."""
        if verdicts is None or _nbytes(verdicts) < self.vbytes * n:
            raise ValueError("verdict buffer too small")
        b = GclBatch(frames=_ptr(frames), frames_len=_frames_len(frames, frames_len), stride=stride,
                     offs=_ptr(offs), olflags=_ptr(olflags), rss=_ptr(rss), fdir_hi=_ptr(fdir_hi),
                     pkt_len=None, n=n, dst_hint=_ptr(dst_hint))
        o = GclE2eOpts(mode=mode, nstreams=nstreams, chunk=0)
        return _check(group_lib().gcl_group_classify_host(self._g, ctypes.byref(b), _ptr(verdicts),
                                                          ctypes.byref(o)), "gcl_group_classify_host")

    def exchange(self):
        return _check(group_lib().gcl_group_exchange(self._g), "gcl_group_exchange")

    def read(self):
        """(node counts u64[R], node stats u64[8], per-GPU vectors u64[n, R + 8])
        of the last exchange."""
        c = np.zeros(self.max_runtimes, dtype=np.uint64)
        s = np.zeros(NR_STATS, dtype=np.uint64)
        p = np.zeros((self.n, self.max_runtimes + NR_STATS), dtype=np.uint64)
        _check(group_lib().gcl_group_read(self._g, c.ctypes.data, s.ctypes.data, p.ctypes.data),
               "gcl_group_read")
        return c, s, p

    def reset(self):
        return _check(group_lib().gcl_group_reset(self._g), "gcl_group_reset")

    def sync(self):
        return _check(group_lib().gcl_group_sync(self._g), "gcl_group_sync")

    def rccl_ranks(self):
        """gcl_group_rccl_ranks: ranks of the RCCL communicators (ncclCommCount), 0 for a host exchange."""
        r = ctypes.c_int()
        _check(group_lib().gcl_group_rccl_ranks(self._g, ctypes.byref(r)), "gcl_group_rccl_ranks")
        return r.value

    def test_fault(self, what=GROUP_FAULT_EXCHANGE):
        """gcl_group_test_fault (tests): every later RCCL exchange fails as a
        timed-out enqueue would; 0 clears it."""
        return _check(group_lib().gcl_group_test_fault(self._g, what), "gcl_group_test_fault")


__all__ = [n for n in dir() if not n.startswith("_")]


class RxLoop:
    """gcl_rxloop_*: burst-at-a-time classification by a persistent kernel."""

    def __init__(self, clf, region, slots, max_burst, workers, lifetime_ms, counts, stats,
                 region_len=None, flags=0):
        self.clf, self.max_burst = clf, max_burst
        cfg = GclRxloopCfg(slots=slots, max_burst=max_burst, workers=workers,
                           lifetime_ms=lifetime_ms, region=_ptr(region),
                           region_len=_nbytes(region) if region_len is None else region_len,
                           counts=_ptr(counts), stats=_ptr(stats), flags=flags)
        h = ctypes.c_void_p()
        _check(lib.gcl_rxloop_start(clf._ctx, ctypes.byref(cfg), ctypes.byref(h)), "gcl_rxloop_start")
        self._h = h
        clf._loop = self

    def submit(self, offs, olflags=None, rss=None, fdir_hi=None, dst_hint=None):
        """Returns the ticket, or a negative errno (-EAGAIN: ring full)."""
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        conv = lambda a, dt: None if a is None else np.ascontiguousarray(a, dtype=dt)
        self._keep = [conv(olflags, np.uint8), conv(rss, np.uint32), conv(fdir_hi, np.uint32),
                      conv(dst_hint, np.uint32)]
        o, r, f, d = self._keep
        return lib.gcl_rxloop_submit(self._h, len(offs), _ptr(offs), _ptr(o), _ptr(r), _ptr(f), _ptr(d))

    def wait(self, ticket, n, spin_ns=2_000_000_000):
        """Verdicts of a burst of @n packets (numpy structured array)."""
        out = np.zeros(n, dtype=verdict_dtype(self.clf.vbytes))
        ret = lib.gcl_rxloop_wait(self._h, ticket, out.ctypes.data, spin_ns)
        if ret:
            raise OSError(-ret, f"gcl_rxloop_wait: {os.strerror(-ret)}")
        return out

    def peek(self, ticket, spin_ns=2_000_000_000):
        """The burst's verdict records in place in the ring slot (a numpy
        view of LOOP_REC_DTYPE, valid until release(ticket))."""
        p = ctypes.c_void_p()
        n = ctypes.c_uint32()
        ret = lib.gcl_rxloop_peek(self._h, ticket, spin_ns, ctypes.byref(p), ctypes.byref(n))
        if ret:
            raise OSError(-ret, f"gcl_rxloop_peek: {os.strerror(-ret)}")
        buf = (ctypes.c_uint8 * (16 * n.value)).from_address(p.value)
        return np.frombuffer(buf, dtype=LOOP_REC_DTYPE)

    def release(self, ticket):
        return _check(lib.gcl_rxloop_release(self._h, ticket), "gcl_rxloop_release")

    def trans(self, ticket, n):
        """The burst's transport demux hashes (TRANS_DTYPE[n]), GCL_CFG_TRANS_HASH contexts."""
        out = np.zeros(n, dtype=TRANS_DTYPE)
        _check(lib.gcl_rxloop_trans(self._h, ticket, out.ctypes.data), "gcl_rxloop_trans")
        return out

    def poll_stats(self):
        """{early, stale, late}: how the bursts so far arrived (gcl_rxloop_poll_stats)."""
        out = np.zeros(3, dtype=np.uint64)
        _check(lib.gcl_rxloop_poll_stats(self._h, out.ctypes.data), "gcl_rxloop_poll_stats")
        return dict(zip(("early", "stale", "late"), (int(x) for x in out)))

    def lean_bursts(self):
        """Bursts classified on rxloop64_kernel's lean path (gcl_rxloop_lean_bursts)."""
        out = np.zeros(1, dtype=np.uint64)
        _check(lib.gcl_rxloop_lean_bursts(self._h, out.ctypes.data), "gcl_rxloop_lean_bursts")
        return int(out[0])

    def drive(self, offs, iters, depth=1):
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lat = np.zeros(iters, dtype=np.uint64)
        el = ctypes.c_uint64()
        _check(lib.gcl_rxloop_drive(self._h, len(offs), _ptr(offs), iters, depth, lat.ctypes.data,
                                    ctypes.byref(el)), "gcl_rxloop_drive")
        return lat, el.value

    def stop(self):
        if self._h:
            h, self._h = self._h, None
            if getattr(self.clf, "_loop", None) is self:
                self.clf._loop = None
            _check(lib.gcl_rxloop_stop(h), "gcl_rxloop_stop")

    def __del__(self):
        try:
            self.stop()
        except Exception:
            pass
