"""Cases and an independent model for gcl_tcp_write (include/gclassify.h).

The model is written from the reference's runtime/net/tcp.c (tcp_write_wait
:1259-1307, tcp_write_finish :1309-1349, tcp_write3 :1362-1380, tcp_writev2
:1392-1422) and tcp_out.c (tcp_tx_send :313-386, __tcp_add_tcphdr :54-81) as
loops over a simulated mbuf.  It shares nothing with csrc/gcl_tcpwrite.h: no
closed form, no count of passes; the C size_t arithmetic of the hold test is
done modulo 2^64 as the reference's compiler does it.
"""
import numpy as np

from caladan_amd import gclassify as G

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
ACK, PSH = 0x10, 0x08
HDR = 54                 # Ethernet + IPv4 + TCP
SIZEOF_TCP_HDR = 20
EAGAIN, ENOSPC, EPIPE, ENOBUFS = 11, 28, 32, 105
ESTABLISHED = 4          # TCP_STATE_ESTABLISHED; a state below it stands for GCL_WR_BELOW_EST
NOW = 0x1234_5678_9ABC


def wraps_lte(a, b):
    """inc/base/stddef.h"""
    d = (a - b) & M32
    return d == 0 or d >= 0x80000000


def conn(**kw):
    """one connection's write; the defaults are an established connection with room"""
    c = dict(flags=G.WR_WANT, snd_una=1000, snd_nxt=1000, snd_wnd=65535, rcv_nxt=7000, rcv_wnd=4096, wscale=0,
             mss=1448, ecn=0, err=0, tx_last_ack=7000, pend_len=0, pend_frame_off=0, src_off=0, len=0, vecs=None,
             lip=0x0A000001, rip=0x0A000002, lport=80, rport=5555)
    c.update(kw)
    if c["vecs"] is not None:
        c["flags"] |= G.WR_VEC
    return c


class Batch:
    """the arrays of one call"""

    def __init__(self, conns, use_voff=True, voff=None):
        self.conns = conns
        self.nconn = n = len(conns)
        self.use_voff = use_voff
        self.wr = np.zeros(max(n, 1), dtype=G.TCP_WR_DTYPE)
        self.conn = np.zeros(max(n, 1), dtype=G.TCP_CONN_DTYPE)
        self.addr = np.zeros(max(n, 1), dtype=G.TCP_ADDR_DTYPE)
        self.voff = np.zeros(n + 1, dtype=np.uint32)
        vecs = []
        for i, c in enumerate(conns):
            w = self.wr[i]
            for f in ("src_off", "len", "tx_last_ack", "pend_frame_off", "pend_len", "err", "ecn", "flags"):
                w[f] = c[f]
            w["snd_mss"] = c["mss"]
            for f in ("snd_una", "snd_nxt", "snd_wnd", "rcv_nxt", "rcv_wnd"):
                self.conn[i][f] = c[f]
            for f in ("lip", "rip", "lport", "rport"):
                self.addr[i][f] = c[f]
            self.addr[i]["rcv_wscale"] = c["wscale"]
            self.voff[i] = len(vecs)
            vecs += c["vecs"] or []
            self.voff[i + 1] = len(vecs)
        self.nvec = len(vecs)
        self.iov = np.zeros(max(self.nvec, 1), dtype=G.RD_IOV_DTYPE)
        for i, (off, ln) in enumerate(vecs):
            self.iov[i]["off"], self.iov[i]["len"] = off, ln
        if voff is not None:               # garbage offsets, as given
            self.voff = np.array(voff, dtype=np.uint32)
            assert len(self.voff) == n + 1

    def run_host(self, seg_cap, item_cap, frame_base=0, frame_stride=2048, frames_len=0, counts=None):
        return G.tcp_write_host(NOW, self.wr, self.conn, self.addr, seg_cap, item_cap,
                                voff=self.voff if self.use_voff else None, iov=self.iov, frame_stride=frame_stride,
                                frame_base=frame_base, frames_len=frames_len, nconn=self.nconn, nvec=self.nvec,
                                counts=counts)

    def expect(self, seg_cap, item_cap, frame_base=0, frame_stride=2048, frames_len=0):
        return model(self, seg_cap, item_cap, frame_base, frame_stride, frames_len)

    def enough(self):
        """caps that hold every segment and item: the model's own totals"""
        t = model(self, 1 << 31, 1 << 31, 0, 1 << 20, 0, totals_only=True)
        return max(int(t[0]), 1), max(int(t[2]), 1)


class Mbuf:
    def __init__(self, seg_seq, frame_off):
        self.seg_seq = self.seg_end = seg_seq
        self.length = 0          # mbuf_length: the payload, no header pushed yet
        self.frame_off = frame_off
        self.flags = ACK
        self.sent_as = None      # its index among the connection's sent segments


class Sim:
    """one connection while tcp_write3 / tcp_writev2 runs"""

    def __init__(self, c, alloc):
        self.mss = c["mss"]
        self.snd_nxt = c["snd_nxt"]
        self.tx_pending = None
        if c["pend_len"]:
            m = Mbuf((c["snd_nxt"] - c["pend_len"]) & M32, c["pend_frame_off"])
            m.length = c["pend_len"]
            m.seg_end = c["snd_nxt"]
            self.tx_pending = m
        self.alloc = alloc       # net_tx_alloc_mbuf_sz: the next slot's frame_off
        self.txq = []
        self.items = []          # (src_off, len, dst_off, mbuf)
        self.shorts = 0

    def tcp_tx_send(self, buf, length, push):
        pos, end = 0, length
        while True:                              # do {
            if self.tx_pending is not None:
                m = self.tx_pending
                self.tx_pending = None
                seglen = min(end - pos, self.mss - m.length)
                m.seg_end = (m.seg_end + seglen) & M32
            else:
                seglen = min(end - pos, self.mss)
                m = Mbuf(self.snd_nxt, self.alloc())
                m.seg_end = (self.snd_nxt + seglen) & M32
            self.items.append((buf + pos, seglen, m.frame_off + HDR + m.length, m))   # memcpy(mbuf_put())
            m.length += seglen
            self.snd_nxt = (self.snd_nxt + seglen) & M32
            pos += seglen
            if not push and pos == end and ((m.length - SIZEOF_TCP_HDR) & M64) < self.mss:
                self.tx_pending = m
                break
            if not push and pos == end:
                self.shorts += 1                 # the under-20 tail
            if push and pos == end:
                m.flags |= PSH
            m.sent_as = len(self.txq)
            self.txq.append(m)
            if not pos < end:                    # } while (pos < end)
                break
        return pos


def run_conn(c, vecs, winlen, alloc):
    """tcp_write3 or tcp_writev2 behind tcp_write_wait; returns the Sim and ret"""
    s = Sim(c, alloc)
    if vecs is None:
        return s, s.tcp_tx_send(c["src_off"], min(c["len"], winlen), True)
    sent = 0
    for i, (off, ln) in enumerate(vecs):
        if winlen <= 0:
            break
        if not ln:
            continue
        ret = s.tcp_tx_send(off, min(ln, winlen), i == len(vecs) - 1 and ln <= winlen)
        winlen -= ret
        sent += ret
    return s, sent


def model(b, seg_cap, item_cap, frame_base, frame_stride, frames_len, totals_only=False):
    n = b.nconn
    oc = np.zeros(max(n, 1), dtype=G.WR_CONN_OUT_DTYPE)
    segs, items = [], []
    counts = np.zeros(G.WRC_NR, dtype=np.uint64)
    S = I = K = 0            # wanted by the connections that went ahead
    named = 0                # vectors named by the wanted vector writes before
    done_segs = done_items = done_slots = done_ret = 0
    slot_cap = None if not frames_len else (max(frames_len - frame_base, 0) // frame_stride)
    for i, c in enumerate(b.conns):
        fl = c["flags"]
        o = oc[i]
        o["snd_nxt"], o["pend_len"], o["pend_frame_off"] = c["snd_nxt"], c["pend_len"], c["pend_frame_off"]
        o["first_seg"], o["first_item"] = min(S, seg_cap), min(I, item_cap)
        status, ret, flags = G.WRS_NONE, 0, 0
        vecs, bad = None, False
        if fl & G.WR_VEC:
            if not b.use_voff:
                bad = True
            else:
                lo, hi = int(b.voff[i]), int(b.voff[i + 1])
                bad = lo > hi or hi > b.nvec or hi - lo > G.WR_MAX_IOV
                if not bad:
                    vecs = [(int(v["off"]), int(v["len"])) for v in b.iov[lo:hi]]
                    if named + len(vecs) > b.nvec:
                        bad = True
                    if fl & G.WR_WANT:
                        named += len(vecs)
        full = wraps_lte((c["snd_una"] + c["snd_wnd"]) & M32, c["snd_nxt"])
        go = False
        if not fl & G.WR_WANT:
            pass
        elif bad or c["mss"] == 0 or c["pend_len"] > c["mss"] or HDR + c["mss"] > frame_stride:
            status = G.WRS_REFUSED
        else:
            # tcp_write_wait
            tx_closed, zero_wnd = bool(fl & G.WR_TX_CLOSED), bool(fl & G.WR_ZERO_WND)
            state = ESTABLISHED - 1 if fl & G.WR_BELOW_EST else ESTABLISHED
            if not tx_closed and (state < ESTABLISHED or fl & G.WR_TX_EXCL or full):
                if not zero_wnd and full:
                    flags |= G.WRO_ZWND_ARM
                if fl & G.WR_NONBLOCK:
                    status, ret = G.WRS_AGAIN, -EAGAIN
                else:
                    status = G.WRS_BLOCK
            else:
                if zero_wnd:
                    flags |= G.WRO_ZWND_CLEAR          # c->zero_wnd = false
                winlen = (c["snd_una"] + c["snd_wnd"] - c["snd_nxt"]) & M32
                if tx_closed:
                    status, ret = G.WRS_CLOSED, (-c["err"] if c["err"] else -EPIPE)
                elif winlen < (c["len"] if (fl & G.WR_NO_PARTIAL and not fl & G.WR_VEC) else 0):
                    status, ret = G.WRS_NOSPC, -ENOSPC
                else:
                    go = True
        if go:
            flags |= G.WRO_ACKS_RESET | G.WRO_TXWAKE
            slots = [0]

            def alloc():
                slots[0] += 1
                return (frame_base + (K + slots[0] - 1) * frame_stride) & M64
            s, ret = run_conn(c, vecs, winlen, alloc)
            fits = S + len(s.txq) <= seg_cap and I + len(s.items) <= item_cap and \
                (slot_cap is None or K + slots[0] <= slot_cap)
            if fits and not totals_only:
                status = G.WRS_DONE
                tx_last_ack = c["rcv_nxt"] if s.txq else c["tx_last_ack"]      # __tcp_add_tcphdr
                if c["rcv_nxt"] != tx_last_ack:
                    flags |= G.WRO_ACK_TS
                if wraps_lte((c["snd_una"] + c["snd_wnd"]) & M32, s.snd_nxt):
                    flags |= G.WRO_POLLOUT_CLEAR
                for m in s.txq:
                    segs.append(dict(c=i, flags=m.flags, seq=m.seg_seq, end=m.seg_end, paylen=m.length,
                                     frame_off=m.frame_off))
                for src, ln, dst, m in s.items:
                    items.append((src & M64, ln, dst & M64, i, G.WR_SEG_HELD if m.sent_as is None else S + m.sent_as))
                o["snd_nxt"], o["nseg"], o["nitems"] = s.snd_nxt, len(s.txq), len(s.items)
                p = s.tx_pending
                o["pend_len"], o["pend_frame_off"] = (p.length, p.frame_off) if p else (0, 0)
                counts[G.WRC_SEGS] += len(s.txq)
                counts[G.WRC_PUSH] += sum(1 for m in s.txq if m.flags & PSH)
                counts[G.WRC_HELD] += p is not None
                counts[G.WRC_SHORT] += s.shorts
                counts[G.WRC_ITEMS] += len(s.items)
                counts[G.WRC_BYTES] += ret
                done_segs, done_items = done_segs + len(s.txq), done_items + len(s.items)
                done_slots, done_ret = done_slots + slots[0], done_ret + ret
            else:
                status, ret, flags = G.WRS_NOSPACE, -ENOBUFS, 0
            S, I, K = S + len(s.txq), I + len(s.items), K + slots[0]
        o["ret"], o["status"], o["flags"] = ret, status, flags
        counts[status] += 1
    totals = np.array([S, done_segs, I, done_items, done_slots, done_ret], dtype=np.uint64)
    if totals_only:
        return totals
    ns, ni = len(segs), len(items)
    exp = dict(out_conn=oc[:n], totals=totals, counts=counts,
               desc=np.zeros(ns, dtype=G.TXH_DESC_DTYPE), frame_off=np.zeros(ns, dtype=np.uint64),
               seg_conn=np.zeros(ns, dtype=np.uint32), txq_ent=np.zeros(ns, dtype=G.TXQ_ENT_DTYPE),
               txq_cold=np.zeros(ns, dtype=G.TXQ_COLD_DTYPE), src_off=np.zeros(ni, dtype=np.uint64),
               len=np.zeros(ni, dtype=np.uint16), dst_off=np.zeros(ni, dtype=np.uint64),
               item_conn=np.zeros(ni, dtype=np.uint32), item_seg=np.zeros(ni, dtype=np.uint32))
    for k, sg in enumerate(segs):
        c = b.conns[sg["c"]]
        d = exp["desc"][k]
        d["lip"], d["rip"], d["lport"], d["rport"] = c["lip"], c["rip"], c["lport"], c["rport"]
        d["proto"], d["tcp_flags"], d["tcp_off"], d["ecn"] = 6, sg["flags"], 5, c["ecn"]
        d["seq"], d["ack"] = sg["seq"], c["rcv_nxt"]
        d["win"] = (c["rcv_wnd"] >> (c["wscale"] & 31)) & 0xFFFF       # hton16(win >> rcv_wscale)
        d["paylen"] = sg["paylen"]
        exp["frame_off"][k], exp["seg_conn"][k] = sg["frame_off"], sg["c"]
        e, q = exp["txq_ent"][k], exp["txq_cold"][k]
        e["seg_seq"], e["seg_end"], e["ts"] = sg["seq"], sg["end"], NOW
        q["frame_off"], q["tcp_flags"], q["tcp_off"], q["flags"] = sg["frame_off"], sg["flags"], 5, G.TXQE_INFLIGHT
    for k, it in enumerate(items):
        for f, v in zip(G.WR_ITEM_FIELDS, it):
            exp[f][k] = v
    return exp


def raw(a, nbytes):
    """the first @nbytes bytes of a numpy array or a torch tensor's numpy copy"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:nbytes].tobytes()


def check(b, got, exp, counts=None):
    """every output byte of @got (numpy arrays of any element type) against the model's"""
    n = b.nconn
    goc = np.frombuffer(raw(got["out_conn"], 48 * n), dtype=G.WR_CONN_OUT_DTYPE)
    for i in range(n):
        assert goc[i].tobytes() == exp["out_conn"][i].tobytes(), (i, goc[i], exp["out_conn"][i])
    assert raw(got["totals"], 48) == exp["totals"].tobytes(), (np.frombuffer(raw(got["totals"], 48), dtype=np.uint64),
                                                                exp["totals"])
    for f in G.WR_SEG_FIELDS + G.WR_ITEM_FIELDS:
        want = exp[f].tobytes()
        have = raw(got[f], len(want))
        if have != want:
            w = G.WR_OUT_WIDTH[f]
            k = next(k for k in range(len(exp[f])) if have[k * w:(k + 1) * w] != want[k * w:(k + 1) * w])
            raise AssertionError((f, k, have[k * w:(k + 1) * w].hex(), exp[f][k]))
    if counts is not None:
        assert np.asarray(counts).tolist() == exp["counts"].tolist(), (counts, exp["counts"])


def W(**kw):
    return conn(**kw)


def hand_cases():
    """(name, conns, {conn: (status, ret, snd_nxt_out, nseg, nitems, pend_len_out, flags)}, segs, voff)

    voff, when not None, replaces the CSR offsets the vectors were laid out with.
    segs, when given, lists (conn, tcp_flags, seq, paylen) of every sent segment in order.  All numbers are
    worked out by hand from the reference's loops; OK = ACKS_RESET | TXWAKE."""
    OK = G.WRO_ACKS_RESET | G.WRO_TXWAKE
    D, V = G.WRS_DONE, lambda *lens: [(4096 * (i + 1), ln) for i, ln in enumerate(lens)]
    cases = []
    # mss 100.  Vectors 100 + 19, !push on the first, the second is last and fits: push.  So to see the
    # under-20 rule the short tail must end a vector that is not the last: 119 bytes then an EMPTY last
    # vector (push never comes).  119 = 100 (sent, ACK) + 19: fill 19, (19 - 20) wraps: not < mss: sent
    # short, ACK without PSH; nothing held.
    cases.append(("vec_tail_19_sent_short", [W(mss=100, vecs=V(119, 0))],
                  {0: (D, 119, 1119, 2, 2, 0, OK)}, [(0, ACK, 1000, 100), (0, ACK, 1100, 19)]))
    # 120 = 100 + 20: fill 20, 20 - 20 = 0 < 100: held.
    cases.append(("vec_tail_20_held", [W(mss=100, vecs=V(120, 0))],
                  {0: (D, 120, 1120, 1, 2, 20, OK)}, [(0, ACK, 1000, 100)]))
    # vectors 100, 1, 0 at mss 100: the first is a full segment, fill 100 >= 20: HELD; the second finds it
    # full: takes 0 (an item of 0 bytes), sent without PSH; then a new segment takes 1 byte: fill 1: short.
    cases.append(("held_full_mss_then_one_byte", [W(mss=100, vecs=V(100, 1, 0))],
                  {0: (D, 101, 1101, 2, 3, 0, OK)}, [(0, ACK, 1000, 100), (0, ACK, 1100, 1)]))
    # window 50 (snd_wnd 50), one vector of 80, mss 100: min(80, 50) = 50 with push = (last && 80 <= 50) =
    # false: fill 50: held; ret = winlen = 50; the window is now full: POLLOUT_CLEAR; nothing sent and
    # rcv_nxt == tx_last_ack: no ACK_TS.
    cases.append(("last_vector_longer_than_window", [W(mss=100, snd_wnd=50, vecs=V(80))],
                  {0: (D, 50, 1050, 0, 1, 50, OK | G.WRO_POLLOUT_CLEAR)}, []))
    # vectors 30, 0: the last is empty, so push never comes: 30 held.  rcv_nxt != tx_last_ack and nothing
    # sent: ACK_TS.
    cases.append(("trailing_empty_vector", [W(mss=100, tx_last_ack=6999, vecs=V(30, 0))],
                  {0: (D, 30, 1030, 0, 1, 30, OK | G.WRO_ACK_TS)}, []))
    # 40 held (seg_seq 960), a plain write of 0 bytes: one pass takes 0, push && pos == end: PSH, sent
    # with its 40 bytes from seq 960; ret 0.  tx_last_ack becomes rcv_nxt: no ACK_TS though they differed.
    cases.append(("pending_flushed_by_empty_write", [W(mss=100, pend_len=40, pend_frame_off=777, tx_last_ack=1)],
                  {0: (D, 0, 1000, 1, 1, 0, OK)}, [(0, ACK | PSH, 960, 40)]))
    cases.append(("empty_write_nothing_held", [W(mss=100)], {0: (D, 0, 1000, 1, 1, 0, OK)}, [(0, ACK | PSH, 1000, 0)]))
    # three vectors 30, 30, 30 at mss 100: held 30, held 60, then push: one segment of 90 with PSH.
    cases.append(("segment_gathers_three_vectors", [W(mss=100, vecs=V(30, 30, 30))],
                  {0: (D, 90, 1090, 1, 3, 0, OK)}, [(0, ACK | PSH, 1000, 90)]))
    # NO_PARTIAL: window 99 against len 100: -ENOSPC; window 100: goes, one segment, window full after.
    cases.append(("no_partial_one_byte_short",
                  [W(mss=100, snd_wnd=99, len=100, flags=G.WR_WANT | G.WR_NO_PARTIAL),
                   W(mss=100, snd_wnd=100, len=100, flags=G.WR_WANT | G.WR_NO_PARTIAL),
                   W(mss=100, snd_wnd=99, len=100)],
                  {0: (G.WRS_NOSPC, -28, 1000, 0, 0, 0, 0), 1: (D, 100, 1100, 1, 1, 0, OK | G.WRO_POLLOUT_CLEAR),
                   2: (D, 99, 1099, 1, 1, 0, OK | G.WRO_POLLOUT_CLEAR)},
                  [(1, ACK | PSH, 1000, 100), (2, ACK | PSH, 1000, 99)]))
    cases.append(("epipe_against_err",
                  [W(flags=G.WR_WANT | G.WR_TX_CLOSED, len=5), W(flags=G.WR_WANT | G.WR_TX_CLOSED, err=104, len=5)],
                  {0: (G.WRS_CLOSED, -32, 1000, 0, 0, 0, 0), 1: (G.WRS_CLOSED, -104, 1000, 0, 0, 0, 0)}, []))
    # a full window (snd_wnd 0): ARM unless zero_wnd is already set; BELOW_EST and TX_EXCL wait without it
    cases.append(("zwnd_arm_with_and_without_nonblock",
                  [W(snd_wnd=0, len=5), W(snd_wnd=0, len=5, flags=G.WR_WANT | G.WR_NONBLOCK),
                   W(snd_wnd=0, len=5, flags=G.WR_WANT | G.WR_ZERO_WND),
                   W(len=5, flags=G.WR_WANT | G.WR_BELOW_EST | G.WR_NONBLOCK), W(len=5, flags=G.WR_WANT | G.WR_TX_EXCL)],
                  {0: (G.WRS_BLOCK, 0, 1000, 0, 0, 0, G.WRO_ZWND_ARM), 1: (G.WRS_AGAIN, -11, 1000, 0, 0, 0, G.WRO_ZWND_ARM),
                   2: (G.WRS_BLOCK, 0, 1000, 0, 0, 0, 0), 3: (G.WRS_AGAIN, -11, 1000, 0, 0, 0, 0),
                   4: (G.WRS_BLOCK, 0, 1000, 0, 0, 0, 0)}, []))
    # tcp.c:1285 runs before the closed test; a closed connection with a full window does not wait
    cases.append(("zwnd_clear_on_closed",
                  [W(flags=G.WR_WANT | G.WR_TX_CLOSED | G.WR_ZERO_WND, snd_wnd=0, len=5),
                   W(flags=G.WR_WANT | G.WR_ZERO_WND, len=5, mss=100)],
                  {0: (G.WRS_CLOSED, -32, 1000, 0, 0, 0, G.WRO_ZWND_CLEAR), 1: (D, 5, 1005, 1, 1, 0, OK | G.WRO_ZWND_CLEAR)},
                  [(1, ACK | PSH, 1000, 5)]))
    # snd_nxt 2^32 - 150, 250 bytes at mss 100: seq wraps inside the second segment
    t = (1 << 32) - 150
    cases.append(("seq_wraps_inside_write", [W(mss=100, snd_una=t, snd_nxt=t, len=250)],
                  {0: (D, 250, 100, 3, 3, 0, OK)},
                  [(0, ACK, t, 100), (0, ACK, t + 100, 100), (0, ACK | PSH, 50, 50)]))
    R = (G.WRS_REFUSED, 0, 1000, 0, 0, 0, 0)
    cases.append(("refused_causes",
                  [W(mss=0, len=5), W(mss=100, pend_len=101, len=5), W(mss=2048 - 54 + 1, len=5),
                   W(mss=100, vecs=V(5)), W(mss=100, vecs=[]), W(mss=2048 - 54, len=5)],
                  {0: R, 1: R[:5] + (101, 0), 2: R, 3: R, 4: R, 5: (D, 5, 1005, 1, 1, 0, OK)}, [(5, ACK | PSH, 1000, 5)],
                  [0, 0, 0, 1, 0, 9, 9]))       # 3: [1, 0) inverted; 4: [0, 9) past nvec = 1
    return [c if len(c) == 5 else c + (None,) for c in cases]


def too_many_vectors():
    """1025 vectors on connection 0 (REFUSED), 1024 on connection 1 (DONE)"""
    return Batch([conn(mss=100, vecs=[(i, 1) for i in range(G.WR_MAX_IOV + 1)]),
                  conn(mss=100, vecs=[(i, 1) for i in range(G.WR_MAX_IOV)])])


def garbage_voff_batch():
    """three vectors; the ranges [0,2) ok, [2,1) inverted, [1,2) overlapping 0's and read again, [2,0)
    inverted, [0,3) naming more vectors with those before than there are, [3,1) inverted, [1, 2^32-1) past
    nvec: DONE, REFUSED, DONE and four REFUSED"""
    cs = [conn(mss=100, vecs=[(0, 50), (100, 50)]), conn(mss=100, vecs=[]), conn(mss=100, vecs=[(200, 10)])] + \
         [conn(mss=100, vecs=[]) for _ in range(4)]
    return Batch(cs, voff=[0, 2, 1, 2, 0, 3, 1, 0xFFFFFFFF])


MSS = (1, 19, 20, 21, 536, 1448)


def random_batch(seed, nconn, maxvec=8, big=False):
    """seeded writes: every flag, windows that cut writes, held tails coming in, empty vectors"""
    rng = np.random.default_rng(seed)
    cs = []
    for _ in range(nconn):
        mss = int(rng.choice(MSS))
        fl = G.WR_WANT if rng.random() < 0.95 else 0
        for bit, p in ((G.WR_NONBLOCK, .3), (G.WR_NO_PARTIAL, .15), (G.WR_TX_CLOSED, .05), (G.WR_TX_EXCL, .05),
                       (G.WR_ZERO_WND, .2), (G.WR_BELOW_EST, .05)):
            if rng.random() < p:
                fl |= bit
        una = int(rng.integers(0, 1 << 32))
        inflight = int(rng.integers(0, 3000))
        wnd = int(rng.choice([0, inflight, inflight + 1, inflight + 19, inflight + int(rng.integers(1, 6000)), 1 << 20]))
        lens = [0, 1, 19, 20, 21, mss - 1, mss, mss + 1, 2 * mss, 2 * mss + 19, 2 * mss + 20, int(rng.integers(0, 5000))]
        if mss == 1:
            lens = [0, 1, 2, 19, 20, 21, 60]
        c = conn(flags=fl, mss=mss, snd_una=una, snd_nxt=(una + inflight) & M32, snd_wnd=wnd,
                 rcv_nxt=int(rng.integers(0, 1 << 32)), rcv_wnd=int(rng.integers(0, 1 << 32)),
                 wscale=int(rng.integers(0, 15)), ecn=int(rng.choice([0, 0x80, 0x82])), err=int(rng.choice([0, 0, 104])),
                 src_off=int(rng.integers(0, 1 << 40)), len=int(rng.choice(lens)),
                 rport=int(rng.integers(1, 65536)))
        c["tx_last_ack"] = c["rcv_nxt"] if rng.random() < 0.5 else int(rng.integers(0, 1 << 32))
        if rng.random() < 0.3:
            c["pend_len"] = int(rng.choice([1, 19, 20, mss, int(rng.integers(1, mss + 1))]))
            c["pend_len"] = min(c["pend_len"], mss) if rng.random() < 0.97 else mss + 1
            c["pend_frame_off"] = int(rng.integers(0, 1 << 40))
        if rng.random() < 0.6:
            nv = int(rng.integers(0, maxvec + 1))
            c["vecs"] = [(int(rng.integers(0, 1 << 40)), int(rng.choice(lens))) for _ in range(nv)]
            c["flags"] |= G.WR_VEC
        cs.append(c)
    return Batch(cs)
