"""Cases and an independent model for gcl_tcp_read (include/gclassify.h).

The model is written from runtime/net/tcp.c and shares nothing with the
library: a connection's receive queue is a list of [bytearray, fin] mbufs and
the application's buffer a list of bytearrays, and tcp_wait_rx, tcp_read_wait,
tcp_read_wait_peek and copy_into_iov are walked as the reference walks them.
It yields out_conn, the ACK descriptors and the destination bytes.  The item
arrays come from a separate, direct statement of rule 5d (rule_items); applying
those items must reproduce the model's destination bytes, which ties rule 5d
to copy_into_iov.
"""
import numpy as np

from caladan_amd import gclassify as G

M32 = 0xFFFFFFFF
EAGAIN = 11


def wraps_gte(a, b):
    """inc/base/stddef.h: (int32_t)(b - a) <= 0"""
    d = (b - a) & M32
    return d == 0 or d >= 0x80000000


# ---------------------------------------------------------------- the model

class ModelConn:
    def __init__(self, q, rd, cn):
        self.rxq = [[bytearray(d), bool(fin)] for d, fin in q]
        self.rx_closed = bool(rd["flags"] & G.RD_RX_CLOSED)
        self.rx_exclusive = bool(rd["flags"] & G.RD_RX_EXCL)
        self.err = rd["err"]
        self.rcv_nxt, self.rcv_wnd = cn["rcv_nxt"], cn["rcv_wnd"]
        self.tx_last_ack, self.tx_last_win, self.winmax = rd["tx_last_ack"], rd["tx_last_win"], rd["winmax"]
        self.flags = 0


def tcp_wait_rx(c, nonblocking):
    """tcp.c:850-876: 1, a negative errno or 0, or "block" where it would wait"""
    if not c.rx_closed and (c.rx_exclusive or not c.rxq):
        return -EAGAIN if nonblocking else "block"
    if c.rx_closed:
        return -c.err
    return 1


def tcp_read_wait(c, length, nonblocking):
    """tcp.c:878-934: (ret, the popped list q, mout)"""
    ret = tcp_wait_rx(c, nonblocking)
    if ret == "block" or ret <= 0:
        return ret, [], None
    q, mout, readlen = [], None, 0
    while readlen < length:
        if not c.rxq:
            break
        m = c.rxq[0]
        if m[1]:
            c.rx_closed = True           # tcp_conn_shutdown_rx
            c.flags |= G.RDO_RX_CLOSED
            if len(m[0]) == 0:
                break
        if length - readlen < len(m[0]):
            c.rx_exclusive = True
            mout = m
            readlen = length
            break
        q.append(c.rxq.pop(0))
        readlen += len(m[0])
    c.rcv_wnd = (c.rcv_wnd + readlen) & M32
    if wraps_gte((c.rcv_nxt + c.rcv_wnd) & M32, (c.tx_last_ack + c.tx_last_win + c.winmax // 4) & M32):
        c.flags |= G.RDO_ACK
    if not c.rxq:
        c.flags |= G.RDO_POLLIN_CLEAR
    return readlen, q, mout


def tcp_read_wait_peek(c, length, nonblocking):
    """tcp.c:963-988"""
    ret = tcp_wait_rx(c, nonblocking)
    if ret == "block" or ret <= 0:
        return ret
    readlen = 0
    for m in c.rxq:
        readlen += len(m[0])
        if readlen >= length:
            break
    c.rx_exclusive = True
    return min(readlen, length)


def copy_into_iov(iov, maxbytes, q, m_extra):
    """tcp.c:1133-1185; @iov: a list of bytearrays to fill"""
    mi, i, mbuf_off, iov_off, readlen = 0, 0, 0, 0, 0
    while mi < len(q) and i < len(iov) and readlen < maxbytes:
        m, vp = q[mi][0], iov[i]
        cpylen = min(len(vp) - iov_off, len(m) - mbuf_off, maxbytes - readlen)
        vp[iov_off:iov_off + cpylen] = m[mbuf_off:mbuf_off + cpylen]
        iov_off += cpylen
        mbuf_off += cpylen
        readlen += cpylen
        if mbuf_off == len(m):
            mi += 1
            mbuf_off = 0
        if iov_off == len(vp):
            i += 1
            iov_off = 0
    if m_extra is not None:
        assert len(m_extra[0]) > maxbytes - readlen
        while True:
            vp = iov[i]
            cpylen = len(vp) - iov_off
            assert cpylen <= maxbytes - readlen
            vp[iov_off:iov_off + cpylen] = m_extra[0][:cpylen]
            del m_extra[0][:cpylen]      # mbuf_pull; seg_seq += cpylen
            iov_off = 0
            readlen += cpylen
            i += 1
            if i >= len(iov):
                break
    assert readlen == maxbytes


def model_read(q, vec_lens, rd, cn):
    """One tcp_read2 / tcp_readv2 on a connection.  Returns (status, ret, npop,
    pull, rcv_wnd, flags, the vectors' bytes or None where none were written)."""
    c = ModelConn(q, rd, cn)
    nonblocking = bool(rd["flags"] & G.RD_NONBLOCK)
    length = sum(vec_lens)               # iov_len()
    iov = [bytearray(n) for n in vec_lens]
    if not rd["flags"] & G.RD_WANT:
        return G.RDS_NONE, 0, 0, 0, c.rcv_wnd, 0, None
    n0 = len(c.rxq)
    if rd["flags"] & G.RD_PEEK:
        ret = tcp_read_wait_peek(c, length, nonblocking)
        q_, m = c.rxq, None
    else:
        ret, q_, m = tcp_read_wait(c, length, nonblocking)
    if ret == "block":
        return G.RDS_BLOCK, 0, 0, 0, c.rcv_wnd, 0, None
    if ret <= 0 and (c.rx_closed and rd["flags"] & G.RD_RX_CLOSED):
        return G.RDS_CLOSED, ret, 0, 0, c.rcv_wnd, 0, None
    if ret == -EAGAIN:
        return G.RDS_AGAIN, ret, 0, 0, c.rcv_wnd, 0, None
    pull = 0
    if ret > 0:
        before = len(m[0]) if m is not None else 0
        copy_into_iov(iov, ret, q_, m)
        pull = before - len(m[0]) if m is not None else 0
    if rd["flags"] & G.RD_PEEK:
        # tcp_read_peek: ret <= 0 returns with rx_exclusive set, else tcp_read_finish_peek
        c.flags |= G.RDO_RXWAKE if ret > 0 else G.RDO_EXCL_LEFT
        npop = 0
    else:
        npop = n0 - len(c.rxq)
        if m is not None:                # tcp_read_finish
            c.flags |= G.RDO_PARTIAL | G.RDO_RXWAKE
    return G.RDS_DONE, ret, npop, pull, c.rcv_wnd, c.flags, iov if ret > 0 else None


def rule_items(ent_lens, vec_lens, ret):
    """Rule 5d, stated directly: (entry, vector, from, to) of every item"""
    if ret <= 0:
        return []
    A, B = np.concatenate(([0], np.cumsum(ent_lens, dtype=np.uint64))), np.concatenate(([0], np.cumsum(vec_lens, dtype=np.uint64)))
    ne = next(i for i in range(1, len(A)) if A[i] >= ret)
    nv = next(j for j in range(1, len(B)) if B[j] >= ret)
    cuts = sorted([(int(A[i]), 0) for i in range(1, ne)] + [(int(B[j]), 1) for j in range(1, nv)])
    items, i, j, pos = [], 0, 0, 0
    for val, kind in cuts + [(ret, 2)]:
        items.append((i, j, pos, val))
        pos = val
        i += kind == 0
        j += kind == 1
    assert len(items) == ne + nv - 1
    return items


# ---------------------------------------------------------------- batches

def rd_rec(flags=G.RD_WANT, tx_last_ack=0, tx_last_win=0, winmax=0, err=0):
    return dict(flags=flags, tx_last_ack=tx_last_ack, tx_last_win=tx_last_win, winmax=winmax, err=err)


def cn_rec(rcv_nxt=1000, rcv_wnd=5000, snd_nxt=77):
    return dict(rcv_nxt=rcv_nxt, rcv_wnd=rcv_wnd, snd_nxt=snd_nxt)


NO_ACK = dict(tx_last_ack=1000, tx_last_win=5000, winmax=0x7FFFFFFF * 2)  # far ahead of any window here


class Batch:
    """The arrays of one call.  @queues: per connection a list of (len, fin);
    @reads: per connection (vec_lens, rd, cn), vec_lens the vectors' lengths
    (one length without @use_voff).  @qoff / @voff override the CSR offsets
    over the concatenated entries and vectors (garbage ranges)."""

    def __init__(self, queues, reads, use_voff, seed=1, qoff=None, voff=None):
        rng = np.random.default_rng(seed)
        self.nconn = len(queues)
        self.use_voff = use_voff
        ents = [e for q in queues for e in q]
        self.nent = len(ents)
        self.ent = np.zeros(max(self.nent, 1), dtype=G.RDQ_ENT_DTYPE)
        # the source region: every mbuf's data with a gap behind it
        off, offs = 5, []
        for ln, _ in ents:
            offs.append(off)
            off += ln + 3
        self.src = rng.integers(0, 256, off + 8, dtype=np.uint8)
        for k, (ln, fin) in enumerate(ents):
            self.ent[k] = (offs[k], ln, G.RDQE_FIN if fin else 0, 0)
        self.qoff = np.asarray(qoff if qoff is not None else np.concatenate(([0], np.cumsum([len(q) for q in queues]))),
                               dtype=np.uint32)
        vecs = [v for vl, _, _ in reads for v in vl]
        self.nvec = len(vecs) if use_voff else 0
        self.iov = np.zeros(max(len(vecs), 1), dtype=G.RD_IOV_DTYPE)
        doff, doffs = 7, []
        for ln in vecs:
            doffs.append(doff)
            doff += ln + 2
        self.dst_len = doff + 8
        for k, ln in enumerate(vecs):
            self.iov[k] = (doffs[k], ln, 0)
        vstart = np.concatenate(([0], np.cumsum([len(vl) for vl, _, _ in reads]))).astype(np.int64)
        self.voff = np.asarray(voff if voff is not None else vstart, dtype=np.uint32) if use_voff else None
        self.rd = np.zeros(max(self.nconn, 1), dtype=G.TCP_RD_DTYPE)
        self.conn = np.zeros(max(self.nconn, 1), dtype=G.TCP_CONN_DTYPE)
        self.addr = np.zeros(max(self.nconn, 1), dtype=G.TCP_ADDR_DTYPE)
        self.reads = reads
        for c, (vl, rd, cn) in enumerate(reads):
            r = self.rd[c]
            if not use_voff:
                assert len(vl) == 1
                r["dst_off"], r["len"] = doffs[int(vstart[c])], vl[0]
            else:
                r["dst_off"], r["len"] = int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 32))  # ignored
            for f in ("tx_last_ack", "tx_last_win", "winmax", "err", "flags"):
                r[f] = rd[f]
            for f in ("rcv_nxt", "rcv_wnd", "snd_nxt"):
                self.conn[c][f] = cn[f]
            self.conn[c]["snd_una"] = int(rng.integers(0, 1 << 32))
            a = self.addr[c]
            a["lip"], a["rip"] = int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32))
            a["lport"], a["rport"] = int(rng.integers(1, 1 << 16)), int(rng.integers(1, 1 << 16))
            a["rcv_wscale"] = int(rng.integers(0, 256)) if c % 3 else 0

    def ranges(self, c):
        """(e0, n, v0, m, bad) of connection c, as the rule cuts them"""
        lo, hi = int(self.qoff[c]), int(self.qoff[c + 1])
        bad = lo > hi or hi > self.nent
        e0, n = (0, 0) if bad else (lo, hi - lo)
        if not self.use_voff:
            return e0, n, None, 1, bad
        lo, hi = int(self.voff[c]), int(self.voff[c + 1])
        vbad = lo > hi or hi > self.nvec
        v0, m = (0, 0) if vbad else (lo, hi - lo)
        return e0, n, v0, m, bad or vbad

    def expect(self, item_cap, seg_cap, frame_base=0, frame_stride=64):
        """Everything a call writes, from the model and rule_items"""
        oc = np.zeros(max(self.nconn, 1), dtype=G.RD_CONN_OUT_DTYPE)
        items, segs, counts = [], [], np.zeros(G.RDC_NR, dtype=np.uint64)
        dst = np.zeros(self.dst_len, dtype=np.uint8)
        wanted = nseg = retsum = 0
        for c in range(self.nconn):
            e0, n, v0, m, bad = self.ranges(c)
            _, rd, cn = self.reads[c]
            ent = self.ent[e0:e0 + n]
            if self.use_voff:
                vec = [(int(v["off"]), int(v["len"])) for v in self.iov[v0:v0 + m]]
            else:
                vec = [(int(self.rd[c]["dst_off"]), int(self.rd[c]["len"]))]
            o = oc[c]
            o["first_item"] = min(wanted, item_cap)
            if bad:
                o["status"], o["rcv_wnd"] = G.RDS_BADRANGE, cn["rcv_wnd"]
                continue
            q = [(bytes(self.src[int(e["off"]):int(e["off"]) + int(e["len"])]), e["flags"] & G.RDQE_FIN) for e in ent]
            status, ret, npop, pull, wnd, flags, iov = model_read(q, [ln for _, ln in vec], rd, cn)
            its = rule_items([int(e["len"]) for e in ent], [ln for _, ln in vec], ret)
            written = 0
            for i, j, a, b in its:
                if wanted + written < item_cap:
                    A = int(ent["len"][:i].astype(np.uint64).sum())
                    B = sum(ln for _, ln in vec[:j])
                    items.append((int(ent[i]["off"]) + a - A, b - a, vec[j][0] + a - B, c, e0 + i))
                    written += 1
            if iov is not None:
                for (off, ln), data in zip(vec, iov):
                    dst[off:off + ln] = np.frombuffer(bytes(data), dtype=np.uint8)
                # past ret the model's buffers hold zeros the call never writes
                self._mask_tail(dst, vec, ret)
            if written < len(its):
                flags |= G.RDO_ITEM_NOSPACE
            if flags & G.RDO_ACK:
                if nseg < seg_cap:
                    a = self.addr[c]
                    segs.append((a["lip"], a["rip"], a["lport"], a["rport"], 6, 0x10, 5, 0, cn["snd_nxt"], cn["rcv_nxt"],
                                 (wnd >> (int(a["rcv_wscale"]) & 31)) & 0xFFFF, 0, 0, frame_base + nseg * frame_stride, c))
                    counts[G.RDC_ACKS] += 1
                else:
                    flags |= G.RDO_SEG_NOSPACE
                nseg += 1
            wanted += len(its)
            retsum += ret if status == G.RDS_DONE else 0
            o["ret"], o["npop"], o["pull"], o["rcv_wnd"] = ret, npop, pull, wnd
            o["nitems"], o["status"], o["flags"] = written, status, flags
            for slot, st in ((G.RDC_DONE, G.RDS_DONE), (G.RDC_AGAIN, G.RDS_AGAIN), (G.RDC_BLOCK, G.RDS_BLOCK),
                             (G.RDC_CLOSED, G.RDS_CLOSED)):
                counts[slot] += status == st
            counts[G.RDC_PEEKS] += status == G.RDS_DONE and bool(rd["flags"] & G.RD_PEEK)
            counts[G.RDC_POPPED] += npop
            counts[G.RDC_PARTIAL] += bool(flags & G.RDO_PARTIAL)
            counts[G.RDC_RX_CLOSED] += bool(flags & G.RDO_RX_CLOSED)
            counts[G.RDC_ITEMS] += written
            counts[G.RDC_NOSPACE] += bool(flags & (G.RDO_SEG_NOSPACE | G.RDO_ITEM_NOSPACE))
        nbytes = sum(it[1] for it in items)
        counts[G.RDC_BYTES] = nbytes
        return dict(out_conn=oc, items=items, segs=segs, counts=counts, dst=dst,
                    totals=np.array([wanted, min(wanted, item_cap), nbytes, retsum], dtype=np.uint64),
                    seg_totals=np.array([nseg, min(nseg, seg_cap)], dtype=np.uint64))

    @staticmethod
    def _mask_tail(dst, vec, ret):
        at = 0
        for off, ln in vec:
            keep = min(max(ret - at, 0), ln)
            dst[off + keep:off + ln] = 0
            at += ln

    def run_host(self, item_cap, seg_cap, frame_base=0, frame_stride=64, counts=None):
        return G.tcp_read_host(self.qoff, self.ent, self.rd, self.conn, self.addr, item_cap, seg_cap, voff=self.voff,
                               iov=self.iov if self.use_voff else None, frame_stride=frame_stride,
                               frame_base=frame_base, nconn=self.nconn, nent=self.nent, nvec=self.nvec,
                               counts=counts)

    def apply_items(self, out, k):
        """The copies of items [0, k) on a zeroed destination region"""
        dst = np.zeros(self.dst_len, dtype=np.uint8)
        for s, ln, d in zip(out["src_off"][:k], out["len"][:k], out["dst_off"][:k]):
            dst[int(d):int(d) + int(ln)] = self.src[int(s):int(s) + int(ln)]
        return dst

    def item_cap_enough(self):
        return self.nent + max(self.nvec, self.nconn)


def check(b, out, exp, counts=None):
    """@out (host arrays of a call on batch @b) against @exp = b.expect(...)"""
    oc = np.asarray(out["out_conn"]).view(G.RD_CONN_OUT_DTYPE).reshape(-1)[:b.nconn]
    for f in G.RD_CONN_OUT_DTYPE.names:
        got, want = oc[f], exp["out_conn"][f][:b.nconn]
        assert np.array_equal(got, want), (f, np.flatnonzero((got != want).reshape(b.nconn, -1).any(axis=1))[:8],
                                           got[:8], want[:8])
    assert np.array_equal(np.asarray(out["totals"]).view(np.uint64)[:4], exp["totals"]), (out["totals"], exp["totals"])
    assert np.array_equal(np.asarray(out["seg_totals"]).view(np.uint64)[:2], exp["seg_totals"])
    k = len(exp["items"])
    assert k == int(exp["totals"][1])
    if k:
        want = np.array(exp["items"], dtype=np.uint64)
        for col, f in enumerate(G.RD_ITEM_FIELDS):
            got = np.asarray(out[f])[:k]
            got = got.view({8: np.uint64, 4: np.uint32, 2: np.uint16}[got.dtype.itemsize]).astype(np.uint64)
            assert np.array_equal(got, want[:, col]), (f, got[:8], want[:8, col])
    s = len(exp["segs"])
    assert s == int(exp["seg_totals"][1])
    if s:
        desc = np.asarray(out["desc"]).view(G.TXH_DESC_DTYPE).reshape(-1)[:s]
        for k_, seg in enumerate(exp["segs"]):
            assert tuple(int(x) for x in desc[k_].tolist()) == tuple(int(x) for x in seg[:13]), (k_, desc[k_], seg)
            assert int(np.asarray(out["frame_off"]).view(np.uint64)[k_]) == seg[13]
            assert int(np.asarray(out["seg_conn"]).view(np.uint32)[k_]) == seg[14]
            assert int(np.asarray(out["seg_src"]).view(np.uint32)[k_]) == seg[14]
            assert int(np.asarray(out["seg_kind"])[k_]) == G.CTL_ACK
    if counts is not None:
        assert np.array_equal(np.asarray(counts).view(np.uint64)[:G.RDC_NR], exp["counts"]), (counts, exp["counts"])
    if not (exp["out_conn"]["flags"] & G.RDO_ITEM_NOSPACE).any():
        assert np.array_equal(b.apply_items({f: np.asarray(out[f]).view(
            {8: np.uint64, 4: np.uint32, 2: np.uint16}[np.asarray(out[f]).dtype.itemsize]) for f in
            ("src_off", "len", "dst_off")}, k), exp["dst"])


# ---------------------------------------------------------------- hand cases

W = G.RD_WANT


def hand_cases():
    """(name, queues, reads, use_voff, per-connection (status, ret, npop, pull, flags) derived by hand)"""
    na = lambda **kw: rd_rec(**{**NO_ACK, **kw})  # noqa: E731
    cn = cn_rec()
    D, PC = G.RDS_DONE, G.RDO_POLLIN_CLEAR
    PART = G.RDO_PARTIAL | G.RDO_RXWAKE
    cases = []
    # exact fit: A_2 == L, the FIN behind is not examined
    cases.append(("exact_fit", [[(100, 0), (50, 0), (0, 1)]], [([150], na(), cn)], False, [(D, 150, 2, 0, 0)]))
    cases.append(("partial", [[(100, 0), (50, 0)]], [([120], na(), cn)], False, [(D, 120, 1, 20, PART)]))
    # L == 0: nothing examined, the ACK test still runs: 1000 + 5000 >= 1000 + 4000 + 0
    cases.append(("len0_ack", [[(10, 1)]], [([0], rd_rec(tx_last_ack=1000, tx_last_win=4000, winmax=3), cn)], False,
                  [(D, 0, 0, 0, G.RDO_ACK)]))
    cases.append(("fin_data_full", [[(30, 0), (20, 1)]], [([64], na(), cn)], False,
                  [(D, 50, 2, 0, G.RDO_RX_CLOSED | PC)]))
    cases.append(("fin_data_partial", [[(30, 0), (20, 1)]], [([40], na(), cn)], False,
                  [(D, 40, 1, 10, G.RDO_RX_CLOSED | PART)]))
    cases.append(("fin0_head", [[(0, 1), (9, 0)]], [([5], na(), cn)], False, [(D, 0, 0, 0, G.RDO_RX_CLOSED)]))
    cases.append(("fin0_behind", [[(7, 0), (0, 1)]], [([20], na(), cn)], False, [(D, 7, 1, 0, G.RDO_RX_CLOSED)]))
    # a second read after RX_CLOSED: -err
    cases.append(("closed_err", [[(0, 1)], [(0, 1)], []],
                  [([8], na(flags=W | G.RD_RX_CLOSED, err=0), cn), ([8], na(flags=W | G.RD_RX_CLOSED, err=104), cn),
                   ([8], na(flags=W | G.RD_RX_CLOSED | G.RD_RX_EXCL | G.RD_NONBLOCK, err=32), cn)], False,
                  [(G.RDS_CLOSED, 0, 0, 0, 0), (G.RDS_CLOSED, -104, 0, 0, 0), (G.RDS_CLOSED, -32, 0, 0, 0)]))
    cases.append(("again_block_excl", [[], [], [(5, 0)], [(5, 0)], [(5, 0)]],
                  [([8], na(flags=W | G.RD_NONBLOCK), cn), ([8], na(), cn), ([8], na(flags=W | G.RD_RX_EXCL), cn),
                   ([8], na(flags=W | G.RD_RX_EXCL | G.RD_NONBLOCK), cn), ([8], na(flags=0), cn)], False,
                  [(G.RDS_AGAIN, -11, 0, 0, 0), (G.RDS_BLOCK, 0, 0, 0, 0), (G.RDS_BLOCK, 0, 0, 0, 0),
                   (G.RDS_AGAIN, -11, 0, 0, 0), (G.RDS_NONE, 0, 0, 0, 0)]))
    cases.append(("peek", [[(0, 0), (0, 1)], [(10, 1), (0, 1), (10, 0)], [(10, 0)]],
                  [([8], na(flags=W | G.RD_PEEK), cn), ([25], na(flags=W | G.RD_PEEK), cn),
                   ([0], na(flags=W | G.RD_PEEK), cn)], False,
                  [(D, 0, 0, 0, G.RDO_EXCL_LEFT), (D, 20, 0, 0, G.RDO_RXWAKE), (D, 0, 0, 0, G.RDO_EXCL_LEFT)]))
    # the window test with a 32-bit wrap: rcv_nxt + rcv_wnd + ret against 0xFFFFFFF0 + 0x20 + 64 / 4 = 0x20 (mod 2^32)
    wr = rd_rec(tx_last_ack=0xFFFFFFF0, tx_last_win=0x20, winmax=64)
    cases.append(("window_edge", [[(15, 0)], [(16, 0)]],
                  [([64], wr, cn_rec(rcv_nxt=0xFFFFFFF8, rcv_wnd=0x18)), ([64], wr, cn_rec(rcv_nxt=0xFFFFFFF8, rcv_wnd=0x18))],
                  False, [(D, 15, 1, 0, PC), (D, 16, 1, 0, PC | G.RDO_ACK)]))
    # vectors: cuts that coincide with entry cuts, zero-length vectors and entries
    cases.append(("iov_coincide", [[(10, 0), (0, 0), (10, 0), (5, 0)]], [([10, 0, 10, 0, 3], na(), cn)], True,
                  [(D, 23, 3, 3, PART)]))
    cases.append(("iov_one_vec_many_ents", [[(3, 0)] * 9], [([100], na(), cn)], True, [(D, 27, 9, 0, PC)]))
    cases.append(("iov_one_ent_many_vecs", [[(1000, 0)]], [([7] * 11, na(), cn)], True, [(D, 77, 0, 77, PART)]))
    cases.append(("iov_len0", [[(4, 0)]], [([0, 0], na(), cn)], True, [(D, 0, 0, 0, 0)]))
    return cases


def random_batch(seed, nconn, use_voff, maxq=6, one_owner=0):
    """A seeded batch that mixes every status and flag.  @one_owner: connection
    0 owns that many entries."""
    rng = np.random.default_rng(seed)
    lens = np.array([0, 0, 1, 2, 7, 64, 536, 1448, 1448, 65535])
    queues, reads = [], []
    for c in range(nconn):
        n = one_owner if (one_owner and c == 0) else int(rng.integers(0, maxq + 1))
        finp = 0.002 if n > 64 else 0.15
        q = [(int(rng.choice(lens)), int(rng.random() < finp)) for _ in range(n)]
        tot = sum(ln for ln, _ in q)
        A = np.cumsum([ln for ln, _ in q]) if q else np.array([0])
        pick = int(rng.integers(0, 6))
        L = [0, tot, tot // 2, tot + 9, int(rng.choice(A)), int(rng.integers(0, tot + 2))][pick]
        if use_voff:
            nv = int(rng.integers(0, 5)) if not (one_owner and c == 0) else int(rng.integers(1, 700))
            cuts = sorted(int(x) for x in rng.integers(0, L + 1, max(nv - 1, 0)))
            if q and nv > 1 and rng.random() < 0.5:   # some vector cuts on entry cuts
                cuts = sorted(min(int(rng.choice(A)), L) if rng.random() < 0.5 else x for x in cuts)
            edges = [0] + cuts + [L]
            vl = [b - a for a, b in zip(edges[:-1], edges[1:])] if nv else []
        else:
            vl = [L]
        fl = W
        r = rng.random()
        if r < 0.08:
            fl = 0
        elif r < 0.2:
            fl |= G.RD_PEEK
        if rng.random() < 0.1:
            fl |= G.RD_NONBLOCK
        if rng.random() < 0.06:
            fl |= G.RD_RX_CLOSED
        if rng.random() < 0.06:
            fl |= G.RD_RX_EXCL
        rcv_nxt, rcv_wnd = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 20))
        if rng.random() < 0.5:   # the ACK test near its edge
            winmax = int(rng.integers(0, 1 << 18))
            tla = rcv_nxt
            tlw = (rcv_wnd + int(rng.integers(0, min(sum(vl), tot) + 2)) - winmax // 4) & M32
        else:
            winmax, tla, tlw = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))
        queues.append(q)
        reads.append((vl, rd_rec(fl, tla, tlw, winmax, int(rng.integers(0, 120))),
                      cn_rec(rcv_nxt, rcv_wnd, int(rng.integers(0, 1 << 32)))))
    return Batch(queues, reads, use_voff, seed=seed)


def bad_range_batch(use_voff):
    """Inverted and out-of-range qoff (and voff): connections 1, 3 and 4 of five are BADRANGE"""
    queues = [[(10, 0)] * 5, [], [(10, 0)], [], [(4, 0)] * 2]
    reads = [([8, 8], rd_rec(**NO_ACK), cn_rec()) for _ in range(5)]
    if not use_voff:
        reads = [([16], rd, cn) for _, rd, cn in reads]
        # [0,5) good, [5,2) inverted, [2,6) good and overlapping, [6,99) past nent = 8, then [99, 8) inverted
        return Batch(queues, reads, False, qoff=[0, 5, 2, 6, 99, 8])
    return Batch(queues, reads, True, voff=[0, 2, 1, 4, 0xFFFFFFFF, 10])
