"""GPU: gcl_tcp_write (include/gclassify.h) against its host twin and the model of
tests/tcpwritecases.py, bit for bit over outputs and a workspace pre-filled with
0xFF: the hand cases, random batches with forced range counts, one connection
owning every segment so that the emission crosses blocks, 1 024 vectors on one
connection, each cap one short, garbage vector offsets, no connections; the
same plain writes through gcl_tx_seg; and chained: the items through
gcl_copy_batch, the segments through gcl_tx_hdr and gcl_l4_csum FILL, the queue
records through gcl_tcp_txq."""
import numpy as np
import pytest
import torch

from tests import tcpwritecases as T
from tests import txqcases as tq
from tests.test_gpu_tcprx import dev

pytestmark = pytest.mark.gpu

GUARD = 8
SEG_DT = (("desc", torch.uint8, 32), ("frame_off", torch.int64, 0), ("seg_conn", torch.int32, 0),
          ("txq_ent", torch.uint8, 16), ("txq_cold", torch.uint8, 16))
ITEM_DT = (("src_off", torch.int64, 0), ("len", torch.int16, 0), ("dst_off", torch.int64, 0),
           ("item_conn", torch.int32, 0), ("item_seg", torch.int32, 0))


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def clf(g):
    c = g.Classifier(0, 16, g.HASH_JENKINS)
    yield c
    c.close()


def rec(a, width):
    return dev(a) if len(a) else torch.zeros((1, width), dtype=torch.uint8, device="cuda")


def ff(n, dt, width=0):
    shape = (n, width) if width else (n,)
    return torch.full(shape, 0xFF if dt == torch.uint8 else -1, dtype=dt, device="cuda")


def run_gpu(g, clf, b, seg_cap, item_cap, blocks=0, frame_base=0, frame_stride=2048, frames_len=0, counts=None,
            calls=1):
    """@calls calls over 0xFF-filled outputs with GUARD elements behind each and a 0xFF-filled workspace:
    the outputs as numpy arrays, the guards and everything past the totals checked"""
    whole = {f: ff(seg_cap + GUARD, dt, w) for f, dt, w in SEG_DT}
    whole.update({f: ff(item_cap + GUARD, dt, w) for f, dt, w in ITEM_DT})
    whole.update(out_conn=ff(b.nconn + GUARD, torch.uint8, 48), totals=ff(6 + GUARD, torch.int64))
    nvec = b.nvec if b.use_voff else 0
    ws = ff(g.tcp_write_workspace(b.nconn, nvec, blocks) + 64, torch.uint8)
    voff, iov = (dev(b.voff), rec(b.iov[:b.nvec], 16)) if b.use_voff else (None, None)
    wr, conn, addr = rec(b.wr[:b.nconn], 48), rec(b.conn[:b.nconn], 48), rec(b.addr[:b.nconn], 16)
    for _ in range(calls):
        clf.tcp_write(T.NOW, wr, conn, addr, b.nconn, seg_cap, item_cap, voff=voff, iov=iov, nvec=nvec,
                      frame_stride=frame_stride, frame_base=frame_base, frames_len=frames_len, blocks=blocks,
                      out=whole, counts=counts, workspace=ws)
    torch.cuda.synchronize()
    got = {f: t.cpu().numpy() for f, t in whole.items()}
    assert (got["out_conn"][b.nconn:] == 0xFF).all() and (got["totals"][6:] == -1).all() and (ws[-64:] == 0xFF).all()
    s, k = int(got["totals"][1]), int(got["totals"][3])
    assert s <= seg_cap and k <= item_cap
    for f, dt, _ in SEG_DT:        # nothing at or past the written totals is touched
        assert (got[f][s:] == (0xFF if dt == torch.uint8 else -1)).all(), f
    for f, _, _ in ITEM_DT:
        assert (got[f][k:] == -1).all(), f
    return got


def check(g, clf, b, seg_cap=None, item_cap=None, blocks=0, frame_base=0, frame_stride=2048, frames_len=0, exp=None):
    """GPU == host twin == model, every output byte"""
    es, ei = (None, None) if seg_cap is not None and item_cap is not None else b.enough()
    seg_cap, item_cap = es if seg_cap is None else seg_cap, ei if item_cap is None else item_cap
    cnt = torch.full((g.WRC_NR,), 5, dtype=torch.int64, device="cuda")
    got = run_gpu(g, clf, b, seg_cap, item_cap, blocks, frame_base, frame_stride, frames_len, counts=cnt)
    cnt = cnt.cpu().numpy().view(np.uint64) - np.uint64(5)
    hcnt = np.zeros(g.WRC_NR, dtype=np.uint64)
    host = b.run_host(seg_cap, item_cap, frame_base, frame_stride, frames_len, hcnt)
    s, k = int(host["totals"][1]), int(host["totals"][3])
    assert T.raw(got["out_conn"], 48 * b.nconn) == host["out_conn"][:b.nconn].tobytes()
    assert T.raw(got["totals"], 48) == host["totals"].tobytes()
    for f, n in [(f, s) for f in g.WR_SEG_FIELDS] + [(f, k) for f in g.WR_ITEM_FIELDS]:
        assert T.raw(got[f], n * g.WR_OUT_WIDTH[f]) == T.raw(host[f], n * g.WR_OUT_WIDTH[f]), f
    assert cnt.tolist() == hcnt.tolist()
    T.check(b, got, exp if exp is not None else b.expect(seg_cap, item_cap, frame_base, frame_stride, frames_len), cnt)
    return got


HAND = T.hand_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(g, clf, case):
    _, conns, want, segs, voff = case
    got = check(g, clf, T.Batch(conns, voff=voff))
    oc = np.frombuffer(T.raw(got["out_conn"], 48 * len(conns)), dtype=g.WR_CONN_OUT_DTYPE)
    for c, (status, ret, snd_nxt, nseg, nitems, pend_len, flags) in want.items():
        o = oc[c]
        assert (o["status"], o["ret"], o["snd_nxt"], o["nseg"], o["nitems"], o["pend_len"], o["flags"]) == \
            (status, ret, snd_nxt, nseg, nitems, pend_len, flags), (c, o)
    d = np.frombuffer(T.raw(got["desc"], 32 * len(segs)), dtype=g.TXH_DESC_DTYPE)
    assert [(int(x["tcp_flags"]), int(x["seq"]), int(x["paylen"])) for x in d] == [(f, s & T.M32, n) for _, f, s, n in segs]


@pytest.mark.parametrize("blocks", [1, 3, 0])
@pytest.mark.parametrize("seed,nconn", [(1, 63), (2, 257), (3, 3 * T.G.WR_TILE + 5)])
def test_random(g, clf, seed, nconn, blocks, memo={}):
    if (seed, nconn) not in memo:       # the model's answer once per batch
        b = T.random_batch(seed, nconn)
        es, ei = b.enough()
        memo[seed, nconn] = (b, es, ei, b.expect(es, ei, 1 << 33, 1536))
    b, es, ei, exp = memo[seed, nconn]
    check(g, clf, b, es, ei, blocks=blocks, frame_base=1 << 33, frame_stride=1536, exp=exp)


@pytest.mark.parametrize("blocks", [0, 3])
def test_one_connection_owns_every_segment(g, clf, blocks):
    """mss 1, 3000 bytes: 3000 segments and items on connection 1 of 3, emitted across blocks; with
    vectors the same bytes as 7 uneven vectors, a held tail coming in"""
    plain = T.Batch([T.conn(mss=1, len=2), T.conn(mss=1, len=3000, src_off=1 << 20), T.conn(mss=100, len=5)])
    got = check(g, clf, plain, blocks=blocks, frame_stride=256)
    assert got["totals"][:6].tolist() == [3003, 3003, 3003, 3003, 3003, 3007]
    vec = T.Batch([T.conn(mss=1, len=2),
                   T.conn(mss=21, pend_len=20, pend_frame_off=99, vecs=[(0, 1000), (5000, 0), (9000, 19), (10000, 41),
                                                                           (20000, 1), (30000, 1939), (40000, 0)]),
                   T.conn(mss=100, len=5)])
    check(g, clf, vec, blocks=blocks, frame_stride=256)


def test_1024_vectors_of_one_byte(g, clf):
    got = check(g, clf, T.too_many_vectors())
    oc = np.frombuffer(T.raw(got["out_conn"], 96), dtype=g.WR_CONN_OUT_DTYPE)
    assert oc["status"].tolist() == [g.WRS_REFUSED, g.WRS_DONE]
    # every 1-byte vector is a tail under 20 bytes: sent short, one segment each, the last one pushed
    assert (oc["nseg"][1], oc["nitems"][1], oc["ret"][1]) == (1024, 1024, 1024)


@pytest.mark.parametrize("which", ["segs", "items", "frames"])
def test_each_cap_one_short(g, clf, which):
    b = T.random_batch(11, 48)
    es, ei = b.enough()
    slots = int(b.expect(es, ei)["totals"][4])
    kw = dict(segs=dict(seg_cap=es - 1, item_cap=ei), items=dict(seg_cap=es, item_cap=ei - 1),
              frames=dict(seg_cap=es, item_cap=ei, frame_base=4096, frames_len=4096 + slots * 2048 - 1))[which]
    got = check(g, clf, b, **kw)
    st = np.frombuffer(T.raw(got["out_conn"], 48 * b.nconn), dtype=g.WR_CONN_OUT_DTYPE)["status"]
    assert (st == g.WRS_NOSPACE).any()
    check(g, clf, b, seg_cap=0, item_cap=ei)
    check(g, clf, b, seg_cap=es // 2, item_cap=ei // 2)


def test_garbage_voff_and_no_voff(g, clf):
    got = check(g, clf, T.garbage_voff_batch())
    st = np.frombuffer(T.raw(got["out_conn"], 48 * 7), dtype=g.WR_CONN_OUT_DTYPE)["status"]
    assert st.tolist() == [g.WRS_DONE, g.WRS_REFUSED, g.WRS_DONE] + [g.WRS_REFUSED] * 4
    check(g, clf, T.Batch([T.conn(mss=100, vecs=[(0, 5)]), T.conn(mss=100, len=5)], use_voff=False))


def test_counts_accumulate_over_two_calls_and_no_connections(g, clf):
    b = T.random_batch(5, 70)
    es, ei = b.enough()
    cnt = torch.zeros(g.WRC_NR, dtype=torch.int64, device="cuda")
    run_gpu(g, clf, b, es, ei, counts=cnt, calls=2)
    assert np.array_equal(cnt.cpu().numpy().view(np.uint64), 2 * b.expect(es, ei)["counts"])
    got = run_gpu(g, clf, T.Batch([]), 4, 4)
    assert not got["totals"][:6].any()


def test_refusals(g, clf):
    b = T.random_batch(3, 8)
    voff, iov = dev(b.voff), rec(b.iov[:b.nvec], 16)
    wr, conn, addr = rec(b.wr[:b.nconn], 48), rec(b.conn[:b.nconn], 48), rec(b.addr[:b.nconn], 16)

    def call(**kw):
        a = dict(nconn=b.nconn, seg_cap=64, item_cap=64, voff=voff, iov=iov, nvec=b.nvec)
        a.update(kw)
        return clf.tcp_write(T.NOW, wr, conn, addr, a.pop("nconn"), a.pop("seg_cap"), a.pop("item_cap"), **a)

    call()
    small = torch.zeros(g.tcp_write_workspace(b.nconn, b.nvec) - 1, dtype=torch.uint8, device="cuda")
    for kw in (dict(frame_stride=53), dict(frame_stride=(1 << 20) + 1), dict(blocks=1025), dict(workspace=small),
               dict(workspace=small[1:]),
               dict(seg_cap=(1 << 31) + 1, out={f: torch.zeros((16, w) if w else 16, dtype=dt, device="cuda")
                                                for f, dt, w in SEG_DT})):
        with pytest.raises((OSError, ValueError, RuntimeError)):
            call(**kw)
    torch.cuda.synchronize()


def test_same_plain_writes_as_tx_seg(g, clf):
    """plain writes, nothing pending, slots with lead 0: desc, src_off, len and frame_off are what
    gcl_tx_seg writes when it is handed the winlen and the wire window gcl_tcp_write worked out"""
    rng = np.random.default_rng(4)
    cs = []
    for _ in range(200):
        mss = int(rng.choice([1, 19, 20, 21, 536, 1448]))
        una = int(rng.integers(0, 1 << 32))
        cs.append(T.conn(mss=mss, snd_una=una, snd_nxt=(una + int(rng.integers(0, 50))) & T.M32,
                         snd_wnd=int(rng.integers(51, 9000)), len=int(rng.integers(0, 60 if mss == 1 else 6000)),
                         rcv_nxt=int(rng.integers(0, 1 << 32)), rcv_wnd=int(rng.integers(0, 1 << 20)),
                         wscale=int(rng.integers(0, 8)), ecn=int(rng.choice([0, 0x82])),
                         src_off=int(rng.integers(0, 1 << 40)), rport=int(rng.integers(1, 65536))))
    b = T.Batch(cs)
    es, ei = b.enough()
    got = run_gpu(g, clf, b, es, ei, frame_base=8192, frame_stride=1536)
    send = np.zeros(len(cs), dtype=g.SEG_SEND_DTYPE)
    for i, c in enumerate(cs):
        s = send[i]
        for f in ("lip", "rip", "lport", "rport", "ecn", "mss", "snd_nxt", "len", "src_off"):
            s[f] = c[f]
        s["proto"], s["ack"] = 6, c["rcv_nxt"]
        s["win"] = (c["rcv_wnd"] >> c["wscale"]) & 0xFFFF
        s["winlen"] = (c["snd_una"] + c["snd_wnd"] - c["snd_nxt"]) & T.M32
    seg = clf.tx_seg(dev(send), len(cs), es, stride=1536, lead=0, frame_base=8192)
    torch.cuda.synchronize()
    n = int(got["totals"][1])
    assert n == es == ei and int(seg["total_segs"].cpu().numpy()[0]) == n
    assert T.raw(got["desc"], 32 * n) == T.raw(seg["desc"].cpu().numpy(), 32 * n)
    assert T.raw(got["frame_off"], 8 * n) == T.raw(seg["frame_off"].cpu().numpy(), 8 * n)
    assert T.raw(got["src_off"], 8 * n) == T.raw(seg["src_off"].cpu().numpy(), 8 * n)
    assert T.raw(got["len"], 2 * n) == T.raw(seg["len"].cpu().numpy(), 2 * n)
    assert (got["dst_off"][:n] == got["frame_off"][:n] + 54).all()


def test_chain_write_copy_hdr_csum_txq(g, clf):
    """three connections write through vectors, one of them onto a held tail: gcl_copy_batch moves the
    items, gcl_tx_hdr and gcl_l4_csum FILL finish the frames, every frame's L4 checksum verifies on the
    CPU, the payloads in seq order are the first ret bytes of the vectors, gcl_tcp_txq pops every
    emitted record once snd_una reaches snd_nxt, and the slot of the frame that stays held is not
    touched by the header and checksum calls"""
    stride, base, held = 256, 4096, 512
    rng = np.random.default_rng(9)
    app = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    lip = tq.NET["addr"]
    clf.neigh_set([(lip + 1 + k, bytes([2, 0, 0, 0, 1, k])) for k in range(3)])
    vecs = [[(100, 150), (900, 0), (2000, 19), (3000, 301)],          # all of it, pushed
            [(5000, 90), (6000, 100), (7000, 0)],                      # onto 30 held bytes; 20 stay held
            [(9000, 400), (10000, 400)]]                               # cut by the window of 500: 100 held
    cs = [T.conn(mss=200, vecs=vecs[0], lip=lip, rip=lip + 1, rport=1001, snd_una=5000, snd_nxt=5000),
          T.conn(mss=200, vecs=vecs[1], lip=lip, rip=lip + 2, rport=1002, pend_len=30, pend_frame_off=held,
                 snd_una=(1 << 32) - 100, snd_nxt=(1 << 32) - 70),
          T.conn(mss=200, vecs=vecs[2], lip=lip, rip=lip + 3, rport=1003, snd_wnd=500)]
    b = T.Batch(cs)
    es, ei = b.enough()
    exp = b.expect(es, ei, base, stride)
    nslots = int(exp["totals"][4])
    frames = torch.from_numpy(tq.region(base + (nslots + 1) * stride)).cuda()
    before = frames.cpu().numpy().copy()
    out = clf.tcp_write(T.NOW, dev(b.wr), dev(b.conn), dev(b.addr), 3, es, ei, voff=dev(b.voff), iov=dev(b.iov),
                        nvec=b.nvec, frame_stride=stride, frame_base=base)
    T.check(b, {f: t.cpu().numpy() for f, t in out.items()}, exp)
    n, k = int(exp["totals"][1]), int(exp["totals"][3])
    clf.copy_batch(dev(app), out["src_off"], out["len"], k, frames, dst_off=out["dst_off"], olflags=False, rss=False)
    net = g.txh_net(lip, tq.NET["netmask"], tq.NET["gateway"], tq.NET["mac"])
    hdr = clf.tx_hdr(out["desc"], out["frame_off"], n, frames, net)
    clf.l4_csum(frames, n, hdr["pkt_len"], mode=g.L4_FILL, offs=out["frame_off"], tx_olflags=hdr["tx_olflags"])
    torch.cuda.synchronize()
    fr = frames.cpu().numpy()
    pkt_len = hdr["pkt_len"].cpu().numpy()[:n].view(np.uint16)
    offs = exp["frame_off"]
    assert (hdr["status"].cpu().numpy()[:n] == g.TXH_OK).all()
    assert (pkt_len == 54 + exp["desc"]["paylen"]).all()
    st = g.l4_csum_host(fr, pkt_len, mode=g.L4_VERIFY, offs=offs, n=n)
    assert (st[:n] == g.L4_GOOD).all()
    oc = exp["out_conn"]
    for c in range(3):
        stream = b"".join(app[o:o + ln].tobytes() for o, ln in vecs[c])[:int(oc["ret"][c])]
        pay = b"".join(fr[int(offs[j]) + 54:int(offs[j]) + 54 + int(exp["desc"]["paylen"][j])].tobytes()
                       for j in range(n) if exp["seg_conn"][j] == c)
        tail = int(oc["pend_len"][c])
        if tail:      # the held tail lies in its frame behind the header's room, not yet sent
            o = int(oc["pend_frame_off"][c]) + 54
            pay += fr[o:o + tail].tobytes()
        lead = cs[c]["pend_len"]     # bytes that were held before the call are not this call's
        assert pay[lead:] == stream and len(stream) == int(oc["ret"][c]), c
    assert oc["pend_len"].tolist() == [0, 20, 100] and oc["ret"].tolist() == [470, 190, 500]
    # the frame that stays held: only its payload bytes were written; the 54 bytes of headers are untouched
    for c in (1, 2):
        o = int(oc["pend_frame_off"][c])
        assert (fr[o:o + 54] == before[o:o + 54]).all(), c
    # the retransmit queues: the emitted records per connection, all acknowledged
    qoff = np.zeros(4, dtype=np.uint32)
    np.cumsum(oc["nseg"], out=qoff[1:])
    conn2 = b.conn.copy()
    conn2["snd_nxt"] = oc["snd_nxt"]
    conn2["snd_una"] = oc["snd_nxt"]
    tx = clf.tcp_txq(T.NOW + 10, dev(qoff), out["txq_ent"], out["txq_cold"], n, dev(conn2), dev(b.addr), 3, 4,
                     frame_stride=stride, frame_base=base)
    torch.cuda.synchronize()
    toc = np.frombuffer(T.raw(tx["out_conn"].cpu().numpy(), 32 * 3), dtype=g.TXQ_CONN_OUT_DTYPE)
    assert toc["nacked"].tolist() == oc["nseg"].tolist() and toc["nretx"].tolist() == [0, 0, 0]
