"""GPU: gcl_tx_seg (include/gclassify.h) against the model of tests/segcases.py
and against its host twin: exact equality of every output array, each
per-segment array allocated longer than seg_cap and pre-filled so that an
entry at or past *total_segs that was touched shows, of the totals and of the
counters; the shapes where the kernels can go wrong (tile and range
boundaries, one write spanning hundreds of tiles, tiles spanning more writes
than they have lanes, a NOSPACE cut inside a range and on its boundary); and
the chain: bytes written go through the whole transmit side, are looped back
through the receive side and come out as they went in."""
import ctypes
import errno

import numpy as np
import pytest
import torch

from tests import segcases as sc

pytestmark = pytest.mark.gpu

SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


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


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return torch.from_numpy(a.view(np.uint8).reshape(len(a), -1)).cuda()
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype))).cuda()


def host(t, dt):
    return t.cpu().numpy().reshape(-1).view(dt)


def run_gpu(g, clf, case, send_idx=True, counts=True, calls=1, stream=None):
    """@calls calls over sentinel-filled device outputs; (outputs as numpy, counts - their fill)."""
    m, cap = len(case["send"]), case["seg_cap"]
    blank = sc.blank(m, cap)
    out = {f: dev(a) for f, a in blank.items()}
    if not send_idx:
        out["send_idx"] = None
    cnt = torch.full((g.SEGC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    send = dev(case["send"]) if m else torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
    for _ in range(calls):
        clf.tx_seg(send, m, cap, stride=case["stride"], lead=case["lead"], frame_base=case["frame_base"],
                   frames_len=case["frames_len"], udp_max=case["udp_max"], blocks=case.get("blocks", 0),
                   out=out, counts=cnt, stream=stream)
    torch.cuda.synchronize()
    got = {f: (None if out[f] is None else host(out[f], blank[f].dtype)) for f in blank}
    return got, None if cnt is None else cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


def check(g, clf, case, want=None, what="", **kw):
    """GPU == host twin (== model when given), whole arrays with their guards"""
    hgot, hcnt = sc.run_host(g, case)
    got, cnt = run_gpu(g, clf, case, **kw)
    sc.compare(got, hgot, (what, "host"))
    assert cnt.tolist() == hcnt.tolist(), what
    if want is not None:
        sc.compare(got, want, (what, "model"))
        assert cnt.tolist() == want["counts"].tolist(), what
    return got, cnt


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_gpu_equals_model_and_host(g, clf, name):
    check(g, clf, sc.cases()[name], sc.models()[name], name)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes_around_the_tile(g, clf, m):
    rng = np.random.default_rng(100 + m)
    for stride in (0, 2048):
        case = sc.random_case(rng, m, stride=stride)
        check(g, clf, case, sc.model(case), (m, stride), send_idx=stride == 0)
    if m == 0:
        got, _ = run_gpu(g, clf, sc.random_case(rng, 0))
        assert got["total_segs"][0] == 0 and got["total_bytes"][0] == 0
        assert (got["status"] == sc.SENTINEL).all()


def test_skew_one_write_spans_hundreds_of_tiles(g, clf):
    rows = [dict(mss=100, len=int(50 + i)) for i in range(300)]
    rows.insert(150, dict(mss=1, len=70000, winlen=70000, snd_nxt=sc.M32 - 1234))
    for stride in (0, 64):
        case = sc.case(sc.sends(rows), 100000, stride=stride, lead=3)
        if stride:      # 100-byte segments do not fit 64-byte slots: 5-byte ones, checked against the twin
            case["send"]["mss"][case["send"]["mss"] == 100] = 5
        got, cnt = check(g, clf, case, None if stride else sc.model(case), ("skew", stride))
        assert int(got["nseg"][150]) == 70000 and int(cnt[sc.C_OK]) == 301


def test_gaps_of_refused_writes_inside_a_tile(g, clf):
    rows = []
    for r in range(12):
        rows += [dict(proto=0)] * 600
        rows += [dict(mss=50, len=50 * (1 + r % 3))] * (1 + r % 4) + [dict(proto=17, mss=0, len=9)]
    rows += [dict(proto=0)] * 700
    case = sc.case(sc.sends(rows), 4096, lead=1)
    got, cnt = check(g, clf, case, sc.model(case), "gaps")
    assert int(cnt[sc.C_REFUSED]) == 12 * 600 + 700 and 12 < int(got["total_segs"][0]) < 256
    # and whole tiles of segments with gaps between their writes
    rows = []
    for r in range(40):
        rows += [dict(proto=1)] * (600 if r % 5 == 0 else r % 3)
        rows += [dict(mss=10, len=10 * (1 + (7 * r) % 40))]
    case = sc.case(sc.sends(rows), 4096, stride=128)
    got, _ = check(g, clf, case, sc.model(case), "gaps2")
    assert int(got["total_segs"][0]) > 600


def test_ranges_and_the_nospace_cut(g, clf):
    """several ranges of the scan (blocks = 4 over 3000 writes: 768 each), the
    cut inside a range and exactly on a range boundary, by segments and by
    frames_len"""
    rng = np.random.default_rng(7)
    base = sc.random_case(rng, 3000, stride=0, refused=0.2, blocks=4)
    ample = sc.model(base)
    live = ample["status"] == sc.OK
    csum = np.cumsum(np.where(live, ample["nseg"], 0).astype(np.int64))
    check(g, clf, base, ample, "ample")
    for at in (768, 1536, 1000, 2990, 1):
        # a cap that write at - 1 just fits and a live write at `at` does not: the cut is at index `at`
        while not live[at]:
            at += 1
        cap = int(csum[at - 1])
        case = dict(base, seg_cap=cap)
        got, _ = check(g, clf, case, sc.model(case), ("cut", at))
        assert got["status"][at] == sc.NOSPACE and int(got["total_segs"][0]) == cap
        assert (got["status"][:at] != sc.NOSPACE).all()
        flen = base["frame_base"] + base["lead"] + int(ample["total_bytes"][0])   # ample room: no byte cut
        case = dict(base, seg_cap=int(csum[-1]), frames_len=flen)
        # the same cut made by frames_len: room for the frames of the writes before `at` and one byte less
        used = int(sc.model(dict(base, seg_cap=cap))["total_bytes"][0])
        first_len = (34 + (20 if base["send"]["proto"][at] == 6 else 8) + 15) // 16 * 16
        case["frames_len"] = base["frame_base"] + base["lead"] + used + first_len - 1
        got, _ = check(g, clf, case, sc.model(case), ("byte cut", at))
        assert got["status"][at] == sc.NOSPACE and int(got["total_segs"][0]) == cap
    for blocks in (1, 3, 1024, 0):
        case = dict(base, blocks=blocks, seg_cap=int(csum[-1]) // 2)
        check(g, clf, case, what=("blocks", blocks))


def test_counts_accumulate_stream_and_optional_outputs(g, clf):
    case, want = sc.cases()["cap7_packed"], sc.models()["cap7_packed"]
    got, cnt = run_gpu(g, clf, case, calls=2)
    sc.compare(got, want, "twice")
    assert cnt.tolist() == (2 * want["counts"]).tolist()
    stream = torch.cuda.Stream()
    got, cnt = run_gpu(g, clf, case, send_idx=False, counts=False, stream=stream.cuda_stream)
    sc.compare(got, want, "stream")
    assert cnt is None and got["send_idx"] is None


def test_errors(g, clf):
    case = sc.cases()["cap7_packed"]
    m, cap = len(case["send"]), 16
    out = {f: dev(a) for f, a in sc.blank(m, cap).items()}
    send = dev(case["send"])
    ws = torch.empty(g.tx_seg_workspace(m), dtype=torch.uint8, device="cuda")

    def call(in_kw=None, out_kw=None, ctx=clf._ctx, counts=None, wsp=ws.data_ptr(), wsn=ws.numel()):
        o = {f: out[f].data_ptr() for f in g.SEG_OUT_FIELDS}
        o.update(out_kw or {})
        kw = dict(size=ctypes.sizeof(g.GclSegIn), send=send.data_ptr(), m=m, seg_cap=cap, udp_max=1472)
        kw.update(in_kw or {})
        sin, sout = g.GclSegIn(**kw), g.GclSegOut(**o)
        return g.lib.gcl_tx_seg(ctx, ctypes.byref(sin), ctypes.byref(sout), counts, wsp, wsn, None)

    assert call() == 0
    assert call(out_kw=dict(send_idx=None)) == 0
    assert call(dict(m=0, send=None), dict(status=None, desc=None)) == 0
    assert call(dict(seg_cap=0), dict(desc=None, frame_off=None, src_off=None, len=None, dst_off=None)) == 0
    assert call(ctx=None) == -errno.EINVAL
    for kw in (dict(size=60), dict(send=None), dict(m=2 ** 31 + 1), dict(seg_cap=2 ** 31 + 1),
               dict(stride=(1 << 20) + 1), dict(lead=65536), dict(udp_max=65508), dict(blocks=1025),
               dict(send=send.data_ptr() + 8)):
        assert call(kw) == -errno.EINVAL, kw
    for f in g.SEG_OUT_FIELDS:
        if f != "send_idx":
            assert call(out_kw={f: None}) == -errno.EINVAL, f
    for f, by in (("sent", 2), ("nseg", 2), ("desc", 8), ("frame_off", 4), ("len", 1), ("send_idx", 2),
                  ("total_segs", 4)):
        assert call(out_kw={f: out[f].data_ptr() + by}) == -errno.EINVAL, f
    assert call(counts=out["frame_off"].data_ptr() + 4) == -errno.EINVAL
    assert call(wsp=None) == -errno.EINVAL and call(wsp=ws.data_ptr() + 8) == -errno.EINVAL
    assert call(wsn=ws.numel() - 1) == -errno.EINVAL
    torch.cuda.synchronize()


def test_chain_bytes_written_are_the_bytes_received(g):
    """gcl_tx_seg -> gcl_copy_batch -> gcl_tx_hdr -> gcl_l4_csum FILL, looped
    back through gcl_copy_batch -> gcl_classify -> gcl_l4_csum VERIFY ->
    gcl_l4_payload -> gcl_copy_batch: every TCP segment verifies GOOD and each
    connection's received bytes, ordered by seq, are the bytes written."""
    rng = np.random.default_rng(42)
    addr, peer, mac = g.runtime_ip(0), g.runtime_ip(1), bytes([2, 0, 0, 0, 0, 9])
    conns = [dict(proto=6, lport=5000 + i, mss=int(ms), isn=int(isn), nbytes=int(nb))
             for i, (ms, isn, nb) in enumerate([(100, 7, 30000), (536, sc.M32 - 5000, 60000), (1460, 1 << 31, 90000),
                                                (7, 12345, 5000), (1, sc.M32, 1200), (1000, 99, 0)])]
    conns += [dict(proto=17, lport=6000 + i, mss=0, isn=0, nbytes=int(nb)) for i, nb in enumerate([5000, 1472])]
    rows, streams, at = [], {}, 0
    for c in conns:
        streams[c["lport"]] = rng.integers(0, 256, c["nbytes"], dtype=np.uint8)
        c["src"], c["done"] = at, 0
        at += c["nbytes"] + int(rng.integers(0, 50))
    src = np.zeros(at + 1, dtype=np.uint8)
    for c in conns:
        src[c["src"]:c["src"] + c["nbytes"]] = streams[c["lport"]]
    live = list(conns)
    while live:     # the connections' writes interleaved, each with its own snd_nxt
        c = live[int(rng.integers(0, len(live)))]
        left = c["nbytes"] - c["done"]
        n = min(left, int(rng.integers(0, 4000 if c["proto"] == 6 else 600)))
        if c["proto"] == 6 and rng.random() < 0.2:
            n = left if left < 9000 else n
        rows.append(dict(proto=c["proto"], lip=0, rip=peer, lport=c["lport"], rport=80, mss=c["mss"],
                         snd_nxt=(c["isn"] + c["done"]) & sc.M32, len=n + (50 if rng.random() < 0.1 else 0),
                         winlen=n, src_off=c["src"] + c["done"], ecn=0) if c["proto"] == 6 else
                    dict(proto=17, lip=0, rip=peer, lport=c["lport"], rport=80, mss=0, len=n, winlen=0,
                         src_off=c["src"] + c["done"], ecn=0))
        c["done"] += n
        if c["done"] == c["nbytes"]:
            live.remove(c)
    send = sc.sends(rows)
    cap = 8192
    want = sc.model(sc.case(send, cap, lead=0))
    total = int(want["total_segs"][0])
    assert 2000 < total < cap and (want["status"] == sc.OK).all()

    c = g.Classifier(0, 16, g.HASH_JENKINS)
    try:
        c.runtime_set(1, peer, 4, 4, [0, 1, 2, 3])
        c.neigh_set([(peer, mac)])
        seg = c.tx_seg(dev(send), len(send), cap)
        torch.cuda.synchronize()
        n = int(seg["total_segs"].cpu()[0])
        assert n == total
        frames = torch.zeros(int(seg["total_bytes"].cpu()[0]), dtype=torch.uint8, device="cuda")
        dsrc = torch.from_numpy(src).cuda()
        c.copy_batch(dsrc, seg["src_off"], seg["len"], n, frames, dst_off=seg["dst_off"], olflags=False, rss=False)
        net = g.txh_net(addr, 0xFFFFFF00, g.runtime_ip(9), mac)
        hdr = c.tx_hdr(seg["desc"], seg["frame_off"], n, frames, net)
        c.l4_csum(frames, n, hdr["pkt_len"], mode=g.L4_FILL, offs=seg["frame_off"], tx_olflags=hdr["tx_olflags"])
        # the loopback
        stride = 1536
        pool = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
        pkt_len, olflags, rss = c.copy_batch(frames, seg["frame_off"], hdr["pkt_len"], n, pool, dst_stride=stride,
                                             tx_olflags=hdr["tx_olflags"], hash=hdr["hash"])
        verd = torch.zeros(n * c.vbytes, dtype=torch.uint8, device="cuda")
        c.classify(pool, n, stride, verdicts=verd, olflags=olflags, rss=rss)
        st = c.l4_csum(pool, n, pkt_len, mode=g.L4_VERIFY, stride=stride)
        pay = c.l4_payload(pool, n, pkt_len, stride=stride, l4_status=st)
        torch.cuda.synchronize()
        rx = torch.zeros(max(int(pay["total"].cpu()[0]), 1), dtype=torch.uint8, device="cuda")
        c.copy_batch(pool, pay["src_off"], pay["len"], n, rx, dst_off=pay["dst_off"], olflags=False, rss=False)
        torch.cuda.synchronize()

        assert (host(hdr["status"], np.uint8)[:n] == g.TXH_OK).all()
        v = verd.cpu().numpy().reshape(-1).view(g.verdict_dtype(c.vbytes))[:n]
        assert ((v["action"] & g.ACT_MASK) == g.ACT_DELIVER).all() and (v["uniqid"] == 1).all()
        tcp = want["desc"]["proto"][:n] == 6
        st = st.cpu().numpy()[:n]
        assert (st[tcp] == g.L4_GOOD).all() and (st[~tcp] == g.L4_NONE).all()
        kind = pay["kind"].cpu().numpy()[:n]
        assert (kind[tcp] == g.PAY_TCP).all() and (kind[~tcp] == g.PAY_UDP).all()
        meta = pay["meta"].cpu().numpy().reshape(-1).view(g.PAY_META_DTYPE)[:n]
        off, ln = host(pay["dst_off"], np.uint64)[:n], host(pay["len"], np.uint16)[:n]
        rxb = rx.cpu().numpy()
        assert int(ln.sum()) == sum(cn["nbytes"] for cn in conns) == int(pay["total"].cpu()[0])
        for cn in conns:
            mine = np.nonzero(meta["rport"] == cn["lport"])[0]
            assert (meta["rip"][mine] == addr).all()
            if cn["proto"] == 6:    # ordered by seq, relative to the connection's first byte
                rel = (meta["seq"][mine].astype(np.int64) - cn["isn"]) & sc.M32
                mine = mine[np.argsort(rel, kind="stable")]
            data = np.concatenate([rxb[int(off[j]):int(off[j]) + int(ln[j])] for j in mine]) if len(mine) else \
                np.zeros(0, dtype=np.uint8)
            assert np.array_equal(data, streams[cn["lport"]]), cn["lport"]
    finally:
        c.close()
