"""GPU: gcl_l4_payload (include/gclassify.h), the payload descriptors and the
packed receive layout of a list of packets.  Every case compares every output
array, total, seg_bytes and the counters for exact equality with the numpy
definition (tests/paycases.py) AND with the host twin gcl_l4_payload_host;
every output buffer starts as a sentinel and carries a guard that must come
back unchanged.  torch only holds buffers."""
import ctypes
import functools

import numpy as np
import pytest

from tests import l4cases as lc
from tests import paycases as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = 22
SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    assert gclassify.PAYC_NR == pc.NR and gclassify.PAY_MAX_BLOCKS == pc.MAX_BLOCKS
    return gclassify


@pytest.fixture(scope="module")
def clf(g):
    c = g.Classifier(0, 16, g.HASH_NIC, 0, 0x01)
    yield c
    c.close()


def dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == pc.META:
        return torch.from_numpy(a.view(np.uint8).reshape(-1, 16)).cuda()
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype))).cuda()


def host(t, like):
    """A device buffer back as numpy in @like's dtype."""
    return None if t is None else t.cpu().numpy().reshape(-1).view(like.dtype)


@functools.lru_cache(maxsize=None)
def region(key, shift):
    """The case's frame region @shift bytes into a device tensor, kept."""
    case = CASES[key]()
    flen = case["frames_len"]
    buf = np.full(flen + shift, lc.FILLBYTE, dtype=np.uint8)
    buf[shift:] = case["frames"][:flen]
    return torch.from_numpy(buf).cuda()[shift:]


CASES = {"grid": pc.grid_case, "filter": lambda: pc.filter_case()[0], "big": lambda: pc.big_case()[0],
         "na": lambda: pc.na_case(None), "na_payload": lambda: pc.na_case("payload"),
         "na_header": lambda: pc.na_case("header")}


def run(g, clf, key, what, order=None, sock=None, st=None, seg_off=None, align=0, blocks=0, counts=True,
        meta=True, shift=0, stream=None, workspace=None, pk=None, twin=True):
    """One gcl_l4_payload over case @key, held to the model and to the host
    twin; returns (model, counts)."""
    case = CASES[key]()
    want = pc.model(case, order, sock, st, seg_off, align, pk=pk)
    n, m = len(case["pkt_len"]), len(want["kind"])
    nseg = len(seg_off) - 1 if seg_off is not None else 0
    blank = pc.blank_outputs(m, nseg, with_seg=seg_off is not None, with_meta=meta)
    if twin:
        tw = g.l4_payload_host(case["frames"][:case["frames_len"]], case["pkt_len"], stride=case["stride"],
                               offs=case["offs"], n=n, order=order, m=m, sock=sock, l4_status=st,
                               seg_off=seg_off, nseg=nseg, align=align, out={k: None if v is None else v.copy()
                                                                             for k, v in blank.items()})
        pc.compare(tw, want, m, nseg, what + " (twin)")
    out = {k: dev(v) for k, v in blank.items()}
    cnt = torch.full((pc.NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    fr = region(key, shift)
    args = dict(stride=case["stride"], offs=dev(case["offs"]), order=dev(order), m=m, sock=dev(sock),
                l4_status=dev(st), seg_off=dev(seg_off), nseg=nseg, align=align, blocks=blocks, out=out,
                counts=cnt, workspace=workspace, stream=stream)
    plen = dev(case["pkt_len"])
    if stream is not None:
        torch.cuda.synchronize()
    got = clf.l4_payload(fr, n, plen, **args)
    torch.cuda.synchronize()
    pc.compare({k: host(got[k], blank[k]) if blank[k] is not None else None for k in blank}, want, m, nseg,
               what)
    if counts:
        c = cnt.cpu().numpy().view(np.uint64) - np.uint64(5)
        assert c.tolist() == want["counts"].tolist() and int(c[:6].sum()) == m, what
    return want, cnt


def test_grid_every_header_length_payload_and_alignment(g, clf):
    """TCP data offsets 5..15 x six payload lengths, four UDP payloads, 16
    frame alignments; the region's base shifted so that frames are 4-B aligned
    (the window loads) and not (the bytewise form); align 1, 16 and 256."""
    pk = pc.packets(pc.grid_case())
    for align in (1, 16, 256):
        want, _ = run(g, clf, "grid", f"grid align {align}", align=align, pk=pk)
        assert (want["kind"] != pc.NA).all()
    for shift in (1, 4, 9):
        run(g, clf, "grid", f"grid base + {shift}", align=16, shift=shift, pk=pk, twin=False)
    run(g, clf, "grid", "grid without meta and counts", meta=False, counts=False, pk=pk)


@pytest.mark.parametrize("key", ["na", "na_payload", "na_header"])
def test_na_reasons_one_frame_each(g, clf, key):
    """Every non-eligibility, data offset 4, hl > tot - 20, a pkt_len one
    short, offsets at and past frames_len, and a frame cut by frames_len
    inside the TCP header and one byte before the payload's end."""
    for shift in (0, 1, 4, 8, 12):
        want, _ = run(g, clf, key, f"{key} base + {shift}", shift=shift)
    kinds = dict(zip(pc.NA_NAMES, want["kind"].tolist()))
    assert kinds["good_udp"] == pc.K_UDP and kinds["good_tcp"] == pc.K_TCP
    assert kinds["cut"] == (pc.K_TCP if key == "na" else pc.NA)
    assert sum(k == pc.NA for k in kinds.values()) == (14 if key == "na" else 15)


def test_filters_and_their_priority(g, clf):
    _, sock, st = pc.filter_case()
    n = len(sock)
    want, _ = run(g, clf, "filter", "filters", sock=sock, st=st, align=16)
    assert all((want["kind"] == k).sum() >= 8 for k in (pc.K_UDP, pc.K_TCP, pc.NA, pc.NOSOCK, pc.BADCSUM))
    run(g, clf, "filter", "sock alone", sock=sock)
    run(g, clf, "filter", "l4_status alone", st=st)
    order = np.array([0, n, 1, 0xFFFFFFFF], dtype=np.uint32)
    want, _ = run(g, clf, "filter", "oor first", order=order, sock=sock, st=st)
    assert want["kind"].tolist() == [pc.K_UDP, pc.OOR, pc.K_TCP, pc.OOR]


@pytest.mark.parametrize("name", ["permutation", "shorter", "longer"])
def test_orders_and_segments(g, clf, name):
    """A permutation, m < n, m > n with duplicates and entries >= n, and
    seg_off values past m and out of order.  (A real gcl_plan order with
    seg_off = bucket_off is the end-to-end test's.)"""
    _, sock, st = pc.filter_case()
    order, seg = pc.orders(len(sock))[name]
    run(g, clf, "filter", name, order=order, sock=sock, st=st, seg_off=seg, align=16)
    run(g, clf, "filter", name + " dense, 3 ranges", order=order, seg_off=seg, blocks=3)


@pytest.mark.parametrize("blocks", pc.SCAN_BLOCKS + (0,))
def test_scan_carries_over_tiles_and_ranges(g, clf, blocks):
    """m = 3 * 256 * k + 5 with every range of every blocks value longer than
    a tile, so that each block's tile loop carries; the ragged last tile."""
    case, sock, st, order = pc.scan_case()
    seg = np.array([0, pc.SCAN_M // 2, pc.SCAN_M - 1, pc.SCAN_M], dtype=np.uint32)
    run(g, clf, "filter", f"scan blocks {blocks}", order=order, sock=sock, st=st, seg_off=seg, align=16,
        blocks=blocks, pk=SCAN_PK(), twin=blocks == 0)


@functools.lru_cache(maxsize=None)
def SCAN_PK():
    return pc.packets(pc.filter_case()[0])


@pytest.mark.parametrize("blocks", [0, 3])
def test_the_carry_is_64_bit(g, clf, blocks):
    """70 000 entries naming one maximal UDP datagram, align 256: the model's
    total is 70 000 x 65 536 > 2^32, at the memory cost of one frame."""
    _, order = pc.big_case()
    want, _ = run(g, clf, "big", f"big blocks {blocks}", order=order, align=256, blocks=blocks,
                  seg_off=np.array([69999, 65536, 70000], dtype=np.uint32), twin=blocks == 0)
    assert int(want["total"][0]) == pc.BIG_M * 65536 > 1 << 32
    assert int(want["dst_off"][-1]) > 1 << 32


def test_reuse_accumulate_m_zero_and_null_counts(g, clf):
    """Two different batches back to back on one stream with one workspace
    that holds garbage; counts accumulating over both; m == 0; counts NULL."""
    _, sock, st = pc.filter_case()
    stream = torch.cuda.Stream()
    ws = torch.full((g.l4_payload_workspace(1 << 20),), 0xFF, dtype=torch.uint8, device="cuda")
    wa, ca = run(g, clf, "filter", "first", sock=sock, st=st, workspace=ws, stream=stream.cuda_stream)
    wb, cb = run(g, clf, "grid", "second", align=16, workspace=ws, stream=stream.cuda_stream)
    # the same two calls with nothing between them, into one counts array
    fa, fb = pc.filter_case()[0], pc.grid_case()
    cnt = torch.zeros(pc.NR, dtype=torch.int64, device="cuda")
    args = [(region("filter", 0), len(sock), dev(fa["pkt_len"]), dict(offs=dev(fa["offs"]), sock=dev(sock),
                                                                    l4_status=dev(st))),
            (region("grid", 0), len(fb["pkt_len"]), dev(fb["pkt_len"]), dict(offs=dev(fb["offs"]), align=16))]
    torch.cuda.synchronize()
    outs = [clf.l4_payload(fr, n, pl, counts=cnt, workspace=ws, stream=stream.cuda_stream, **kw)
            for fr, n, pl, kw in args]
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().view(np.uint64).tolist() == (wa["counts"] + wb["counts"]).tolist()
    for o, w in zip(outs, (wa, wb)):
        assert (host(o["dst_off"], w["dst_off"])[:len(w["kind"])] == w["dst_off"]).all()
        assert host(o["total"], w["total"]).tolist() == w["total"].tolist()
        assert (host(o["meta"], w["meta"])[:len(w["kind"])] == w["meta"]).all()
    # m == 0: total and seg_bytes are zeroed, nothing else is touched
    for order in (np.zeros(1, dtype=np.uint32), None):
        blank = pc.blank_outputs(0, 2)
        out = {k: dev(v) for k, v in blank.items()}
        cnt = torch.full((pc.NR,), 9, dtype=torch.int64, device="cuda")
        clf.l4_payload(region("filter", 0), len(sock) if order is not None else 0, dev(fa["pkt_len"]),
                       offs=dev(fa["offs"]), order=dev(order), m=0,
                       seg_off=dev(np.array([0, 1, 7], dtype=np.uint32)), nseg=2, out=out, counts=cnt,
                       workspace=ws)
        torch.cuda.synchronize()
        want = {"seg_bytes": np.zeros(3, dtype=np.uint64), "total": np.zeros(1, dtype=np.uint64)}
        pc.compare({k: host(out[k], blank[k]) for k in blank}, want, 0, 2, "m == 0", written=False)
        assert (cnt == 9).all() and (ws == 0xFF).sum() > 0


E2E = (16, 4, 4096, 1536, 7000)  # runtimes, kthreads, packets, slot bytes, the registered port


def e2e_inputs(runtime_ip):
    """The end-to-end batch and what every step must say about it, by
    construction and by the numpy definitions; no GPU is touched."""
    rng = np.random.default_rng(81)
    R, T, n, slot, PORT = E2E
    frs, key, why = [], np.zeros(n, dtype=np.int64), []
    for i in range(n):
        tcp = rng.random() < 0.5
        pay = int(rng.choice([0, int(rng.integers(1, 200)), 1460 if tcp else 1472], p=[0.1, 0.6, 0.3]))
        f = pc.tcp_frame(rng, int(rng.integers(5, 9)), pay) if tcp else pc.udp_frame(rng, pay)
        r = int(rng.integers(0, R))
        w = {0: "unreg_ip", 1: "unreg_port", 2: "spoiled", 3: "fragment"}.get(i % 16, "good")
        ip = 0x0A090909 if w == "unreg_ip" else runtime_ip(r)
        port = PORT + 1 if w == "unreg_port" else PORT
        f[0:12] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2)
        f[30:34] = list(ip.to_bytes(4, "big"))
        f[36:38] = (port >> 8, port & 0xFF)
        if w == "fragment":
            f[20:22] = (0x20, 0x00)
        frs.append(f)
        key[i] = R if w == "unreg_ip" else r
        why.append(w)
    why = np.array(why)
    case = lc.filled(lc.slots(frs, slot))
    lc.spoil(case, rng, np.nonzero(why == "spoiled")[0], where="last")
    # what each step must say, by construction and by the numpy definitions
    st_want = lc.model(case, lc.VERIFY)[0]
    cookie = lambda i: 2 * int(key[i]) + (case["frames"][i * slot + 23] == lc.UDP)  # noqa: E731
    sock_want = np.array([pc.S_NA if why[i] == "unreg_ip" else pc.S_MISS if why[i] == "unreg_port"
                          else cookie(i) for i in range(n)], dtype=np.uint32)
    order_want = np.argsort(key, kind="stable").astype(np.uint32)
    boff_want = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=R + 1))]).astype(np.uint32)
    pk = pc.packets(case)
    want = pc.model(case, order_want, sock_want, st_want, boff_want, 0, pk=pk)
    kept_pkt = np.zeros(n, dtype=bool)
    kept_pkt[order_want[(want["kind"] == pc.K_UDP) | (want["kind"] == pc.K_TCP)]] = True
    assert kept_pkt.sum() >= n // 4 and (kept_pkt == (why == "good")).all()
    assert all((want["kind"] == k).sum() >= n // 16 for k in (pc.NA, pc.BADCSUM, pc.NOSOCK))
    assert (st_want[why == "spoiled"] == lc.BAD).all() and (st_want[why == "good"] != lc.BAD).all()
    streams = [b"".join(case["frames"][int(pk[2][i]):int(pk[2][i]) + int(pk[1][i])].tobytes()
                        for i in range(n) if key[i] == r and kept_pkt[i]) for r in range(R + 1)]
    assert all(len(s) > 1000 for s in streams[:R]) and streams[R] == b""
    assert sum(len(s) for s in streams) == int(want["total"][0])

    return case, key, why, st_want, sock_want, order_want, boff_want, pk, want, streams


def test_end_to_end_receive_streams(g):
    """classify -> sock_lookup -> l4_csum VERIFY -> plan -> l4_payload ->
    copy_batch over 4096 mixed TCP/UDP packets for 16 runtimes, some with a
    spoiled checksum, an unregistered port, an unregistered address or a
    fragment: bytes [seg_bytes[r], seg_bytes[r + 1]) of the receive buffer are
    runtime r's kept payloads in packet order."""
    R, T, n, slot, PORT = E2E
    case, key, why, st_want, sock_want, order_want, boff_want, pk, want, streams = e2e_inputs(g.runtime_ip)

    clf = g.Classifier(0, R, g.HASH_JENKINS)
    for r in range(R):
        clf.runtime_set(r, g.runtime_ip(r), T, T, g.steer_flows(T, list(range(T))))
        clf.sock_set(r, [(g.runtime_ip(r), PORT, proto, g.SOCK_MATCH_3TUPLE, 2 * r + (proto == lc.UDP))
                         for proto in (lc.TCP, lc.UDP)])
    fr, plen = dev(case["frames"]), dev(case["pkt_len"])
    v = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    clf.classify(fr, n, slot, verdicts=v)
    sock = clf.sock_lookup(fr, n, slot, verdicts=v)
    status = clf.l4_csum(fr, n, plen, mode=g.L4_VERIFY, stride=slot, len_hint=1500)
    order, boff = clf.plan(v, n)
    blank = pc.blank_outputs(n, R + 1)
    out = {k: dev(a) for k, a in blank.items()}
    cnt = torch.zeros(pc.NR, dtype=torch.int64, device="cuda")
    clf.l4_payload(fr, n, plen, stride=slot, order=order, m=n, sock=sock, l4_status=status, seg_off=boff,
                   nseg=R + 1, out=out, counts=cnt)
    total = int(want["total"][0])
    rx = torch.full((total + 4096,), pc.SENTINEL, dtype=torch.uint8, device="cuda")
    ccnt = torch.zeros(g.COPY_NR, dtype=torch.int64, device="cuda")
    clf.copy_batch(fr, out["src_off"], out["len"], n, rx[:total], dst_off=out["dst_off"], counts=ccnt,
                   olflags=False, rss=False)
    torch.cuda.synchronize()
    verd = v.cpu().numpy().view(g.VERDICT_DTYPE)
    assert (np.where(verd["action"] & g.ACT_MASK <= g.ACT_WAKE, verd["uniqid"], R) == key).all()
    assert (status.cpu().numpy()[:n] == st_want).all()
    elig = pk[0][:n] != pc.NA
    assert (sock.cpu().numpy().view(np.uint32)[:n][elig] == sock_want[elig]).all()
    assert (order.cpu().numpy().view(np.uint32)[:n] == order_want).all()
    assert (boff.cpu().numpy().view(np.uint32) == boff_want).all()
    pc.compare({k: host(out[k], blank[k]) for k in blank}, want, n, R + 1, "end to end")
    assert cnt.cpu().numpy().view(np.uint64).tolist() == want["counts"].tolist()
    assert ccnt.cpu().numpy().tolist()[:3] == [n, 0, total]
    got, seg = rx.cpu().numpy(), want["seg_bytes"]
    assert (got[total:] == pc.SENTINEL).all()
    for r in range(R + 1):
        assert got[int(seg[r]):int(seg[r + 1])].tobytes() == streams[r], f"runtime {r}'s stream"
    assert int(seg[R + 1]) == total
    clf.close()


def test_error_returns(g, clf):
    case, sock, st = pc.filter_case()
    n = len(sock)
    blank = pc.blank_outputs(n, 1)
    out = {k: dev(a) for k, a in blank.items()}
    seg, order = dev(np.array([0, n], dtype=np.uint32)), dev(np.arange(n, dtype=np.uint32))
    d_sock, offs, plen, fr = dev(sock), dev(case["offs"]), dev(case["pkt_len"]), region("filter", 0)
    cnt = torch.full((pc.NR,), 9, dtype=torch.int64, device="cuda")
    need = g.l4_payload_workspace(n)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    size = ctypes.sizeof(g.GclPayIn)
    P = lambda t: t.data_ptr()  # noqa: E731

    def call(ctx=clf._ctx, bb=True, ii=True, oo=True, frames=P(fr), flen=case["frames_len"], stride=0,
             offs=P(offs), plen=P(plen), nn=n, sz=size, align=0, order=None, m=n, sock=None, st=None,
             seg_off=P(seg), nseg=1, blocks=0, counts=P(cnt), w=P(ws), wb=need, **o):
        b = g.GclBatch(frames=frames, frames_len=flen, stride=stride, offs=offs, pkt_len=plen, n=nn)
        i = g.GclPayIn(size=sz, align=align, order=order, m=m, sock=sock, l4_status=st, seg_off=seg_off,
                       nseg=nseg, blocks=blocks)
        ptrs = {f: P(out[f]) for f in g.PAY_OUT_FIELDS}
        ptrs.update(o)
        po = g.GclPayOut(**ptrs)
        return g.lib.gcl_l4_payload(ctx, ctypes.byref(b) if bb else None, ctypes.byref(i) if ii else None,
                                    ctypes.byref(po) if oo else None, counts, w, wb, None)

    assert call(ctx=None) == -EINVAL
    assert call(bb=False) == -EINVAL and call(ii=False) == -EINVAL and call(oo=False) == -EINVAL
    assert call(sz=size - 8) == -EINVAL and call(sz=0) == -EINVAL
    for align in (3, 6, 12, 48, 255, 512, 1 << 31):
        assert call(align=align) == -EINVAL, align
    assert call(m=n - 1) == -EINVAL and call(m=n + 1) == -EINVAL          # no order: m must be n
    assert call(order=P(order), m=(1 << 31) + 1) == -EINVAL
    assert call(blocks=pc.MAX_BLOCKS + 1) == -EINVAL
    for f in ("src_off", "len", "dst_off", "kind", "total"):
        assert call(**{f: None}) == -EINVAL, f
    for f in ("src_off", "len", "dst_off", "total", "seg_bytes", "meta"):
        assert call(**{f: P(out[f]) + 1}) == -EINVAL, f
    assert call(meta=P(out["meta"]) + 8) == -EINVAL
    assert call(seg_bytes=None) == -EINVAL and call(seg_off=None) == -EINVAL
    assert call(order=P(order) + 2) == -EINVAL and call(sock=P(d_sock) + 1) == -EINVAL
    assert call(seg_off=P(seg) + 2) == -EINVAL and call(counts=P(cnt) + 4) == -EINVAL
    assert call(plen=None) == -EINVAL and call(plen=P(plen) + 1) == -EINVAL
    assert call(frames=None) == -EINVAL and call(flen=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1, order=P(order)) == -EINVAL
    for stride in (0, 8, 15, 24, 72, (1 << 20) + 16):
        assert call(offs=None, stride=stride) == -EINVAL, stride
    assert call(w=None) == -EINVAL and call(w=P(ws) + 8) == -EINVAL and call(wb=need - 1) == -EINVAL
    assert call(blocks=7, wb=g.l4_payload_workspace(n, 7) - 1) == -EINVAL
    assert g.l4_payload_workspace(n, 7) == 64 and need == 8 * pc.MAX_BLOCKS
    sz_t = ctypes.c_size_t()
    assert g.lib.gcl_l4_payload_workspace((1 << 31) + 1, 0, ctypes.byref(sz_t)) == -EINVAL
    assert g.lib.gcl_l4_payload_workspace(n, pc.MAX_BLOCKS + 1, ctypes.byref(sz_t)) == -EINVAL
    assert g.lib.gcl_l4_payload_workspace(n, 0, None) == -EINVAL
    torch.cuda.synchronize()  # nothing was launched
    assert all((t.cpu().numpy().view(np.uint8) == pc.SENTINEL).all() for t in out.values())
    assert (cnt == 9).all() and (ws == 0xFF).all()
    assert call(meta=None, counts=None, seg_off=None, seg_bytes=None, align=256, blocks=pc.MAX_BLOCKS) == 0
    assert call(order=P(order), m=0, nn=0, frames=None, plen=None) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        clf.l4_payload(fr, n, None, offs=offs)
    with pytest.raises(ValueError):
        clf.l4_payload(fr, n, plen, offs=offs, order=order, m=n + 1)
    with pytest.raises(ValueError):
        clf.l4_payload(fr, n, plen, offs=offs, sock=d_sock[:n - 1])
    with pytest.raises(ValueError):
        clf.l4_payload(fr, n, plen, offs=offs, counts=cnt[:3])
