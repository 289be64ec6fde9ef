"""GPU: gcl_tcp_tick and gcl_tcp_rx_acks (include/gclassify.h) against their
host twins and the model of tests/tcptmrcases.py, byte for byte over
sentinel-filled outputs with guards, on the named cases, on random sweeps and
on the shapes where the kernels can go wrong: the wave and block edges, forced
range counts so that the scan of the block sums has work, every lane or no lane
emitting, one emitter at the first and the last lane of a block, seg_cap at
every cut, a dirty workspace, 2^20 connections; and the two chains: sweep ->
tx_hdr -> l4_csum FILL against the reference's own header bytes
(tests/golden/tcpctl_ref.json), and tcp_rx -> tcp_rx_acks -> tx_hdr against the
ACK numbers and windows of the model's per-segment tcp_tx_ack."""
import ctypes
import errno

import numpy as np
import pytest
import torch

from tests import tcprxcases as rc
from tests import tcptmrcases as tm
from tests.test_gpu_tcprx import dev, run_gpu as run_tcp_rx

pytestmark = pytest.mark.gpu


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
    """a record array for the device; an empty one still gets an address"""
    return dev(a) if len(a) else torch.zeros((1, width), dtype=torch.uint8, device="cuda")


def back(out, blank):
    return {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}


def run_tick(g, clf, case, counts=True, calls=1, workspace=None):
    """@calls sweeps over sentinel-filled device outputs: (outputs as numpy, counts of the last call)"""
    nconn = len(case["tmr"])
    blank = tm.blank(nconn, case["seg_cap"])
    out = {f: dev(a) for f, a in blank.items()}
    tmr, conn, addr = rec(case["tmr"], 64), rec(case["conn"], 48), rec(case["addr"], 16)
    cnt = None
    for _ in range(calls):
        cnt = torch.full((g.TICKC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
        clf.tcp_tick(case["now"], tmr, conn, addr, nconn, case["seg_cap"], frame_stride=case["frame_stride"],
                     frame_base=case["frame_base"], blocks=case.get("blocks", 0), out=out, counts=cnt,
                     workspace=workspace)
    torch.cuda.synchronize()
    return back(out, blank), None if cnt is None else cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


def check(g, clf, case, what, model=True, **kw):
    """GPU == host twin (== model), whole arrays with their guards"""
    nconn = len(case["tmr"])
    hgot, hcnt = tm.run_host(g, case)
    got, cnt = run_tick(g, clf, case, **kw)
    want = {f: hgot[f][:len(hgot[f]) - tm.GUARD] for f in hgot}
    k = int(want["totals"][1])
    want.update({f: want[f][:k] for f, _ in tm.SEG})
    tm.compare(got, want, nconn, case["seg_cap"], (what, "host"))
    assert cnt.tolist() == hcnt.tolist(), what
    if model:
        want = tm.model(case)
        tm.compare(got, want, nconn, case["seg_cap"], (what, "model"))
        assert cnt.tolist() == want["counts"].tolist(), what
    return got


@pytest.mark.parametrize("name", sorted(tm.cases()))
def test_named_cases(g, clf, name):
    check(g, clf, tm.cases()[name], name)


T = tm.TILE


@pytest.mark.parametrize("nconn", [1, 63, 64, 65, T - 1, T, T + 1, 3000])
def test_wave_and_block_edges(g, clf, nconn):
    check(g, clf, tm.random_case(20 + nconn, nconn, due=0.8), nconn)


@pytest.mark.parametrize("blocks", [1, 2, 7, tm.MAX_BLOCKS])
def test_forced_ranges(g, clf, blocks):
    """one range walks twelve tiles; 1024 ranges leave most of them empty and fill the scan of the sums"""
    check(g, clf, tm.random_case(31, 3000, due=0.7, blocks=blocks), blocks)
    check(g, clf, tm.random_case(32, 5 * T + 9, due=1.0, blocks=blocks, segs=lambda k: 3), (blocks, "full"))


@pytest.mark.parametrize("segs", [0, 1, 2, 3])
def test_every_lane_emits_the_same(g, clf, segs):
    got = check(g, clf, tm.random_case(33, 3 * T + 5, segs=lambda k: segs), segs)
    assert got["totals"][:2].tolist() == [bin(segs).count("1") * (3 * T + 5)] * 2


@pytest.mark.parametrize("at", [0, 63, 64, T - 1, T, 2 * T - 1, 4 * T - 1])
def test_one_emitter_at_a_block_edge(g, clf, at):
    """the only connection with segments sits at the first or last lane of a wave or of a block's tile"""
    got = check(g, clf, tm.random_case(34, 4 * T, blocks=4, segs=lambda k: 3 if k == at else 0), at)
    assert got["seg_conn"][:2].tolist() == [at, at] and got["seg_kind"][:2].tolist() == [tm.K_ACK, tm.K_PROBE]


@pytest.mark.parametrize("cap", [0, 1, 2 * T - 1, 2 * T, 2 * T + 1, 2 * (T + 40) - 1, 2 * (T + 40)])
def test_seg_cap_at_every_cut(g, clf, cap):
    """T + 40 connections of two segments each: a cap of 0, one that cuts
    between an ACK and its probe (odd), one at a block's end, total - 1 and the
    total"""
    nconn = T + 40
    got = check(g, clf, tm.random_case(35, nconn, seg_cap=cap, segs=lambda k: 3), cap)
    lost = (got["out_tmr"]["action"][:nconn] & tm.A_NOSPACE) != 0
    assert lost.tolist() == [2 * k + 2 > cap for k in range(nconn)]


def test_dirty_workspace_reused_by_different_sweeps(g, clf):
    ws = torch.full((g.tcp_tick_workspace(3000),), 0xFF, dtype=torch.uint8, device="cuda")
    a = tm.random_case(36, 3000, due=0.9)
    b = tm.random_case(37, 1000, due=0.2, seg_cap=50)
    check(g, clf, a, "dirty", workspace=ws, calls=2)
    check(g, clf, b, "other", workspace=ws)
    check(g, clf, a, "again", workspace=ws)


def test_counts_null_and_accumulated(g, clf):
    case = tm.random_case(38, 1500, due=0.9, seg_cap=900)
    want = tm.model(case)
    got, cnt = run_tick(g, clf, case, counts=False)
    tm.compare(got, want, 1500, 900, "no counts")
    tmr, conn, addr = dev(case["tmr"]), dev(case["conn"]), dev(case["addr"])
    cnt = torch.zeros(g.TICKC_NR, dtype=torch.int64, device="cuda")
    for _ in range(2):
        clf.tcp_tick(case["now"], tmr, conn, addr, 1500, 900, counts=cnt)
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == (2 * want["counts"]).tolist()
    assert want["counts"][tm.C_SEGS] == 900 and want["counts"][6] > 0


def test_a_million_connections(g, clf):
    nconn = tm.MAX_CONN
    small = tm.random_case(39, 4096, due=0.3)
    case = dict(small, tmr=np.tile(small["tmr"], nconn // 4096), conn=np.tile(small["conn"], nconn // 4096),
                addr=np.tile(small["addr"], nconn // 4096), seg_cap=nconn)
    # the copies differ: every 4096 connections the clock has moved on by one timeout's worth of cases
    case["tmr"]["next_timeout"] += (np.arange(nconn, dtype=np.uint64) >> np.uint64(12)) % np.uint64(3)
    got = check(g, clf, case, "2^20", model=False)          # the model walks every connection in Python: too slow
    want = tm.model(small)
    k = int(want["totals"][0])
    assert 500 < k < 4096 and int(got["totals"][0]) > 100 * k
    for f, _ in tm.SEG[:1] + tm.SEG[2:]:
        assert (got[f][:k] == want[f][:k]).all(), f
    assert (got["out_tmr"][:4096] == want["out_tmr"]).all()


# ---------------------------------------------------------------- the ACKs of a gcl_tcp_rx call
def rx_outputs(g, rx):
    got, _ = rc.run_host(g, rx)
    m = len(rx["pkt_len"]) if rx.get("order") is None else len(rx["order"])
    return {f: got[f][:m].copy() for f, _ in rc.ENTRY}


def run_rxack(g, clf, rx, rxout, addr, seg_cap, frame_base=0, frame_stride=64, counts=True, blocks=0, calls=1,
              workspace=None):
    blank = tm.blank(0, seg_cap, tick=False)
    out = {f: dev(a) for f, a in blank.items()}
    m, n, nconn = len(rxout["verdict"]), len(rx["sock"]), len(rx["conn"])

    def some(a, dt=torch.int32):
        return dev(a) if len(a) else torch.zeros(1, dtype=dt, device="cuda")

    args = (some(rxout["verdict"], torch.uint8), some(rxout["sflags"], torch.uint8), some(rxout["rcv_nxt_after"]), m,
            some(rx["sock"]), n, rec(rx["conn"], 48), rec(addr, 16), nconn, seg_cap)
    order = dev(rx["order"]) if rx.get("order") is not None else None
    cnt = None
    for _ in range(calls):
        cnt = torch.full((g.TICKC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
        clf.tcp_rx_acks(*args, order=order, frame_stride=frame_stride, frame_base=frame_base, blocks=blocks, out=out,
                        counts=cnt, workspace=workspace)
    torch.cuda.synchronize()
    return back(out, blank), None if cnt is None else cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


def check_rxack(g, clf, rx, rxout, addr, seg_cap, what, model=True, **kw):
    hkw = {k: v for k, v in kw.items() if k in ("frame_base", "frame_stride", "blocks")}
    hgot, hcnt = tm.run_rxack_host(g, rx, rxout, addr, seg_cap, **hkw)
    got, cnt = run_rxack(g, clf, rx, rxout, addr, seg_cap, **kw)
    want = {f: hgot[f][:len(hgot[f]) - tm.GUARD] for f in hgot}
    k = int(want["totals"][1])
    want.update({f: want[f][:k] for f, _ in tm.SEG})
    tm.compare(got, want, 0, seg_cap, (what, "host"))
    assert cnt.tolist() == hcnt.tolist(), what
    if model:
        want = tm.rxack_model(rx, rxout, addr, seg_cap, kw.get("frame_base", 0), kw.get("frame_stride", 64))
        tm.compare(got, want, 0, seg_cap, (what, "model"))
        assert cnt.tolist() == want["counts"].tolist(), what
    return got


@pytest.mark.parametrize("m", [1, 63, 64, 65, T - 1, T, T + 1])
def test_rx_acks_wave_and_block_edges(g, clf, m):
    rx = rc.random_case(40 + m, m, 3, fault=0.02)
    check_rxack(g, clf, rx, rx_outputs(g, rx), tm.random_addr(41, 3), m, m, frame_base=777, frame_stride=54)


def test_rx_acks_m_zero_writes_totals(g, clf):
    rx = rc.cases()["m_zero"]
    got = check_rxack(g, clf, rx, rx_outputs(g, rx), tm.random_addr(42, 2), 4, "m == 0")
    assert got["totals"][:2].tolist() == [0, 0]


@pytest.mark.parametrize("blocks", [0, 1, 2, tm.MAX_BLOCKS])
def test_rx_acks_of_a_stream_in_a_plans_order(g, clf, blocks):
    rx = rc.random_case(43, 4000, 40)
    plan = np.argsort(rx["sock"] % 3, kind="stable")
    rx = dict(rx, order=np.concatenate([plan, np.arange(150)]).astype(np.uint32))
    rxout = rx_outputs(g, rx)
    got = check_rxack(g, clf, rx, rxout, tm.random_addr(44, 40), 4150, blocks, blocks=blocks)
    total = int(got["totals"][0])
    assert total > 400
    if blocks == 0:
        for cap in (0, 1, total - 1, total):
            check_rxack(g, clf, rx, rxout, tm.random_addr(44, 40), cap, ("cap", cap))


@pytest.mark.parametrize("every", [True, False])
def test_rx_acks_on_every_entry_and_on_none(g, clf, every):
    m, nconn = 3 * T + 7, 5
    rng = np.random.default_rng(45)
    rx = dict(sock=rng.integers(0, nconn, size=m).astype(np.uint32), conn=rc.random_case(46, 8, nconn)["conn"])
    ln = rng.integers(1, 1460, size=m).astype(np.uint16)
    nxt, after = rx["conn"]["rcv_nxt"].astype(np.uint64), np.zeros(m, dtype=np.uint32)
    for j in range(m):
        c = int(rx["sock"][j])
        nxt[c] = (nxt[c] + np.uint64(ln[j])) & np.uint64(tm.M32)
        after[j] = nxt[c]
    rxout = dict(verdict=np.full(m, rc.FAST, dtype=np.uint8), copy_len=ln, rcv_nxt_after=after,
                 sflags=np.full(m, 0xFF if every else 0xFF & ~rc.SF_ACK_NOW, dtype=np.uint8))
    got = check_rxack(g, clf, rx, rxout, tm.random_addr(47, nconn), m, every)
    assert got["totals"][:2].tolist() == ([m, m] if every else [0, 0])
    if every:
        assert got["seg_src"][:m].tolist() == list(range(m))


def test_rx_acks_hostile_order_and_sock(g, clf):
    """every entry asks; order and sock point outside: the guards emit nothing for those, nothing is out of bounds"""
    rx = rc.random_case(48, 500, 9)
    m, n = 700, 500
    rng = np.random.default_rng(49)
    rx = dict(rx, order=rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32), sock=rx["sock"].copy())
    rx["order"][::2] = rng.integers(0, n + 50, size=m // 2)
    rx["sock"][::3] = rng.integers(9, 1 << 32, size=len(rx["sock"][::3]), dtype=np.uint64)
    rxout = dict(verdict=np.full(m, rc.FAST, dtype=np.uint8), sflags=np.full(m, 0xFF, dtype=np.uint8),
                 rcv_nxt_after=rng.integers(0, 1 << 32, size=m, dtype=np.uint64).astype(np.uint32),
                 copy_len=np.zeros(m, dtype=np.uint16))
    got = check_rxack(g, clf, rx, rxout, tm.random_addr(50, 9), m, "hostile", model=False)
    assert 0 < int(got["totals"][0]) < m // 2
    rx["sock"][:] = 0xFFFFFFFF
    got = check_rxack(g, clf, rx, rxout, tm.random_addr(50, 9), m, "all outside", model=False)
    assert got["totals"][:2].tolist() == [0, 0]


# ---------------------------------------------------------------- the chains
def test_sweep_chain_gives_the_references_headers(g, clf):
    """sweep -> tx_hdr -> l4_csum FILL on one stream, for every named case
    that sends: bytes 34-53 of each frame as tx_hdr leaves them are the
    reference's tcp_push_tcphdr bytes, FILL changes only the two sum fields,
    and VERIFY over the result says good."""
    segs = tm.load_golden()["segs"]
    net = g.txh_net(tm.NET["addr"], tm.NET["netmask"], tm.NET["gateway"], tm.NET["mac"])
    clf.neigh_set([(0x0A000014 + k, bytes([2, 0, 0, 0, 1, k])) for k in range(3)])
    at = 0
    for name in sorted(tm.cases()):
        case = dict(tm.cases()[name], frame_base=128, frame_stride=64)
        want = tm.model(case)
        k = int(want["totals"][1])
        if k == 0:
            continue
        nconn = len(case["tmr"])
        out = clf.tcp_tick(case["now"], dev(case["tmr"]), dev(case["conn"]), dev(case["addr"]), nconn, case["seg_cap"],
                           frame_stride=64, frame_base=128)
        frames = torch.full((128 + 64 * k + 128,), tm.SENTINEL, dtype=torch.uint8, device="cuda")
        hdr = clf.tx_hdr(out["desc"], out["frame_off"], k, frames, net)
        torch.cuda.synchronize()
        before = frames.cpu().numpy().copy()
        assert out["totals"].cpu().numpy().tolist() == [int(want["totals"][0]), k]
        assert (hdr["status"].cpu().numpy()[:k] == g.TXH_OK).all() and (hdr["pkt_len"].cpu().numpy()[:k] == 54).all()
        for j in range(k):
            r = segs[at + j]
            assert (r["case"], r["k"]) == (name, j)
            assert before[128 + 64 * j + 34:128 + 64 * j + 54].tobytes().hex() == r["tcphdr"], (name, j)
        clf.l4_csum(frames, k, hdr["pkt_len"], mode=g.L4_FILL, offs=out["frame_off"], tx_olflags=hdr["tx_olflags"])
        st = clf.l4_csum(frames, k, hdr["pkt_len"], mode=g.L4_VERIFY, offs=out["frame_off"])
        torch.cuda.synchronize()
        after = frames.cpu().numpy()
        assert (st.cpu().numpy()[:k] == g.L4_GOOD).all(), name
        same = np.ones(len(after), dtype=bool)
        for j in range(k):
            o = 128 + 64 * j
            same[[o + 24, o + 25, o + 50, o + 51]] = False       # the IPv4 and the TCP sum
        assert (after[same] == before[same]).all() and (after[:128] == tm.SENTINEL).all()
        assert (after[128 + 64 * k:] == tm.SENTINEL).all(), name
        at += k
    assert at == len(segs)


def test_receive_chain_acks_carry_the_models_numbers(g, clf):
    """tcp_rx on a random stream -> tcp_rx_acks -> tx_hdr, all on the GPU: the
    frames' ack numbers and windows are those of the model's per-segment
    tcp_tx_ack calls, in list order."""
    rx = rc.random_case(51, 4096, 60)
    nconn, m = 60, 4096
    addr = tm.random_addr(52, nconn)
    addr["rip"] = 0x0A000014 + np.arange(nconn) % 3
    want_rx = rc.model(rx)
    want = tm.rxack_model(rx, want_rx, addr, m, 0, 64)
    k = int(want["totals"][0])
    assert k > 500
    got_rx, _ = run_tcp_rx(g, clf, rx)
    dv = {f: dev(got_rx[f][:m]) for f in ("verdict", "sflags", "rcv_nxt_after")}
    out = clf.tcp_rx_acks(dv["verdict"], dv["sflags"], dv["rcv_nxt_after"], m, dev(rx["sock"]), m, dev(rx["conn"]),
                          dev(addr), nconn, m)
    net = g.txh_net(tm.NET["addr"], tm.NET["netmask"], tm.NET["gateway"], tm.NET["mac"])
    frames = torch.zeros(64 * k, dtype=torch.uint8, device="cuda")
    hdr = clf.tx_hdr(out["desc"], out["frame_off"], k, frames, net)
    torch.cuda.synchronize()
    assert out["totals"].cpu().numpy().tolist() == [k, k]
    assert (hdr["status"].cpu().numpy()[:k] != g.TXH_REFUSED).all()
    fr = frames.cpu().numpy().reshape(k, 64).astype(np.uint32)
    be32 = lambda o: fr[:, o] << 24 | fr[:, o + 1] << 16 | fr[:, o + 2] << 8 | fr[:, o + 3]
    assert be32(42).tolist() == want["desc"]["ack"].tolist()
    assert (fr[:, 48] << 8 | fr[:, 49]).tolist() == want["desc"]["win"].tolist()
    assert be32(38).tolist() == want["desc"]["seq"].tolist()
    assert out["seg_src"].cpu().numpy().view(np.uint32)[:k].tolist() == want["seg_src"].tolist()


def test_error_returns(g, clf):
    case = tm.cases()["mixed"]
    nconn, cap = 7, case["seg_cap"]
    out = {f: dev(a) for f, a in tm.blank(nconn, cap).items()}
    tmr, conn, addr = dev(case["tmr"]), dev(case["conn"]), dev(case["addr"])
    ok = dict(now=case["now"], tmr=tmr, conn=conn, addr=addr, nconn=nconn, seg_cap=cap, out=out)
    clf.tcp_tick(**ok)
    torch.cuda.synchronize()

    def refused(**kw):
        with pytest.raises(OSError) as e:
            clf.tcp_tick(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    big = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    refused(frame_stride=53)
    refused(blocks=tm.MAX_BLOCKS + 1)
    for f in out:
        refused(out=dict(out, **{f: None}), workspace=big)
    for f in ("tmr", "conn", "addr"):
        refused(**{f: None})
        refused(**{f: big[8:]})
    refused(out=dict(out, out_tmr=big[8:]))
    refused(out=dict(out, desc=big[8:]))
    refused(out=dict(out, frame_off=big[4:]))
    refused(out=dict(out, totals=big[4:]))
    need = g.tcp_tick_workspace(nconn)
    refused(workspace=big[:need - 1])
    refused(workspace=big[8:])
    clf.tcp_tick(**dict(ok, workspace=big[:need]))
    clf.tcp_tick(**dict(ok, blocks=3, workspace=big[:16]))
    tin, tout = g._tick_structs(case["now"], tmr, conn, addr, nconn, cap, 0, 64, 0, out, None)

    def raw():
        return g.lib.gcl_tcp_tick(clf._ctx, ctypes.byref(tin), ctypes.byref(tout), None, big.data_ptr(), need, None)

    assert raw() == 0
    tin.size = 56
    assert raw() == -errno.EINVAL
    tin.size, tin.nconn = ctypes.sizeof(g.GclTickIn), tm.MAX_CONN + 1
    assert raw() == -errno.EINVAL
    tin.nconn, tin.seg_cap = nconn, (1 << 31) + 1
    assert raw() == -errno.EINVAL
    tin.seg_cap = cap
    assert g.lib.gcl_tcp_tick(None, ctypes.byref(tin), ctypes.byref(tout), None, big.data_ptr(), need, None) == \
        -errno.EINVAL
    assert raw() == 0
    # gcl_tcp_rx_acks
    rx = rc.cases()["two_interleaved"]
    rxout = rx_outputs(g, rx)
    aout = {f: dev(a) for f, a in tm.blank(0, 8, tick=False).items()}
    aok = dict(verdict=dev(rxout["verdict"]), sflags=dev(rxout["sflags"]), rcv_nxt_after=dev(rxout["rcv_nxt_after"]),
               m=6, sock=dev(rx["sock"]), n=6, conn=dev(rx["conn"]), addr=dev(tm.random_addr(5, 2)), nconn=2, seg_cap=8,
               out=aout)
    clf.tcp_rx_acks(**aok)

    def arefused(**kw):
        with pytest.raises(OSError) as e:
            clf.tcp_rx_acks(**dict(aok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    arefused(frame_stride=10)
    arefused(blocks=tm.MAX_BLOCKS + 1)
    for f in aout:
        arefused(out=dict(aout, **{f: None}), workspace=big)
    for f in ("verdict", "sflags", "rcv_nxt_after", "sock", "conn", "addr"):
        arefused(**{f: None})
    arefused(order=big[2:])
    arefused(sock=big[1:])
    arefused(conn=big[8:])
    arefused(workspace=big[:g.tcp_rx_acks_workspace(6) - 1])
    rin, rout = g._rxack_structs(aok["verdict"], aok["sflags"], aok["rcv_nxt_after"], aok["sock"], aok["conn"],
                                 aok["addr"], 6, 6, 2, None, 8, 0, 64, 0, aout, None)
    rin.m = (1 << 31) + 1
    assert g.lib.gcl_tcp_rx_acks(clf._ctx, ctypes.byref(rin), ctypes.byref(rout), None, big.data_ptr(), 4096,
                                 None) == -errno.EINVAL
    rin.m, rin.size = 6, 96
    assert g.lib.gcl_tcp_rx_acks(clf._ctx, ctypes.byref(rin), ctypes.byref(rout), None, big.data_ptr(), 4096,
                                 None) == -errno.EINVAL
    torch.cuda.synchronize()
