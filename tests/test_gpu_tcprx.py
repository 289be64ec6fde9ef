"""GPU: gcl_tcp_rx (include/gclassify.h) against its host twin and the model of
tests/tcprxcases.py, byte for byte over sentinel-filled outputs with guards,
on the named cases, on random streams and on the shapes where the kernels can
go wrong: the wave boundary and the chunk loop of the walk, a stop at lanes 0,
63 and 64, runs split by the grouping's ranges, one and two grouping passes,
2^20 connections, one-segment runs, a plan's order and a dirty workspace; and
the chain: the bytes every connection accepted come out of gcl_copy_batch as
the stream the model's rxq holds."""
import ctypes
import errno

import numpy as np
import pytest
import torch

from tests import l4cases as lc
from tests import paycases as pc
from tests import tcprxcases as rc

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


def run_gpu(g, clf, case, counts=True, calls=1, workspace=None):
    """@calls calls over sentinel-filled device outputs: (outputs as numpy, counts of the last call)"""
    order = case.get("order")
    n, nconn = len(case["pkt_len"]), len(case["conn"])
    m = n if order is None else len(order)
    blank = rc.blank(m, nconn)
    out = {f: dev(a) for f, a in blank.items()}
    frames, plen = dev(case["frames"]), dev(case["pkt_len"]) if n else torch.zeros(1, dtype=torch.int16, device="cuda")
    offs = dev(case["offs"]) if case["offs"] is not None and n else None
    sock = dev(case["sock"]) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    st = dev(case["st"]) if case.get("st") is not None else None
    conn = dev(case["conn"])
    cnt = None
    for _ in range(calls):
        cnt = torch.full((g.TCPRXC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
        clf.tcp_rx(frames, n, plen, sock, conn, nconn, stride=case["stride"] or 16 * (offs is None), offs=offs,
                   frames_len=case["frames_len"], order=dev(order) if order is not None else None, m=m,
                   l4_status=st, align=case.get("align", 0), blocks=case.get("blocks", 0), out=out, counts=cnt,
                   workspace=workspace)
    torch.cuda.synchronize()
    got = {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    return got, None if cnt is None else cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


def check(g, clf, case, what, model=True, **kw):
    """GPU == host twin (== model), whole arrays with their guards"""
    hgot, hcnt = rc.run_host(g, case)
    got, cnt = run_gpu(g, clf, case, **kw)
    order = case.get("order")
    m, nconn = len(case["pkt_len"]) if order is None else len(order), len(case["conn"])
    rc.compare(got, hgot, m, nconn, (what, "host"))
    assert cnt.tolist() == hcnt.tolist(), what
    if model:
        want = rc.model(case)
        rc.compare(got, want, m, nconn, (what, "model"))
        assert cnt.tolist() == want["counts"].tolist(), what
    return got


@pytest.mark.parametrize("name", sorted(rc.cases()))
def test_named_cases(g, clf, name):
    check(g, clf, rc.cases()[name], name)


@pytest.mark.parametrize("seed,m,nconn,align", [(1, 4096, 300, 0), (2, 3000, 37, 64), (3, 4096, 1, 0),
                                                  (4, 2000, 300, 256)])
def test_random_streams(g, clf, seed, m, nconn, align):
    check(g, clf, rc.random_case(seed, m, nconn, align=align), seed)


def one_conn(nseg, stop=None, seed=7):
    """one connection, @nseg in-order segments, a FIN on segment @stop"""
    case = rc.random_case(seed, nseg, 1, fault=0, pays=100)
    case["conn"]["rcv_wnd"], case["conn"]["flags"] = 1 << 24, rc.ELIGIBLE
    case["conn"]["snd_wnd"], case["conn"]["snd_wscale"] = 1 << 30, 0
    for o in case["offs"]:                      # a full window in every segment: the send side never fills
        case["frames"][int(o) + 48:int(o) + 50] = 0xFF
    if stop is not None:
        case["frames"][int(case["offs"][stop]) + 47] |= rc.TCP_FIN
    return case


@pytest.mark.parametrize("nseg", [63, 64, 65, 129])
def test_wave_boundary_and_chunk_loop(g, clf, nseg):
    got = check(g, clf, one_conn(nseg), nseg)
    assert got["out_conn"]["nfast"][0] == nseg


@pytest.mark.parametrize("stop", [0, 63, 64])
def test_stop_at_lane(g, clf, stop):
    got = check(g, clf, one_conn(200, stop), stop)
    assert got["out_conn"]["first_slow"][0] == stop and got["out_conn"]["nfast"][0] == stop


@pytest.mark.parametrize("blocks", [1, 2, 7, rc.MAX_BLOCKS])
def test_runs_split_by_ranges(g, clf, blocks):
    case = dict(rc.random_case(11, 3000, 5), blocks=blocks)
    check(g, clf, case, blocks)


@pytest.mark.parametrize("nconn", [1, rc.PASS_CONN, rc.PASS_CONN + 1])
def test_one_and_two_grouping_passes(g, clf, nconn):
    # cookies at both ends of the range, so that the last connection has a run
    case = rc.random_case(12, 1500, nconn, flow=lambda k: (0, nconn - 1, nconn // 2, (k * 7) % nconn)[k % 4])
    got = check(g, clf, case, nconn)
    assert got["out_conn"]["nfast"][nconn - 1] + got["out_conn"]["nslow"][nconn - 1] > 0


def test_a_million_connections_three_live(g, clf):
    nconn, live = rc.MAX_CONN, (0, 123456, rc.MAX_CONN - 1)
    small = rc.random_case(13, 600, 3, fault=0.01)
    case = dict(small, conn=np.zeros(nconn, dtype=rc.CONN), sock=small["sock"].copy())
    for k, c in enumerate(live):
        case["conn"][c] = small["conn"][k]
        case["sock"][small["sock"] == k] = c
    got = check(g, clf, case, "2^20", model=False)       # the model walks every connection in Python: too slow
    want = rc.model(small)
    for f, _ in rc.ENTRY[:4]:
        assert (got[f][:600] == want[f]).all(), f
    assert (got["out_conn"][list(live)] == want["out_conn"]).all()
    assert int(got["conn_off"][nconn]) == int(want["conn_off"][3])


def test_4096_connections_of_one_segment(g, clf):
    case = rc.random_case(14, 4096, 4096, fault=0.02, flow=lambda k: (k * 2731) % 4096)
    got = check(g, clf, case, "4096 x 1")
    assert (got["out_conn"]["nfast"][:4096] + got["out_conn"]["nslow"][:4096] <= 1).all()


def test_a_plans_order(g, clf):
    case = rc.random_case(15, 3000, 40)
    rng = np.random.default_rng(16)
    plan = np.argsort(case["sock"] % 3, kind="stable")
    order = np.concatenate([plan, rng.integers(0, 3009, size=200)]).astype(np.uint32)
    check(g, clf, dict(case, order=order), "plan")
    check(g, clf, dict(case, order=order[1000:2000].copy()), "one runtime's range")


def test_dirty_workspace_reused_and_no_order_dependence(g, clf):
    case = rc.random_case(17, 4000, rc.PASS_CONN + 500, align=16)
    need = g.tcp_rx_workspace(4000, len(case["conn"]))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    a = check(g, clf, case, "dirty", workspace=ws, calls=2)
    b = check(g, clf, case, "again", workspace=ws)
    for f in a:
        assert (a[f].view(np.uint8) == b[f].view(np.uint8)).all(), f
    got, cnt = run_gpu(g, clf, case, counts=False)
    rc.compare(got, rc.model(case), 4000, len(case["conn"]), "no counts")


E2E = (4096, 1536, 7000, 48)  # packets, slot bytes, the first registered port, connections


def test_end_to_end_in_order_streams(g):
    """classify -> sock_lookup -> l4_csum VERIFY -> plan -> l4_payload ->
    tcp_rx -> copy_batch for one runtime with 48 TCP sockets: connection c's
    region of the receive buffer is the byte stream the model's rxq holds."""
    n, slot, PORT, nconn = E2E
    R, T = 16, 4
    small = rc.random_case(18, n, nconn, fault=0.03)
    frs = []
    for i in range(n):
        o = int(small["offs"][i])
        f = small["frames"][o:o + int(small["pkt_len"][i])].copy()
        ck = int(small["sock"][i])
        port = PORT + ck if ck < nconn else PORT + nconn + 5      # an unregistered port: MISS
        f[0:12] = (2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2)
        f[30:34] = list(g.runtime_ip(3).to_bytes(4, "big"))
        f[36:38] = (port >> 8, port & 0xFF)
        frs.append(f)
    case = lc.filled(lc.slots(frs, slot))
    rng = np.random.default_rng(19)
    lc.spoil(case, rng, np.nonzero(small["st"] == lc.BAD)[0], where="last")
    st_want = lc.model(case, lc.VERIFY)[0]
    tcp = np.array([f[23] == lc.TCP for f in frs])
    sock_want = np.where(small["sock"] < nconn, small["sock"], pc.S_MISS).astype(np.uint32)
    sock_want[~tcp] = pc.S_MISS                                  # only TCP sockets are registered
    case.update(sock=sock_want, st=st_want, conn=small["conn"], align=64)
    want = rc.model(case, with_rxq=True)
    assert (want["verdict"] == rc.FAST).sum() > n // 4 and len(set(want["verdict"].tolist())) >= 4
    pay = pc.model(case, None, sock_want, st_want)

    clf = g.Classifier(0, R, g.HASH_JENKINS)
    clf.runtime_set(3, g.runtime_ip(3), T, T, g.steer_flows(T, list(range(T))))
    clf.sock_set(3, [(g.runtime_ip(3), PORT + c, lc.TCP, g.SOCK_MATCH_3TUPLE, c) for c in range(nconn)])
    fr, plen = dev(case["frames"]), dev(case["pkt_len"])
    v = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    clf.classify(fr, n, slot, verdicts=v)
    sock = clf.sock_lookup(fr, n, slot, verdicts=v)
    status = clf.l4_csum(fr, n, plen, mode=g.L4_VERIFY, stride=slot, len_hint=1500)
    order, boff = clf.plan(v, n)
    boff_h = boff.cpu().numpy().view(np.uint32)
    lo, hi = int(boff_h[3]), int(boff_h[4])
    assert (lo, hi) == (0, n)                                    # every packet is runtime 3's
    mine = order[lo:hi]
    pout = clf.l4_payload(fr, n, plen, stride=slot, order=mine, m=n, sock=sock, l4_status=status)
    blank = rc.blank(n, nconn)
    out = {f: dev(a) for f, a in blank.items()}
    conn = dev(case["conn"])
    both = []
    for _ in range(2):
        clf.tcp_rx(fr, n, plen, sock, conn, nconn, stride=slot, order=mine, m=n, l4_status=status, align=64,
                   out=out)
        total = int(want["conn_off"][nconn])
        rx = torch.full((total + 4096,), rc.SENTINEL, dtype=torch.uint8, device="cuda")
        clf.copy_batch(fr, pout["src_off"], out["copy_len"], n, rx[:total], dst_off=out["dst_off"], olflags=False,
                       rss=False)
        torch.cuda.synchronize()
        both.append(rx.cpu().numpy())
    assert (order.cpu().numpy().view(np.uint32)[:n] == np.arange(n)).all()
    assert (pout["len"].cpu().numpy().view(np.uint16)[:n] == pay["len"]).all()
    rc.compare({f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}, want, n, nconn, "e2e")
    off = want["conn_off"]
    for c in range(nconn):
        assert both[0][int(off[c]):int(off[c]) + len(want["rxq"][c])].tobytes() == want["rxq"][c], f"connection {c}"
    assert sum(len(s) for s in want["rxq"]) == int(want["counts"][rc.C_BYTES]) > 100000
    assert (both[0] == both[1]).all() and (both[0][total:] == rc.SENTINEL).all()
    clf.close()


def test_error_returns(g, clf):
    case = rc.cases()["two_interleaved"]
    m, nconn = 6, 2
    out = {f: dev(a) for f, a in rc.blank(m, nconn).items()}
    fr, plen, sock, conn, offs = (dev(case[k]) for k in ("frames", "pkt_len", "sock", "conn", "offs"))
    ok = dict(frames=fr, n=m, pkt_len=plen, sock=sock, conn=conn, nconn=nconn, offs=offs, out=out)
    clf.tcp_rx(**ok)
    torch.cuda.synchronize()

    def refused(**kw):
        with pytest.raises(OSError) as e:
            clf.tcp_rx(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(align=3)
    refused(m=5)
    refused(blocks=rc.MAX_BLOCKS + 1)
    for f in out:
        refused(out=dict(out, **{f: None}) if f != "conn_off" else dict(out, conn_off=None),
                workspace=torch.zeros(1 << 20, dtype=torch.uint8, device="cuda"))
    odd = torch.zeros(8 * m + 64, dtype=torch.uint8, device="cuda")
    refused(out=dict(out, dst_off=odd[4:]))
    refused(out=dict(out, out_conn=odd[8:]))
    refused(conn=odd[8:8 + 48 * nconn + 8])
    need = g.tcp_rx_workspace(m, nconn)
    big = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    refused(workspace=big[:need - 1])
    refused(workspace=big[8:])
    clf.tcp_rx(**dict(ok, workspace=big[:need]))
    rin = g.GclTcprxIn(size=ctypes.sizeof(g.GclTcprxIn), m=m, sock=sock.data_ptr(), conn=conn.data_ptr(),
                       nconn=rc.MAX_CONN + 1)
    rout = g.GclTcprxOut(**{f: out[f].data_ptr() for f in g.TCPRX_OUT_FIELDS})
    b = g.GclBatch(frames=fr.data_ptr(), frames_len=case["frames_len"], n=m, pkt_len=plen.data_ptr(),
                   offs=offs.data_ptr())
    def raw():
        return g.lib.gcl_tcp_rx(clf._ctx, ctypes.byref(b), ctypes.byref(rin), ctypes.byref(rout), None,
                                big.data_ptr(), need, None)

    assert raw() == -errno.EINVAL                 # nconn past the cap
    rin.nconn = nconn
    assert raw() == 0
    rin.size = 48                                 # a wrong in->size
    assert raw() == -errno.EINVAL
    rin.size = ctypes.sizeof(g.GclTcprxIn)
    order = torch.arange(m, dtype=torch.int32, device="cuda")
    rin.order, rin.m = order.data_ptr(), (1 << 31) + 1     # only the limit can refuse this
    assert raw() == -errno.EINVAL
    rin.m = m
    assert raw() == 0
    rin.order = odd.data_ptr() + 2                # order and sock that are not 4-B aligned
    assert raw() == -errno.EINVAL
    rin.order, rin.sock = order.data_ptr(), odd.data_ptr() + 1
    assert raw() == -errno.EINVAL
    rin.sock = None
    assert raw() == -errno.EINVAL
    torch.cuda.synchronize()
