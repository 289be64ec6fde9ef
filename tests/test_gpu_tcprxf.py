"""GPU: gcl_tcp_rx_full (include/gclassify.h) against its host twin and the
model of tests/tcprxfcases.py, byte for byte over sentinel-filled outputs with
guards, on the named cases (their frames start at every alignment), on the
random streams and on the shapes where the walk can go wrong: runs of 1, 63,
64, 65 and 129 segments, a stop at lane 0, lane 63 and lane 0 of the second
chunk, one and two grouping passes, 1, 3 and the cap of ranges, an empty list,
an order with repeats and strays, a dirty workspace, counts over two calls;
and the chain into gcl_tcp_rx_acks and gcl_copy_batch."""
import errno

import numpy as np
import pytest
import torch

from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests import tcptmrcases as tc

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


def run_gpu(g, clf, case, counts=True, calls=1, workspace=None, keep=None):
    """@calls calls over sentinel-filled device outputs: (outputs as numpy, counts summed over the calls)"""
    m, nconn = fc.dims(case)
    n, order = len(case["pkt_len"]), case.get("order")
    blank = fc.blank(m, nconn)
    out = {f: dev(a) for f, a in blank.items()}
    frames, plen = dev(case["frames"]), dev(case["pkt_len"]) if n else torch.zeros(1, dtype=torch.int16, device="cuda")
    offs = dev(case["offs"]) if case["offs"] is not None and n else None
    sock = dev(case["sock"]) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    st = dev(case["st"]) if case.get("st") is not None else None
    rep = dev(case["rep_acks"]) if case.get("rep_acks") is not None else None
    cnt = torch.full((g.TCPRXFC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    for _ in range(calls):
        clf.tcp_rx_full(frames, n, plen, sock, dev(case["conn"]), nconn, stride=case["stride"] or 16 * (offs is None),
                        offs=offs, frames_len=case["frames_len"], order=dev(order) if order is not None else None,
                        m=m, l4_status=st, align=case.get("align", 0), blocks=case.get("blocks", 0), rep_acks=rep,
                        out=out, counts=cnt, workspace=workspace)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(out, frames=frames, sock=sock)
    got = {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    return got, None if cnt is None else cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


@pytest.fixture(scope="module")
def wanted():
    """the model's outputs, computed once per case"""
    memo = {}

    def of(key, case):
        if key not in memo:
            memo[key] = fc.model(case)
        return memo[key]
    return of


def check(g, clf, case, what, want=None, **kw):
    """GPU == host twin == model, whole arrays with their guards"""
    m, nconn = fc.dims(case)
    hgot, hcnt = fc.run_host(g, case)
    got, cnt = run_gpu(g, clf, case, **kw)
    fc.compare(got, hgot, m, nconn, (what, "host"))
    calls = kw.get("calls", 1)
    assert cnt.tolist() == (hcnt * np.uint64(calls)).tolist(), what
    want = fc.model(case) if want is None else want
    fc.compare(got, want, m, nconn, (what, "model"))
    assert hcnt.tolist() == want["counts"].tolist(), what
    return got


@pytest.mark.parametrize("name", sorted(fc.cases()))
def test_named_cases(g, clf, wanted, name):
    case, exp = fc.cases()[name]
    got = check(g, clf, case, name, want=wanted(name, case))
    fc.check_expected(dict(got, counts=wanted(name, case)["counts"]), exp, name)


@pytest.mark.parametrize("k", range(len(fc.STREAMS)))
def test_random_streams(g, clf, wanted, k):
    check(g, clf, fc.stream(k), k, want=wanted(("stream", k), fc.stream(k)))


def one_conn(nseg, stop=None, seed=7):
    """one connection, @nseg segments of text and pure ACKs, none of which stops it; a FIN on segment @stop"""
    case = fc.random_case(seed, nseg, 1, stops=0, noise=0)
    case["conn"]["rcv_wnd"], case["conn"]["flags"] = 1 << 24, rc.ELIGIBLE
    if stop is not None:
        case["frames"][int(case["offs"][stop]) + 47] |= rc.TCP_FIN
    return case


@pytest.mark.parametrize("nseg", [1, 63, 64, 65, 129])
def test_wave_boundary_and_chunk_loop(g, clf, nseg):
    got = check(g, clf, one_conn(nseg), nseg)
    assert got["out_conn"]["nfast"][0] == nseg and got["out_ext"]["nrule2"][0] > (nseg > 1)


@pytest.mark.parametrize("stop", [0, 63, 64])
def test_stop_at_lane(g, clf, stop):
    got = check(g, clf, one_conn(200, stop), stop)
    assert got["out_conn"]["first_slow"][0] == stop and got["out_conn"]["nfast"][0] == stop
    assert got["out_conn"]["nslow"][0] == 200 - stop


@pytest.mark.parametrize("blocks", [1, 3, rc.MAX_BLOCKS])
def test_runs_split_by_ranges(g, clf, wanted, blocks):
    case = fc.random_case(11, 3000, 5, stops=0.001)
    check(g, clf, dict(case, blocks=blocks), blocks, want=wanted("ranges", case))


@pytest.mark.parametrize("nconn", [1, rc.PASS_CONN, rc.PASS_CONN + 1])
def test_one_and_two_grouping_passes(g, clf, nconn):
    # cookies at both ends of the range, so that the last connection has a run
    case = fc.random_case(12, 1500, nconn, flow=lambda k: (0, nconn - 1, nconn // 2, (k * 7) % nconn)[k % 4])
    got = check(g, clf, case, nconn)
    assert got["out_conn"]["nfast"][nconn - 1] + got["out_conn"]["nslow"][nconn - 1] > 0


def test_a_plans_order(g, clf):
    case = fc.random_case(15, 3000, 40)
    rng = np.random.default_rng(16)
    plan = np.argsort(case["sock"] % 3, kind="stable")
    order = np.concatenate([plan, rng.integers(0, 3009, size=200)]).astype(np.uint32)
    check(g, clf, dict(case, order=order), "plan")


def test_dirty_workspace_reused_and_counts_accumulate(g, clf, wanted):
    case = fc.stream(0)
    m, nconn = fc.dims(case)
    need = g.tcp_rx_full_workspace(m, nconn)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    want = wanted(("stream", 0), case)
    a = check(g, clf, case, "dirty, two calls", want=want, workspace=ws, calls=2)
    b = check(g, clf, case, "again", want=want, workspace=ws)
    for f in a:
        assert (a[f].view(np.uint8) == b[f].view(np.uint8)).all(), f
    got, cnt = run_gpu(g, clf, case, counts=False)
    fc.compare(got, want, m, nconn, "no counts")


def test_rep_acks_null_is_zeros(g, clf):
    case = fc.case_of("dupacks_1_2_3_4")
    check(g, clf, dict(case, rep_acks=None), "NULL", want=fc.model(dict(case, rep_acks=np.zeros(1, dtype=np.uint8))))


CHAIN = ("tail_clip_then_window_0", "two_interleaved", "wrap", "duplicate_order", "fast_ack_fast")


@pytest.mark.parametrize("name", CHAIN)
def test_chain_acks_and_copy(g, clf, wanted, name):
    """the call's device outputs straight into gcl_tcp_rx_acks and gcl_copy_batch"""
    case = fc.case_of(name)
    m, nconn = fc.dims(case)
    want = fc.model(case, with_rxq=True)
    keep = {}
    run_gpu(g, clf, case, keep=keep)
    order = case.get("order")
    addr = tc.random_addr(3, nconn)
    blank = tc.blank(0, m + 1, tick=False)
    aout = {f: dev(a) for f, a in blank.items()}
    clf.tcp_rx_acks(keep["verdict"], keep["sflags"], keep["rcv_nxt_after"], m, keep["sock"], len(case["sock"]),
                    dev(case["conn"]), dev(addr), nconn, m + 1, order=dev(order) if order is not None else None,
                    out=aout)
    pay = pc.model(case, order, case["sock"], case.get("st"))
    total = int(want["conn_off"][nconn])
    rx = torch.full((total + 64,), fc.SENTINEL, dtype=torch.uint8, device="cuda")
    clf.copy_batch(keep["frames"], dev(pay["src_off"].astype(np.uint64)), keep["copy_len"], m, rx[:total],
                   dst_off=keep["dst_off"], olflags=False, rss=False)
    torch.cuda.synchronize()
    acks = {f: aout[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    ref = tc.rxack_model(case, {f: want[f] for f in ("verdict", "sflags", "rcv_nxt_after", "copy_len")}, addr, m + 1,
                         0, 64)
    tc.compare(acks, ref, nconn, m + 1, name)
    assert int(acks["totals"][1]) == int(want["counts"][fc.C_ACKS])
    rxh = rx.cpu().numpy()
    for c in range(nconn):
        o = int(want["conn_off"][c])
        assert rxh[o:o + len(want["rxq"][c])].tobytes() == want["rxq"][c], (name, c)
    assert (rxh[total:] == fc.SENTINEL).all()


def test_error_returns(g, clf):
    case = fc.case_of("two_interleaved")
    m, nconn = 6, 2
    out = {f: dev(a) for f, a in fc.blank(m, nconn).items()}
    fr, plen, sock, conn, offs = (dev(case[k]) for k in ("frames", "pkt_len", "sock", "conn", "offs"))
    ok = dict(frames=fr, n=m, pkt_len=plen, sock=sock, conn=conn, nconn=nconn, offs=offs, out=out)
    clf.tcp_rx_full(**ok)
    torch.cuda.synchronize()
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def refused(**kw):
        with pytest.raises(OSError) as e:
            clf.tcp_rx_full(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(align=3)
    refused(m=5)
    refused(blocks=rc.MAX_BLOCKS + 1)
    for f in out:
        refused(out=dict(out, **{f: None}), workspace=big)
    odd = torch.zeros(8 * m + 64, dtype=torch.uint8, device="cuda")
    refused(out=dict(out, out_ext=odd[8:]))
    refused(out=dict(out, out_conn=odd[8:]))
    need = g.tcp_rx_full_workspace(m, nconn)
    assert need == g.tcp_rx_workspace(m, nconn) + 16 * nconn
    refused(workspace=big[:need - 1])             # gcl_tcp_rx's size is not enough
    refused(workspace=big[8:])
    clf.tcp_rx_full(**dict(ok, workspace=big[:need]))
    torch.cuda.synchronize()
