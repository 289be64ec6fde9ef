"""GPU: gcl_tcp_rx_ooo (include/gclassify.h) against its host twin and the
model of tests/tcprxocases.py, byte for byte over sentinel-filled outputs with
guards, on the named cases, on the random streams and on the shapes where the
walk with the queue in the wave's lanes can go wrong: live queue lengths 0, 1,
63 and 64, a pop that empties 64 entries in one segment, an entry queued in the
first 64-record chunk and drained in the second and in the third, a stop at
lane 0 and at lane 63 with a queue, 1, 3 and the cap of ranges, an empty list,
nq = 0 with q_off NULL, a dirty workspace, counts over two calls, qout
overflow; and the chain into gcl_tcp_rx_acks and gcl_copy_batch."""
import errno

import numpy as np
import pytest
import torch

from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests import tcprxocases as oc
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
    z = oc.sizes(case)
    m, nconn, nq = z["m"], z["nconn"], z["nq"]
    n, order = len(case["pkt_len"]), case.get("order")
    blank = oc.blank(case)
    out = {f: dev(a) for f, a in blank.items()}
    frames, plen = dev(case["frames"]), dev(case["pkt_len"]) if n else torch.zeros(1, dtype=torch.int16, device="cuda")
    offs = dev(case["offs"]) if case["offs"] is not None and n else None
    sock = dev(case["sock"]) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    st = dev(case["st"]) if case.get("st") is not None else None
    rep = dev(case["rep_acks"]) if case.get("rep_acks") is not None else None
    q_off = dev(case["q_off"]) if case.get("q_off") is not None else None
    q = dev(case["q"]) if nq else None
    cnt = torch.full((g.TCPRXOC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    for _ in range(calls):
        clf.tcp_rx_ooo(frames, n, plen, sock, dev(case["conn"]), nconn, stride=case["stride"] or 16 * (offs is None),
                       offs=offs, frames_len=case["frames_len"], order=dev(order) if order is not None else None,
                       m=m, l4_status=st, align=case.get("align", 0), blocks=case.get("blocks", 0), rep_acks=rep,
                       q_off=q_off, q=q, nq=nq, q_out_cap=z["cap"], out=out, counts=cnt, workspace=workspace)
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
            memo[key] = oc.model(case)
        return memo[key]
    return of


def check(g, clf, case, what, want=None, **kw):
    """GPU == host twin == model, whole arrays with their guards"""
    hgot, hcnt = oc.run_host(g, case)
    got, cnt = run_gpu(g, clf, case, **kw)
    oc.compare(got, hgot, case, (what, "host"))
    calls = kw.get("calls", 1)
    assert cnt.tolist() == (hcnt * np.uint64(calls)).tolist(), what
    want = oc.model(case) if want is None else want
    oc.compare(got, want, case, (what, "model"))
    assert hcnt.tolist() == want["counts"].tolist(), what
    return got


@pytest.mark.parametrize("name", sorted(oc.cases()))
def test_named_cases(g, clf, wanted, name):
    case, exp = oc.cases()[name]
    want = wanted(name, case)
    got = check(g, clf, case, name, want=want)
    oc.check_expected(dict(got, counts=want["counts"], qout=got["qout"][:len(want["qout"])]), exp, name)


@pytest.mark.parametrize("k", range(len(oc.STREAMS)))
def test_random_streams(g, clf, wanted, k):
    check(g, clf, oc.stream(k), k, want=wanted(("stream", k), oc.stream(k)))


def test_parity_with_tcp_rx_full_streams_on_empty_queues(g, clf):
    """a gcl_tcp_rx_full stream through this call with q_off NULL and nq = 0"""
    case = fc.stream(1)
    got = check(g, clf, case, "rxf stream 1")
    assert int(got["totals"][0]) == 0


def one_conn(segs, q=None, **kw):
    c = rc.conn1(snd_wl1=50000, flags=oc.ESTABLISHED | rc.ELIGIBLE, **kw)
    case = rc.build([c], segs)
    if q is not None:
        case["q_off"], case["q"] = np.array([0, len(q)], dtype=np.uint32), oc.ents(q)
    return case


def piece(rng, k, ln=10, **kw):
    """the 10-byte segment number k of a connection whose rcv_nxt is 100"""
    return rc.seg(rng, 0, 100 + 10 * k, ln, **kw)


@pytest.mark.parametrize("qlen", [0, 1, 63, 64])
def test_live_queue_lengths_and_a_pop_of_all(g, clf, qlen):
    """@qlen input entries right behind a one-segment hole: an insert into the
    middle of that queue, a refused duplicate, then the hole's segment, whose
    drain pops every entry in one segment"""
    rng = np.random.default_rng(qlen)
    q = [(110 + 10 * k, 120 + 10 * k) for k in range(qlen)]
    segs = []
    if 0 < qlen < 64:
        q.pop(qlen // 2)                              # its place is filled from the list
        segs.append(piece(rng, 1 + qlen // 2))
    segs += [piece(rng, 1), piece(rng, 0)]
    got = check(g, clf, one_conn(segs, q), qlen)
    assert got["out_conn"]["rcv_nxt"][0] == 110 + 10 * max(qlen, 1) and int(got["totals"][0]) == 0
    assert got["out_conn"]["nfast"][0] == len(segs)


@pytest.mark.parametrize("run", [65, 129])
def test_queued_in_the_first_chunk_drained_in_a_later_one(g, clf, run):
    """the hole's segment comes last of @run: entries 0 (queued in chunk 0) and
    64 (chunk 1) are drained by a segment of chunk 1 or 2; pure ACKs fill the rest"""
    rng = np.random.default_rng(run)
    segs = [piece(rng, 1)] + [rc.seg(rng, 0, 100, 0) for _ in range(63)] + [piece(rng, 2)]
    segs += [rc.seg(rng, 0, 100, 0) for _ in range(run - 66)] + [piece(rng, 0)]
    got = check(g, clf, one_conn(segs), run)
    assert got["oflags"][0] == oc.QD and got["oflags"][64] == oc.QD and got["copy_len"][0] == 10
    assert got["out_conn"]["rcv_nxt"][0] == 130


@pytest.mark.parametrize("stop", [0, 63])
def test_stop_at_lane_with_a_queue(g, clf, stop):
    rng = np.random.default_rng(stop)
    segs = [piece(rng, 2 + k) for k in range(70)]
    segs[stop] = rc.seg(rng, 0, 100, 0, flags=rc.TCP_ACK | rc.TCP_FIN)
    got = check(g, clf, one_conn(segs, [(5000, 5010)]), stop)      # at lane 63 the queue is full as well
    assert got["out_conn"]["first_slow"][0] == stop and got["out_conn"]["nslow"][0] == 70 - stop
    assert int(got["totals"][0]) == 1 + stop


@pytest.mark.parametrize("blocks", [1, 3, rc.MAX_BLOCKS])
def test_runs_split_by_ranges(g, clf, wanted, blocks):
    case = oc.random_case(11, 2000, 5)
    check(g, clf, dict(case, blocks=blocks), blocks, want=wanted("ranges", case))


def test_empty_list_keeps_the_queues(g, clf):
    case = oc.case_of("garbage_q_off")
    empty = rc.build([rc.conn1(flags=oc.ESTABLISHED)] * 3, [])
    empty["q_off"], empty["q"] = case["q_off"], case["q"]
    got = check(g, clf, empty, "m = 0")
    assert got["qout_off"][:4].tolist() == [0, 2, 2, 4]


def test_dirty_workspace_reused_and_counts_accumulate(g, clf, wanted):
    case = oc.stream(0)
    z = oc.sizes(case)
    need = g.tcp_rx_ooo_workspace(z["m"], z["nconn"], 0, z["nq"])
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    want = wanted(("stream", 0), case)
    a = check(g, clf, case, "dirty, two calls", want=want, workspace=ws, calls=2)
    b = check(g, clf, case, "again", want=want, workspace=ws)
    for f in a:
        assert (a[f].view(np.uint8) == b[f].view(np.uint8)).all(), f
    got, cnt = run_gpu(g, clf, case, counts=False)
    oc.compare(got, want, case, "no counts")


def test_qout_overflow(g, clf, wanted):
    case = oc.stream(1)
    want = wanted(("stream", 1), case)
    total = int(want["totals"][0])
    assert total > 8
    for cap in (0, total // 2, total - 1):
        got = check(g, clf, dict(case, q_out_cap=cap), cap, want=want)
        assert int(got["totals"][0]) == total


def shuffled_stream():
    """one connection's 60 segments in a shuffled order (a window of 2^20 takes them all)"""
    rng = np.random.default_rng(5)
    at, segs = 100, []
    for _ in range(60):
        ln = int(rng.integers(1, 1461))
        segs.append(rc.seg(rng, 0, at, ln))
        at += ln
    rng.shuffle(segs)
    return one_conn(segs)


@pytest.mark.parametrize("name", ["hole_filled_by_next", "head_and_tail_clip_on_one", "wrap_inside_the_queue",
                                  "shuffled"])
def test_chain_acks_and_copy(g, clf, name):
    """the call's device outputs straight into gcl_tcp_rx_acks and gcl_copy_batch (src_off + skip)"""
    case = shuffled_stream() if name == "shuffled" else oc.case_of(name)
    z = oc.sizes(case)
    m, nconn = z["m"], z["nconn"]
    want = oc.model(case, with_rxq=True)
    keep = {}
    run_gpu(g, clf, case, keep=keep)
    addr = tc.random_addr(3, nconn)
    blank = tc.blank(0, m + 1, tick=False)
    aout = {f: dev(a) for f, a in blank.items()}
    clf.tcp_rx_acks(keep["verdict"], keep["sflags"], keep["rcv_nxt_after"], m, keep["sock"], len(case["sock"]),
                    dev(case["conn"]), dev(addr), nconn, m + 1, out=aout)
    pay = pc.model(case, None, case["sock"], case.get("st"))
    total = int(want["conn_off"][nconn])
    rx = torch.full((total + 64,), fc.SENTINEL, dtype=torch.uint8, device="cuda")
    src = dev(pay["src_off"].astype(np.uint64)) + keep["skip"][:m].view(torch.int16).to(torch.int64)
    clf.copy_batch(keep["frames"], src, keep["copy_len"], m, rx[:total], dst_off=keep["dst_off"], olflags=False,
                   rss=False)
    torch.cuda.synchronize()
    acks = {f: aout[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    # the ACK model moves each window by copy_len in list order; here a segment's drain accepts bytes that
    # copy_len books on the entries it drained, so the model is given what each segment accepted in all
    moved, at = np.zeros(m, dtype=np.uint32), [int(c["rcv_nxt"]) for c in case["conn"]]
    for j in np.nonzero(want["verdict"] == rc.FAST)[0]:
        ck = int(case["sock"][j])
        moved[j] = (int(want["rcv_nxt_after"][j]) - at[ck]) & rc.M32
        at[ck] = int(want["rcv_nxt_after"][j])
    ref = tc.rxack_model(case, dict({f: want[f] for f in ("verdict", "sflags", "rcv_nxt_after")}, copy_len=moved),
                         addr, m + 1, 0, 64)
    tc.compare(acks, ref, nconn, m + 1, name)
    assert int(acks["totals"][1]) == int(want["counts"][oc.C_ACKS])
    rxh = rx.cpu().numpy()
    for c in range(nconn):
        o = int(want["conn_off"][c])
        assert rxh[o:o + len(want["rxq"][c])].tobytes() == want["rxq"][c], (name, c)
    assert (rxh[total:] == fc.SENTINEL).all()
    if name == "shuffled":
        assert int(want["out_conn"]["rcv_nxt"][0]) - 100 == total and int(want["totals"][0]) == 0


def test_error_returns(g, clf):
    case = oc.case_of("unsorted_input_queue")
    z = oc.sizes(case)
    m, nconn, nq = z["m"], z["nconn"], z["nq"]
    out = {f: dev(a) for f, a in oc.blank(case).items()}
    fr, plen, sock, conn, offs = (dev(case[k]) for k in ("frames", "pkt_len", "sock", "conn", "offs"))
    ok = dict(frames=fr, n=m, pkt_len=plen, sock=sock, conn=conn, nconn=nconn, offs=offs, out=out,
              q_off=dev(case["q_off"]), q=dev(case["q"]), nq=nq, q_out_cap=z["cap"])
    clf.tcp_rx_ooo(**ok)
    torch.cuda.synchronize()
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def refused(**kw):
        with pytest.raises(OSError) as e:
            clf.tcp_rx_ooo(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(align=3)
    refused(blocks=rc.MAX_BLOCKS + 1)
    for f in out:
        refused(out=dict(out, **{f: None}), workspace=big)
    refused(q=None)
    odd = torch.zeros(16 * 8 + 64, dtype=torch.uint8, device="cuda")
    refused(out=dict(out, qout=odd[8:]))
    refused(out=dict(out, qin_dst_off=odd[4:]))
    refused(q=odd[8:])
    need = g.tcp_rx_ooo_workspace(m, nconn, 0, nq)
    assert need == g.tcp_rx_full_workspace(m, nconn) + 32 * nconn + 16 + 16 * (nq + m)
    refused(workspace=big[:need - 1])
    refused(workspace=big[8:])
    clf.tcp_rx_ooo(**dict(ok, workspace=big[:need]))
    torch.cuda.synchronize()
