"""GPU: gcl_tcp_txq (include/gclassify.h) against its host twin and the model of
tests/txqcases.py, byte for byte over sentinel-filled outputs with guards, on
the named cases, on random batches and on the shapes where the kernels can go
wrong: the wave and block edges, queues around the length from which the whole
wave walks one, a queue that crosses the cooperative stride, long queues among
short ones in one wave, forced range counts so that the scan of the block sums
has work, seg_cap cutting inside a connection and at a connection's end, a
dirty workspace; and chained: head_ts and EMPTY into gcl_tcp_tick, and the
segments of a gcl_tx_seg call retransmitted in place."""
import numpy as np
import pytest
import torch

from tests import tcptmrcases as tm
from tests import txqcases as tq
from tests.test_gpu_tcprx import dev

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


def run_gpu(g, clf, case, counts=True, calls=1, workspace=None):
    """@calls calls over sentinel-filled device outputs with a guard on either side:
    (tq.blank() as the calls left it, as numpy; counts of the last call)"""
    nconn, nent = len(case["conn"]), len(case["ent"])
    blank = tq.blank(nconn, nent, case["seg_cap"])
    whole = {f: dev(a) for f, a in blank.items()}
    out = tq.inner(whole)
    qoff, ent, cold = dev(case["qoff"]), rec(case["ent"], 16), rec(case["cold"], 16)
    conn, addr = rec(case["conn"], 48), rec(case["addr"], 16)
    want = dev(case["want"]) if case.get("want") is not None else None
    cnt = None
    for _ in range(calls):
        cnt = torch.full((g.TXQC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
        clf.tcp_txq(case["now"], qoff, ent, cold, nent, conn, addr, nconn, case["seg_cap"], want=want,
                    frame_stride=case["frame_stride"], frame_base=case["frame_base"], blocks=case.get("blocks", 0),
                    out=out, counts=cnt, workspace=workspace)
    torch.cuda.synchronize()
    return back(whole, blank), None if cnt is None else cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


def check(g, clf, case, what, model=True, **kw):
    """GPU == host twin (== model), whole arrays with their guards; returns the arrays as the call took them"""
    hgot, hcnt = tq.run_host(g, case)
    got, cnt = run_gpu(g, clf, case, **kw)
    want = {f: hgot[f][tq.GUARD:len(hgot[f]) - tq.GUARD] for f in hgot}
    k = int(want["totals"][1])
    want.update({f: want[f][:k] for f, _ in tq.SEG})
    tq.compare(got, want, case, (what, "host"))
    assert cnt.tolist() == hcnt.tolist(), what
    if model:
        want = tq.model(case)
        tq.compare(got, want, case, (what, "model"))
        assert cnt.tolist() == want["counts"].tolist(), what
    return tq.inner(got)


@pytest.mark.parametrize("name", sorted(tq.cases()))
def test_named_cases(g, clf, name):
    check(g, clf, tq.cases()[name], name)


@pytest.mark.parametrize("cap", [None, 40, 0])
def test_all_named_cases_as_one_batch(g, clf, cap):
    check(g, clf, tq.all_named(seg_cap=cap), cap)


T, L = tq.TILE, tq.LONG


@pytest.mark.parametrize("nconn", [1, 63, 64, 65, T + 1])
def test_wave_and_block_edges(g, clf, nconn):
    check(g, clf, tq.random_case(20 + nconn, nconn, due=0.8), nconn)


def long_case(seed, lens, **kw):
    """queues of the given lengths, mostly due, a few hostile entries"""
    kw.setdefault("due", 0.9)
    kw.setdefault("hostile", 0.02)
    return tq.random_case(seed, len(lens), qlen=lambda k, r: lens[k], **kw)


@pytest.mark.parametrize("n", [L - 1, L, L + 1, 64 * 3 + 1])
@pytest.mark.parametrize("want", [tq.W_RTO, tq.W_RTO | tq.W_FAST, tq.W_FAST, 0, tq.W_EXCL])
def test_a_queue_around_the_threshold_and_across_the_stride(g, clf, n, want):
    """alone, and with every kind of head: all acknowledged but the last few, none, a young tail"""
    check(g, clf, long_case(40 + n, [n], want=lambda k, r: want), (n, want))
    h = np.zeros(n, dtype=tq.ENT)
    for acked, young in ((0, n), (n - 3, n), (n, n), (64, 70), (1, 64), (63, 65), (n - 1, n - 1)):
        acked, young = min(acked, n), min(young, n)
        h["seg_seq"] = 100000 + 10 * (np.arange(n) - acked)
        h["seg_end"] = h["seg_seq"] + 10
        h["ts"] = tq.DUE
        h["ts"][young:] = tq.NOW - 5
        case = tq.build([tq.conn([tq.ent(int(e["seg_seq"]), int(e["seg_end"]), ts=int(e["ts"])) for e in h],
                                 una=100000, want=want)])
        check(g, clf, case, (n, want, acked, young))


def test_seventeen_refused_then_sixteen_in_a_long_queue(g, clf):
    q = tq.run_of(70, off=3) + tq.run_of(20, seq=8000) + tq.run_of(60, seq=10000)
    got = check(g, clf, tq.build([tq.conn(q, want=tq.W_RTO | tq.W_FAST)]), "refused")
    assert got["out_conn"]["nretx"][0] == 16 and got["state"][:150].tolist() == [5] * 70 + [2] * 16 + [0] * 64


@pytest.mark.parametrize("n", [20, 70])
@pytest.mark.parametrize("cap", [15, 16])
def test_room_ends_where_the_batch_ends(g, clf, n, cap):
    """the 16th wanted entry with room for 15: the room is asked first, NOSPACE and no BATCH; with room for 16, BATCH"""
    got = check(g, clf, tq.build([tq.conn(tq.run_of(n))], seg_cap=cap), (n, cap))
    assert got["out_conn"]["flags"][0] == (tq.O_NOSPACE if cap == 15 else tq.O_BATCH)
    assert got["state"][:17].tolist() == [tq.RETX] * 15 + [tq.NOSPACE if cap == 15 else tq.RETX, tq.KEPT]


def test_long_queues_between_short_ones_in_one_wave(g, clf):
    check(g, clf, long_case(50, [2, 3, 200, 1, 0, 5]), "one")
    check(g, clf, long_case(51, [2, 150, 3, 0, 64, 5, 70, 1], seg_cap=30), "three, capped")
    lens = [1] * 64
    lens[0], lens[63] = 90, 130
    check(g, clf, long_case(52, lens), "first and last lane")
    check(g, clf, long_case(53, [L] * 5 + [L - 1] * 5, want=lambda k, r: tq.W_RTO | tq.W_FAST), "all long")


@pytest.mark.parametrize("blocks", [1, 2, 7])
def test_forced_ranges(g, clf, blocks):
    """block sums that cross connections: one range walks all tiles, an odd count leaves ragged ranges"""
    check(g, clf, tq.random_case(31, 5 * T + 9, due=0.8, blocks=blocks), blocks)
    check(g, clf, tq.random_case(32, 3 * T + 1, due=1.0, hostile=0.0, blocks=blocks, seg_cap=700), (blocks, "cap"))


@pytest.mark.parametrize("cap", [0, 1, 4, 5, 6, 9, 10, 14, 15])
def test_seg_cap_inside_a_connection_and_at_its_end(g, clf, cap):
    """three connections of five segments each: the cap at every kind of cut"""
    conns = [tq.conn(tq.run_of(5) + [tq.ent(1500, 1600, ts=tq.NOW)], want=tq.W_RTO | (tq.W_FAST if k == 1 else 0))
             for k in range(3)]
    got = check(g, clf, tq.build(conns, seg_cap=cap), cap)
    assert got["out_conn"]["nretx"][:3].tolist() == [max(0, min(5, cap - 5 * k)) for k in range(3)]
    assert ((got["out_conn"]["flags"][:3] & tq.O_NOSPACE) != 0).tolist() == [cap < 5 * k + 5 for k in range(3)]


def test_a_random_batch_of_a_few_thousand(g, clf):
    case = tq.random_case(60, 3000, due=0.5, bad_qoff=0.01)
    got = check(g, clf, case, "random")
    assert got["totals"][1] > 500
    check(g, clf, tq.random_case(61, 3000, due=0.9, seg_cap=5000, qlen=lambda k, r: r.choice([0, 1, 2, 4, 70])),
          "random, capped")


def test_dirty_workspace_reused_on_one_stream(g, clf):
    """two calls that reuse one workspace agree with two fresh ones"""
    ws = torch.full((g.tcp_txq_workspace(3000),), 0xFF, dtype=torch.uint8, device="cuda")
    a = tq.random_case(62, 3000, due=0.9)
    b = tq.random_case(63, 1000, due=0.4, seg_cap=50)
    check(g, clf, a, "dirty", workspace=ws, calls=2)
    check(g, clf, b, "other", workspace=ws)
    check(g, clf, a, "again", workspace=ws)


def test_counts_null_and_accumulated(g, clf):
    case = tq.random_case(64, 1500, due=0.9, seg_cap=300)
    want = tq.model(case)
    got, _ = run_gpu(g, clf, case, counts=False)
    tq.compare(got, want, case, "no counts")
    got, cnt = run_gpu(g, clf, case, calls=1)
    assert cnt.tolist() == want["counts"].tolist() and want["counts"][tq.C_NOSPACE] > 0


def test_no_connections(g, clf):
    out = {"totals": torch.full((3,), 7, dtype=torch.int64, device="cuda")}
    z = torch.zeros((1, 48), dtype=torch.uint8, device="cuda")
    got = clf.tcp_txq(tq.NOW, torch.zeros(1, dtype=torch.int32, device="cuda"), z, z, 0, z, z, 0, 4, out=out)
    torch.cuda.synchronize()
    assert got["totals"].tolist() == [0, 0, 0]


def test_chained_into_the_timer_sweep(g, clf):
    """head_ts and EMPTY become txq_ts and GCL_TMR_TXQ of the next gcl_tcp_tick:
    its next_timeout is the one tcp_timer_update gives for the queue as
    tcp_retransmit and tcp_write_finish left it"""
    case = tq.random_case(70, 500, due=0.6, hostile=0.0)
    nconn, nent = len(case["conn"]), len(case["ent"])
    got, _ = run_gpu(g, clf, case)
    oc = tq.inner(got)["out_conn"][:nconn]
    tmr = np.zeros(nconn, dtype=tm.TMR)
    tmr["next_timeout"] = 0
    tmr["state"] = tm.ESTABLISHED
    tmr["flags"] = tm.LIVE | np.where(oc["flags"] & tq.O_EMPTY, 0, tm.TXQ).astype(np.uint8) | \
        np.where(case["want"] & tq.W_EXCL, tm.TX_EXCLUSIVE, 0).astype(np.uint8)
    tmr["txq_ts"] = oc["head_ts"]
    later = tq.NOW + 1000
    out = clf.tcp_tick(later, dev(tmr), dev(case["conn"]), dev(case["addr"]), nconn, 4)
    torch.cuda.synchronize()
    nt = out["out_tmr"].cpu().numpy().reshape(-1).view(tm.TMR_OUT)["next_timeout"]
    want = tq.model(case)
    for k in range(nconn):
        # the model's queue after the call: its head's timestamp, read off the mbufs
        woc = want["out_conn"][k]
        c = dict(state=tm.ESTABLISHED, ack_delayed=False, zero_wnd=False, rxq_ooo=False,
                 tx_exclusive=bool(case["want"][k] & tq.W_EXCL),
                 txq=None if woc["flags"] & tq.O_EMPTY else int(woc["head_ts"]))
        tm.tcp_timer_update(c, later)
        assert int(nt[k]) == c["next_timeout"], k


def test_segments_of_tx_seg_retransmitted_in_place(g, clf):
    """the descriptors of a gcl_tx_seg call, as queue entries with snd_una
    unmoved, come back with the original headers' fields up to the fresher ack
    and win"""
    m, mss, stride = 40, 1000, 2048
    rng = np.random.default_rng(5)
    send = np.zeros(m, dtype=g.SEG_SEND_DTYPE)
    send["lip"], send["rip"] = 0x0A000005, 0x0A000100 + np.arange(m)
    send["lport"], send["rport"] = 8000 + np.arange(m), 40000 + 7 * np.arange(m)
    send["proto"], send["mss"] = 6, mss
    send["snd_nxt"] = rng.integers(0, 1 << 32, m)
    send["ack"], send["win"] = 77, 99
    send["len"] = rng.integers(0, 4 * mss, m)
    send["winlen"] = 1 << 20
    seg = g.tx_seg_host(send, 5 * m, stride=stride)
    n = int(seg["total_segs"][0])
    first, nseg = seg["seg_first"], seg["nseg"]
    h, q = np.zeros(n, dtype=tq.ENT), np.zeros(n, dtype=tq.COLD)
    d = seg["desc"][:n]
    h["seg_seq"], h["seg_end"], h["ts"] = d["seq"], d["seq"] + d["paylen"], tq.DUE
    q["frame_off"], q["tcp_flags"], q["tcp_off"] = seg["frame_off"][:n], d["tcp_flags"], d["tcp_off"]
    qoff = np.zeros(m + 1, dtype=np.uint32)
    qoff[1:] = np.cumsum(nseg)
    assert qoff[:-1].tolist() == first.tolist()
    p, a = np.zeros(m, dtype=tq.CONN), np.zeros(m, dtype=tq.ADDR)
    p["snd_una"], p["rcv_nxt"], p["rcv_wnd"] = send["snd_nxt"], 123456, 0x12345
    for f in ("lip", "rip", "lport", "rport"):
        a[f] = send[f]
    a["rcv_wscale"] = 2
    case = dict(now=tq.NOW, qoff=qoff, ent=h, cold=q, conn=p, addr=a, want=np.full(m, tq.W_RTO, np.uint8),
                seg_cap=n, frame_base=0, frame_stride=stride)
    got = check(g, clf, case, "tx_seg")
    assert got["totals"][:3].tolist() == [n, n, 0] and got["seg_ent"][:n].tolist() == list(range(n))
    back_d = got["desc"][:n]
    for f in ("lip", "rip", "lport", "rport", "proto", "tcp_flags", "tcp_off", "ecn", "seq", "paylen", "pad"):
        assert (back_d[f] == d[f]).all(), f
    assert (back_d["ack"] == 123456).all() and (back_d["win"] == (0x12345 >> 2)).all()
    assert (got["frame_off"][:n] == seg["frame_off"][:n]).all() and (got["len"][:n] == 0).all()
    assert (got["state"][:n] == tq.RETX).all()
