"""gcl_tcp_read_host (the host twin of gcl_tcp_read) against the independent
model of tests/tcpreadcases.py: hand-derived cases, seeded random batches, the
caps one short, garbage CSR offsets and the refusals.  CPU only."""
import ctypes

import numpy as np
import pytest

from caladan_amd import gclassify as G
from tests import tcpreadcases as T

HAND = T.hand_cases()


def run_and_check(b, item_cap=None, seg_cap=None, frame_base=0, frame_stride=64):
    item_cap = b.item_cap_enough() if item_cap is None else item_cap
    seg_cap = b.nconn if seg_cap is None else seg_cap
    counts = np.zeros(G.RDC_NR, dtype=np.uint64)
    out = b.run_host(item_cap, seg_cap, frame_base, frame_stride, counts)
    exp = b.expect(item_cap, seg_cap, frame_base, frame_stride)
    T.check(b, out, exp, counts)
    return out, exp


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(case):
    _, queues, reads, use_voff, want = case
    b = T.Batch(queues, reads, use_voff)
    out, exp = run_and_check(b)
    for c, (status, ret, npop, pull, flags) in enumerate(want):
        for src in (out["out_conn"], exp["out_conn"]):   # the twin and the model, each against the hand's numbers
            o = src[c]
            assert (o["status"], o["ret"], o["npop"], o["pull"], o["flags"]) == (status, ret, npop, pull, flags), (c, o)


def test_hand_items_by_hand():
    """iov_coincide spelled out: entries 10, 0, 10, 5 into vectors 10, 0, 10, 0, 3, ret 23"""
    _, queues, reads, use_voff, _ = next(c for c in HAND if c[0] == "iov_coincide")
    b = T.Batch(queues, reads, use_voff)
    out = b.run_host(16, 1)
    e, v = b.ent["off"], b.iov["off"]
    # cuts 10e 10e 10v 10v 20e 20v 20v | 23: the entry cuts first at every tie
    want = [(e[0], 10, v[0], 0), (e[1], 0, v[0] + 10, 1), (e[2], 0, v[0] + 10, 2), (e[2], 0, v[1], 2), (e[2], 10, v[2], 2),
            (e[3], 0, v[2] + 10, 3), (e[3], 0, v[3], 3), (e[3], 3, v[4], 3)]
    assert int(out["totals"][0]) == len(want) == 4 + 5 - 1
    got = list(zip(out["src_off"][:8], out["len"][:8], out["dst_off"][:8], out["item_ent"][:8]))
    assert [tuple(int(x) for x in g) for g in got] == [tuple(int(x) for x in w) for w in want]


@pytest.mark.parametrize("use_voff", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random(seed, use_voff):
    run_and_check(T.random_batch(seed, 200, use_voff), frame_base=1 << 33, frame_stride=128)


@pytest.mark.parametrize("use_voff", [False, True])
def test_one_owner(use_voff):
    run_and_check(T.random_batch(7, 3, use_voff, one_owner=600))


@pytest.mark.parametrize("use_voff", [False, True])
def test_caps_one_short(use_voff):
    b = T.random_batch(11, 120, use_voff)
    full = b.expect(b.item_cap_enough(), b.nconn)
    items, segs = int(full["totals"][0]), int(full["seg_totals"][0])
    assert items > 4 and segs > 2
    out, exp = run_and_check(b, item_cap=items - 1, seg_cap=segs - 1)
    assert int(out["totals"][1]) == items - 1 and int(out["seg_totals"][1]) == segs - 1
    assert np.count_nonzero(out["out_conn"]["flags"] & G.RDO_ITEM_NOSPACE) == 1
    assert np.count_nonzero(out["out_conn"]["flags"] & G.RDO_SEG_NOSPACE) == 1
    # the other words of the connection whose ACK found no room change all the same
    c = int(np.flatnonzero(out["out_conn"]["flags"] & G.RDO_SEG_NOSPACE)[0])
    assert out["out_conn"][c]["rcv_wnd"] == full["out_conn"][c]["rcv_wnd"]
    for cap_i, cap_s in ((0, 0), (1, 1), (items // 2, segs // 2)):
        run_and_check(b, item_cap=cap_i, seg_cap=cap_s)


@pytest.mark.parametrize("use_voff", [False, True])
def test_bad_ranges(use_voff):
    b = T.bad_range_batch(use_voff)
    out, _ = run_and_check(b)
    bad = [1, 3, 4]
    assert list(np.flatnonzero(out["out_conn"]["status"] == G.RDS_BADRANGE)) == bad
    for c in bad:
        o = out["out_conn"][c]
        assert (o["ret"], o["npop"], o["nitems"], o["flags"], o["rcv_wnd"]) == (0, 0, 0, 0, 5000)
    assert (out["out_conn"]["status"][[0, 2]] == G.RDS_DONE).all()


def test_counts_accumulate_and_empty():
    b = T.random_batch(5, 50, True)
    counts = np.zeros(G.RDC_NR, dtype=np.uint64)
    b.run_host(b.item_cap_enough(), b.nconn, counts=counts)
    b.run_host(b.item_cap_enough(), b.nconn, counts=counts)
    assert np.array_equal(counts, 2 * b.expect(b.item_cap_enough(), b.nconn)["counts"])
    e = T.Batch([], [], True)
    out = e.run_host(4, 4)
    assert not out["totals"].any() and not out["seg_totals"].any()


def test_refusals():
    b = T.random_batch(3, 8, True)
    out = b.run_host(b.item_cap_enough(), b.nconn)

    def call(**kw):
        rin, rout = G._rd_structs(b.qoff, b.ent, b.nent, b.voff, b.iov, b.nvec, b.rd, b.conn, b.addr, b.nconn,
                                  b.item_cap_enough(), b.nconn, 0, 64, 0, out, None)
        for k, v in kw.items():
            if hasattr(rout, k):
                setattr(rout, k, v)
            elif hasattr(rout.seg, k) and k != "totals":
                setattr(rout.seg, k, v)
            else:
                setattr(rin, k, v)
        return G.lib.gcl_tcp_read_host(ctypes.byref(rin), ctypes.byref(rout), None)

    assert call() == 0
    for kw in (dict(size=8), dict(nconn=(1 << 20) + 1), dict(nent=(1 << 31) + 1), dict(nvec=(1 << 31) + 1),
               dict(item_cap=(1 << 31) + 1), dict(seg_cap=(1 << 31) + 1), dict(blocks=1025), dict(frame_stride=53),
               dict(totals=None), dict(qoff=None), dict(rd=None), dict(conn=None), dict(addr=None), dict(out_conn=None),
               dict(ent=None), dict(iov=None), dict(src_off=None), dict(item_ent=None), dict(desc=None),
               dict(seg_src=None), dict(qoff=b.qoff.ctypes.data + 2), dict(ent=b.ent.ctypes.data + 8),
               dict(rd=b.rd.ctypes.data + 8), dict(len=out["len"].ctypes.data + 1)):
        assert call(**kw) == -22, kw
    # voff NULL: nvec and iov are not looked at
    assert call(voff=None, iov=None, nvec=1 << 40) == 0
