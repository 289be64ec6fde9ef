"""gcl_tcp_write_host (the host twin of gcl_tcp_write) against the independent
model of tests/tcpwritecases.py: hand-derived cases, seeded random batches, each
cap one short, garbage vector offsets and the refusals.  CPU only."""
import ctypes

import numpy as np
import pytest

from caladan_amd import gclassify as G
from tests import tcpwritecases as T

HAND = T.hand_cases()


def run_and_check(b, seg_cap=None, item_cap=None, frame_base=0, frame_stride=2048, frames_len=0):
    es, ei = b.enough()
    seg_cap, item_cap = es if seg_cap is None else seg_cap, ei if item_cap is None else item_cap
    counts = np.zeros(G.WRC_NR, dtype=np.uint64)
    out = b.run_host(seg_cap, item_cap, frame_base, frame_stride, frames_len, counts)
    exp = b.expect(seg_cap, item_cap, frame_base, frame_stride, frames_len)
    T.check(b, out, exp, counts)
    return out, exp


def by_hand(out_conn, desc, want, segs):
    for c, (status, ret, snd_nxt, nseg, nitems, pend_len, flags) in want.items():
        o = out_conn[c]
        assert (o["status"], o["ret"], o["snd_nxt"], o["nseg"], o["nitems"], o["pend_len"], o["flags"]) == \
            (status, ret, snd_nxt, nseg, nitems, pend_len, flags), (c, o)
    if segs is not None:
        got = [(int(d["tcp_flags"]), int(d["seq"]), int(d["paylen"])) for d in desc[:len(segs)]]
        assert got == [(f, s & T.M32, n) for _, f, s, n in segs]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(case):
    _, conns, want, segs, voff = case
    b = T.Batch(conns, voff=voff)
    out, exp = run_and_check(b)
    for src in (out, exp):       # the twin and the model, each against the hand's numbers
        by_hand(src["out_conn"], src["desc"], want, segs)
        if segs is not None:
            assert int(src["totals"][1]) == len(segs)
            assert src["seg_conn"][:len(segs)].tolist() == [s[0] for s in segs]


def test_hand_items_and_frames_by_hand():
    """three vectors into one segment behind a held tail: pending 10 bytes in the frame at 777, vectors 30,
    30, 30 at mss 100: items land at 777 + 54 + 10, + 40, + 70 and one descriptor of 100 bytes from seq 990
    goes out in the pending frame; no slot is taken.  A second connection's segment takes slot 0."""
    vec = [(5000, 30), (6000, 30), (7000, 30)]
    b = T.Batch([T.conn(mss=100, pend_len=10, pend_frame_off=777, vecs=vec), T.conn(mss=100, len=7, src_off=9000)])
    out, _ = run_and_check(b, frame_base=1 << 20, frame_stride=256)
    assert out["totals"].tolist() == [2, 2, 4, 4, 1, 97]
    items = list(zip(out["src_off"][:4].tolist(), out["len"][:4].tolist(), out["dst_off"][:4].tolist(),
                     out["item_conn"][:4].tolist(), out["item_seg"][:4].tolist()))
    assert items == [(5000, 30, 777 + 54 + 10, 0, 0), (6000, 30, 777 + 54 + 40, 0, 0), (7000, 30, 777 + 54 + 70, 0, 0),
                     (9000, 7, (1 << 20) + 54, 1, 1)]
    assert out["frame_off"][:2].tolist() == [777, 1 << 20]
    d = out["desc"][0]
    assert (d["seq"], d["paylen"], d["tcp_flags"], d["ack"], d["win"]) == (990, 100, T.ACK | T.PSH, 7000, 4096)
    e, q = out["txq_ent"][0], out["txq_cold"][0]
    assert (e["seg_seq"], e["seg_end"], e["ts"]) == (990, 1090, T.NOW)
    assert (q["frame_off"], q["tcp_flags"], q["tcp_off"], q["flags"]) == (777, T.ACK | T.PSH, 5, G.TXQE_INFLIGHT)


def test_held_items_are_marked_and_the_tail_keeps_its_slot():
    """120 bytes then an empty last vector at mss 100: segment 0 sent from slot 0, 20 bytes held in slot 1"""
    b = T.Batch([T.conn(mss=100, vecs=[(0, 120), (500, 0)])])
    out, _ = run_and_check(b, frame_base=4096, frame_stride=512)
    o = out["out_conn"][0]
    assert (o["pend_len"], o["pend_frame_off"], o["nseg"], o["nitems"]) == (20, 4096 + 512, 1, 2)
    assert out["item_seg"][:2].tolist() == [0, G.WR_SEG_HELD] and out["dst_off"][1] == 4096 + 512 + 54
    assert out["totals"].tolist() == [1, 1, 2, 2, 2, 120]


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_random(seed):
    run_and_check(T.random_batch(seed, 64), frame_base=1 << 33, frame_stride=1536)


def test_under_20_rule_is_not_hold_every_short_tail():
    """the model and the twin send a 19-byte tail where a rule that holds every short tail would keep it"""
    b = T.Batch([T.conn(mss=100, vecs=[(0, 119), (0, 0)]), T.conn(mss=19, vecs=[(0, 19), (0, 0)]),
                 T.conn(mss=20, vecs=[(0, 20), (0, 0)])])
    out, _ = run_and_check(b)
    assert out["out_conn"]["pend_len"].tolist() == [0, 0, 20]
    assert out["out_conn"]["nseg"].tolist() == [2, 1, 0]


@pytest.mark.parametrize("which", ["segs", "items", "frames"])
def test_each_cap_one_short(which):
    b = T.random_batch(11, 48)
    es, ei = b.enough()
    full = b.expect(es, ei)
    slots = int(full["totals"][4])
    assert es > 8 and ei > 8 and slots > 8
    kw = dict(segs=dict(seg_cap=es - 1), items=dict(item_cap=ei - 1),
              frames=dict(frame_base=4096, frames_len=4096 + slots * 2048 - 1))[which]
    out, _ = run_and_check(b, **kw)
    st = out["out_conn"]["status"]
    ns = np.flatnonzero(st == G.WRS_NOSPACE)
    assert len(ns) >= 1
    went = np.flatnonzero(full["out_conn"]["status"] == G.WRS_DONE)
    assert (st[went[went >= ns[0]]] == G.WRS_NOSPACE).all()     # a suffix of those that went ahead
    c = ns[0]
    o, w = out["out_conn"][c], b.wr[c]
    assert (o["ret"], o["snd_nxt"], o["nseg"], o["nitems"], o["flags"]) == (-105, b.conn[c]["snd_nxt"], 0, 0, 0)
    assert (o["pend_len"], o["pend_frame_off"]) == (w["pend_len"], w["pend_frame_off"])
    for caps in ((0, ei), (es, 0), (es // 2, ei // 2)):
        run_and_check(b, *caps)
    run_and_check(b, frame_base=4096, frames_len=100)            # below frame_base: no room at all


def test_garbage_voff_and_too_many_vectors():
    b = T.garbage_voff_batch()
    out, _ = run_and_check(b)
    assert out["out_conn"]["status"].tolist() == [G.WRS_DONE, G.WRS_REFUSED, G.WRS_DONE] + [G.WRS_REFUSED] * 4
    b = T.too_many_vectors()
    out, _ = run_and_check(b)
    assert out["out_conn"]["status"].tolist() == [G.WRS_REFUSED, G.WRS_DONE]
    assert out["out_conn"]["nitems"][1] == G.WR_MAX_IOV and out["out_conn"]["ret"][1] == G.WR_MAX_IOV
    nv = T.Batch([T.conn(mss=100, vecs=[(0, 5)])], use_voff=False)   # GCL_WR_VEC without voff
    out, _ = run_and_check(nv)
    assert out["out_conn"]["status"][0] == G.WRS_REFUSED


def test_counts_accumulate_and_empty():
    b = T.random_batch(5, 50)
    es, ei = b.enough()
    counts = np.zeros(G.WRC_NR, dtype=np.uint64)
    b.run_host(es, ei, counts=counts)
    b.run_host(es, ei, counts=counts)
    assert np.array_equal(counts, 2 * b.expect(es, ei)["counts"])
    out = T.Batch([]).run_host(4, 4)
    assert not out["totals"].any()


def test_refusals():
    b = T.random_batch(3, 8)
    es, ei = b.enough()
    out = b.run_host(es, ei)

    def call(**kw):
        win, wout = G._wr_structs(T.NOW, b.voff, b.iov, b.nvec, b.wr, b.conn, b.addr, b.nconn, es, ei, 0, 2048, 0, 0,
                                  out, None)
        for k, v in kw.items():
            setattr(wout if hasattr(wout, k) else win, k, v)
        return G.lib.gcl_tcp_write_host(ctypes.byref(win), ctypes.byref(wout), None)

    assert call() == 0
    for kw in (dict(size=8), dict(nconn=(1 << 20) + 1), dict(nvec=(1 << 31) + 1), dict(seg_cap=(1 << 31) + 1),
               dict(item_cap=(1 << 31) + 1), dict(blocks=1025), dict(frame_stride=53), dict(frame_stride=(1 << 20) + 1),
               dict(totals=None), dict(wr=None), dict(conn=None), dict(addr=None), dict(out_conn=None), dict(iov=None),
               dict(desc=None), dict(txq_cold=None), dict(src_off=None), dict(item_seg=None),
               dict(voff=b.voff.ctypes.data + 2), dict(wr=b.wr.ctypes.data + 8), dict(iov=b.iov.ctypes.data + 8),
               dict(len=out["len"].ctypes.data + 1), dict(txq_ent=out["txq_ent"].ctypes.data + 8)):
        assert call(**kw) == -22, kw
    # voff NULL: nvec and iov are not looked at
    assert call(voff=None, iov=None, nvec=1 << 40) == 0
    assert G.lib.gcl_tcp_write_workspace(1, 1, 0, None) == -22
    for args in (((1 << 20) + 1, 0, 0), (1, (1 << 31) + 1, 0), (1, 0, 1025)):
        with pytest.raises(OSError):
            G.tcp_write_workspace(*args)
