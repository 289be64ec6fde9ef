"""gcl_tcp_shut_host (the host twin of gcl_tcp_shut) against the independent model
of tests/shutcases.py: the whole enumeration of op x state x flags x how, the
three cases called out by name, random batches of 5 000 connections, each cap
one short, no connections, accumulated counts and every refusal."""
import ctypes

import numpy as np
import pytest

from caladan_amd import gclassify as G
from tests import shutcases as T

GUARD = 4


def run_and_check(b, seg_cap=None, exp=None, **kw):
    seg_cap = b.nconn if seg_cap is None else seg_cap
    counts = np.zeros(G.SHUTC_NR, dtype=np.uint64)
    got = b.run_host(seg_cap, counts=counts, guard=GUARD, **kw)
    exp = exp if exp is not None else b.expect(seg_cap, **kw)
    T.check(b, got, exp, counts, seg_cap=seg_cap, guard=GUARD)
    return np.frombuffer(T.raw(got["out_conn"], 48 * b.nconn), dtype=G.SHUT_CONN_OUT_DTYPE), got, exp


@pytest.fixture(scope="module")
def enum():
    b = T.enumeration()
    return b, b.expect(b.nconn, frame_base=1 << 33, frame_stride=1536)


def test_enumeration(enum):
    b, exp = enum
    assert T.ENUM_LIVE == 4000 and b.nconn == 2 * 4000 + 5 * len(T.BAD_STATES) * 2 * 5
    # the whole product is there as written: LIVE, in its own state, with its own flags and how
    live = slice(0, T.ENUM_LIVE)
    assert (b.tmr["flags"][live] & G.TMR_LIVE).all()
    assert not (b.tmr["flags"][T.ENUM_LIVE:2 * T.ENUM_LIVE] & G.TMR_LIVE).any()
    seen = set(zip(b.shut["op"][live].tolist(), b.tmr["state"][live].tolist(),
                   (b.tmr["flags"][live] & G.TMR_TX_EXCLUSIVE).tolist(), b.shut["flags"][live].tolist(),
                   b.shut["how"][live].tolist()))
    assert len(seen) == 4000 and set(b.tmr["state"][live].tolist()) == set(range(10))
    assert set(b.tmr["state"][2 * T.ENUM_LIVE:].tolist()) == set(T.BAD_STATES)
    oc, _, _ = run_and_check(b, exp=exp, frame_base=1 << 33, frame_stride=1536)
    assert (oc["status"][T.ENUM_LIVE:2 * T.ENUM_LIVE] == G.SHUTS_NONE).all()
    bad = oc["status"][2 * T.ENUM_LIVE:]
    assert set(bad.tolist()) == {G.SHUTS_NONE, G.SHUTS_REFUSED} and \
        (bad == G.SHUTS_NONE).tolist() == (b.shut["op"][2 * T.ENUM_LIVE:] == G.SHUT_OP_NONE).tolist()
    # the plainest cases, by their place in the product
    i = T.enum_index(G.SHUT_OP_SHUTDOWN, T.ESTABLISHED, how=1)
    assert (b.shut["op"][i], b.shut["how"][i], b.shut["flags"][i], b.tmr["state"][i]) == (1, 1, 0, T.ESTABLISHED)
    assert (oc[i]["status"], oc[i]["state"], oc[i]["nseg"], oc[i]["nput"]) == (G.SHUTS_DONE, T.FIN_WAIT1, 1, 0)
    assert oc[i]["snd_nxt"] == (int(b.conn["snd_nxt"][i]) + 1) & T.M32
    i = T.enum_index(G.SHUT_OP_CLOSE, T.ESTABLISHED, how=-1)
    assert (oc[i]["status"], oc[i]["state"], oc[i]["nseg"], oc[i]["nput"]) == (G.SHUTS_DONE, T.FIN_WAIT1, 1, 1)
    i = T.enum_index(G.SHUT_OP_ABORT, T.CLOSE_WAIT, x=1)
    assert (oc[i]["status"], oc[i]["state"], oc[i]["nseg"], oc[i]["err"]) == (G.SHUTS_ABORT_WAIT, T.CLOSED, 0, 103)
    assert set(oc["status"].tolist()) == set(range(G.SHUTS_NOSPACE))        # every status but the cap's
    cnt = exp["counts"]
    assert all(cnt[k] > 0 for k in (G.SHUTC_FIN, G.SHUTC_RST, G.SHUTC_FAIL, G.SHUTC_PUT, G.SHUTC_WARN))
    assert oc["nput"].max() == 2 and set(oc["state"][oc["nseg"] == 1].tolist()) >= {T.FIN_WAIT1, T.LAST_ACK, T.CLOSED}


@pytest.mark.parametrize("case", T.NAMED, ids=[c.__name__ for c in T.NAMED])
def test_named_cases(case):
    c, want = case()
    oc, got, _ = run_and_check(T.Batch([T.conn(), c, T.conn()]), 3)
    for f, v in want.items():
        assert oc[1][f] == v, (f, oc[1])
    kinds = np.ascontiguousarray(got["seg_kind"]).view(np.uint8)
    if case is T.case_warn_leaves_timer:
        assert kinds[0] == G.CTL_FIN
    else:
        d = np.frombuffer(T.raw(got["desc"], 32), dtype=G.TXH_DESC_DTYPE)[0]
        assert kinds[0] == G.CTL_RST and (d["tcp_flags"], d["seq"], d["ack"], d["win"]) == (0x04, 1000, 0, 0)
        assert int(got["totals"][0]) == 1


@pytest.mark.parametrize("seed", [1, 2])
def test_random(seed):
    oc, _, exp = run_and_check(T.random_batch(seed, 5000), frame_base=4096, frame_stride=128)
    assert exp["totals"][0] > 1000 and (oc["status"] == G.SHUTS_BLOCK).sum() > 50


def test_garbage():
    run_and_check(T.random_batch(9, 5000, garbage=True))


@pytest.mark.parametrize("how", ["seg_cap", "frames_len"])
def test_cap_one_short(how):
    b = T.random_batch(4, 700)
    full, _, exp = run_and_check(b)
    wanted = int(exp["totals"][0])
    assert wanted > 100
    kw = dict(seg_cap=wanted - 1) if how == "seg_cap" else \
        dict(seg_cap=wanted, frame_base=640, frame_stride=96, frames_len=640 + 96 * wanted - 1)
    oc, got, exp = run_and_check(b, **kw)
    assert exp["totals"].tolist() == [wanted, wanted - 1]
    last = np.flatnonzero(full["nseg"] == 1)[-1]
    assert np.flatnonzero(oc["status"] == G.SHUTS_NOSPACE).tolist() == [last]  # exactly the last one that wants
    o = oc[last]
    assert (o["ret"], o["err"], o["flags"], o["nseg"], o["nput"], o["first_seg"]) == (-105, 0, 0, 0, 0, 0)
    assert (o["snd_nxt"], o["state"], o["tmr_flags"], o["next_timeout"], o["txq_ts"]) == \
        (b.conn[last]["snd_nxt"], b.tmr[last]["state"], b.tmr[last]["flags"], b.tmr[last]["next_timeout"],
         b.tmr[last]["txq_ts"])
    others = np.arange(b.nconn) != last
    assert oc[others].tobytes() == full[others].tobytes()
    # no room at all: no segment array is needed, and every wanting connection is NOSPACE
    oc, _, _ = run_and_check(b, 0)
    assert (oc["status"] == G.SHUTS_NOSPACE).sum() == wanted
    run_and_check(b, wanted, frame_base=4096, frames_len=100)           # frames_len below frame_base


def test_counts_accumulate_and_empty():
    b = T.random_batch(5, 300)
    counts = np.zeros(G.SHUTC_NR, dtype=np.uint64)
    b.run_host(300, counts=counts)
    b.run_host(300, counts=counts)
    assert counts.tolist() == [2 * x for x in b.expect(300)["counts"]]
    out = T.Batch([]).run_host(4)
    assert out["totals"][:2].tolist() == [0, 0]


def test_refusals():
    b = T.random_batch(3, 8)
    out = b.run_host(8)

    def call(counts=None, **kw):
        sin, sout = G._shut_structs(T.NOW, b.shut, b.tmr, b.conn, b.addr, b.nconn, 8, 0, 64, 0, 0, out, None)
        for k, v in kw.items():
            tgt = sin if hasattr(sin, k) else sout if hasattr(sout, k) else sout.seg
            setattr(tgt, k, v)
        return G.lib.gcl_tcp_shut_host(ctypes.byref(sin), ctypes.byref(sout), counts)

    assert call() == 0
    cnt = np.zeros(G.SHUTC_NR + 1, dtype=np.uint64)
    assert call(counts=cnt.ctypes.data) == 0 and cnt[:G.SHUTS_NR].sum() == b.nconn and cnt[-1] == 0
    assert call(counts=cnt.ctypes.data + 4) == -22 and cnt[:G.SHUTS_NR].sum() == b.nconn     # misaligned counts
    for kw in (dict(size=8), dict(nconn=(1 << 20) + 1), dict(seg_cap=(1 << 31) + 1), dict(blocks=1025),
               dict(frame_stride=53), dict(totals=None), dict(shut=None), dict(tmr=None), dict(conn=None),
               dict(addr=None), dict(out_conn=None), dict(desc=None), dict(frame_off=None), dict(seg_conn=None),
               dict(seg_kind=None), dict(seg_src=None), dict(txq_ent=None), dict(txq_cold=None),
               dict(shut=b.shut.ctypes.data + 8), dict(tmr=b.tmr.ctypes.data + 8), dict(conn=b.conn.ctypes.data + 4),
               dict(addr=b.addr.ctypes.data + 8), dict(out_conn=out["out_conn"].ctypes.data + 8),
               dict(desc=out["desc"].ctypes.data + 8), dict(frame_off=out["frame_off"].ctypes.data + 4),
               dict(seg_conn=out["seg_conn"].ctypes.data + 2), dict(seg_src=out["seg_src"].ctypes.data + 2),
               dict(txq_ent=out["txq_ent"].ctypes.data + 8), dict(txq_cold=out["txq_cold"].ctypes.data + 8),
               dict(totals=out["totals"].ctypes.data + 4)):
        assert call(**kw) == -22, kw
    assert G.lib.gcl_tcp_shut_host(None, None, None) == -22
    # seg_cap 0 takes no per-segment array; nconn 0 takes no per-connection array
    assert call(seg_cap=0, desc=None, txq_ent=None, seg_kind=None) == 0
    assert call(nconn=0, shut=None, tmr=None, out_conn=None, desc=None) == 0
    assert G.lib.gcl_tcp_shut_workspace(1, 0, None) == -22
    for args in (((1 << 20) + 1, 0), (1, 1025)):
        with pytest.raises(OSError):
            G.tcp_shut_workspace(*args)
    assert G.tcp_shut_workspace(100, 3) == 16 + 112 and G.tcp_shut_workspace(0, 0) == 4096
