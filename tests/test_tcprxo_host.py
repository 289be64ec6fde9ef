"""CPU: gcl_tcp_rx_ooo_host (csrc/gcl_host.c with the rule of
csrc/gcl_tcprxo.h that the GPU walk shares) against the transcription of
tcp_rx_text and tcp_rx_append_text over a linked list in tests/tcprxocases.py:
the hand-derived values of the named cases, every output byte of the named
cases and of random streams (reordering, loss, retransmits that overlap) over
sentinel-filled outputs with guards, parity with gcl_tcp_rx_full_host on every
case of tests/tcprxfcases.py, the copy chain on a shuffled stream, and every
-EINVAL."""
import errno

import numpy as np
import pytest

from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests import tcprxocases as oc


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def check(g, case, what):
    want = oc.model(case)
    got, cnt = oc.run_host(g, case)
    oc.compare(got, want, case, what)
    assert cnt.tolist() == want["counts"].tolist(), what
    return want


@pytest.mark.parametrize("name", sorted(oc.cases()))
def test_model_gives_the_hand_derived_values(name):
    case, exp = oc.cases()[name]
    oc.check_expected(oc.model(case), exp, name)


@pytest.mark.parametrize("name", sorted(oc.cases()))
def test_named_cases(g, name):
    case, exp = oc.cases()[name]
    want = check(g, case, name)
    got, cnt = oc.run_host(g, case)
    oc.check_expected(dict(got, counts=cnt, qout=got["qout"][:len(want["qout"])]), exp, name)


@pytest.mark.parametrize("k", range(len(oc.STREAMS)))
def test_random_streams(g, k):
    want = check(g, oc.stream(k), f"stream {k}")
    oc.check_mix(want)


def test_counts_accumulate_and_may_be_null(g):
    case = oc.case_of("three_in_reverse")
    want = oc.model(case)
    got, _ = oc.run_host(g, case, counts=False)
    oc.compare(got, want, case, "no counts")
    a, ca = oc.run_host(g, case)
    assert ca.tolist() == want["counts"].tolist()


def test_parity_with_gcl_tcp_rx_full(g):
    """with all queues empty, every connection that gcl_tcp_rx_full's model
    does not stop on out-of-order or head-clipped text gets byte-identical
    shared outputs from both calls and an empty output queue.  A connection it
    does stop there is compared entry by entry up to that segment (@prefix): in
    stop_ooo_text and stop_head_clipped_text it is the only connection."""
    named = [(n, c) for n, (c, _) in sorted(fc.cases().items())]
    total = 0
    for name, case in named + [(f"stream {k}", fc.stream(k)) for k in range(len(fc.STREAMS))]:
        m, nconn = fc.dims(case)
        full, fcnt = fc.run_host(g, case)
        mod = fc.model(case)
        new, _ = oc.run_host(g, case)
        order = case.get("order")
        idx = np.arange(m) if order is None else order.astype(np.int64)
        pay = pc.model(case, order, case["sock"], case.get("st"))
        # the connections gcl_tcp_rx_full's model stops on text off rcv_nxt: its first_slow entry has len > 0,
        # none of FIN / RST / URG / SYN, and the connection is eligible
        skip, prefix = set(), set()
        for ck in range(nconn):
            fs = int(mod["out_conn"]["first_slow"][ck])
            if fs == rc.NONE or not (int(case["conn"][ck]["flags"]) & rc.ELIGIBLE):
                continue
            i = int(idx[fs])
            o = int(case["offs"][i]) if case["offs"] is not None else i * case["stride"]
            if int(pay["len"][fs]) > 0 and not (int(case["frames"][o + 47]) & 0x27):
                skip.add(ck)
        whole = [ck for ck in range(nconn) if ck not in skip]
        for ck in whole:
            assert full["out_conn"][ck].tobytes() == new["out_conn"][ck].tobytes(), (name, ck)
            assert full["out_ext"][ck].tobytes() == new["out_ext"][ck].tobytes(), (name, ck)
            assert int(full["conn_off"][ck + 1]) - int(full["conn_off"][ck]) == \
                int(new["conn_off"][ck + 1]) - int(new["conn_off"][ck]), (name, ck)
            assert int(new["qout_off"][ck + 1]) == int(new["qout_off"][ck]), (name, ck)
        for j in range(m):
            i = int(idx[j])
            ck = int(case["sock"][i]) if i < len(case["sock"]) else rc.NONE
            if int(full["verdict"][j]) <= rc.DROP and ck in skip:
                if j >= int(mod["out_conn"]["first_slow"][ck]):
                    continue
                prefix.add(ck)
            for f in ("verdict", "sflags", "rcv_nxt_after", "copy_len"):
                assert int(full[f][j]) == int(new[f][j]), (name, f, j)
            if int(full["copy_len"][j]):
                assert int(full["dst_off"][j]) - int(full["conn_off"][ck]) == \
                    int(new["dst_off"][j]) - int(new["conn_off"][ck]), (name, j)
            assert int(new["oflags"][j]) == 0 and int(new["skip"][j]) == 0, (name, j)
        if not skip:                                  # nothing moved: the layouts are the same bytes too
            for f in ("dst_off", "conn_off"):
                assert full[f].tobytes() == new[f].tobytes(), (name, f)
        assert len(whole) + len(prefix) >= 1, name
        total += len(whole) + len(prefix)
        if not skip:
            assert int(new["totals"][0]) == 0, name
    print("connections compared:", total)
    assert total > 600


def test_chain_copy_of_a_shuffled_stream(g):
    """gcl_copy_batch_host with src_off + skip reproduces each connection's byte stream"""
    rng = np.random.default_rng(5)
    cs = [rc.conn1(snd_wl1=50000, rcv_nxt=100), rc.conn1(snd_wl1=50000, rcv_nxt=0xFFFFF000)]
    segs, streams = [], []
    for ck, c in enumerate(cs):
        at, mine = c["rcv_nxt"], []
        for _ in range(40):
            ln = int(rng.integers(1, 1461))
            mine.append(rc.seg(rng, ck, at, ln))
            at += ln
        streams.append(b"".join(f[54:].tobytes() if hasattr(f, "tobytes") else bytes(f[54:]) for _, f in mine))
        again = rc.seg(rng, ck, c["rcv_nxt"] + 700, 900)      # a retransmit across boundaries: refused or clipped
        again[1][54:954] = np.frombuffer(streams[ck][700:1600], dtype=np.uint8)
        mine.append(again)
        segs += mine
    perm = rng.permutation(len(segs))
    case = rc.build(cs, [segs[int(p)] for p in perm], align=64)
    want = check(g, case, "shuffled")
    got, _ = oc.run_host(g, case)
    m = len(perm)
    pay = pc.model(case, None, case["sock"], None)
    total = int(got["conn_off"][2])
    dst = np.full(total, rc.SENTINEL, dtype=np.uint8)
    g.copy_batch_host(case["frames"], pay["src_off"].astype(np.uint64) + got["skip"][:m].astype(np.uint64),
                      got["copy_len"][:m].copy(), dst, dst_off=got["dst_off"][:m].copy())
    assert int(got["totals"][0]) == 0
    for ck in range(2):
        o = int(got["conn_off"][ck])
        nbytes = (int(got["out_conn"]["rcv_nxt"][ck]) - cs[ck]["rcv_nxt"]) & rc.M32
        assert nbytes == len(streams[ck])
        assert dst[o:o + nbytes].tobytes() == streams[ck], ck


def test_error_returns(g):
    case = oc.case_of("unsorted_input_queue")
    out = oc.blank(case)
    ok = dict(frames=case["frames"], pkt_len=case["pkt_len"], sock=case["sock"], conn=case["conn"],
              offs=case["offs"], q_off=case["q_off"], q=case["q"], q_out_cap=oc.qcap(case), out=out)
    g.tcp_rx_ooo_host(**ok)

    def refused(**kw):
        with pytest.raises(OSError) as e:
            g.tcp_rx_ooo_host(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(align=3)
    refused(m=5)
    refused(blocks=rc.MAX_BLOCKS + 1)
    for f in out:
        refused(out=dict(out, **{f: None}))
    refused(q=None, nq=2)
    odd = np.zeros(256, dtype=np.uint8)
    refused(out=dict(out, qout=odd[8:]))
    refused(out=dict(out, skip=odd[1:]))
    refused(out=dict(out, qin_len=odd[1:]))
    refused(out=dict(out, qin_dst_off=odd[4:]))
    refused(out=dict(out, qout_off=odd[2:]))
    refused(out=dict(out, totals=odd[4:]))
    refused(q_off=odd[2:])
    g.tcp_rx_ooo_host(**dict(ok, q_out_cap=0, out=dict(out, qout=None)))      # no room asked: qout may be NULL
    assert g.tcp_rx_ooo_workspace(100, 10, 0, 7) == g.tcp_rx_full_workspace(100, 10) + 320 + 16 + 16 * 107
    with pytest.raises(OSError):
        g.tcp_rx_ooo_workspace(100, 10, 0, (1 << 31) + 1)
