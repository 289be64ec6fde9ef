"""CPU: gcl_tcp_rx, gcl_tcp_rx_full and gcl_tcp_rx_ooo against what the
REFERENCE's own tcp_rx_conn did (tests/golden/tcprx_ref.json, recorded by
tests/golden/make_tcprx_ref.py from runtime/net/tcp_in.c compiled in place).
The Python models of tests/tcprxcases.py, tcprxfcases.py and tcprxocases.py and
the host twins gcl_tcp_rx_host, gcl_tcp_rx_full_host and gcl_tcp_rx_ooo_host
must each give, on every recorded case, what tests/tcprxrefcases.py reads off
the trace; tests/test_gpu_tcprx_ref.py holds the kernels to the same file."""
import importlib.util
import os

import numpy as np
import pytest

from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests import tcprxocases as oc
from tests import tcprxrefcases as rr
from tests.tcprxcases import M32, TCP_ACK, wraps_gt

MODS = {"rx": rc, "full": fc, "ooo": oc}


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def _generator():
    path = os.path.join(os.path.dirname(rr.PATH), "make_tcprx_ref.py")
    spec = importlib.util.spec_from_file_location("make_tcprx_ref", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_traces_are_what_the_reference_gives():
    """Where oracle/_ref is built, the generator's result in memory equals
    the committed file, text and all."""
    from oracle import orc
    if orc.ref_tcpin() is None:
        pytest.skip("oracle/_ref/libtcpin_ref.so not built (no reference tree)")
    gen = _generator()
    fresh = gen.build()
    assert fresh == rr.load()
    with open(rr.PATH) as f:
        assert f.read() == gen.dumps(fresh)


def _rows():
    """(name, connection, segment index, frame dict, trace dict) of every recorded segment"""
    for name in rr.names():
        segs, tr = rr.segments(rr.case_of(name)), rr.traces(name)
        for k, rows in tr.items():
            for s, (sg, t) in enumerate(zip(segs[k], rows)):
                yield name, k, s, sg, t


def test_fixture_holds_every_edge():
    """A regeneration cannot quietly lose a case or an edge the traces exist for."""
    assert os.path.getsize(rr.PATH) <= 192 * 1024
    d = rr.load()
    stored = [r["case"] for r in d["cases"]]
    assert stored == rr.names() and d["words"] == list(rr.WORDS)
    assert set(rr.named()) == {"rx:" + n for n in rc.cases()} | {"full:" + n for n in fc.cases()} | \
        {"ooo:" + n for n in oc.cases()}
    assert {n.split(":")[0] for n in rr.STREAMS} == {"rx", "full", "ooo"}
    for name in rr.names():         # every connection with a segment is there, with every segment
        segs = rr.segments(rr.case_of(name))
        tr = rr.traces(name)
        assert all(len(tr.get(k, [])) == len(s) for k, s in enumerate(segs)), name
    seen = set()
    for name, k, s, sg, t in _rows():
        pre = t["pre"]
        if pre["state"] != rr.TCP_STATE_ESTABLISHED or any(x["state"] != rr.TCP_STATE_ESTABLISHED for x in [t]):
            continue
        cw = rr.conn_words(rr.case_of(name), k)
        ln, seq, ack = sg["len"], sg["seq"], sg["ack"]
        mine = [x for x in t["linked"] if x[0] == s]
        others = [x for x in t["linked"] if x[0] != s]
        acceptable = rr.is_acceptable(pre, ln, seq, sg["flags"])
        if not t["slow"] and mine:
            seen.add("fast path")
        if t["slow"] and ln == 0 and t["freed"] == [s]:
            seen.add("slow pure ack")
        if t["fastrtx"]:
            assert pre["rep_acks"] + 1 >= 3 and t["rep_acks"] == 0
            seen.add("dup ack at the threshold")
        if t["slow"] and ln == 0 and t["snd_una"] == pre["snd_una"] == ack and t["snd_wnd"] != pre["snd_wnd"]:
            seen.add("window update, same ack")
        if t["slow"] and not acceptable and t["tx_ack"] and t["freed"] == [s] and not t["linked"]:
            seen.add("unacceptable, acked")
            if ln > 0 and pre["rcv_wnd"] == 0:
                seen.add("zero window refusal")
        if mine and mine[0][1] == 0 and mine[0][2] < ln:
            seen.add("tail clip")
        if any(x[1] > 0 for x in t["linked"]):
            seen.add("head clip")
        if t["slow"] and s in t["q"] and s not in pre["q"]:
            at, n = t["q"].index(s), len(t["q"])
            if n >= 2:
                seen.add("insert at head" if at == 0 else "insert at tail" if at == n - 1 else "insert in the middle")
        if t["slow"] and ln > 0 and acceptable and wraps_gt(seq, pre["rcv_nxt"]) and t["freed"] == [s] and \
                pre["ooo_len"] > 0 and sg["flags"] & TCP_ACK and not wraps_gt(ack, cw["snd_nxt"]):
            assert t["q"] == pre["q"]
            seen.add("refused duplicate")
        if len(others) >= 2:
            seen.add("drain of several")
        if any(x != s for x in t["freed"]):
            seen.add("freed in the drain")
        if t["slow"] and ln > 0 and s not in t["freed"] and pre["acks_delayed_cnt"] == 0 and t["tx_ack"] and t["q"]:
            seen.add("dup ack of :574")
        if t["pollout"]:
            seen.add("pollout")
        if t["rcv_nxt"] < pre["rcv_nxt"] and (t["rcv_nxt"] - pre["rcv_nxt"]) & M32 < 1 << 16:
            seen.add("seq wraps")
        if t["conn_ack"] and t["snd_una"] < pre["snd_una"] and (t["snd_una"] - pre["snd_una"]) & M32 < 1 << 20:
            seen.add("ack wraps")
    want = {"fast path", "slow pure ack", "dup ack at the threshold", "window update, same ack",
            "unacceptable, acked", "zero window refusal", "tail clip", "head clip", "insert at head",
            "insert in the middle", "insert at tail", "refused duplicate", "drain of several", "freed in the drain",
            "dup ack of :574", "pollout", "seq wraps", "ack wraps"}
    assert want <= seen, want - seen
    # the streams: one with reordering and loss, one with retransmits that overlap what is there
    for name, need in (("ooo:reorder_and_loss", ("q",)), ("ooo:overlapping_retransmits", ("clip", "freed"))):
        tr = rr.traces(name)
        rows = [t for rows in tr.values() for t in rows]
        if "q" in need:
            assert sum(len(t["q"]) > len(t["pre"]["q"]) for t in rows) >= 5, name
        if "clip" in need:
            assert any(x[1] > 0 for t in rows for x in t["linked"]), name
        if "freed" in need:
            assert any(t["slow"] and len(t["freed"]) > (1 if t["freed"][:1] == [s] else 0) for s, t in enumerate(rows))


@pytest.mark.parametrize("kind", rr.KINDS)
def test_models_give_what_the_reference_did(kind):
    total = 0
    for name in rr.names():
        got = MODS[kind].model(rr.case_of(name))
        total += rr.check(rr.expected(kind, name), got, got["counts"], (kind, "model", name))
    assert total >= {"rx": 150, "full": 300, "ooo": 800}[kind]


@pytest.mark.parametrize("kind", rr.KINDS)
def test_host_twins_give_what_the_reference_did(g, kind):
    total = 0
    for name in rr.names():
        got, cnt = MODS[kind].run_host(g, rr.case_of(name))
        total += rr.check(rr.expected(kind, name), got, cnt, (kind, "host", name))
    assert total >= {"rx": 150, "full": 300, "ooo": 800}[kind]


def test_the_invisible_writes_stay_few():
    """WND_INVISIBLE and REP_INVISIBLE leave most of the traces binding"""
    for kind in rr.KINDS:
        es = [rr.expected(kind, name) for name in rr.names()]
        compared = sum(e.compared for e in es)
        assert sum(e.loose for e in es) * 20 <= compared, kind
        firm = sum(int((~e.rep_loose & ((e.out["out_conn"]["flags"] & rc.REP_ACKS_RESET) != 0)).sum()) for e in es)
        # the named cases that enter with rep_acks != 0 and reset it: fast_acked_resets_rep_acks on the fast path,
        # and under the slow rules pure_ack_moves_una, pure_ack_window_only, rep_acks_2_on_entry,
        # rep_acks_255_on_entry and dup_with_nothing_in_flight
        assert firm >= (1 if kind == "rx" else 6), (kind, firm)


@pytest.mark.parametrize("kind", rr.KINDS)
def test_host_copy_chain_gives_the_reference_rxq(g, kind):
    """gcl_copy_batch_host over src_off + skip, copy_len and dst_off leaves, per
    connection, exactly the bytes of the mbufs the reference linked into
    c->rxq, in its order, up to the stop"""
    done = 0
    for name in rr.copy_cases():
        case = rr.case_of(name)
        e = rr.expected(kind, name)
        if not e.m:
            continue
        got, _ = MODS[kind].run_host(g, case)
        pay = pc.model(case, case.get("order"), case["sock"], case.get("st"))
        src = pay["src_off"].astype(np.uint64)
        if kind == "ooo":
            src = src + got["skip"][:e.m].astype(np.uint64)
        total = int(got["conn_off"][e.nconn])
        if not total:
            assert not any(x[2] for r in e.rxq for x in r), (kind, name)
            continue
        dst = np.full(total + 64, rc.SENTINEL, dtype=np.uint8)
        g.copy_batch_host(case["frames"], src, got["copy_len"][:e.m].copy(), dst[:total],
                          dst_off=got["dst_off"][:e.m].copy(), n=e.m, src_len=case["frames_len"], dst_len=total,
                          olflags=False, rss=False)
        for k in range(e.nconn):
            want = rr.rxq_bytes(e, name, k)
            o = int(got["conn_off"][k])
            assert dst[o:o + len(want)].tobytes() == want, (kind, name, k)
            done += len(want)
        assert (dst[total:] == rc.SENTINEL).all()
    assert done > 10000
