"""CPU: gcl_tcp_txq_host (csrc/gcl_host.c with the rule of csrc/gcl_txq.h that
the GPU kernels share) against the line-by-line transcription of tcp_conn_ack,
tcp_tx_retransmit, tcp_tx_retransmit_one and tcp_tx_fast_retransmit_start in
tests/txqcases.py: every output byte of the named cases and of random batches,
sentinel-filled outputs with guards, the counters, the struct layouts and every
-EINVAL."""
import ctypes
import errno

import numpy as np
import pytest

from tests import txqcases as tq


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def check(g, case, what):
    want = tq.model(case)
    got, cnt = tq.run_host(g, case)
    tq.compare(got, want, case, what)
    assert cnt.tolist() == want["counts"].tolist(), what
    return want


@pytest.mark.parametrize("name", sorted(tq.cases()))
def test_named_cases(g, name):
    check(g, tq.cases()[name], name)


def test_named_cases_say_what_their_names_say():
    """the model's own answers for the named cases: the cases test what they claim"""
    w = {k: tq.model(c) for k, c in tq.cases().items()}
    st = {k: v["state"].tolist() for k, v in w.items()}
    oc = {k: v["out_conn"] for k, v in w.items()}
    K, A, R, RC, NS, RF, T = tq.KEPT, tq.ACKED, tq.RETX, tq.RETX_COPY, tq.NOSPACE, tq.REFUSED, tq.TRIMMED
    NOW, young = tq.NOW, tq.NOW - tq.TCP_RETRANSMIT_TIMEOUT + 1
    assert st["end_eq_una"] == [A, R, R] and st["end_eq_una_plus_1"] == [R | T, R]
    assert st["end_eq_una_wrap"] == [A, R, R] and st["end_eq_una_plus_1_wrap"] == [R | T, R]
    assert w["end_eq_una_plus_1"]["desc"]["paylen"].tolist() == [1, 99]
    assert st["una_behind_the_wrap"] == [A, R | T] and w["una_behind_the_wrap"]["desc"]["seq"][0] == 0xFFFFFFF8
    assert st["age_299999"] == [K] and st["age_300000"] == [R] and st["ts_ahead_of_now"] == [R]
    assert oc["age_299999"]["head_ts"][0] == NOW - 299999 and oc["age_300000"]["head_ts"][0] == NOW
    assert st["young_then_due"] == [K, K]
    assert st["seventeen_due"] == [R] * 16 + [K] and oc["seventeen_due"]["flags"][0] == tq.O_BATCH
    assert st["sixteen_due"] == [R] * 16 and oc["sixteen_due"]["flags"][0] == tq.O_BATCH
    assert st["acked_behind_unacked"] == [R, K, R] and oc["acked_behind_unacked"]["nacked"][0] == 0
    assert st["young_acked_head"] == [A, K] and oc["young_acked_head"]["head_ts"][0] == tq.DUE
    assert st["all_acked"] == [A] * 3 and oc["all_acked"]["flags"][0] == tq.O_EMPTY
    d = w["trim_1"]
    assert st["trim_1"] == [R | T] and (d["desc"]["seq"][0], d["desc"]["paylen"][0]) == (1001, 99)
    assert d["frame_off"][0] == tq.cases()["trim_1"]["cold"]["frame_off"][0] + 1 and d["len"][0] == 0
    d = w["trim_all_but_one"]
    assert (d["desc"]["seq"][0], d["desc"]["paylen"][0]) == (1099, 1)
    assert d["frame_off"][0] == tq.cases()["trim_all_but_one"]["cold"]["frame_off"][0] + 99
    d = w["trim_inflight"]
    assert st["trim_inflight"] == [RC | T] and d["len"][0] == 60 and d["frame_off"][0] == 1 << 20
    assert d["src_off"][0] == tq.cases()["trim_inflight"]["cold"]["frame_off"][0] + 54 + 40
    assert w["trim_fin"]["desc"]["paylen"][0] == 50 and w["fin_paylen_0"]["desc"]["paylen"][0] == 0
    assert st["fin_paylen_0"] == [R] and w["fin_paylen_0"]["desc"]["tcp_flags"][0] == tq.TCP_FIN | tq.TCP_ACK
    assert st["syn_with_options"] == [R] and w["syn_with_options"]["desc"]["tcp_off"][0] == 10
    assert st["syn_with_options_inflight"] == [RC] and w["syn_with_options_inflight"]["len"][0] == 20
    assert st["inflight"] == [RC, R] and w["inflight"]["len"].tolist() == [100, 0]
    assert w["inflight"]["dst_off"][0] == (1 << 20) + 54
    assert st["fast_alone"] == [A, RC, K] and oc["fast_alone"]["head_ts"][0] == NOW
    assert st["fast_and_rto_same_head"] == [R, R] and oc["fast_and_rto_same_head"]["nretx"][0] == 2
    assert st["fast_and_rto_young_head"] == [RC, K]
    assert st["seventeen_due_and_fast"] == [R] * 16 + [K] and oc["seventeen_due_and_fast"]["nretx"][0] == 16
    assert oc["fast_empty_queue"]["flags"][0] == tq.O_EMPTY and oc["fast_all_acked"]["flags"][0] == tq.O_EMPTY
    assert st["fast_trim"] == [RC | T] and w["fast_trim"]["len"][0] == 70
    assert st["excl_with_everything"] == [K, K] and oc["excl_with_everything"]["flags"][0] == tq.O_DEFERRED
    assert oc["excl_with_everything"]["nacked"][0] == 0 and w["excl_with_everything"]["totals"][0] == 0
    assert oc["excl_empty"]["flags"][0] == tq.O_DEFERRED | tq.O_EMPTY
    assert st["want_null"] == [A, K] and st["want_zero"] == [A, K]
    for k in ("refuse_off_4", "refuse_off_16", "refuse_paylen", "refuse_trim_with_options"):
        assert st[k] == [RF, R] and w[k]["counts"][tq.C_REFUSED] == 1 and oc[k]["head_ts"][0] == NOW, k
    assert st["paylen_65535"] == [R] and w["paylen_65535"]["desc"]["paylen"][0] == 65535
    assert st["refuse_fin_without_sequence"] == [RF, R]
    assert st["refuse_copy_past_stride"] == [RF, RC, RF]
    assert st["refuse_fast_past_stride"] == [R, RF]
    assert st["seventeen_refused_then_sixteen"] == [RF] * 17 + [R] * 16 + [K]
    assert st["nospace_first"] == [NS, K, K, K] and st["nospace_middle"] == [R, NS, K, K]
    assert st["nospace_last"] == [R, R, NS, K] and st["space_for_all"] == [R, R, R, K]
    for k in ("nospace_first", "nospace_middle", "nospace_last"):
        assert oc[k]["flags"][0] == tq.O_NOSPACE and w[k]["totals"][0] == 3, k
    assert oc["nospace_middle"]["head_ts"][0] == NOW and oc["nospace_first"]["head_ts"][0] == NOW
    assert st["nospace_fast"] == [R, R, NS] and oc["nospace_fast"]["head_ts"][1] == NOW
    assert st["nospace_fast_after_walk"] == [NS] and w["nospace_fast_after_walk"]["counts"][tq.C_NOSPACE] == 1
    assert st["nospace_then_refused_kept"] == [R, NS, K, NS, K, RF]
    assert st["seg_cap_0"] == [NS, K, A, A, NS] and w["seg_cap_0"]["totals"].tolist() == [3, 0, 0]
    assert oc["cap_at_a_connection_end"]["flags"].tolist() == [0, 0, tq.O_NOSPACE]
    assert oc["cap_at_a_connection_end"]["first"].tolist() == [0, 2, 5]
    assert oc["bad_qoff"]["flags"].tolist() == [0, tq.O_BADRANGE | tq.O_EMPTY, tq.O_BADRANGE | tq.O_EMPTY,
                                                tq.O_BADRANGE | tq.O_EMPTY, tq.O_EMPTY]
    assert st["bad_qoff"] == [R, R, R, R, R, tq.SENTINEL]
    assert young < NOW


def test_all_named_cases_as_one_batch(g):
    for cap in (None, 40, 0):
        check(g, tq.all_named(seg_cap=cap), ("all", cap))


@pytest.mark.parametrize("seed", range(6))
def test_random_batches(g, seed):
    w = check(g, tq.random_case(100 + seed, 400, due=0.6), seed)
    assert all(w["counts"][k] > 0 for k in (tq.C_ACKED, tq.C_RETX, tq.C_COPIED, tq.C_TRIMMED, tq.C_REFUSED,
                                            tq.C_DEFERRED, tq.C_BYTES)), w["counts"]
    check(g, tq.random_case(200 + seed, 300, due=0.8, seg_cap=150 + 40 * seed, bad_qoff=0.05), (seed, "cap"))
    check(g, tq.random_case(300 + seed, 50, qlen=lambda k, r: r.choice([0, 63, 64, 65, 130, 200]), due=0.9,
                            hostile=0.02), (seed, "long"))


def test_counts_null_and_accumulated(g):
    case = tq.random_case(7, 200, due=0.7)
    want = tq.model(case)
    got, _ = tq.run_host(g, case, counts=False)
    tq.compare(got, want, case, "no counts")
    cnt = np.zeros(tq.NR, dtype=np.uint64)
    for _ in range(2):
        g.tcp_txq_host(case["now"], case["qoff"], case["ent"], case["cold"], case["conn"], case["addr"],
                       case["seg_cap"], want=case["want"], frame_stride=case["frame_stride"],
                       frame_base=case["frame_base"], counts=cnt)
    assert cnt.tolist() == (2 * want["counts"]).tolist()


def test_struct_layouts(g):
    assert g.TXQ_ENT_DTYPE == tq.ENT and g.TXQ_COLD_DTYPE == tq.COLD and g.TXQ_CONN_OUT_DTYPE == tq.CONN_OUT
    assert ctypes.sizeof(g.GclTxqIn) == 96 and ctypes.sizeof(g.GclTxqOut) == 80
    offs = {f: getattr(g.GclTxqIn, f).offset for f, _ in g.GclTxqIn._fields_}
    assert offs == dict(size=0, blocks=4, now=8, qoff=16, ent=24, cold=32, nent=40, conn=48, addr=56, want=64,
                        nconn=72, frame_stride=76, seg_cap=80, frame_base=88)
    assert [getattr(g.GclTxqOut, f).offset for f in g.TXQ_OUT_FIELDS] == list(range(0, 80, 8))
    assert [tq.ENT.fields[f][1] for f in ("seg_seq", "seg_end", "ts")] == [0, 4, 8]
    assert [tq.COLD.fields[f][1] for f in ("frame_off", "tcp_flags", "tcp_off", "flags", "pad")] == [0, 8, 9, 10, 11]
    assert [tq.CONN_OUT.fields[f][1] for f in ("head_ts", "nacked", "nretx", "first", "flags", "pad")] == \
        [0, 8, 12, 16, 20, 21]
    assert (g.TXQ_W_RTO, g.TXQ_W_FAST, g.TXQ_W_EXCL, g.TXQE_INFLIGHT) == (tq.W_RTO, tq.W_FAST, tq.W_EXCL, tq.INFLIGHT)
    assert (g.TXQS_KEPT, g.TXQS_ACKED, g.TXQS_RETX, g.TXQS_RETX_COPY, g.TXQS_NOSPACE, g.TXQS_REFUSED,
            g.TXQS_TRIMMED) == (0, 1, 2, 3, 4, 5, 0x80)
    assert (g.TXQO_EMPTY, g.TXQO_DEFERRED, g.TXQO_NOSPACE, g.TXQO_BATCH, g.TXQO_BADRANGE) == (1, 2, 4, 8, 16)
    assert (g.TXQC_NR, g.TXQ_MAX_BLOCKS, g.TXQ_MAX_CONN, g.TXQ_TILE, g.TXQ_LONG) == \
        (tq.NR, tq.MAX_BLOCKS, tq.MAX_CONN, tq.TILE, tq.LONG)


def structs(g, case, out, **kw):
    """the two structs of a call over @case, fields overridden by @kw ("o_" + name: an output pointer)"""
    nconn, nent = len(case["conn"]), len(case["ent"])
    qin, qout = g._txq_structs(case["now"], case["qoff"], case["ent"], case["cold"], nent, case["conn"],
                               case["addr"], case["want"], nconn, case["seg_cap"], case["frame_base"],
                               case["frame_stride"], 0, out, None)
    for k, v in kw.items():
        if k.startswith("o_"):
            setattr(qout, k[2:], v)
        else:
            setattr(qin, k, v)
    return qin, qout


def test_einval(g):
    case = tq.cases()["inflight"]
    out = tq.blank(1, 2, case["seg_cap"])
    call = lambda qin, qout, cnt=None: g.lib.gcl_tcp_txq_host(ctypes.byref(qin), ctypes.byref(qout), cnt)
    qin, qout = structs(g, case, out)
    assert call(qin, qout) == 0
    assert g.lib.gcl_tcp_txq_host(None, ctypes.byref(qout), None) == -errno.EINVAL
    assert g.lib.gcl_tcp_txq_host(ctypes.byref(qin), None, None) == -errno.EINVAL
    bad = [dict(size=95), dict(size=0), dict(nconn=tq.MAX_CONN + 1), dict(nent=(1 << 31) + 1),
           dict(seg_cap=(1 << 31) + 1), dict(blocks=tq.MAX_BLOCKS + 1), dict(frame_stride=53), dict(o_totals=None),
           dict(qoff=None), dict(conn=None), dict(addr=None), dict(o_out_conn=None), dict(ent=None),
           dict(cold=None), dict(o_state=None)]
    bad += [{"o_" + f: None} for f in g.TXQ_SEG_FIELDS]
    for f, a in (("qoff", 2), ("ent", 8), ("cold", 8), ("conn", 8), ("addr", 8)):
        bad.append({f: getattr(qin, f) + a})
    for f, a in (("out_conn", 8), ("desc", 8), ("frame_off", 4), ("src_off", 4), ("len", 1), ("dst_off", 4),
                 ("seg_conn", 2), ("seg_ent", 2), ("totals", 4)):
        bad.append({"o_" + f: getattr(qout, f) + a})
    for kw in bad:
        assert call(*structs(g, case, out, **kw)) == -errno.EINVAL, kw
    cnt = np.zeros(tq.NR + 1, dtype=np.uint64)
    assert call(qin, qout, cnt.ctypes.data + 4) == -errno.EINVAL
    # what is not refused: no want, no entries without their arrays, no segments without theirs, the caps themselves
    ok = [dict(want=None), dict(frame_stride=54), dict(blocks=tq.MAX_BLOCKS),
          dict(nconn=0, qoff=None, conn=None, addr=None, o_out_conn=None, o_desc=None),
          dict(seg_cap=0, o_desc=None, o_frame_off=None, o_src_off=None, o_len=None, o_dst_off=None,
               o_seg_conn=None, o_seg_ent=None)]
    for kw in ok:
        assert call(*structs(g, case, out, **kw)) == 0, kw
    empty = tq.cases()["empty_queue"]
    out = tq.blank(1, 0, empty["seg_cap"])  # held while the call writes it
    qin, qout = structs(g, empty, out, ent=None, cold=None, o_state=None)
    assert call(qin, qout) == 0
    need = ctypes.c_size_t()
    assert g.lib.gcl_tcp_txq_workspace(tq.MAX_CONN + 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_txq_workspace(1, tq.MAX_BLOCKS + 1, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tcp_txq_workspace(1, 0, None) == -errno.EINVAL
    assert g.tcp_txq_workspace(tq.MAX_CONN) == 4 * tq.MAX_BLOCKS and g.tcp_txq_workspace(5, 3) == 16
