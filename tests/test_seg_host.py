"""CPU: gcl_tx_seg_host (csrc/gcl_host.c, with the rule of csrc/gcl_seg.h that
the GPU kernels share) against the independent model of tests/segcases.py,
field for field: every output array whole, with its sentinel-filled tail past
*total_segs, the totals and the counters; then the properties the header
states, on random batches, and the error returns."""
import ctypes
import errno

import numpy as np
import pytest

from tests import segcases as sc


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def test_dtypes_match(g):
    assert sc.SEND_DTYPE == g.SEG_SEND_DTYPE and sc.DESC_DTYPE == g.TXH_DESC_DTYPE
    assert (sc.OK, sc.REFUSED, sc.NOSPACE) == (g.SEG_OK, g.SEG_REFUSED, g.SEG_NOSPACE)
    assert (sc.C_SEGS, sc.C_BYTES, sc.C_PUSH, sc.C_NR) == (g.SEGC_SEGS, g.SEGC_BYTES, g.SEGC_PUSH, g.SEGC_NR)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_host_equals_model(g, name):
    case, want = sc.cases()[name], sc.models()[name]
    got, cnt = sc.run_host(g, case)
    sc.compare(got, want, name)
    assert cnt.tolist() == want["counts"].tolist(), name
    total = int(want["total_segs"][0])
    for f in sc.SEG_DTYPE:      # nothing at or past *total_segs was touched
        assert (got[f][total:].view(np.uint8) == sc.SENTINEL).all(), (name, f)


def test_grid_covers_every_status_and_shape():
    want = sc.models()
    st = np.concatenate([w["status"] for w in want.values()])
    assert {sc.OK, sc.REFUSED, sc.NOSPACE} <= set(st.tolist())
    w = want["packed_lead0"]
    n = int(w["total_segs"][0])
    d = w["desc"][:n]
    assert (d["paylen"] == 0).any() and (d["paylen"] == 65535).any()
    assert ((d["tcp_flags"] == 0x18) & (d["paylen"] == 0)).any()       # the empty ACK|PSH segment
    assert (w["nseg"] > 40).any() and (w["nseg"] == 1).any()
    seq = d["seq"].astype(np.int64)
    assert (np.diff(seq) < -(1 << 31)).any()                            # seq wrapped 2^32
    assert (np.diff(w["src_off"][:n].astype(np.float64)) < -1e18).any() # src_off wrapped 2^64


@pytest.mark.parametrize("seed", range(6))
def test_random_batches_and_properties(g, seed):
    rng = np.random.default_rng(seed)
    m = int(rng.integers(1, 400))
    case = sc.random_case(rng, m, refused=float(rng.choice([0.0, 0.1, 0.9])))
    if seed % 2:
        case["seg_cap"] = int(rng.integers(0, 2 * m))
    want = sc.model(case)
    got, cnt = sc.run_host(g, case, send_idx=seed != 3)
    sc.compare(got, want, seed)
    assert cnt.tolist() == want["counts"].tolist()
    st, first, nseg = got["status"], got["seg_first"].astype(np.int64), got["nseg"].astype(np.int64)
    assert int(cnt[sc.C_OK] + cnt[sc.C_REFUSED] + cnt[sc.C_NOSPACE]) == m
    assert int(nseg.sum()) == int(got["total_segs"][0]) <= case["seg_cap"]
    assert (np.diff(first) >= 0).all()
    live = st[st != sc.REFUSED]
    k = int((live == sc.OK).sum())
    assert (live[:k] == sc.OK).all() and (live[k:] == sc.NOSPACE).all()   # NOSPACE is a suffix
    ok = st == sc.OK
    assert (first[ok] == np.concatenate([[0], np.cumsum(nseg[ok])[:-1]])).all()
    assert (got["sent"][~ok] == 0).all() and (got["snd_nxt_out"][~ok] == case["send"]["snd_nxt"][~ok]).all()
    n = int(got["total_segs"][0])
    if seed != 3:
        assert (got["send_idx"][:n] == np.repeat(np.arange(m), nseg)).all()
    assert (got["len"][:n] == got["desc"]["paylen"][:n]).all()
    # frames do not overlap and keep the layout's alignment
    fo = got["frame_off"][:n].astype(np.int64)
    flen = 34 + np.where(got["desc"]["proto"][:n] == 6, 20, 8) + got["len"][:n]
    assert (fo[1:] >= fo[:-1] + flen[:-1]).all()
    assert ((fo - case["frame_base"] - case["lead"]) % (case["stride"] or 16) == 0).all()


def test_counts_accumulate_and_m_zero(g):
    case = sc.cases()["cap7_packed"]
    want = sc.models()["cap7_packed"]["counts"]
    cnt = np.zeros(sc.C_NR, dtype=np.uint64)
    for _ in range(2):
        g.tx_seg_host(case["send"], case["seg_cap"], lead=case["lead"], counts=cnt)
    assert cnt.tolist() == (2 * want).tolist()
    out = sc.blank(0, 4)
    g.tx_seg_host(case["send"][:0], 4, m=0, out=out)
    assert out["total_segs"][0] == 0 and out["total_bytes"][0] == 0
    assert (out["status"] == sc.SENTINEL).all() and (out["len"].view(np.uint8) == sc.SENTINEL).all()


def test_errors(g):
    case = sc.cases()["cap7_packed"]
    m, cap = len(case["send"]), 16
    out = sc.blank(m, cap)
    send = case["send"]

    def call(in_kw=None, out_kw=None, counts=None):
        o = {f: out[f].ctypes.data for f in g.SEG_OUT_FIELDS}
        o.update(out_kw or {})
        kw = dict(size=ctypes.sizeof(g.GclSegIn), send=send.ctypes.data, m=m, seg_cap=cap, udp_max=1472)
        kw.update(in_kw or {})
        sin, sout = g.GclSegIn(**kw), g.GclSegOut(**o)
        return g.lib.gcl_tx_seg_host(ctypes.byref(sin), ctypes.byref(sout), counts)

    assert call() == 0
    assert call(out_kw=dict(send_idx=None)) == 0
    assert call(dict(m=0, send=None), dict(status=None, desc=None)) == 0
    assert call(dict(seg_cap=0), dict(desc=None, frame_off=None, src_off=None, len=None, dst_off=None)) == 0
    for kw in (dict(size=60), dict(send=None), dict(m=2 ** 31 + 1), dict(seg_cap=2 ** 31 + 1),
               dict(stride=(1 << 20) + 1), dict(lead=65536), dict(udp_max=65508), dict(blocks=1025),
               dict(send=send.ctypes.data + 8)):
        assert call(kw) == -errno.EINVAL, kw
    for f in g.SEG_OUT_FIELDS:
        if f != "send_idx":
            assert call(out_kw={f: None}) == -errno.EINVAL, f
    for f, by in (("sent", 2), ("snd_nxt_out", 1), ("seg_first", 2), ("nseg", 2), ("desc", 8), ("frame_off", 4),
                  ("src_off", 4), ("len", 1), ("dst_off", 4), ("send_idx", 2), ("total_segs", 4),
                  ("total_bytes", 4)):
        assert call(out_kw={f: out[f].ctypes.data + by}) == -errno.EINVAL, f
    assert call(counts=out["frame_off"].ctypes.data + 4) == -errno.EINVAL
    assert g.lib.gcl_tx_seg_host(None, None, None) == -errno.EINVAL
    need = ctypes.c_size_t()
    assert g.lib.gcl_tx_seg_workspace(2 ** 31 + 1, 0, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tx_seg_workspace(10, 1025, ctypes.byref(need)) == -errno.EINVAL
    assert g.lib.gcl_tx_seg_workspace(10, 0, None) == -errno.EINVAL
    assert g.tx_seg_workspace(10, 2) == 32 * 2 + 16 + 160
