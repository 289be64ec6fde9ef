"""GPU: gcl_tx_hdr (include/gclassify.h) against the model of
tests/txhcases.py and against its host twin: exact equality of the whole frame
region with its guard bands, of every output array with its sentinel guard and
of the counters, at several byte alignments of the region; snapshot semantics
of gcl_neigh_set; the transmit chain through gcl_l4_csum, gcl_copy_batch and
gcl_classify; the error returns."""
import ctypes
import errno

import numpy as np
import pytest
import torch

from tests import test_txh_host as th
from tests import txhcases as tc

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
    c = g.Classifier(0, 16, g.HASH_NIC, 0, 0x01)   # no Toeplitz in the classify tables: tx_hdr brings its own
    yield c
    c.close()


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == th_desc_dtype():
        return torch.from_numpy(a.view(np.uint8).reshape(-1, 32)).cuda()
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype))).cuda()


def th_desc_dtype():
    from caladan_amd import gclassify
    return gclassify.TXH_DESC_DTYPE


def host(t, dt):
    return t.cpu().numpy().reshape(-1).view(dt)


def run_gpu(g, clf, case, shift=0, with_hash=True, counts=True, stream=None, set_neigh=True):
    """One call over the case's region placed @shift bytes into a device
    buffer of its own; returns (outputs as numpy, the buffer from the front
    guard on, counts)."""
    m, flen = len(case["desc"]), case["frames_len"]
    if set_neigh:
        # the context's table has no hash_bits knob; the truncated-hash image is the host table's
        clf.neigh_set(case["neigh"])
    buf = torch.full((shift + tc.GUARD + flen + tc.GUARD,), tc.SENTINEL, dtype=torch.uint8, device="cuda")
    out = {f: dev(a) for f, a in th.blank_outputs(m).items()}
    if not with_hash:
        out["hash"] = None
    cnt = torch.full((g.TXHC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    clf.tx_hdr(dev(case["desc"]), dev(case["frame_off"]), m, buf[shift + tc.GUARD:], g.txh_net(**case["net"]),
               frames_len=flen, shm_base=case["shm_base"], cap=case["cap"], out=out, counts=cnt, stream=stream)
    torch.cuda.synchronize()
    got = {f: (None if out[f] is None else host(out[f], tc.OUT_DTYPE[f])) for f in tc.OUT_DTYPE}
    return got, buf[shift:].cpu().numpy(), None if cnt is None else cnt.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_gpu_equals_model_and_host(g, clf, name):
    case, want = tc.models()[name]
    m = len(case["desc"])
    hgot, hbuf, _ = th.run_host(g, case)
    for shift, with_hash, counts in ((0, True, True), (1, False, True), (4, True, False), (9, True, True)):
        got, buf, cnt = run_gpu(g, clf, case, shift, with_hash, counts)
        th.compare(got, want, m, (name, shift))
        assert np.array_equal(buf, want["frames"]), (name, shift)
        assert np.array_equal(buf, hbuf)
        for f in tc.OUT_DTYPE:
            if got[f] is not None:
                assert np.array_equal(got[f], hgot[f]), (name, f)
        if counts:
            assert (cnt - 5).tolist() == want["counts"].tolist(), (name, shift)


def test_non_default_stream_and_blocks_per_cu(g, clf):
    case, want = tc.models()["big"]
    m = len(case["desc"])
    stream = torch.cuda.Stream()
    got, buf, cnt = run_gpu(g, clf, case, 5, stream=stream.cuda_stream)
    th.compare(got, want, m, "stream")
    assert np.array_equal(buf, want["frames"]) and (cnt - 5).tolist() == want["counts"].tolist()
    clf.tune(blocks_per_cu=1)
    try:
        got, buf, cnt = run_gpu(g, clf, case, 2)
    finally:
        clf.tune()
    th.compare(got, want, m, "one block per CU")
    assert np.array_equal(buf, want["frames"]) and (cnt - 5).tolist() == want["counts"].tolist()


def test_neigh_set_is_a_snapshot(g, clf):
    case = tc.route()[0]
    empty = dict(case, neigh=[])
    want_a, want_b = tc.model(empty), tc.model(case)
    m = len(case["desc"])
    stream = torch.cuda.Stream()
    clf.neigh_set([])
    flen = case["frames_len"]
    bufs, outs = [], []
    for k in range(2):
        if k == 1:
            clf.neigh_set(case["neigh"])    # between the two calls, neither has been waited for
        buf = torch.full((tc.GUARD + flen + tc.GUARD,), tc.SENTINEL, dtype=torch.uint8, device="cuda")
        out = {f: dev(a) for f, a in th.blank_outputs(m).items()}
        clf.tx_hdr(dev(case["desc"]), dev(case["frame_off"]), m, buf[tc.GUARD:], g.txh_net(**case["net"]),
                   frames_len=flen, shm_base=case["shm_base"], out=out, stream=stream.cuda_stream)
        bufs.append(buf)
        outs.append(out)
    torch.cuda.synchronize()
    for buf, out, want in zip(bufs, outs, (want_a, want_b)):
        th.compare({f: host(out[f], tc.OUT_DTYPE[f]) for f in tc.OUT_DTYPE}, want, m, "snapshot")
        assert np.array_equal(buf.cpu().numpy(), want["frames"])
    assert want_a["status"].tolist() != want_b["status"].tolist()


def test_neigh_table_leaves_classify_and_sock_lookup_alone(g):
    c = g.Classifier(0, 16, g.HASH_JENKINS)
    try:
        for r in range(4):
            c.runtime_set(r, g.runtime_ip(r), 4, 4, [0, 1, 2, 3])
        c.sock_set(1, [(g.runtime_ip(1), 9000, 17, g.SOCK_MATCH_3TUPLE, 77)])
        n, stride = 4096, 64
        frames = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
        g.generate(g.WL_UDP64, n, stride, 4, frames)
        v0 = torch.zeros(n * c.vbytes, dtype=torch.uint8, device="cuda")
        v1 = torch.zeros(n * c.vbytes, dtype=torch.uint8, device="cuda")
        c.classify(frames, n, stride, verdicts=v0)
        s0 = c.sock_lookup(frames, n, stride, verdicts=v0)
        torch.cuda.synchronize()
        v0, s0 = v0.cpu().numpy().copy(), s0.cpu().numpy().copy()
        assert v0.any()
        c.neigh_set(tc.BASE_NEIGH)
        case = tc.route()[0]
        run_gpu(g, c, case)
        c.neigh_set(tc.big_neigh())
        run_gpu(g, c, case, set_neigh=False)
        c.classify(frames, n, stride, verdicts=v1)
        s1 = c.sock_lookup(frames, n, stride, verdicts=v1)
        torch.cuda.synchronize()
        assert np.array_equal(v0, v1.cpu().numpy()) and np.array_equal(s0, s1.cpu().numpy())
    finally:
        c.close()


def _fill_payloads(case, frames):
    """the caller's part of every frame: option bytes and payload"""
    for j in range(len(case["desc"])):
        d = case["desc"][j]
        o = int(case["frame_off"][j])
        hl = 4 * int(d["tcp_off"]) if d["proto"] == 6 else 8
        frames[o + 54:o + 34 + hl] = 1
        frames[o + 34 + hl:o + 34 + hl + int(d["paylen"])] = np.arange(int(d["paylen"]), dtype=np.uint8) ^ (j & 0xFF)


def test_chain_fill_verify_copy_classify(g):
    """gcl_tx_hdr -> gcl_l4_csum FILL -> VERIFY on the device, and for the
    local entries on through gcl_copy_batch and gcl_classify: each is
    delivered to the runtime that owns the next hop, with the hash the txpkt
    payload carries.  The hint is do_toeplitz over netcfg.addr (core.c:730),
    while a GCL_HASH_TOEPLITZ context hashes the frame's own source address,
    so the two agree for the segments a runtime really sends, whose laddr.ip
    is 0 or its own address: the grid's non-zero lip is net.addr here."""
    case = tc.grid()
    case["desc"]["lip"] = np.where(case["desc"]["lip"] != 0, tc.ADDR, 0)
    m, flen = len(case["desc"]), case["frames_len"]
    c = g.Classifier(0, 16, g.HASH_TOEPLITZ, g.CFG_HASH16, rss_key=tc.RSS_KEY)
    try:
        c.runtime_set(3, tc.LOCAL_IP, 4, 4, [0, 1, 2, 3])
        c.runtime_set(5, tc.ADDR, 4, 4, [0, 1, 2, 3])
        c.neigh_set(case["neigh"])
        host_frames = np.full(flen, tc.SENTINEL, dtype=np.uint8)
        _fill_payloads(case, host_frames)
        frames = torch.from_numpy(host_frames).cuda()
        offs = dev(case["frame_off"])
        out = c.tx_hdr(dev(case["desc"]), offs, m, frames, g.txh_net(**case["net"]), shm_base=case["shm_base"])
        st = c.l4_csum(frames, m, out["pkt_len"], mode=g.L4_VERIFY, offs=offs)
        tcp = case["desc"]["proto"] == 6
        torch.cuda.synchronize()
        assert (host(out["status"], np.uint8)[:m] == g.TXH_OK).all()
        assert (st.cpu().numpy()[:m][~tcp] == g.L4_NONE).all()
        c.l4_csum(frames, m, out["pkt_len"], mode=g.L4_FILL, offs=offs, tx_olflags=out["tx_olflags"])
        st = c.l4_csum(frames, m, out["pkt_len"], mode=g.L4_VERIFY, offs=offs).cpu().numpy()[:m]
        assert (st[tcp] == g.L4_GOOD).all() and (st[~tcp] == g.L4_NONE).all()
        c.l4_csum(frames, m, out["pkt_len"], mode=g.L4_FILL, offs=offs)    # every packet: UDP too
        st = c.l4_csum(frames, m, out["pkt_len"], mode=g.L4_VERIFY, offs=offs).cpu().numpy()[:m]
        assert (st == g.L4_GOOD).all()
        # the loopback: copy into an rx pool, classify with the cmd's dst_ip as the hint
        stride = 1600
        pool = torch.zeros(m * stride, dtype=torch.uint8, device="cuda")
        pkt_len, olflags, rss = c.copy_batch(frames, offs, out["pkt_len"], m, pool, dst_stride=stride,
                                             tx_olflags=out["tx_olflags"], hash=out["hash"])
        cmd = host(out["cmd"], np.uint64)[:m]
        hint = dev((cmd & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        verd = torch.zeros(m * c.vbytes, dtype=torch.uint8, device="cuda")
        c.classify(pool, m, stride, verdicts=verd, olflags=olflags, rss=rss, dst_hint=hint)
        torch.cuda.synchronize()
        v = verd.cpu().numpy().reshape(-1).view(g.verdict_dtype(c.vbytes))[:m]
        fl = host(out["tx_olflags"], np.uint8)[:m]
        local = (fl & g.TXFLAG_LOCAL_HINT) != 0
        assert local.sum() > 100 and (~local).sum() > 100
        assert ((fl & g.TXFLAG_LOCAL) != 0).tolist() == local.tolist()
        pay = host(out["payload"], np.uint64)[:m]
        assert ((v["action"][local] & g.ACT_MASK) == g.ACT_DELIVER).all()
        assert (v["uniqid"][local] == 3).all()
        want_hash = np.array([g.lib.gcl_txpkt_rss(int(p)) for p in pay[local]], dtype=np.uint32)
        assert v["hash"][local].tolist() == want_hash.tolist()
        assert (want_hash == (host(out["hash"], np.uint32)[:m][local] & 0xFFFF)).all()
    finally:
        c.close()


def test_errors(g, clf):
    case = tc.route()[0]
    m = len(case["desc"])
    frames = torch.zeros(case["frames_len"], dtype=torch.uint8, device="cuda")
    desc, offs = dev(case["desc"]), dev(case["frame_off"])
    out = {f: dev(a) for f, a in th.blank_outputs(m).items()}
    net = g.txh_net(**case["net"])

    def call(tin_kw=None, out_kw=None, ctx=clf._ctx, counts=None):
        o = {f: out[f].data_ptr() for f in g.TXH_OUT_FIELDS}
        o.update(out_kw or {})
        kw = dict(size=ctypes.sizeof(g.GclTxhIn), desc=desc.data_ptr(), frame_off=offs.data_ptr(), m=m,
                  frames=frames.data_ptr(), frames_len=frames.numel(), net=net)
        kw.update(tin_kw or {})
        tin, tout = g.GclTxhIn(**kw), g.GclTxhOut(**o)
        return g.lib.gcl_tx_hdr(ctx, ctypes.byref(tin), ctypes.byref(tout), counts, None)

    assert call() == 0
    assert call(out_kw=dict(hash=None)) == 0
    assert call(dict(m=0, desc=None, frames=None)) == 0
    assert call(ctx=None) == -errno.EINVAL
    for kw in (dict(size=80), dict(desc=None), dict(frame_off=None), dict(frames=None), dict(m=2 ** 31 + 1),
               dict(frames_len=2 ** 64 - 1), dict(desc=desc.data_ptr() + 8), dict(frame_off=offs.data_ptr() + 4)):
        assert call(kw) == -errno.EINVAL, kw
    for f in ("cmd", "payload", "pkt_len", "tx_olflags", "status"):
        assert call(out_kw={f: None}) == -errno.EINVAL, f
    for f, by in (("cmd", 4), ("payload", 2), ("pkt_len", 1), ("hash", 2)):
        assert call(out_kw={f: out[f].data_ptr() + by}) == -errno.EINVAL, f
    assert call(counts=out["cmd"].data_ptr() + 4) == -errno.EINVAL
    assert g.lib.gcl_tx_hdr(clf._ctx, None, None, None, None) == -errno.EINVAL
    assert g.lib.gcl_neigh_set(None, None, 0) == -errno.EINVAL
    assert g.lib.gcl_neigh_set(clf._ctx, None, 2) == -errno.EINVAL
    with pytest.raises(OSError) as e:
        clf.neigh_set([(5, tc.MAC), (5, tc.MAC)])
    assert e.value.errno == errno.EEXIST
    torch.cuda.synchronize()
