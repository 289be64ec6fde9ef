"""CPU: gcl_l4_payload_host (include/gcl_host.h), the rule of gcl_l4_payload
on the CPU, against the numpy definition (tests/paycases.py): exact equality
of every output array, total, seg_bytes and the counters; every output buffer
starts as a sentinel and carries a guard that must come back unchanged."""
import ctypes

import numpy as np
import pytest

from tests import l4cases as lc
from tests import paycases as pc

EINVAL = 22


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    assert gclassify.PAYC_NR == pc.NR and gclassify.PAY_MAX_BLOCKS == pc.MAX_BLOCKS
    assert gclassify.PAY_META_DTYPE == pc.META
    return gclassify


def check(g, case, what, order=None, sock=None, st=None, seg_off=None, align=0, counts=True, meta=True,
          frames_len=None, shift=0, pk=None):
    """One call over the case's region placed @shift bytes into a buffer of
    its own, held to the model; returns (model, counts)."""
    flen = case["frames_len"] if frames_len is None else frames_len
    case = dict(case, frames_len=flen)
    want = pc.model(case, order, sock, st, seg_off, align, pk=pk)
    n, m = len(case["pkt_len"]), len(want["kind"])
    nseg = len(seg_off) - 1 if seg_off is not None else 0
    buf = np.full(flen + shift, lc.FILLBYTE, dtype=np.uint8)
    buf[shift:] = case["frames"][:flen]
    out = pc.blank_outputs(m, nseg, with_seg=seg_off is not None, with_meta=meta)
    cnt = np.full(pc.NR, 5, dtype=np.uint64) if counts else None
    got = g.l4_payload_host(buf[shift:], case["pkt_len"], stride=case["stride"], offs=case["offs"], n=n,
                            order=order, m=m, sock=sock, l4_status=st, seg_off=seg_off, nseg=nseg,
                            align=align, out=out, counts=cnt)
    pc.compare(got, want, m, nseg, what)
    if counts:
        assert (cnt - 5).tolist() == want["counts"].tolist(), what
    return want, cnt


def test_grid_every_header_length_payload_and_alignment(g):
    case = pc.grid_case()
    pk = pc.packets(case)
    n = len(case["pkt_len"])
    for align in (1, 16, 256):
        want, _ = check(g, case, f"grid align {align}", align=align, pk=pk)
        assert (want["kind"] != pc.NA).all() and (want["dst_off"] % align == 0).all()
    want, _ = check(g, case, "grid dense", align=0, pk=pk)
    assert int((want["kind"] == pc.K_TCP).sum()) == 16 * 66 and int((want["kind"] == pc.K_UDP).sum()) == 16 * 4
    assert n == 16 * 70 and set(want["len"].tolist()) == {0, 1, 15, 16, 17, 1460, 1472}
    # src_off is the byte behind the L4 header: the payload the frame was built with
    hl = (want["src_off"] - case["offs"] - 34).astype(int)
    assert set(hl[want["kind"] == pc.K_TCP].tolist()) == set(range(20, 61, 4))
    assert (hl[want["kind"] == pc.K_UDP] == 8).all()
    for shift in (1, 4, 9):
        check(g, case, f"grid base + {shift}", shift=shift, align=16, pk=pk)
    check(g, case, "grid without meta and counts", meta=False, counts=False, pk=pk)


@pytest.mark.parametrize("cut", [None, "payload", "header"])
def test_na_reasons_one_frame_each(g, cut):
    case = pc.na_case(cut)
    want, cnt = check(g, case, f"na cut {cut}")
    kinds = dict(zip(pc.NA_NAMES, want["kind"].tolist()))
    assert kinds.pop("good_udp") == pc.K_UDP and kinds.pop("good_tcp") == pc.K_TCP
    assert kinds.pop("cut") == (pc.K_TCP if cut is None else pc.NA)
    assert set(kinds.values()) == {pc.NA} and len(kinds) == 14
    for shift in (1, 2, 8):
        check(g, case, f"na cut {cut} base + {shift}", shift=shift)


def test_filters_and_their_priority(g):
    case, sock, st = pc.filter_case()
    n = len(sock)
    want, _ = check(g, case, "filters", sock=sock, st=st, align=16)
    k = want["kind"].reshape(len(pc.SOCKS), len(pc.STATUSES), 4)
    bad_t = [i for i, t in enumerate(pc.STATUSES) if t & 0xF == lc.BAD]
    bad_s = [i for i, s in enumerate(pc.SOCKS) if s > pc.COOKIE_MAX]
    assert bad_t == [1, 4] and bad_s == [2, 3, 4, 5]
    for si in range(len(pc.SOCKS)):
        for ti in range(len(pc.STATUSES)):
            exp = pc.BADCSUM if ti in bad_t else pc.NOSOCK if si in bad_s else None
            assert k[si, ti, 0] == (exp or pc.K_UDP) and k[si, ti, 1] == (exp or pc.K_TCP)
            assert k[si, ti, 2] == pc.NA and k[si, ti, 3] == pc.NA  # NA beats both filters
    only_sock, _ = check(g, case, "sock alone", sock=sock)
    only_st, _ = check(g, case, "l4_status alone", st=st)
    assert (only_sock["kind"] != pc.BADCSUM).all() and (only_st["kind"] != pc.NOSOCK).all()
    # out of range beats everything
    order = np.array([0, n, 1, 0xFFFFFFFF], dtype=np.uint32)
    want, _ = check(g, case, "oor first", order=order, sock=sock, st=st)
    assert want["kind"].tolist() == [pc.K_UDP, pc.OOR, pc.K_TCP, pc.OOR]


@pytest.mark.parametrize("name", ["permutation", "shorter", "longer"])
def test_orders_and_segments(g, name):
    case, sock, st = pc.filter_case()
    order, seg = pc.orders(len(sock))[name]
    want, _ = check(g, case, name, order=order, sock=sock, st=st, seg_off=seg, align=16)
    if name == "longer":
        assert (want["kind"] == pc.OOR).sum() >= 52 and len(order) > len(sock)
        assert len(set(want["seg_bytes"].tolist())) > 4
    check(g, case, name + " dense", order=order, seg_off=seg)


def test_scan_carries(g):
    case, sock, st, order = pc.scan_case()
    pk = pc.packets(case)
    seg = np.array([0, pc.SCAN_M // 2, pc.SCAN_M - 1, pc.SCAN_M], dtype=np.uint32)
    want, _ = check(g, case, "scan", order=order, sock=sock, st=st, seg_off=seg, align=16, pk=pk)
    assert len(want["kind"]) == pc.SCAN_M == 3 * 256 * pc.SCAN_K + 5
    assert all((want["kind"] == k).sum() > 1000 for k in range(6))
    big, order = pc.big_case()
    want, cnt = check(g, big, "64-bit carry", order=order, align=256)
    assert int(want["total"][0]) == pc.BIG_M * 65536 > 1 << 32
    assert int(cnt[pc.C_BYTES]) - 5 == pc.BIG_M * pc.BIG_PAY


def test_counts_accumulate_and_m_zero(g):
    case, sock, st = pc.filter_case()
    a, _ = check(g, case, "first", sock=sock, st=st)
    grid = pc.grid_case()
    b = pc.model(grid)
    cnt = np.zeros(pc.NR, dtype=np.uint64)
    g.l4_payload_host(case["frames"], case["pkt_len"], offs=case["offs"], sock=sock, l4_status=st, counts=cnt)
    g.l4_payload_host(grid["frames"], grid["pkt_len"], offs=grid["offs"], counts=cnt)
    assert cnt.tolist() == (a["counts"] + b["counts"]).tolist()
    # m == 0: total and seg_bytes are zeroed, nothing else is touched
    for order in (np.zeros(1, dtype=np.uint32), None):
        out = pc.blank_outputs(0, 2)
        cnt = np.full(pc.NR, 9, dtype=np.uint64)
        n = len(sock) if order is not None else 0
        g.l4_payload_host(case["frames"], case["pkt_len"], offs=case["offs"], n=n, order=order, m=0,
                          seg_off=np.array([0, 1, 7], dtype=np.uint32), nseg=2, out=out, counts=cnt)
        want = {"seg_bytes": np.zeros(3, dtype=np.uint64), "total": np.zeros(1, dtype=np.uint64)}
        pc.compare(out, want, 0, 2, "m == 0", written=False)
        assert (cnt == 9).all()


def test_error_returns(g):
    case, sock, st = pc.filter_case()
    n = len(sock)
    out = pc.blank_outputs(n, 1)
    seg = np.array([0, n], dtype=np.uint32)
    order = np.arange(n, dtype=np.uint32)
    cnt = np.full(pc.NR, 9, dtype=np.uint64)
    size = ctypes.sizeof(g.GclPayIn)
    P = lambda a: a.ctypes.data  # noqa: E731

    def call(bb=True, ii=True, oo=True, frames=P(case["frames"]), flen=case["frames_len"], stride=0,
             offs=P(case["offs"]), plen=P(case["pkt_len"]), nn=n, sz=size, align=0, order=None, m=n,
             sock=None, st=None, seg_off=P(seg), nseg=1, blocks=0, counts=P(cnt), **o):
        b = g.GclBatch(frames=frames, frames_len=flen, stride=stride, offs=offs, pkt_len=plen, n=nn)
        i = g.GclPayIn(size=sz, align=align, order=order, m=m, sock=sock, l4_status=st, seg_off=seg_off,
                       nseg=nseg, blocks=blocks)
        ptrs = {f: P(out[f]) for f in g.PAY_OUT_FIELDS}
        ptrs.update(o)
        po = g.GclPayOut(**ptrs)
        return g.lib.gcl_l4_payload_host(ctypes.byref(b) if bb else None, ctypes.byref(i) if ii else None,
                                         ctypes.byref(po) if oo else None, counts)

    assert call(bb=False) == -EINVAL and call(ii=False) == -EINVAL and call(oo=False) == -EINVAL
    assert call(sz=size - 8) == -EINVAL and call(sz=0) == -EINVAL
    for align in (3, 6, 12, 48, 255, 512, 1 << 31):
        assert call(align=align) == -EINVAL, align
    assert call(m=n - 1) == -EINVAL and call(m=n + 1) == -EINVAL          # no order: m must be n
    assert call(order=P(order), m=(1 << 31) + 1) == -EINVAL
    assert call(blocks=pc.MAX_BLOCKS + 1) == -EINVAL
    for f in ("src_off", "len", "dst_off", "kind", "total"):
        assert call(**{f: None}) == -EINVAL, f
    for f in ("src_off", "len", "dst_off", "total", "seg_bytes", "meta"):
        assert call(**{f: P(out[f]) + 1}) == -EINVAL, f
    assert call(meta=P(out["meta"]) + 8) == -EINVAL
    assert call(seg_bytes=None) == -EINVAL and call(seg_off=None) == -EINVAL
    assert call(order=P(order) + 2) == -EINVAL and call(sock=P(sock) + 1) == -EINVAL
    assert call(seg_off=P(seg) + 2) == -EINVAL and call(counts=P(cnt) + 4) == -EINVAL
    assert call(plen=None) == -EINVAL and call(plen=P(case["pkt_len"]) + 1) == -EINVAL
    assert call(frames=None) == -EINVAL and call(flen=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1, order=P(order)) == -EINVAL
    for stride in (0, 8, 15, 24, 72, (1 << 20) + 16):
        assert call(offs=None, stride=stride) == -EINVAL, stride
    assert all((a.view(np.uint8) == pc.SENTINEL).all() for a in out.values()) and (cnt == 9).all()
    assert call(meta=None, counts=None, seg_off=None, seg_bytes=None, align=256, blocks=pc.MAX_BLOCKS) == 0
    assert call(order=P(order), m=0, nn=0, frames=None, plen=None) == 0
    with pytest.raises(ValueError):
        g.l4_payload_host(case["frames"], case["pkt_len"], offs=case["offs"], order=order, m=n + 1)
    with pytest.raises(ValueError):
        g.l4_payload_host(case["frames"], case["pkt_len"], offs=case["offs"], sock=sock[:n - 1])
    with pytest.raises(ValueError):
        g.l4_payload_host(case["frames"], case["pkt_len"], offs=case["offs"], seg_off=seg, nseg=2)
    with pytest.raises(ValueError):
        g.l4_payload_host(case["frames"], case["pkt_len"], offs=case["offs"], counts=cnt[:3])
