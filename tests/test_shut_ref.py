"""The FIN of gcl_tcp_shut_host against the reference's own tcp_push_tcphdr
(tests/golden/tcpfin_ref.json, recorded by tests/golden/make_tcpfin_ref.py with
flags 0x11): the twin's FIN descriptors go through gcl_tx_hdr_host, whose TCP
header is the reference's with tx offloads (the pseudo-header sum in the sum
field), and then through gcl_l4_csum_host FILL, whose header is the
reference's without them (the whole checksum)."""
import importlib.util
import os

import numpy as np
import pytest

from caladan_amd import gclassify as G
from tests import shutcases as T

STRIDE = 64


def _generator():
    path = os.path.join(os.path.dirname(T.GOLDEN), "make_tcpfin_ref.py")
    spec = importlib.util.spec_from_file_location("make_tcpfin_ref", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_headers_are_what_the_reference_gives():
    """Where oracle/_ref is built, the generator's result in memory equals the
    committed file, text and all."""
    from oracle import orc
    if orc.ref_tcpout() is None:
        pytest.skip("oracle/_ref/libtcpout_ref.so not built (no reference tree)")
    gen = _generator()
    fresh = gen.build()
    assert fresh == T.load_golden()
    with open(T.GOLDEN) as f:
        assert f.read() == gen.dumps(fresh)


def test_golden_holds_every_edge():
    segs = T.load_golden()["segs"]
    assert os.path.getsize(T.GOLDEN) < 32 * 1024 and 24 <= len(segs) <= 60
    assert [{k: r[k] for k in r if not k.startswith("hdr_")} for r in segs] == T.golden_inputs()
    assert {r["wscale"] for r in segs} == {0, 7}
    assert T.M32 in {r["seq"] for r in segs} and 0 in {r["seq"] for r in segs}
    assert any(r["rcv_wnd"] >> r["wscale"] > 0xFFFF for r in segs)      # the hton16 truncation
    assert any(r["wscale"] == 7 and 0 < r["rcv_wnd"] >> 7 <= 0xFFFF for r in segs)
    for r in segs:      # no_tx_offloads both ways: the two headers differ in the sum field alone
        a, b = bytes.fromhex(r["hdr_offload"]), bytes.fromhex(r["hdr_full"])
        assert len(a) == len(b) == 20 and a[:16] + a[18:] == b[:16] + b[18:] and a[13] == 0x11 and a[12] == 0x50
        assert int.from_bytes(a[4:8], "big") == r["seq"] and int.from_bytes(a[8:12], "big") == r["ack"]


def test_fin_descriptors_give_the_references_header_bytes():
    segs = T.load_golden()["segs"]
    b = T.golden_batch()
    k = len(segs)
    got = b.run_host(k, frame_stride=STRIDE)
    assert got["totals"][:2].tolist() == [k, k]
    assert (np.ascontiguousarray(got["seg_kind"]).view(np.uint8)[:k] == G.CTL_FIN).all()
    desc = np.frombuffer(T.raw(got["desc"], 32 * k), dtype=G.TXH_DESC_DTYPE).copy()
    off = np.frombuffer(T.raw(got["frame_off"], 8 * k), dtype=np.uint64).copy()
    ent = np.frombuffer(T.raw(got["txq_ent"], 16 * k), dtype=G.TXQ_ENT_DTYPE)
    assert off.tolist() == [STRIDE * j for j in range(k)]
    assert ent["seg_end"].tolist() == [(r["seq"] + 1) & T.M32 for r in segs]
    frames = np.full(k * STRIDE, 0xA5, dtype=np.uint8)
    net = G.txh_net(T.NET["addr"], T.NET["netmask"], T.NET["gateway"], T.NET["mac"])
    tbl = G.NeighTable()
    tbl.set(T.NEIGH)
    hdr = G.tx_hdr_host(desc, off, frames, net, table=tbl)
    assert (hdr["status"][:k] == G.TXH_OK).all() and (hdr["pkt_len"][:k] == 54).all()
    for j, r in enumerate(segs):
        assert frames[j * STRIDE + 34:j * STRIDE + 54].tobytes().hex() == r["hdr_offload"], j
    st = G.l4_csum_host(frames, hdr["pkt_len"], mode=G.L4_FILL, offs=off, n=k)    # both sums filled
    for j, r in enumerate(segs):
        assert frames[j * STRIDE + 34:j * STRIDE + 54].tobytes().hex() == r["hdr_full"], (j, st[j])
    assert (G.l4_csum_host(frames, hdr["pkt_len"], mode=G.L4_VERIFY, offs=off, n=k)[:k] == G.L4_GOOD).all()
