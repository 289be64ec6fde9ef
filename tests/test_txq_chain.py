"""CPU: the frames that gcl_tcp_txq_host -> gcl_copy_batch_host ->
gcl_tx_hdr_host leave in a tx region, against the reference's own
tcp_push_tcphdr bytes (tests/golden/txq_ref.json, made by
tests/golden/make_txq_ref.py): for every named case of tests/txqcases.py that
retransmits, in place and by copy, trimmed and with a FIN, the golden header
stands in front of the payload bytes that stay and nothing else moved."""
import importlib.util
import os

import numpy as np
import pytest

from tests import txqcases as tq


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def _generator():
    path = os.path.join(os.path.dirname(tq.GOLDEN), "make_txq_ref.py")
    spec = importlib.util.spec_from_file_location("make_txq_ref", path)
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
    assert fresh == tq.load_golden()
    with open(tq.GOLDEN) as f:
        assert f.read() == gen.dumps(fresh)


def test_golden_holds_every_edge():
    d = tq.load_golden()
    assert os.path.getsize(tq.GOLDEN) <= 64 * 1024
    segs = d["segs"]
    assert [{k: v for k, v in r.items() if k != "tcphdr"} for r in segs] == tq.golden_inputs()
    assert len(segs) > 100
    by = {(r["by_copy"], r["trim"] > 0, bool(r["flags"] & tq.TCP_FIN)) for r in segs}
    assert {(False, False, False), (True, False, False), (False, True, False), (True, True, False),
            (False, True, True), (False, False, True)} <= by
    assert any(r["paylen"] == 0 for r in segs) and any(r["trim"] == 99 and r["paylen"] == 1 for r in segs)
    assert any(r["seq"] > 0xFFFFFF00 for r in segs)
    # only what the reference's header struct or an IPv4 packet cannot hold is left out
    left = [(n, r["k"]) for n in sorted(tq.cases()) for r in tq.sent_segments(tq.cases()[n]) if not tq.in_golden(r)]
    assert left == [("paylen_65535", 0), ("syn_with_options", 0), ("syn_with_options_inflight", 0)]
    for r in segs:
        h = bytes.fromhex(r["tcphdr"])
        assert len(h) == 20 and h[12] == 0x50 and h[13] == r["flags"]
        assert int.from_bytes(h[4:8], "big") == r["seq"] and int.from_bytes(h[8:12], "big") == r["ack"]


def chain(g, case):
    """the three calls over a fresh region: (inner outputs of the first, the region, tx_hdr's refusals)"""
    full, _ = tq.run_host(g, case)
    got = tq.inner(full)
    k = int(got["totals"][1])
    reg = tq.region(tq.region_size(case))
    if k == 0:
        return got, reg, []
    g.copy_batch_host(reg, got["src_off"][:k].copy(), got["len"][:k].copy(), reg, dst_off=got["dst_off"][:k].copy(),
                      olflags=False, rss=False)
    net = g.txh_net(tq.NET["addr"], tq.NET["netmask"], tq.NET["gateway"], tq.NET["mac"])
    out = g.tx_hdr_host(got["desc"][:k].copy(), got["frame_off"][:k].copy(), reg, net)
    return got, reg, (out["status"][:k] == g.TXH_REFUSED).tolist()


def test_chain_leaves_the_references_headers_in_front_of_the_payload(g):
    segs = tq.load_golden()["segs"]
    sent = 0
    for name in sorted(tq.cases()):
        case = tq.cases()[name]
        got, reg, refused = chain(g, case)
        sent += tq.check_chain(name, case, got, reg, [r for r in segs if r["case"] == name], refused)
    assert sent > 100


def test_chain_catches_a_frame_one_byte_off(g):
    """the check itself: the same region with one in-place frame's headers a
    byte too low, as a frame_off without the trim would put them, fails"""
    case = tq.cases()["trim_1"]
    segs = [r for r in tq.load_golden()["segs"] if r["case"] == "trim_1"]
    got, reg, refused = chain(g, case)
    tq.check_chain("trim_1", case, got, reg, segs, refused)
    f = int(got["frame_off"][0])
    moved = tq.region(len(reg))
    moved[f - 1:f - 1 + tq.HDR] = reg[f:f + tq.HDR]
    with pytest.raises(AssertionError):
        tq.check_chain("trim_1", case, got, moved, segs, refused)
