"""CPU: the transmit headers and the L4 / IPv4 checksums against bytes the
REFERENCE's own code produced (tests/golden/txpath_ref.json, recorded by
tests/golden/make_txpath_ref.py from runtime/net/tcp_out.c, inc/net/chksum.h
and runtime/net/core.c compiled in place).  The Python models of
tests/txhcases.py and tests/l4cases.py and the host twins gcl_tx_hdr_host,
gcl_l4_csum_host and gcl_rx_csum_flags must reproduce every recorded byte;
tests/test_gpu_txpath_ref.py holds the kernels to the same file."""
import importlib.util
import os

import numpy as np
import pytest

from tests import l4cases as lc
from tests import test_txh_host as th
from tests import txhcases as tc
from tests import txpathcases as tp

TCP, UDP = 6, 17


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def d():
    return tp.load()


def _generator():
    path = os.path.join(os.path.dirname(tp.PATH), "make_txpath_ref.py")
    spec = importlib.util.spec_from_file_location("make_txpath_ref", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_vectors_are_what_the_reference_gives():
    """Where oracle/_ref is built, the generator's result in memory equals
    the committed file, text and all."""
    from oracle import orc
    if orc.ref_tcpout() is None or orc.ref_txip() is None:
        pytest.skip("oracle/_ref/libtcpout_ref.so or libcore_ref.so not built (no reference tree)")
    gen = _generator()
    fresh = gen.build()
    assert fresh == tp.load()
    with open(tp.PATH) as f:
        assert f.read() == gen.dumps(fresh)


def _l4sum(r, p):
    """the exact sum of the record's L4 bytes (sum field 0) as 16-bit words in memory order"""
    h = bytearray(bytes.fromhex(r["l4hdr_offload"]))
    fo = 16 if r["proto"] == TCP else 6
    h[fo:fo + 2] = b"\0\0"
    return lc.words(np.frombuffer(bytes(h) + p, dtype=np.uint8))


def test_fixture_holds_every_edge(d):
    """A regeneration cannot quietly lose a case the vectors exist for."""
    assert os.path.getsize(tp.PATH) <= 192 * 1024
    l4, pay = d["l4"], tp.payloads()
    tcp = [r for r in l4 if r["proto"] == TCP]
    udp = [r for r in l4 if r["proto"] == UDP]
    assert {0, 1, 2, 3, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 535, 536, 1459, 1460, 8960} \
        <= {r["paylen"] for r in tcp}
    assert {0, 1, 1471, 1472} <= {r["paylen"] for r in udp}
    assert all(r["off"] == 5 for r in tcp)
    edge = {0, 2 ** 32 - 1, 2 ** 31 - 1, 2 ** 31}
    assert edge <= {r["seq"] for r in tcp} and edge <= {r["ack"] for r in tcp}
    wire = {(r["win"] >> r["wscale"]) & 0xFFFF for r in tcp}
    assert {0, 0xFFFF} <= wire
    assert any(r["wscale"] == 0 for r in tcp) and any(r["wscale"] and r["win"] >> r["wscale"] for r in tcp)
    assert any(r["win"] >> r["wscale"] > 0xFFFF for r in tcp)      # the hton16 truncation
    assert {0x10, 0x18, 0xFF} <= {r["flags"] for r in tcp}
    assert any(14 + 20 + 20 + r["paylen"] == 65535 for r in tcp)
    # stored up to 1472 bytes; anything longer is the formula's
    assert all(("hex" in r) != ("gen" in r) and ("hex" in r or r["paylen"] > 0) for r in l4)
    assert all("hex" in r or r["paylen"] > 1472 or len(set(pay[i])) == 1 for i, r in enumerate(l4))
    assert "gen" in next(r for r in tcp if r["paylen"] == 65535 - 54)
    for proto in (TCP, UDP):
        mine = [(r, p) for r, p in zip(l4, pay) if r["proto"] == proto]
        assert any(p and set(p) == {0} for _, p in mine)
        assert any(set(p) == {0xFF} and len(p) & 1 for _, p in mine)
        assert any(set(p) == {0xFF} and not len(p) & 1 for _, p in mine)
        # the complemented sum is 0 and the reference returned 0xFFFF
        zr = [(r, p) for r, p in mine if r["cksum"] == 0xFFFF]
        assert zr, proto
        for r, p in zr:
            ph = r["phdr"]
            assert lc.fold(_l4sum(r, p) + ph) == 0xFFFF
    sums = {_l4sum(r, p) for r, p in zip(l4, pay)}
    assert {0x1FFFE, 0x2FFFE} <= sums       # one and two carries over 0xFFFE
    # ipv4_udptcp_cksum's own sum 0x1FFFE before its one carry
    assert any(lc.fold(_l4sum(r, p)) == 0xFFFF and r["phdr"] == 0xFFFF and r["cksum"] == 0xFFFF
               for r, p in zip(l4, pay))
    ips = d["ip"]
    assert {r["aux"][1] for r in ips if r["aux"] and r["aux"][0]} == set(range(256))
    assert any(r["aux"] is None for r in ips) and any(r["aux"] and not r["aux"][0] and r["aux"][1] & 3 for r in ips)
    assert any(r["lip"] == 0 and r["daddr"] == tc.LOOPBACK and r["saddr"] == tc.LOOPBACK for r in ips)
    assert any(r["lip"] == 0 and r["daddr"] != tc.LOOPBACK and r["saddr"] == d["net"]["addr"] for r in ips)
    assert "core.c:693-698" in d["source"] and "model only" in d["source"]
    for r in ips:       # no_tx_offloads both ways: the sum field is 0, or the recorded ipv4_cksum
        off, full = bytes.fromhex(r["hdr_offload"]), bytes.fromhex(r["hdr_full"])
        assert off[10:12] == b"\0\0" and full[:10] + full[12:] == off[:10] + off[12:]
        assert full[10] | full[11] << 8 == r["cksum"]
    rt = d["route"]
    assert {0, 0xFFFFFF00, 0xFFFFFFFF} <= {r["netmask"] for r in rt}
    for mask in (0xFFFFFF00, 0xFFFFFFFF):
        mine = [r for r in rt if r["netmask"] == mask]
        assert any(r["nh"] == r["daddr"] != r["gateway"] for r in mine), hex(mask)     # on the subnet
        assert any(r["nh"] == r["gateway"] != r["daddr"] for r in mine), hex(mask)     # off it
    assert any(r["daddr"] == r["gateway"] for r in rt)
    assert all(r["nh"] == r["daddr"] for r in rt if r["netmask"] == 0)


# --- the models -----------------------------------------------------------------

def test_model_tx_hdr_reproduces_the_reference_headers():
    for ip_csum in (False, True):
        case, expect = tp.txh_case(ip_csum)
        want = tc.model(case)
        tp.check_txh(case, expect, want["frames"], want, f"model ip_csum={ip_csum}")


def test_model_route_is_net_get_ip_route():
    for case, hops in tp.route_cases():
        want = tc.model(case)
        tp.check_route(case, hops, want["frames"], want, case["name"])


def test_model_pieces_are_the_chksum_routines(d):
    """raw_cksum and ipv4_phdr_cksum are the folds the two models are built from"""
    for r in d["raw"]:
        b = bytes.fromhex(r["buf"])
        assert lc.fold(lc.words(np.frombuffer(b, dtype=np.uint8))) == r["sum"], r
        s = tc.csum16(b)    # the same sum over big-endian words: the reference's value with its bytes swapped
        assert (s >> 8 | (s & 0xFF) << 8) == r["sum"], r
    for r in d["l4"]:
        hl = (20 if r["proto"] == TCP else 8) + r["paylen"]
        ph = r["lip"].to_bytes(4, "big") + r["rip"].to_bytes(4, "big") + bytes([0, r["proto"]]) + hl.to_bytes(2, "big")
        assert tc.csum16(ph).to_bytes(2, "big") == bytes([r["phdr"] & 0xFF, r["phdr"] >> 8]), r["name"]


@pytest.mark.parametrize("place", ["slots", "packed"])
def test_model_l4_fill_and_verify(place):
    frs = tp.l4_frames()
    case = tp.l4_slots(frs) if place == "slots" else tp.l4_packed(frs)
    st, _, frames = lc.model(case, lc.FILL)
    tp.check_filled(case, frames, st, f"model {place}")
    good = dict(case, frames=frames)
    st, _, _ = lc.model(good, lc.VERIFY)
    assert (st == lc.GOOD).all()
    st, _, _ = lc.model(case, lc.VERIFY)     # as left for the NIC: UDP carries no checksum
    udp = np.array([f[23] == UDP for f in frs])
    assert (st[udp] == lc.NONE).all()
    bad = tp.l4_packed(tp.flipped_frames())
    st, _, _ = lc.model(bad, lc.VERIFY)
    assert (st == lc.BAD).all()


# --- the host twins -----------------------------------------------------------------

def test_host_tx_hdr_reproduces_the_reference_headers(g):
    for ip_csum in (False, True):
        case, expect = tp.txh_case(ip_csum)
        got, buf, _ = th.run_host(g, case)
        tp.check_txh(case, expect, buf, got, f"host ip_csum={ip_csum}")


def test_host_route_is_net_get_ip_route(g):
    for case, hops in tp.route_cases():
        got, buf, _ = th.run_host(g, case)
        tp.check_route(case, hops, buf, got, case["name"])


def _host_l4(g, case, mode):
    fr = case["frames"].copy()
    st = g.l4_csum_host(fr, case["pkt_len"], mode=mode, stride=case["stride"], offs=case["offs"],
                        n=len(case["pkt_len"]))
    return st[:len(case["pkt_len"])], fr


@pytest.mark.parametrize("place", ["slots", "packed"])
def test_host_l4_fill_and_verify(g, place):
    frs = tp.l4_frames()
    case = tp.l4_slots(frs) if place == "slots" else tp.l4_packed(frs)
    st, frames = _host_l4(g, case, g.L4_FILL)
    tp.check_filled(case, frames, st, f"host {place}")
    st, _ = _host_l4(g, dict(case, frames=frames), g.L4_VERIFY)     # VERIFY over what FILL produced
    assert (st == g.L4_GOOD).all()
    # frames that carry the reference's own checksums, not ours
    ref = tp.l4_packed(tp.l4_frames(full=True))
    st, _ = _host_l4(g, ref, g.L4_VERIFY)
    assert (st == g.L4_GOOD).all()
    st, _ = _host_l4(g, case, g.L4_VERIFY)
    udp = np.array([f[23] == UDP for f in frs])
    assert (st[udp] == g.L4_NONE).all()
    st, _ = _host_l4(g, tp.l4_packed(tp.flipped_frames()), g.L4_VERIFY)
    assert (st == g.L4_BAD).all()


def test_host_rx_csum_flags_is_ipv4_cksum(g):
    from tests import csumcases as cc
    fr, good = tp.rx_frames()
    got = np.array([g.rx_csum_flags(f.tobytes(), 0) for f in fr])
    assert (got[good] == cc.GOOD).all() and (got[~good] == cc.BAD).all()
    assert good.sum() > 300 and (~good).sum() == 2 * good.sum()
