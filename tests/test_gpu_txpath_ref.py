"""GPU: gcl_tx_hdr, gcl_l4_csum and gcl_rx_csum against bytes the REFERENCE's
own code produced (tests/golden/txpath_ref.json: runtime/net/tcp_out.c,
inc/net/chksum.h and runtime/net/core.c compiled in place, recorded by
tests/golden/make_txpath_ref.py).  Only tests/golden is read; the vectors and
the checks are those of tests/test_txpath_ref.py (tests/txpathcases.py), so a
kernel is held to the reference directly and not through the model or its
host twin.  Every test is one to three launches over a few hundred frames."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # before the package's library, as in tests/test_gpu_txh.py

from tests import l4cases as lc  # noqa: E402
from tests import txhcases as tc  # noqa: E402
from tests import txpathcases as tp  # noqa: E402

pytestmark = pytest.mark.gpu

UDP = 17
CANARY = 64


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def clf(g):
    c = g.Classifier(0, 16, g.HASH_NIC, 0, 0x01)
    yield c
    c.close()


def dev(a):
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
    return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()


def run_txh(g, clf, case):
    """(the outputs, the frame region from its front guard on)"""
    m, flen = len(case["desc"]), case["frames_len"]
    clf.neigh_set(case["neigh"])
    buf = torch.full((tc.GUARD + flen + tc.GUARD,), tc.SENTINEL, dtype=torch.uint8, device="cuda")
    desc = torch.from_numpy(case["desc"].view(np.uint8).reshape(-1, 32)).cuda()
    out = clf.tx_hdr(desc, dev(case["frame_off"]), m, buf[tc.GUARD:], g.txh_net(**case["net"]), frames_len=flen,
                     shm_base=case["shm_base"], cap=case["cap"])
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:tc.GUARD] == tc.SENTINEL).all() and (host[tc.GUARD + flen:] == tc.SENTINEL).all()
    return {"status": out["status"].cpu().numpy()[:m]}, host


@pytest.mark.parametrize("ip_csum", [False, True])
def test_tx_hdr_writes_the_reference_headers(g, clf, ip_csum):
    """Bytes 14..53 (TCP) or 14..41 (UDP) of every frame are net_push_iphdr's
    header followed by tcp_push_tcphdr's (UDP: the four fields of
    udp_send_raw), without and with GCL_TXH_IP_CSUM (netcfg.no_tx_offloads);
    the destination mac is that of net_get_ip_route's next hop."""
    case, expect = tp.txh_case(ip_csum)
    out, buf = run_txh(g, clf, case)
    tp.check_txh(case, expect, buf, out, f"gpu ip_csum={ip_csum}")


def test_tx_hdr_routes_as_net_get_ip_route(g, clf):
    for case, hops in tp.route_cases():
        out, buf = run_txh(g, clf, case)
        tp.check_route(case, hops, buf, out, case["name"])


def run_l4(clf, case, mode):
    """(status, the region after the call); guard bands and the status tail checked"""
    n, flen = len(case["pkt_len"]), case["frames_len"]
    host = np.full(flen + 2 * lc.GUARD, lc.FILLBYTE, dtype=np.uint8)
    host[lc.GUARD:lc.GUARD + flen] = case["frames"][:flen]
    buf = torch.from_numpy(host).cuda()
    st = torch.full((n + CANARY,), 0x77, dtype=torch.uint8, device="cuda")
    clf.l4_csum(buf[lc.GUARD:lc.GUARD + flen], n, dev(case["pkt_len"]), mode=mode, stride=case["stride"],
                offs=dev(case["offs"]) if case["offs"] is not None else None, status=st)
    torch.cuda.synchronize()
    got, st = buf.cpu().numpy(), st.cpu().numpy()
    assert (got[:lc.GUARD] == lc.FILLBYTE).all() and (got[lc.GUARD + flen:] == lc.FILLBYTE).all()
    assert (st[n:] == 0x77).all()
    return st[:n], got[lc.GUARD:lc.GUARD + flen]


@pytest.mark.parametrize("place", ["slots", "packed"])
def test_l4_fill_writes_the_reference_checksums(g, clf, place):
    """GCL_L4_FILL over the frames as net_tx_ip leaves them for the NIC: the
    sum field is the reference's ipv4_udptcp_cksum, the TCP header as a whole
    its no_tx_offloads = 1 header and the IP header net_push_iphdr's with
    ipv4_cksum; in slots, and packed with frame i at an offset that is i mod
    16 (every alignment of the wide loads, the 65535-byte segment included).
    VERIFY over the result is GOOD."""
    frs = tp.l4_frames()
    case = tp.l4_slots(frs) if place == "slots" else tp.l4_packed(frs)
    st, frames = run_l4(clf, case, g.L4_FILL)
    tp.check_filled(case, frames, st, f"gpu {place}")
    st, after = run_l4(clf, dict(case, frames=frames), g.L4_VERIFY)
    assert (st == g.L4_GOOD).all() and np.array_equal(after, frames)


def test_l4_verify_judges_the_reference_checksums(g, clf):
    """Frames carrying the reference's own checksums are GOOD; with one bit
    flipped in the first, a middle or the last covered byte BAD (a one-bit
    change is never a multiple of 0xFFFF); a UDP datagram as udp_send_raw
    leaves it, the field 0, is NONE."""
    ref = tp.l4_frames(full=True)
    st, _ = run_l4(clf, tp.l4_packed(ref), g.L4_VERIFY)
    assert (st == g.L4_GOOD).all()
    st, _ = run_l4(clf, tp.l4_packed(tp.flipped_frames()), g.L4_VERIFY)
    assert len(st) == 3 * len(ref) and (st == g.L4_BAD).all()
    frs = tp.l4_frames()
    st, _ = run_l4(clf, tp.l4_packed(frs), g.L4_VERIFY)
    udp = np.array([f[23] == UDP for f in frs])
    assert udp.sum() >= 10 and (st[udp] == g.L4_NONE).all()


def test_rx_csum_accepts_ipv4_cksum(g, clf):
    """IPv4 headers carrying the reference's ipv4_cksum resolve to good, and
    with one bit flipped, in the header or in the sum itself, to bad."""
    from tests import csumcases as cc
    fr, good = tp.rx_frames()
    n = len(fr)
    out = torch.full((n + CANARY,), 0x5A, dtype=torch.uint8, device="cuda")
    clf.rx_csum(dev(fr.reshape(-1)), n, 64, olflags_out=out, olflags=torch.zeros(n, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == 0x5A).all()
    assert (got[:n][good] == cc.GOOD).all() and (got[:n][~good] == cc.BAD).all()
