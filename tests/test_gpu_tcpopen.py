"""GPU: gcl_tcp_rx_open (include/gclassify.h) against its host twin, byte for
byte over sentinel-filled outputs with guards (open[], the segment arrays, the
tx region), and against the independent model of tests/tcpopencases.py: the
hand-derived cases, random lists of 1, 63, 64, 65 and 4097 entries, 1, 3 and 64
ranges so that duplicates, the backlog running out and the emit scan cross
range boundaries, the tuple table at its minimum and at the library's choice,
order given and NULL, misaligned frames, one listener taking everything, 4096
listeners, the same list twice, and the chain into gcl_tx_hdr and gcl_l4_csum."""
import numpy as np
import pytest
import torch

from tests import tcpopencases as oc

pytestmark = pytest.mark.gpu

SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
HAND = oc.hand_cases()


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def clf(g):
    c = g.Classifier(0, 16, g.HASH_JENKINS)
    yield c
    c.close()


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        return torch.from_numpy(a.view(np.uint8).reshape(len(a), -1).copy()).cuda()
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype)).copy()).cuda()


def run_gpu(g, clf, c, blocks=0, counts=True, keep=None):
    """one call over sentinel-filled device outputs: (outputs as numpy, the counts it added)"""
    blank = oc.blank(c)
    out = {f: dev(a) for f, a in blank.items()}
    n, m, nl = c["n"], c["m"], len(c["listen"])
    one32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.full((oc.C_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    res = {k: v for k, v in out.items() if k != "tx_all"}
    clf.tcp_rx_open(dev(c["frames"]), n, dev(c["pkt_len"]), dev(c["sock"]) if n else one32, m,
                    dev(c["listen"]) if nl else None, nl, dev(c["iss"]), c["seg_cap"], c["open_cap"],
                    out["tx_all"][64:], offs=dev(c["offs"]) if n else None,
                    order=None if c["order"] is None else dev(c["order"]),
                    l4_status=None if c["l4_status"] is None else dev(c["l4_status"]), listen_base=oc.LISTEN_BASE,
                    frame_stride=oc.TX_STRIDE, frame_base=oc.TX_BASE, tx_frames_len=c["tx_len"], blocks=blocks,
                    hash_slots=c["hash_slots"], out=res, counts=cnt)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(out)
    got = {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    return got, None if cnt is None else (cnt.cpu().numpy().view(np.uint64) - np.uint64(5)).tolist()


def check(g, clf, c, what, **kw):
    """GPU == host twin, every byte of every output with its guards, and the counts; then the model"""
    hgot, hcnt = oc.run_host(g, c)
    got, cnt = run_gpu(g, clf, c, **kw)
    oc.same(got, hgot, what)
    assert cnt == hcnt, (what, cnt, hcnt)
    oc.check_model(c, got, cnt, what)
    return got


@pytest.mark.parametrize("blocks", [0, 1, 3])
def test_hand_cases(g, clf, blocks):
    for name in sorted(HAND):
        c, verdicts = HAND[name]
        got = check(g, clf, c, (name, blocks), blocks=blocks)
        assert got["verdict"][:c["m"]].tolist() == verdicts, name


@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("blocks", [1, 3, 64])
def test_random_lists(g, clf, m, blocks):
    for seed in (20, 21):
        c = oc.random_case(seed + m, m, nlisten=1 + (seed + m) % 5, lead=(seed + m) % 4, caps=seed == 21,
                           hash_slots=0 if seed == 20 else max(2, 1 << (2 * m - 1).bit_length()))
        check(g, clf, c, (m, blocks, seed), blocks=blocks)


def test_order_null_and_counts_null(g, clf):
    c = oc.random_case(31, 700, with_order=False)
    hgot, _ = oc.run_host(g, c, counts=False)
    got, _ = run_gpu(g, clf, c, counts=False, blocks=3)
    oc.same(got, hgot, "identity order")


@pytest.mark.parametrize("blocks", [0, 3, 64])
def test_one_listener_takes_everything(g, clf, blocks):
    """2000 SYNs of 1500 tuples on one listener whose backlog runs out at 1000: ACCEPT, LATER and FULL all cross
    the range boundaries"""
    pk = [(oc.syn(rport=1 + (x * 7) % 1500, opts=oc.MSS), oc.L0) for x in range(2000)]
    c = oc.case(pk, [oc.listener(backlog=1000)])
    got = check(g, clf, c, ("one listener", blocks), blocks=blocks)
    v = got["verdict"][:2000].tolist()
    assert (v.count(oc.ACCEPT), v.count(oc.LATER), v.count(oc.FULL)) == (1000, 500, 500)
    assert int(got["backlog_out"][0]) == 0


@pytest.mark.parametrize("blocks", [0, 3])
def test_4096_listeners(g, clf, blocks):
    nl = 4096
    pk = [(oc.syn(rport=1 + x % 3000, lport=1 + (x * 5) % nl), oc.LISTEN_BASE + (x * 5) % nl) for x in range(6000)]
    lq = [oc.listener(backlog=x % 3) for x in range(nl)]
    got = check(g, clf, oc.case(pk, lq), ("4096 listeners", blocks), blocks=blocks)
    assert sum(got["backlog_out"][:nl].tolist()) < sum(x % 3 for x in range(nl))


def test_same_list_twice_gives_identical_bytes(g, clf):
    c = oc.random_case(41, 4097, nlisten=3, hash_slots=1 << 14)
    a, _ = run_gpu(g, clf, c, blocks=64)
    b, _ = run_gpu(g, clf, c, blocks=64)
    oc.same(a, b, "twice")


def test_m_zero_is_a_noop(g, clf):
    c = oc.case([], [oc.listener()])
    got, cnt = run_gpu(g, clf, c)
    assert cnt == [0] * oc.C_NR
    for f, a in got.items():
        assert (a.view(np.uint8) == oc.SENTINEL).all(), f


def test_chain_into_tx_hdr_and_fill(g, clf):
    """gcl_tcp_rx_open -> gcl_tx_hdr -> gcl_l4_csum FILL on the device == the host twins in the same order"""
    c = oc.chain_case()
    hout, hhdr, hst = oc.host_chain(g, c)
    keep = {}
    got, _ = run_gpu(g, clf, c, keep=keep)
    k = int(got["seg_totals"][1])
    assert k == int(hout["seg_totals"][1]) == 4
    clf.neigh_set([(oc.RIP, oc.MAC_R)])
    # a view, not a raw address: tx_hdr and l4_csum allocate their outputs on the device of @frames
    txp, txl = keep["tx_all"][64:], c["tx_len"]
    assert txp.is_cuda
    hdr = clf.tx_hdr(keep["desc"], keep["frame_off"], k, txp, oc.net_of(g), frames_len=txl)
    assert all(v.is_cuda for v in hdr.values())
    st = clf.l4_csum(txp, k, hdr["pkt_len"], mode=g.L4_FILL, offs=keep["frame_off"], frames_len=txl,
                     tx_olflags=hdr["tx_olflags"], status=torch.zeros(k, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    clf.neigh_set([])
    assert keep["tx_all"].cpu().numpy().tobytes() == hout["tx_all"].tobytes()
    assert hdr["pkt_len"][:k].cpu().numpy().view(np.uint16).tolist() == hhdr["pkt_len"][:k].tolist()
    assert st[:k].cpu().numpy().tolist() == hst[:k].tolist()
