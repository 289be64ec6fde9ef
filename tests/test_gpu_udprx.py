"""GPU: gcl_udp_rx (include/gclassify.h) against its host twin, byte for byte
over sentinel-filled outputs with guards, and the twin against the independent
model of tests/udprxcases.py: the hand-derived cases, random lists of 1, 63, 64,
65 and 4097 entries, 1, 3, 64 and 1024 ranges so that a socket's room runs out
across a wave boundary and across a range boundary, 1, 2048 and 2049 sockets
(one and two grouping passes), 2^20 sockets, one socket taking everything, a
0xFF-filled workspace, the same list twice, and the chain through
gcl_l4_payload and gcl_copy_batch."""
import numpy as np
import pytest
import torch

from tests import udprxcases as uc

pytestmark = pytest.mark.gpu

SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
HAND = uc.hand_cases()


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


def run_gpu(g, clf, c, blocks=0, counts=True, keep=None, ws_fill=None):
    """one call over sentinel-filled device outputs: (outputs as numpy, the counts it added)"""
    blank = uc.blank(c)
    out = {f: dev(a) for f, a in blank.items()}
    n, m, ns = c["n"], c["m"], len(c["usock"])
    one32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    cnt = torch.full((uc.C_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    ws = None
    if ws_fill is not None:
        ws = torch.full((g.udp_rx_workspace(m, ns, blocks),), ws_fill, dtype=torch.uint8, device="cuda")
    clf.udp_rx(dev(c["frames"]), n, dev(c["pkt_len"]), dev(c["sock"]) if n else one32,
               dev(c["usock"]) if ns else None, ns, offs=dev(c["offs"]) if n else None,
               order=None if c["order"] is None else dev(c["order"]), m=m,
               l4_status=None if c["l4_status"] is None else dev(c["l4_status"]), sock_base=c["sock_base"],
               align=c["align"], blocks=blocks, out=out, counts=cnt, workspace=ws)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(out)
    got = {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    return got, None if cnt is None else (cnt.cpu().numpy().view(np.uint64) - np.uint64(5)).tolist()


def check(g, clf, c, what, model=True, **kw):
    """GPU == host twin, every byte of every output with its guards, and the counts; then the twin == the model"""
    hgot, hcnt = uc.run_host(g, c)
    got, cnt = run_gpu(g, clf, c, **kw)
    uc.same(got, hgot, what)
    assert cnt == hcnt, (what, cnt, hcnt)
    if model:
        uc.check_model(c, hgot, hcnt, what)
    return got


@pytest.mark.parametrize("blocks", [0, 1, 3])
def test_hand_cases(g, clf, blocks):
    for name in sorted(HAND):
        c, want = HAND[name]
        got = check(g, clf, c, (name, blocks), blocks=blocks)
        uc.check_hand(c, want, got, name)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("blocks", [1, 3, 64])
def test_random_lists(g, clf, m, blocks):
    for seed in (20, 21):
        c = uc.random_case(seed + m, m, nsock=1 + (seed + m) % 7, lead=(seed + m) % 4,
                           sock_base=0 if seed == 21 else uc.SOCK_BASE)
        check(g, clf, c, (m, blocks, seed), blocks=blocks)


def test_max_blocks(g, clf):
    check(g, clf, uc.random_case(33, 4097, nsock=6), "max blocks", blocks=g.UDPRX_MAX_BLOCKS)


def test_order_null_and_counts_null(g, clf):
    c = uc.random_case(31, 700, with_order=False)
    hgot, _ = uc.run_host(g, c, counts=False)
    got, _ = run_gpu(g, clf, c, counts=False, blocks=3)
    uc.same(got, hgot, "identity order")


@pytest.mark.parametrize("nsock", [1, 2048, 2049])
def test_one_and_two_grouping_passes(g, clf, nsock):
    """room 2 everywhere; the sockets either side of the pass boundary and a crowd on the last one"""
    c = uc.random_case(50 + nsock, 4097, nsock=nsock, caps=2)
    hot = [0, nsock - 1, min(2047, nsock - 1), nsock // 2]
    c["sock"][:400] = [uc.SOCK_BASE + hot[x % 4] for x in range(400)]
    got = check(g, clf, c, ("nsock", nsock), blocks=3)
    assert (got["verdict"][:4097] == uc.FULL).any() and (got["verdict"][:4097] == uc.QUEUED).any()


def test_two_to_the_twenty_sockets(g, clf):
    ns = 1 << 20
    cookies = [0, ns - 1, 2047, 2048, ns - 1, 0, 0, 123456, ns, ns - 1, 2048]
    pk = [(uc.frame(3 + x, rport=7000 + x), uc.SOCK_BASE + s) for x, s in enumerate(cookies)]
    c = uc.case(pk, [uc.usock(0, 2)])
    us = np.zeros(ns, dtype=uc.USOCK)
    us["inq_cap"] = 2
    c["usock"] = us
    got = check(g, clf, c, "2^20 sockets", model=False)
    Q, F, N = uc.QUEUED, uc.FULL, uc.NOSOCK
    assert got["verdict"][:11].tolist() == [Q, Q, Q, Q, Q, Q, F, Q, N, F, Q]
    # socket order: 0 (x2), 2047, 2048 (x2), 123456, ns - 1 (x2)
    assert got["rec_idx"][:11].tolist() == [0, 6, 2, 3, 7, 1, uc.NONE, 5, uc.NONE, uc.NONE, 4]
    assert got["rec_off"][[0, 1, 2047, 2048, 2049, 123456, 123457, ns - 1, ns]].tolist() == [0, 2, 2, 3, 5, 5, 6, 6, 8]
    assert int(got["sock_off"][ns]) == sum(3 + x for x in (0, 1, 2, 3, 4, 5, 7, 10))


@pytest.mark.parametrize("room", [0, 1, 64, 65, 4097])
def test_one_socket_takes_everything(g, clf, room):
    """4097 datagrams on one socket beside a quiet one: the room runs out at a lane, a wave and a tile boundary"""
    pk = [(uc.frame(1 + x % 50, rport=1 + x), uc.S1) for x in range(4097)]
    c = uc.case(pk, [uc.usock(0, 9), uc.usock(-1, room - 1), uc.usock(1, 1)], align=4)
    for blocks in (0, 3, 64):
        got = check(g, clf, c, ("one socket", room, blocks), blocks=blocks)
        v = got["verdict"][:4097]
        assert (v[:room] == uc.QUEUED).all() and (v[room:] == uc.FULL).all()
        assert got["sflags"][:4097].tolist() == [0, uc.POLLIN][:room][:2] + [0] * (4097 - min(room, 2))
        o = got["out_sock"][1]
        assert (int(o["inq_len"]), int(o["ntaken"]), int(o["ndropped"])) == (room - 1, room, 4097 - room)


def test_ff_filled_workspace(g, clf):
    c = uc.random_case(61, 4097, nsock=2049, caps=1)
    hgot, hcnt = uc.run_host(g, c)
    got, cnt = run_gpu(g, clf, c, blocks=3, ws_fill=0xFF)
    uc.same(got, hgot, "0xFF workspace")
    assert cnt == hcnt
    c = uc.case([], [uc.usock(3, 9)])
    got, _ = run_gpu(g, clf, c, ws_fill=0xFF)
    uc.same(got, uc.run_host(g, c)[0], "0xFF workspace, m == 0")


def test_same_list_twice_gives_identical_bytes_and_doubled_counts(g, clf):
    c = uc.random_case(41, 4097, nsock=9)
    a, ca = run_gpu(g, clf, c, blocks=64)
    b, cb = run_gpu(g, clf, c, blocks=64)
    uc.same(a, b, "twice")
    assert ca == cb
    cnt = torch.zeros(uc.C_NR, dtype=torch.int64, device="cuda")
    for _ in range(2):
        clf.udp_rx(dev(c["frames"]), c["n"], dev(c["pkt_len"]), dev(c["sock"]), dev(c["usock"]), len(c["usock"]),
                   offs=dev(c["offs"]), order=dev(c["order"]), m=c["m"],
                   l4_status=None if c["l4_status"] is None else dev(c["l4_status"]), sock_base=c["sock_base"],
                   align=c["align"], counts=cnt)
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == [2 * x for x in ca]


def test_blocks_1_against_64(g, clf):
    c = uc.random_case(43, 4097, nsock=2049)
    a, ca = run_gpu(g, clf, c, blocks=1)
    b, cb = run_gpu(g, clf, c, blocks=64)
    uc.same(a, b, "blocks 1 against 64")
    assert ca == cb


def test_chain_payload_rx_copy(g, clf):
    """gcl_l4_payload -> gcl_udp_rx -> gcl_copy_batch on the device == the host twins in the same order"""
    c = uc.chain_case()
    hout, hdst, _ = uc.host_chain(g, c)
    n, ns = c["n"], len(c["usock"])
    fr, plen, sock, offs = dev(c["frames"]), dev(c["pkt_len"]), dev(c["sock"]), dev(c["offs"])
    pay = clf.l4_payload(fr, n, plen, offs=offs, sock=sock, align=c["align"])
    keep = {}
    got, _ = run_gpu(g, clf, c, keep=keep)
    uc.same(got, hout, "chain")
    dst = torch.full((len(hdst),), uc.SENTINEL, dtype=torch.uint8, device="cuda")
    total = int(got["sock_off"][ns])
    clf.copy_batch(fr, pay["src_off"], keep["copy_len"], n, dst[:total], dst_off=keep["dst_off"], olflags=False,
                   rss=False)
    torch.cuda.synchronize()
    assert dst.cpu().numpy().tobytes() == hdst.tobytes()
