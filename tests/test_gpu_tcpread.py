"""GPU: gcl_tcp_read (include/gclassify.h) against its host twin and the model of
tests/tcpreadcases.py, bit for bit over outputs and a workspace pre-filled with
0xFF, on the hand cases, on random batches at the wave and tile edges, with one
connection owning one tile, and one and two scan ranges, plus one entry, with
forced range counts, with and without vectors, with the caps one short, with
garbage CSR offsets; and chained: gcl_tcp_rx_ooo's accepted bytes as the queue,
the items through gcl_copy_batch, the ACKs through gcl_tx_hdr."""
import numpy as np
import pytest
import torch

from tests import tcpreadcases as T
from tests import txqcases as tq
from tests.test_gpu_tcprx import dev

pytestmark = pytest.mark.gpu

GUARD = 8
ITEM_DT = (("src_off", torch.int64), ("len", torch.int16), ("dst_off", torch.int64), ("item_conn", torch.int32),
           ("item_ent", torch.int32))
SEG_DT = (("frame_off", torch.int64), ("seg_conn", torch.int32), ("seg_kind", torch.uint8), ("seg_src", torch.int32))


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


def rec(a, width):
    return dev(a) if len(a) else torch.zeros((1, width), dtype=torch.uint8, device="cuda")


def ff(shape, dt):
    return torch.full(shape, -1, dtype=dt, device="cuda") if dt != torch.uint8 else \
        torch.full(shape, 0xFF, dtype=dt, device="cuda")


def run_gpu(g, clf, b, item_cap, seg_cap, blocks=0, frame_base=0, frame_stride=64, counts=None, calls=1):
    """@calls calls over 0xFF-filled outputs with GUARD elements behind each and
    a 0xFF-filled workspace: the outputs as numpy arrays, the guards checked"""
    whole = {f: ff((item_cap + GUARD,), dt) for f, dt in ITEM_DT}
    whole.update({f: ff((seg_cap + GUARD,), dt) for f, dt in SEG_DT})
    whole.update(desc=ff((seg_cap + GUARD, 32), torch.uint8), out_conn=ff((b.nconn + GUARD, 32), torch.uint8),
                 totals=ff((4 + GUARD,), torch.int64), seg_totals=ff((2 + GUARD,), torch.int64))
    ws = ff((g.tcp_read_workspace(b.nconn, b.nent, b.nvec, blocks) + 64,), torch.uint8)
    qoff, voff = dev(b.qoff), dev(b.voff) if b.use_voff else None
    ent, iov = rec(b.ent[:b.nent], 16), rec(b.iov[:b.nvec], 16) if b.use_voff else None
    rd, conn, addr = rec(b.rd[:b.nconn], 32), rec(b.conn[:b.nconn], 48), rec(b.addr[:b.nconn], 16)
    for _ in range(calls):
        clf.tcp_read(qoff, ent, b.nent, rd, conn, addr, b.nconn, item_cap, seg_cap, voff=voff, iov=iov, nvec=b.nvec,
                     frame_stride=frame_stride, frame_base=frame_base, blocks=blocks, out=whole, counts=counts,
                     workspace=ws)
    torch.cuda.synchronize()
    got = {f: t.cpu().numpy() for f, t in whole.items()}
    assert (got["out_conn"][b.nconn:] == 0xFF).all() and (got["totals"][4:] == -1).all()
    assert (got["seg_totals"][2:] == -1).all() and (ws[-64:] == 0xFF).all()
    k, s = int(got["totals"][1]), int(got["seg_totals"][1])
    assert k <= item_cap and s <= seg_cap
    for f, _ in ITEM_DT:       # nothing at or past totals[1] is written
        assert (got[f][k:] == -1).all(), f
    for f, _ in SEG_DT:
        assert (got[f][s:] == (0xFF if f == "seg_kind" else -1)).all(), f
    assert (got["desc"][s:] == 0xFF).all()
    return got


def check(g, clf, b, item_cap=None, seg_cap=None, blocks=0, frame_base=0, frame_stride=64, exp=None):
    """GPU == host twin == model"""
    item_cap = b.item_cap_enough() if item_cap is None else item_cap
    seg_cap = b.nconn if seg_cap is None else seg_cap
    cnt = torch.full((g.RDC_NR,), 5, dtype=torch.int64, device="cuda")
    got = run_gpu(g, clf, b, item_cap, seg_cap, blocks, frame_base, frame_stride, counts=cnt)
    cnt = cnt.cpu().numpy().view(np.uint64) - np.uint64(5)
    hcnt = np.zeros(g.RDC_NR, dtype=np.uint64)
    host = b.run_host(item_cap, seg_cap, frame_base, frame_stride, hcnt)
    k, s = int(host["totals"][1]), int(host["seg_totals"][1])
    assert got["out_conn"][:b.nconn].tobytes() == host["out_conn"][:b.nconn].tobytes()
    assert got["totals"][:4].tobytes() == host["totals"].tobytes()
    assert got["seg_totals"][:2].tobytes() == host["seg_totals"].tobytes()
    for f, _ in ITEM_DT:
        assert got[f][:k].tobytes() == host[f][:k].tobytes(), f
    for f in ("desc", "frame_off", "seg_conn", "seg_kind", "seg_src"):
        assert got[f][:s].tobytes() == host[f][:s].tobytes(), f
    assert cnt.tolist() == hcnt.tolist()
    T.check(b, got, exp if exp is not None else b.expect(item_cap, seg_cap, frame_base, frame_stride), cnt)
    return got


HAND = T.hand_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(g, clf, case):
    _, queues, reads, use_voff, want = case
    got = check(g, clf, T.Batch(queues, reads, use_voff))
    oc = got["out_conn"].view(g.RD_CONN_OUT_DTYPE).reshape(-1)
    for c, (status, ret, npop, pull, flags) in enumerate(want):
        o = oc[c]
        assert (o["status"], o["ret"], o["npop"], o["pull"], o["flags"]) == (status, ret, npop, pull, flags), (c, o)


@pytest.mark.parametrize("use_voff", [False, True])
@pytest.mark.parametrize("nconn", [1, 63, 64, 65, 257])
def test_wave_and_tile_edges(g, clf, nconn, use_voff):
    check(g, clf, T.random_batch(100 + nconn, nconn, use_voff), frame_base=1 << 33, frame_stride=128)


@pytest.mark.parametrize("use_voff", [False, True])
@pytest.mark.parametrize("blocks", [0, 1, 2, 7])
@pytest.mark.parametrize("owned", [T.G.RD_TILE + 1, 8 * T.G.RD_TILE + 1, 16 * T.G.RD_TILE + 1])
def test_one_connection_owns_the_entries(g, clf, owned, blocks, use_voff, memo={}):
    """257, 2049 and 4097 entries on connection 0: one tile, and with blocks 2 and 7 one and
    two ranges of the scans, plus one entry; two short queues behind it"""
    key = (owned, use_voff)
    if key not in memo:      # the model's answer once per shape
        b = T.random_batch(owned, 3, use_voff, one_owner=owned)
        memo[key] = (b, b.expect(b.item_cap_enough(), b.nconn))
    b, exp = memo[key]
    check(g, clf, b, blocks=blocks, exp=exp)


@pytest.mark.parametrize("blocks", [1, 2, 7])
def test_ranges_of_connections(g, clf, blocks):
    """five tiles of connections cut into 1, 2 and 7 ranges (two of the seven empty)"""
    check(g, clf, T.random_batch(9, 4 * T.G.RD_TILE + 3, True, maxq=3), blocks=blocks)


@pytest.mark.parametrize("use_voff", [False, True])
def test_caps_one_short_and_zero(g, clf, use_voff):
    b = T.random_batch(11, 120, use_voff)
    full = b.expect(b.item_cap_enough(), b.nconn)
    items, segs = int(full["totals"][0]), int(full["seg_totals"][0])
    got = check(g, clf, b, item_cap=items - 1, seg_cap=segs - 1)
    fl = got["out_conn"].view(g.RD_CONN_OUT_DTYPE).reshape(-1)["flags"][:b.nconn]
    assert np.count_nonzero(fl & g.RDO_ITEM_NOSPACE) == 1 and np.count_nonzero(fl & g.RDO_SEG_NOSPACE) == 1
    check(g, clf, b, item_cap=items // 2, seg_cap=0)
    check(g, clf, b, item_cap=0, seg_cap=segs // 2)


@pytest.mark.parametrize("use_voff", [False, True])
def test_bad_ranges(g, clf, use_voff):
    got = check(g, clf, T.bad_range_batch(use_voff))
    st = got["out_conn"].view(g.RD_CONN_OUT_DTYPE).reshape(-1)["status"][:5]
    assert st.tolist() == [g.RDS_DONE, g.RDS_BADRANGE, g.RDS_DONE, g.RDS_BADRANGE, g.RDS_BADRANGE]


def test_counts_accumulate_over_two_calls_and_no_connections(g, clf):
    b = T.random_batch(5, 70, True)
    cnt = torch.zeros(g.RDC_NR, dtype=torch.int64, device="cuda")
    run_gpu(g, clf, b, b.item_cap_enough(), b.nconn, counts=cnt, calls=2)
    assert np.array_equal(cnt.cpu().numpy().view(np.uint64), 2 * b.expect(b.item_cap_enough(), b.nconn)["counts"])
    got = run_gpu(g, clf, T.Batch([], [], True), 4, 4)
    assert not got["totals"][:4].any() and not got["seg_totals"][:2].any()


def test_refusals(g, clf):
    b = T.random_batch(3, 8, False)
    qoff, ent = dev(b.qoff), rec(b.ent[:b.nent], 16)
    rd, conn, addr = rec(b.rd[:b.nconn], 32), rec(b.conn[:b.nconn], 48), rec(b.addr[:b.nconn], 16)

    def call(**kw):
        a = dict(nconn=b.nconn, item_cap=64, seg_cap=8)
        a.update(kw)
        return clf.tcp_read(qoff, ent, b.nent, rd, conn, addr, a.pop("nconn"), a.pop("item_cap"), a.pop("seg_cap"), **a)

    call()
    small = torch.zeros(g.tcp_read_workspace(b.nconn, b.nent) - 1, dtype=torch.uint8, device="cuda")
    for kw in (dict(frame_stride=53), dict(blocks=1025), dict(workspace=small), dict(workspace=small[1:]),
               dict(item_cap=(1 << 31) + 1, out={f: torch.zeros(1 << 4, dtype=dt, device="cuda") for f, dt in ITEM_DT})):
        with pytest.raises((OSError, ValueError, RuntimeError)):
            call(**kw)
    torch.cuda.synchronize()


def test_chain_rx_ooo_read_copy_and_acks(g, clf):
    """gcl_tcp_rx_ooo accepts a shuffled stream; its dst_off / copy_len are the queue; gcl_tcp_read reads all
    of it into four vectors; gcl_copy_batch moves the items: the application's buffer holds the sent payload
    in sequence order; gcl_tx_hdr takes the window-update ACK"""
    from tests import tcprxocases as oc
    from tests.test_gpu_tcprxo import run_gpu as run_ooo, shuffled_stream
    case = shuffled_stream()
    m = oc.sizes(case)["m"]
    want = oc.model(case, with_rxq=True)
    stream = want["rxq"][0]
    total = len(stream)
    keep = {}
    run_ooo(g, clf, case, keep=keep)
    # the accepted bytes in sequence order, as gcl_copy_batch leaves them (tests/test_gpu_tcprxo.py)
    rx = dev(np.frombuffer(stream, dtype=np.uint8).copy())
    ln = keep["copy_len"][:m].view(torch.int16).to(torch.int64) & 0xFFFF
    off = keep["dst_off"][:m].view(torch.int64)
    live = torch.nonzero(ln > 0).reshape(-1)
    live = live[torch.argsort(off[live])]
    nent = int(live.numel())
    assert nent > 1 and int(ln[live].sum()) == total
    ent = torch.zeros((nent, 2), dtype=torch.int64, device="cuda")
    ent[:, 0], ent[:, 1] = off[live], ln[live]
    ent = ent.view(torch.uint8).reshape(nent, 16)
    cuts = [0, total // 3, total // 3, total - 100, total + 50]
    iov = np.zeros(4, dtype=g.RD_IOV_DTYPE)
    iov["len"] = np.diff(cuts)
    at = 16
    for v in (2, 0, 1, 3):      # apart, and out of order
        iov["off"][v] = at
        at += int(iov["len"][v]) + 16
    rdrec = np.zeros(1, dtype=g.TCP_RD_DTYPE)
    rdrec["flags"], rdrec["tx_last_ack"], rdrec["winmax"] = g.RD_WANT, 100, 4
    cn = np.zeros(1, dtype=g.TCP_CONN_DTYPE)
    cn["rcv_nxt"], cn["rcv_wnd"], cn["snd_nxt"] = 100 + total, 1000, 4242
    addr = np.zeros(1, dtype=g.TCP_ADDR_DTYPE)
    addr["lip"], addr["rip"], addr["lport"], addr["rport"] = tq.NET["addr"], tq.NET["addr"] + 1, 80, 5555
    out = clf.tcp_read(dev(np.array([0, nent], dtype=np.uint32)), ent, nent, dev(rdrec), dev(cn), dev(addr), 1,
                       nent + 4, 1, voff=dev(np.array([0, 4], dtype=np.uint32)), iov=dev(iov), nvec=4)
    app = torch.zeros(2 * total + 400, dtype=torch.uint8, device="cuda")
    k = nent + 4 - 1     # ne + nv - 1: the stream ends inside the fourth vector
    clf.copy_batch(rx, out["src_off"], out["len"], k, app, dst_off=out["dst_off"], olflags=False, rss=False)
    frames = torch.zeros(256, dtype=torch.uint8, device="cuda")
    net = g.txh_net(tq.NET["addr"], tq.NET["netmask"], tq.NET["gateway"], tq.NET["mac"])
    hdr = clf.tx_hdr(out["desc"], out["frame_off"], 1, frames, net)
    torch.cuda.synchronize()
    oc_ = out["out_conn"].cpu().numpy().view(g.RD_CONN_OUT_DTYPE).reshape(-1)[0]
    assert (oc_["status"], oc_["ret"], oc_["npop"], oc_["pull"]) == (g.RDS_DONE, total, nent, 0)
    assert oc_["flags"] == g.RDO_ACK | g.RDO_POLLIN_CLEAR and oc_["rcv_wnd"] == 1000 + total
    assert out["totals"].cpu().numpy().tolist() == [k, k, total, total]
    assert out["seg_totals"].cpu().numpy().tolist() == [1, 1]
    apph = app.cpu().numpy()
    got = b"".join(apph[o:o + n].tobytes() for o, n in zip(iov["off"].tolist(), iov["len"].tolist()))
    assert got[:total] == stream and not any(got[total:])
    assert int(hdr["status"].cpu().numpy()[0]) != g.TXH_REFUSED
    d = out["desc"].cpu().numpy().view(g.TXH_DESC_DTYPE).reshape(-1)[0]
    assert (d["seq"], d["ack"], d["win"], d["tcp_flags"]) == (4242, (100 + total) & T.M32, (1000 + total) & 0xFFFF, 0x10)
