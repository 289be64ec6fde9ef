"""GPU: gcl_tcp_rx, gcl_tcp_rx_full and gcl_tcp_rx_ooo against what the
REFERENCE's own tcp_rx_conn did (tests/golden/tcprx_ref.json; the table of
tests/tcprxrefcases.py), over sentinel-filled outputs with guards, on every
recorded case: the named ones, a few segments each, and the recorded streams, a
few hundred.  Each call runs with the default launch and with its list cut
into one and into three ranges; the accepted bytes go through gcl_copy_batch on
the device and must be the reference's c->rxq."""
import numpy as np
import pytest
import torch

from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxfcases as fc
from tests import tcprxocases as oc
from tests import tcprxrefcases as rr

pytestmark = pytest.mark.gpu

SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
MODS = {"rx": rc, "full": fc, "ooo": oc}


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
        return torch.from_numpy(a.view(np.uint8).reshape(len(a), -1)).cuda()
    return torch.from_numpy(a.view(SIGNED.get(a.dtype, a.dtype))).cuda()


def blank_of(kind, case):
    m, nconn = fc.dims(case)
    return {"rx": lambda: rc.blank(m, nconn), "full": lambda: fc.blank(m, nconn), "ooo": lambda: oc.blank(case)}[kind]()


def run_gpu(g, clf, kind, case, blocks):
    """one call of @kind over sentinel-filled device outputs:
    (outputs as numpy with their guards, counts, the device buffers)"""
    m, nconn = fc.dims(case)
    n, order = len(case["pkt_len"]), case.get("order")
    blank = blank_of(kind, case)
    out = {f: dev(a) for f, a in blank.items()}
    frames = dev(case["frames"])
    plen = dev(case["pkt_len"]) if n else torch.zeros(1, dtype=torch.int16, device="cuda")
    offs = dev(case["offs"]) if case["offs"] is not None and n else None
    sock = dev(case["sock"]) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    nr = {"rx": g.TCPRXC_NR, "full": g.TCPRXFC_NR, "ooo": g.TCPRXOC_NR}[kind]
    cnt = torch.full((nr,), 5, dtype=torch.int64, device="cuda")
    kw = dict(stride=case["stride"] or 16 * (offs is None), offs=offs, frames_len=case["frames_len"],
              order=dev(order) if order is not None else None, m=m,
              l4_status=dev(case["st"]) if case.get("st") is not None else None, align=case.get("align", 0),
              blocks=blocks, out=out, counts=cnt)
    if kind != "rx":
        kw["rep_acks"] = dev(case["rep_acks"]) if case.get("rep_acks") is not None else None
    if kind == "ooo":
        z = oc.sizes(case)
        kw.update(q_off=dev(case["q_off"]) if case.get("q_off") is not None else None,
                  q=dev(case["q"]) if z["nq"] else None, nq=z["nq"], q_out_cap=z["cap"])
    call = {"rx": clf.tcp_rx, "full": clf.tcp_rx_full, "ooo": clf.tcp_rx_ooo}[kind]
    call(frames, n, plen, sock, dev(case["conn"]), nconn, **kw)
    torch.cuda.synchronize()
    got = {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    return got, cnt.cpu().numpy().view(np.uint64) - np.uint64(5), dict(out, frames=frames)


def guards(kind, got, case, what):
    """nothing written past an output's documented end"""
    m, nconn = fc.dims(case)
    z = dict(oc.sizes(case), nconn=nconn)
    size = {f: m for f, _ in rc.ENTRY}
    size.update(out_conn=nconn, conn_off=nconn + 1, out_ext=nconn)
    size.update({f: z[by] for f, _, by in oc.OOO_OUT})
    for f, a in got.items():
        k = size[f]
        assert len(a) == k + rc.GUARD and (a[k:].view(np.uint8) == rc.SENTINEL).all(), f"{what}: {f} past its end"


@pytest.mark.parametrize("blocks", [0, 1, 3])
@pytest.mark.parametrize("kind", rr.KINDS)
def test_kernels_give_what_the_reference_did(g, clf, kind, blocks):
    total = 0
    for name in rr.names():
        case = rr.case_of(name)
        got, cnt, _ = run_gpu(g, clf, kind, case, blocks)
        guards(kind, got, case, (kind, name, blocks))
        total += rr.check(rr.expected(kind, name), got, cnt, (kind, "gpu", name, blocks))
    assert total >= {"rx": 150, "full": 300, "ooo": 800}[kind]


@pytest.mark.parametrize("kind", rr.KINDS)
def test_copy_chain_gives_the_reference_rxq(g, clf, kind):
    """the call's device outputs straight into gcl_copy_batch (src_off + skip, copy_len, dst_off): per connection
    exactly the bytes of the mbufs the reference linked into c->rxq, in its order, up to the stop"""
    done = 0
    for name in rr.copy_cases():
        case = rr.case_of(name)
        e = rr.expected(kind, name)
        if not e.m:
            continue
        got, _, d = run_gpu(g, clf, kind, case, 1)
        pay = pc.model(case, case.get("order"), case["sock"], case.get("st"))
        src = dev(pay["src_off"].astype(np.uint64))
        if kind == "ooo":
            src = src + d["skip"][:e.m].view(torch.int16).to(torch.int64)
        total = int(got["conn_off"][e.nconn])
        if not total:
            assert not any(e.rxq) or not any(x[2] for r in e.rxq for x in r), (kind, name)
            continue
        rx = torch.full((total + 64,), rc.SENTINEL, dtype=torch.uint8, device="cuda")
        clf.copy_batch(d["frames"], src, d["copy_len"], e.m, rx[:total], dst_off=d["dst_off"], olflags=False, rss=False)
        torch.cuda.synchronize()
        rxh = rx.cpu().numpy()
        for k in range(e.nconn):
            want = rr.rxq_bytes(e, name, k)
            o = int(got["conn_off"][k])
            assert rxh[o:o + len(want)].tobytes() == want, (kind, name, k)
            done += len(want)
        assert (rxh[total:] == rc.SENTINEL).all()
    assert done > 10000
