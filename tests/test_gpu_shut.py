"""GPU: gcl_tcp_shut (include/gclassify.h) against its host twin and the model of
tests/shutcases.py, bit for bit over 0xFF-filled outputs with guard elements
behind each and a 0xFF-filled workspace: the enumeration, random batches,
everybody / nobody / only the last connection wanting a segment, sizes around
the wave, the block and the grid, in->blocks 0..3, each cap one short, garbage
requests, every refusal of the device entry with its workspace checks, the
workspace reused by a second call, and chained through gcl_tx_hdr
and gcl_l4_csum FILL against the host chain and the reference's FIN header
bytes (tests/golden/tcpfin_ref.json)."""
import numpy as np
import pytest
import torch

from tests import shutcases as T
from tests.test_gpu_tcprx import dev

pytestmark = pytest.mark.gpu

GUARD = 8
SEG_DT = (("desc", torch.uint8, 32), ("frame_off", torch.int64, 0), ("seg_conn", torch.int32, 0),
          ("seg_kind", torch.uint8, 0), ("seg_src", torch.int32, 0), ("txq_ent", torch.uint8, 16),
          ("txq_cold", torch.uint8, 16))


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


def ff(n, dt, width=0):
    shape = (n, width) if width else (n,)
    return torch.full(shape, 0xFF if dt == torch.uint8 else -1, dtype=dt, device="cuda")


def run_gpu(g, clf, b, seg_cap, blocks=0, counts=None, calls=1, **kw):
    """@calls calls over 0xFF-filled outputs with GUARD elements behind each and a 0xFF-filled
    workspace with 64 bytes behind it: the outputs as numpy arrays"""
    whole = {f: ff(seg_cap + GUARD, dt, w) for f, dt, w in SEG_DT}
    whole.update(out_conn=ff(b.nconn + GUARD, torch.uint8, 48), totals=ff(2 + GUARD, torch.int64))
    need = g.tcp_shut_workspace(b.nconn, blocks)
    ws = ff(need + 64, torch.uint8)
    shut, tmr = rec(b.shut, 16), rec(b.tmr, 64)
    conn, addr = rec(b.conn, 48), rec(b.addr, 16)
    for _ in range(calls):
        clf.tcp_shut(T.NOW, shut, tmr, conn, addr, b.nconn, seg_cap, blocks=blocks, out=whole, counts=counts,
                     workspace=ws[:need], **kw)
    torch.cuda.synchronize()
    assert (ws[need:] == 0xFF).all()
    return {f: t.cpu().numpy() for f, t in whole.items()}


def check(g, clf, b, seg_cap=None, blocks=0, exp=None, model=True, calls=1, **kw):
    """GPU == host twin (== model), every output byte, guards intact"""
    seg_cap = b.nconn if seg_cap is None else seg_cap
    cnt = torch.full((g.SHUTC_NR,), 5, dtype=torch.int64, device="cuda")
    got = run_gpu(g, clf, b, seg_cap, blocks, counts=cnt, calls=calls, **kw)
    cnt = (cnt.cpu().numpy().view(np.uint64) - np.uint64(5)) // np.uint64(calls)
    hcnt = np.zeros(g.SHUTC_NR, dtype=np.uint64)
    host = b.run_host(seg_cap, counts=hcnt, guard=GUARD, **kw)
    for f in ("out_conn", "totals") + g.SHUT_SEG_FIELDS:
        assert T.raw(got[f], got[f].nbytes) == T.raw(host[f], got[f].nbytes), f    # guards and all
    assert cnt.tolist() == hcnt.tolist()
    if model:
        T.check(b, got, exp if exp is not None else b.expect(seg_cap, **kw), cnt, seg_cap=seg_cap, guard=GUARD)
    return np.frombuffer(T.raw(got["out_conn"], 48 * b.nconn), dtype=g.SHUT_CONN_OUT_DTYPE), got


def test_enumeration(g, clf):
    b = T.enumeration()
    exp = b.expect(b.nconn, frame_base=1 << 33, frame_stride=1536)
    for blocks in (0, 1, 2, 3):
        check(g, clf, b, blocks=blocks, exp=exp, frame_base=1 << 33, frame_stride=1536)


@pytest.mark.parametrize("case", T.NAMED, ids=[c.__name__ for c in T.NAMED])
def test_named_cases(g, clf, case):
    c, want = case()
    oc, _ = check(g, clf, T.Batch([T.conn(), c, T.conn()]), 3)
    for f, v in want.items():
        assert oc[1][f] == v, (f, oc[1])


@pytest.fixture(scope="module")
def random_batches():
    """seed -> (batch, the model's answer): computed once, shared by the cases, left unchanged"""
    res = {}
    for seed in (1, 2):
        b = T.random_batch(seed, 5000)
        res[seed] = (b, b.expect(5000, frame_base=4096, frame_stride=128))
    return res


@pytest.mark.parametrize("blocks", [0, 1, 2, 3])
@pytest.mark.parametrize("seed", [1, 2])
def test_random(g, clf, random_batches, seed, blocks):
    b, exp = random_batches[seed]
    check(g, clf, b, blocks=blocks, exp=exp, frame_base=4096, frame_stride=128)


SIZES = sorted({0, 1, 63, 64, 65, T.G.SHUT_TILE - 1, T.G.SHUT_TILE, T.G.SHUT_TILE + 1} |
               {k * T.G.SHUT_TILE + d for k in (2, 3) for d in (-1, 0, 1)})


@pytest.mark.parametrize("mix", ["mixed", "all", "none", "last"])
def test_sizes_around_wave_block_and_grid(g, clf, mix):
    """nconn 0, 1, one below / at / above the wave, the block, and blocks x block for 1, 2 and 3 blocks"""
    for nconn in SIZES:
        b = T.random_batch(100 + nconn, nconn, mix=mix)
        exp = b.expect(nconn)
        want = {"all": nconn, "none": 0, "last": min(nconn, 1)}.get(mix)
        assert want is None or int(exp["totals"][0]) == want
        for blocks in (0, 1, 2, 3):
            check(g, clf, b, blocks=blocks, exp=exp)


@pytest.mark.parametrize("how", ["seg_cap", "frames_len"])
def test_cap_one_short(g, clf, how):
    b = T.random_batch(4, 700)
    full, _ = check(g, clf, b)
    wanted = int((full["nseg"] == 1).sum())
    kw = dict(seg_cap=wanted - 1) if how == "seg_cap" else \
        dict(seg_cap=wanted, frame_base=640, frame_stride=96, frames_len=640 + 96 * wanted - 1)
    for blocks in (0, 3):
        oc, got = check(g, clf, b, blocks=blocks, **kw)
        assert got["totals"][:2].tolist() == [wanted, wanted - 1]
        last = np.flatnonzero(full["nseg"] == 1)[-1]
        assert np.flatnonzero(oc["status"] == g.SHUTS_NOSPACE).tolist() == [last]
        assert (oc[last]["snd_nxt"], oc[last]["state"], oc[last]["flags"]) == \
            (b.conn[last]["snd_nxt"], b.tmr[last]["state"], 0)
    check(g, clf, b, 0)                                          # no room at all
    check(g, clf, b, wanted // 2, blocks=2)
    check(g, clf, b, wanted, frame_base=4096, frames_len=100)    # frames_len below frame_base


def test_garbage_requests(g, clf):
    """states up to 255, random op, flag and how bytes: what the twin says, guards intact"""
    for seed, nconn, blocks in ((9, 5000, 0), (10, 777, 3)):
        check(g, clf, T.random_batch(seed, nconn, garbage=True), blocks=blocks)
        check(g, clf, T.random_batch(seed, nconn, garbage=True), seg_cap=nconn // 10, blocks=blocks)


def test_refusals(g, clf):
    """every -EINVAL of the device entry itself, the workspace's among them; a refused call launches
    nothing and writes nothing"""
    import ctypes
    b = T.random_batch(3, 300)
    nconn, cap = b.nconn, 300
    out = {f: ff(cap, dt, w) for f, dt, w in SEG_DT}
    out.update(out_conn=ff(nconn, torch.uint8, 48), totals=ff(2, torch.int64))
    ins = [rec(b.shut, 16), rec(b.tmr, 64), rec(b.conn, 48), rec(b.addr, 16)]
    need = g.tcp_shut_workspace(nconn, 3)
    assert need == 16 + 304 and g.tcp_shut_workspace(nconn, 0) == 4096 + 304
    ws = ff(need + 16, torch.uint8)
    cnt = torch.zeros(g.SHUTC_NR + 1, dtype=torch.int64, device="cuda")
    NULL = ctypes.c_void_p(None)

    def call(ctx=clf._ctx, wsp=ws.data_ptr(), ws_bytes=need, counts=None, no_in=False, no_out=False, **kw):
        sin, sout = g._shut_structs(T.NOW, *ins, nconn, cap, 0, 64, 0, 3, out, None)
        for k, v in kw.items():
            tgt = sin if hasattr(sin, k) else sout if hasattr(sout, k) else sout.seg
            setattr(tgt, k, v)
        return g.lib.gcl_tcp_shut(ctx, None if no_in else ctypes.byref(sin), None if no_out else ctypes.byref(sout),
                                  counts, wsp, ws_bytes, None)

    p = {f: t.data_ptr() for f, t in out.items()}
    refused = [dict(ctx=NULL), dict(no_in=True), dict(no_out=True), dict(size=72), dict(nconn=(1 << 20) + 1),
               dict(seg_cap=(1 << 31) + 1), dict(blocks=1025), dict(frame_stride=53), dict(totals=None),
               dict(shut=None), dict(tmr=None), dict(conn=None), dict(addr=None), dict(out_conn=None),
               dict(desc=None), dict(frame_off=None), dict(seg_conn=None), dict(seg_kind=None), dict(seg_src=None),
               dict(txq_ent=None), dict(txq_cold=None),
               dict(shut=ins[0].data_ptr() + 8), dict(tmr=ins[1].data_ptr() + 8), dict(conn=ins[2].data_ptr() + 4),
               dict(addr=ins[3].data_ptr() + 8), dict(out_conn=p["out_conn"] + 8), dict(desc=p["desc"] + 8),
               dict(frame_off=p["frame_off"] + 4), dict(seg_conn=p["seg_conn"] + 2), dict(seg_src=p["seg_src"] + 2),
               dict(txq_ent=p["txq_ent"] + 8), dict(txq_cold=p["txq_cold"] + 8), dict(totals=p["totals"] + 4),
               dict(counts=cnt.data_ptr() + 4),
               dict(wsp=NULL), dict(wsp=ws.data_ptr() + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0),
               dict(blocks=0),                  # the library's choice of blocks takes the larger workspace
               dict(blocks=5)]                  # more ranges than the workspace's 16 bytes of sums hold
    for kw in refused:
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert all(bool((t == (0xFF if t.dtype == torch.uint8 else -1)).all()) for t in out.values())
    assert bool((ws == 0xFF).all()) and not cnt.any()
    # what a refusal does not need: no segment array with seg_cap 0, nothing at all with nconn 0
    assert call(seg_cap=0, desc=None, frame_off=None, seg_conn=None, seg_kind=None, seg_src=None, txq_ent=None,
                txq_cold=None) == 0
    assert call(nconn=0, shut=None, tmr=None, conn=None, addr=None, out_conn=None, desc=None) == 0
    torch.cuda.synchronize()
    assert out["totals"].tolist() == [0, 0] and bool((ws[need:] == 0xFF).all())
    assert call(counts=cnt.data_ptr()) == 0
    torch.cuda.synchronize()
    host = b.run_host(cap)
    assert T.raw(out["out_conn"].cpu().numpy(), 48 * nconn) == T.raw(host["out_conn"], 48 * nconn)
    assert int(cnt[:g.SHUTS_NR].sum()) == nconn and int(cnt[-1]) == 0 and bool((ws[need:] == 0xFF).all())
    with pytest.raises((OSError, ValueError, RuntimeError)):     # and through the binding
        clf.tcp_shut(T.NOW, *ins, nconn, cap, workspace=ws[:need - 1], blocks=3, out=out)
    with pytest.raises((OSError, ValueError, RuntimeError)):
        clf.tcp_shut(T.NOW, *ins, nconn, cap + 1, blocks=3, out=out)        # arrays shorter than seg_cap


def test_workspace_reuse(g, clf):
    """two calls back to back on one stream over one workspace: the same outputs, the counts twice"""
    b = T.random_batch(6, 1500)
    check(g, clf, b, calls=2)
    check(g, clf, b, seg_cap=100, calls=2, blocks=3)


def test_chain_gives_the_host_chains_frames_and_the_references_fin(g, clf):
    """gcl_tcp_shut -> gcl_tx_hdr -> gcl_l4_csum FILL on one stream: the frames equal the host twins'
    chain, and bytes 34-53 of each FIN equal the reference's tcp_push_tcphdr with flags 0x11, before
    FILL with tx offloads and after it without"""
    segs = T.load_golden()["segs"]
    b, k, stride, base = T.golden_batch(), len(segs), 64, 128
    net = g.txh_net(T.NET["addr"], T.NET["netmask"], T.NET["gateway"], T.NET["mac"])
    clf.neigh_set(T.NEIGH)
    out = clf.tcp_shut(T.NOW, dev(b.shut), dev(b.tmr), dev(b.conn), dev(b.addr), b.nconn, k, frame_stride=stride,
                       frame_base=base)
    frames = torch.full((base + stride * k + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    hdr = clf.tx_hdr(out["desc"], out["frame_off"], k, frames, net)
    torch.cuda.synchronize()
    before = frames.cpu().numpy().copy()
    clf.l4_csum(frames, k, hdr["pkt_len"], mode=g.L4_FILL, offs=out["frame_off"])
    torch.cuda.synchronize()
    after = frames.cpu().numpy()
    assert out["totals"].cpu().numpy().tolist() == [k, k]
    assert (hdr["status"].cpu().numpy()[:k] == g.TXH_OK).all()

    host = b.run_host(k, frame_base=base, frame_stride=stride)
    desc = np.frombuffer(T.raw(host["desc"], 32 * k), dtype=g.TXH_DESC_DTYPE).copy()
    off = np.frombuffer(T.raw(host["frame_off"], 8 * k), dtype=np.uint64).copy()
    hframes = np.full(len(after), 0xA5, dtype=np.uint8)
    tbl = g.NeighTable()
    tbl.set(T.NEIGH)
    hh = g.tx_hdr_host(desc, off, hframes, net, table=tbl)
    assert (hframes == before).all()
    g.l4_csum_host(hframes, hh["pkt_len"], mode=g.L4_FILL, offs=off, n=k)
    assert (hframes == after).all()
    for j, r in enumerate(segs):
        o = base + stride * j
        assert before[o + 34:o + 54].tobytes().hex() == r["hdr_offload"], j
        assert after[o + 34:o + 54].tobytes().hex() == r["hdr_full"], j
