"""GPU: gcl_tcp_rx_states (include/gclassify.h) against its host twin, byte for
byte over sentinel-filled outputs with guards, and against what the reference's
own tcp_rx_conn did (tests/golden/tcprxs_ref.json): the named cases with the
default, 1 and 3 grouping ranges, the random lifetimes, the chain through
gcl_copy_batch with the FIN gap and the lost tail byte, and the shapes where
the walk can go wrong: a state change, a FAIL and a FIN on the last segment of
a 64-segment chunk and on the first two of the next, in runs of 65 and 129; an
input queue of exactly 64 entries with its FIN entry at position 0 and at 63;
1, waves-per-block - 1, + 1 and 1000 connections."""
import errno

import numpy as np
import pytest
import torch

from tests import paycases as pc
from tests import tcprxcases as rc
from tests import tcprxocases as oc
from tests import tcprxscases as sc
from tests import tcprxsrefcases as sr
from tests.tcprxcases import TCP_ACK, TCP_FIN, TCP_RST

pytestmark = pytest.mark.gpu

SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}
WAVES = 4          # kRxWaves of csrc/gcl_tcprx.hip: connections per block of the walk


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


def run_gpu(g, clf, case, counts=True, calls=1, keep=None, blocks=None, workspace=None, fill=sc.SENTINEL):
    """@calls calls over @fill-filled device outputs: (outputs as numpy, counts summed over the calls)"""
    z = oc.sizes(case)
    m, nconn, nq = z["m"], z["nconn"], z["nq"]
    n, order = len(case["pkt_len"]), case.get("order")
    blank = sc.blank(case, fill)
    out = {f: dev(a) for f, a in blank.items()}
    frames, plen = dev(case["frames"]), dev(case["pkt_len"]) if n else torch.zeros(1, dtype=torch.int16, device="cuda")
    offs = dev(case["offs"]) if case["offs"] is not None and n else None
    sock = dev(case["sock"]) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    st = dev(case["st"]) if case.get("st") is not None else None
    rep = dev(case["rep_acks"]) if case.get("rep_acks") is not None else None
    q_off = dev(case["q_off"]) if case.get("q_off") is not None else None
    q = dev(case["q"]) if nq else None
    state = dev(case["state"]) if case.get("state") is not None else None
    cnt = torch.full((g.TCPRXSC_NR,), 5, dtype=torch.int64, device="cuda") if counts else None
    for _ in range(calls):
        clf.tcp_rx_states(frames, n, plen, sock, dev(case["conn"]), nconn,
                          stride=case["stride"] or 16 * (offs is None), offs=offs, frames_len=case["frames_len"],
                          order=dev(order) if order is not None else None, m=m, l4_status=st,
                          align=case.get("align", 0), blocks=case.get("blocks", 0) if blocks is None else blocks,
                          rep_acks=rep, q_off=q_off, q=q, nq=nq, q_out_cap=z["cap"], state=state, out=out,
                          counts=cnt, workspace=workspace)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(out, frames=frames, sock=sock)
    got = {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    return got, None if cnt is None else cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


def check(g, clf, case, what, **kw):
    """GPU == host twin, whole arrays with their guards, and the counts"""
    hgot, hcnt = sc.run_host(g, case)
    got, cnt = run_gpu(g, clf, case, **kw)
    sc.compare(got, hgot, case, (what, "host"))
    assert cnt.tolist() == (hcnt * np.uint64(kw.get("calls", 1))).tolist(), what
    return got


@pytest.mark.parametrize("blocks", [0, 1, 3, rc.MAX_BLOCKS])
def test_named_cases_against_host_twin_and_reference(g, clf, blocks):
    total = 0
    for name in sr.names():
        case = sr.case_of(name)
        got = check(g, clf, case, (name, blocks), blocks=blocks)
        total += sr.check(got, name, ("gpu", blocks))
        if name in sc.cases():
            sc.check_expected(got, sc.cases()[name][1], name)
    assert total == sr.comparable()


@pytest.mark.parametrize("name", sorted(sc.STREAMS))
def test_random_lifetimes(g, clf, name):
    """a few thousand segments of random lifetimes, two calls into the same counts"""
    check(g, clf, sc.stream(name), name, calls=2)


def one_conn(segs, state, q=None, **kw):
    case = rc.build([rc.conn1(snd_wl1=50000, **kw)], segs)
    case["state"] = np.array([state], dtype=np.uint8)
    if q is not None:
        case["q_off"], case["q"] = np.array([0, len(q)], dtype=np.uint32), oc.ents(q)
    return case


@pytest.mark.parametrize("n", [65, 129])
@pytest.mark.parametrize("at", [62, 63, 64])
@pytest.mark.parametrize("what", ["state", "fail", "fin"])
def test_events_across_the_chunk_boundary(g, clf, n, at, what):
    """10-byte in-order segments of a connection in FIN_WAIT1 whose FIN the peer
    has not acknowledged; segment @at (and with 129 segments @at + 64) brings
    the ACK of our FIN, a RST or the peer's FIN"""
    rng = np.random.default_rng(n + at)
    segs, seq, hits = [], 100, [at] if n == 65 else [at + 64]
    for k in range(n):
        if k in hits and what == "fail":
            segs.append(rc.seg(rng, 0, seq, 0, ack=4999, flags=TCP_ACK | TCP_RST))
            continue
        fl, ack = TCP_ACK, 4999
        if k in hits:
            fl, ack = (TCP_ACK | TCP_FIN, 4999) if what == "fin" else (TCP_ACK, 5000)
        segs.append(rc.seg(rng, 0, seq, 10, ack=ack, flags=fl))
        seq += 10 + bool(fl & TCP_FIN)
    got = check(g, clf, one_conn(segs, sc.FIN_WAIT1, snd_una=4999), (n, at, what))
    h = hits[0]
    want_ev = {"state": sc.EV_STATE, "fail": sc.EV_FAIL, "fin": sc.EV_STATE | sc.EV_FIN}[what]
    assert int(got["ev"][h]) == want_ev and not got["ev"][:h].any()
    assert got["state_after"][:h].tolist() == [sc.FIN_WAIT1] * h
    if what == "fail":
        assert got["verdict"][:n].tolist() == [rc.FAST] * (h + 1) + [rc.SLOW] * (n - h - 1)
        assert int(got["out_conn"]["first_slow"][0]) == (h + 1 if h + 1 < n else rc.NONE)
    elif what == "fin":                      # CLOSING takes no text: what follows is dropped, not linked
        assert got["state_after"][h:n].tolist() == [sc.CLOSING] * (n - h)
        assert not got["copy_len"][h + 1:n].any() and got["copy_len"][:h + 1].tolist() == [10] * (h + 1)
    else:
        assert got["state_after"][h:n].tolist() == [sc.FIN_WAIT2] * (n - h) and got["copy_len"][:n].tolist() == [10] * n


@pytest.mark.parametrize("pos", [0, 63])
def test_input_queue_of_64_with_a_fin_entry(g, clf, pos):
    """64 input entries of 10 sequence numbers right behind a one-segment hole,
    entry @pos with FIN (its last octet); the hole's segment drains all 64"""
    rng = np.random.default_rng(pos)
    q = [(110 + 10 * k, 120 + 10 * k, 500 + k, TCP_ACK | (TCP_FIN if k == pos else 0)) for k in range(64)]
    got = check(g, clf, one_conn([rc.seg(rng, 0, 100, 10)], sc.ESTABLISHED, q), pos)
    assert int(got["out_conn"]["rcv_nxt"][0]) == 750 and int(got["totals"][0]) == 0
    assert int(got["ev"][0]) == sc.EV_STATE | sc.EV_FIN and int(got["state_out"][0]) == sc.CLOSE_WAIT
    assert got["qin_len"][:64].tolist() == [9 if k == pos else 10 for k in range(64)]
    assert got["qin_dst_off"][:64].tolist() == [10 + 10 * k for k in range(64)]


@pytest.mark.parametrize("nconn", [1, WAVES - 1, WAVES + 1, 1000])
def test_connection_counts(g, clf, nconn):
    check(g, clf, sc.random_case(100 + nconn, nconn=nconn, data=(1, 4)), nconn)


@pytest.mark.parametrize("nconn", [rc.PASS_CONN, rc.PASS_CONN + 1])
def test_one_and_two_grouping_passes(g, clf, nconn):
    """connections 0, PASS_CONN - 1 and nconn - 1 (cookies at both ends of the
    range, the last one in the second pass's second digit) get 65 in-order
    10-byte segments each, interleaved; the last connection enters in
    SYN_RECEIVED and its 65th segment, the first of its second chunk, carries
    the peer's FIN"""
    rng = np.random.default_rng(nconn)
    live, last = sorted({0, rc.PASS_CONN - 1, nconn - 1}), nconn - 1
    segs = [rc.seg(rng, c, 100 + 10 * k, 10, flags=TCP_ACK | (TCP_FIN if (c, k) == (last, 64) else 0))
            for k in range(65) for c in live]
    case = rc.build([rc.conn1(snd_wl1=50000)] * nconn, segs)
    case["state"] = np.full(nconn, sc.ESTABLISHED, dtype=np.uint8)
    case["state"][last] = sc.SYN_RECEIVED
    got = check(g, clf, case, nconn)
    assert got["out_conn"]["nfast"][live].tolist() == [65] * len(live)
    assert got["state_out"][live].tolist() == [sc.ESTABLISHED] * (len(live) - 1) + [sc.CLOSE_WAIT]
    assert int(got["out_conn"]["rcv_nxt"][last]) == 100 + 650 + 1
    assert int(got["ev"][live.index(last)]) & sc.EV_STATE and int(got["ev"][len(segs) - 1]) == sc.EV_STATE | sc.EV_FIN


def test_dirty_workspace_reused_and_counts_accumulate(g, clf):
    """the workspace and every output filled with 0xFF, then two calls on the
    same buffers: every byte of every output is what the host twin leaves in
    buffers filled the same way, and counts holds twice the twin's counters,
    the four the walk adds itself among them"""
    case = sc.stream("lifetimes")
    z = oc.sizes(case)
    need = g.tcp_rx_states_workspace(z["m"], z["nconn"], 0, z["nq"])
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    want, hcnt = sc.run_host(g, case, fill=0xFF)
    got, cnt = run_gpu(g, clf, case, calls=2, workspace=ws, fill=0xFF)
    for f in want:
        bad = np.nonzero(got[f].view(np.uint8) != want[f].view(np.uint8))[0]
        assert not len(bad), f"{f}: byte {bad[0]} of {len(bad)} that differ"
    assert cnt.tolist() == (hcnt * np.uint64(2)).tolist()
    assert all(int(hcnt[k]) > 3 for k in (sc.C_RSTS, sc.C_FAILS, sc.C_FINS, sc.C_STATE_CHANGES))


def test_empty_list(g, clf):
    """a connection with no segment gets its state back"""
    got = check(g, clf, dict(rc.build([rc.conn1()], []), state=np.array([sc.FIN_WAIT2], dtype=np.uint8)), "no segments")
    assert int(got["state_out"][0]) == sc.FIN_WAIT2


@pytest.mark.parametrize("name", ["fin_tail_clip_6_into_3", "established_fin_with_text_then_text",
                                  "fin_queued_then_drained", "fin_head_clipped", "stream"])
def test_copy_chain_leaves_the_fin_gap(g, clf, name):
    """gcl_copy_batch over src_off + skip, copy_len and dst_off puts every
    linked mbuf at its sequence number; the FIN's octet, and the byte a clipped
    FIN segment loses, stay unwritten"""
    case = sc.stream("lifetimes_aligned") if name == "stream" else sc.case_of(name)
    want = sc.model(case, with_rxq=True)
    keep = {}
    run_gpu(g, clf, case, keep=keep)
    m, nconn = oc.sizes(case)["m"], len(case["conn"])
    pay = pc.model(case, None, case["sock"], case.get("st"))
    total = int(want["conn_off"][nconn])
    rx = torch.full((total + 64,), sc.SENTINEL, dtype=torch.uint8, device="cuda")
    src = dev(pay["src_off"].astype(np.uint64)) + keep["skip"][:m].view(torch.int16).to(torch.int64)
    clf.copy_batch(keep["frames"], src, keep["copy_len"], m, rx[:total], dst_off=keep["dst_off"], olflags=False,
                   rss=False)
    torch.cuda.synchronize()
    rxh = rx.cpu().numpy()
    ref = np.full(total + 64, sc.SENTINEL, dtype=np.uint8)
    for c in range(nconn):
        o = int(want["conn_off"][c])
        for at, data in want["rxq"][c]:
            ref[o + at:o + at + len(data)] = np.frombuffer(data, dtype=np.uint8)
    assert (rxh == ref).all(), name
    if name == "fin_tail_clip_6_into_3":        # 2 bytes of text, the lost tail byte, and no room for the FIN's octet
        assert total == 3 and (rxh[2:] == sc.SENTINEL).all()
    if name == "established_fin_with_text_then_text":
        assert total == 31 and rxh[30] == sc.SENTINEL


def test_error_returns(g, clf):
    case = sc.case_of("fin_entry_in_input_queue")
    z = oc.sizes(case)
    m, nconn, nq = z["m"], z["nconn"], z["nq"]
    out = {f: dev(a) for f, a in sc.blank(case).items()}
    fr, plen, sock, conn, offs = (dev(case[k]) for k in ("frames", "pkt_len", "sock", "conn", "offs"))
    ok = dict(frames=fr, n=m, pkt_len=plen, sock=sock, conn=conn, nconn=nconn, offs=offs, out=out,
              q_off=dev(case["q_off"]), q=dev(case["q"]), nq=nq, q_out_cap=z["cap"], state=dev(case["state"]))
    clf.tcp_rx_states(**ok)
    torch.cuda.synchronize()
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")

    def refused(**kw):
        with pytest.raises(OSError) as e:
            clf.tcp_rx_states(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    refused(align=3)
    refused(blocks=rc.MAX_BLOCKS + 1)
    for f in out:
        refused(out=dict(out, **{f: None}), workspace=big)
    refused(q=None)
    odd = torch.zeros(16 * 8 + 64, dtype=torch.uint8, device="cuda")
    refused(out=dict(out, rst_seq=odd[2:]))
    refused(out=dict(out, qout=odd[8:]))
    need = g.tcp_rx_states_workspace(m, nconn, 0, nq)
    assert need == g.tcp_rx_ooo_workspace(m, nconn, 0, nq)
    refused(workspace=big[:need - 1])
    clf.tcp_rx_states(**dict(ok, workspace=big[:need]))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- gcl_tcp_rx_ctl
from tests import tcprxsctlcases as cc  # noqa: E402


def run_ctl(g, clf, case, seg_cap, blocks=0):
    """gcl_tcp_rx_states, then gcl_tcp_rx_ctl over its device outputs: (sentinel-filled outputs as numpy, counts)"""
    keep = {}
    run_gpu(g, clf, case, keep=keep)
    m, nconn = len(case["sock"]), len(case["conn"])
    blank = cc.blank(seg_cap)
    out = {f: dev(a) for f, a in blank.items()}
    cnt = torch.full((g.TICKC_NR,), 5, dtype=torch.int64, device="cuda")
    clf.tcp_rx_ctl(keep["verdict"], keep["sflags"], keep["rcv_nxt_after"], keep["ev"], keep["rst_seq"], m,
                   keep["sock"], len(case["pkt_len"]), dev(case["conn"]), dev(cc.addrs(nconn)), nconn, seg_cap,
                   order=dev(case["order"]) if case.get("order") is not None else None, frame_stride=cc.STRIDE,
                   frame_base=cc.BASE, blocks=blocks, out=out, counts=cnt)
    torch.cuda.synchronize()
    got = {f: out[f].cpu().numpy().reshape(-1).view(blank[f].dtype) for f in blank}
    return got, cnt.cpu().numpy().view(np.uint64) - np.uint64(5)


@pytest.mark.parametrize("blocks", [0, 1, 3])
def test_ctl_against_host_twin_and_reference(g, clf, blocks):
    for name in sr.names():
        case = sr.case_of(name)
        rx, _ = sc.run_host(g, case)
        cap = len(case["sock"]) + 1
        want, wcnt = cc.run_host(g, case, rx, cap)
        got, cnt = run_ctl(g, clf, case, cap, blocks=blocks)
        cc.same(got, want, int(want["totals"][1]), (name, blocks))
        assert cnt.tolist() == wcnt.tolist(), (name, blocks)
        cc.check_against_reference(got, name, ("gpu", blocks))


@pytest.mark.parametrize("short", [None, 1, 0])
def test_ctl_seg_cap_and_many_ranges(g, clf, short):
    """a few thousand entries of random lifetimes with seg_cap of wanted, one below and 0"""
    case = sc.stream("lifetimes")
    rx, _ = sc.run_host(g, case)
    full, _ = cc.run_host(g, case, rx, len(case["sock"]))
    wanted = int(full["totals"][0])
    cap = wanted if short is None else (wanted - 1) * short
    want, wcnt = cc.run_host(g, case, rx, cap)
    got, cnt = run_ctl(g, clf, case, cap, blocks=0 if short is None else 5)
    cc.same(got, want, cap, short)
    assert cnt.tolist() == wcnt.tolist() and got["totals"][:2].tolist() == [wanted, cap]
    assert int((full["seg_kind"][:wanted] == cc.K_RST).sum()) > 3 and int((full["seg_kind"][:wanted] == cc.K_RST_ACK).sum()) > 3


def test_ctl_error_returns(g, clf):
    case = sr.case_of("closed_ack_rst_neither")
    keep = {}
    run_gpu(g, clf, case, keep=keep)
    m, nconn = len(case["sock"]), len(case["conn"])
    out = {f: dev(a) for f, a in cc.blank(m).items()}
    ok = dict(verdict=keep["verdict"], sflags=keep["sflags"], rcv_nxt_after=keep["rcv_nxt_after"], ev=keep["ev"],
              rst_seq=keep["rst_seq"], m=m, sock=keep["sock"], n=m, conn=dev(case["conn"]), addr=dev(cc.addrs(nconn)),
              nconn=nconn, seg_cap=m, out=out)
    clf.tcp_rx_ctl(**ok)
    torch.cuda.synchronize()

    def refused(**kw):
        with pytest.raises(OSError) as e:
            clf.tcp_rx_ctl(**dict(ok, **kw))
        assert e.value.errno == errno.EINVAL, kw

    for f in ("ev", "rst_seq", "verdict", "sock", "conn", "addr"):
        refused(**{f: None})
    big = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for f in out:
        refused(out=dict(out, **{f: None}), workspace=big)
    odd = torch.zeros(4 * m + 64, dtype=torch.uint8, device="cuda")
    refused(rst_seq=odd[2:])
    refused(frame_stride=53)
    assert g.tcp_rx_ctl_workspace(m) == g.tcp_rx_acks_workspace(m)
    refused(workspace=big[:g.tcp_rx_ctl_workspace(m) - 1])
