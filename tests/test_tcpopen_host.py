"""gcl_tcp_rx_open_host (include/gcl_host.h) against the independent Python
model of the rule and the hand-derived verdicts of tests/tcpopencases.py: every
verdict, the option walk in every shape, the backlog, LATER, the caps, the
tuple table at its minimum and every refusal.  No GPU."""
import ctypes
import errno

import numpy as np
import pytest

from caladan_amd import gclassify as g
from tests import tcpopencases as oc

HAND = oc.hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    c, verdicts = HAND[name]
    out, counts = oc.run_host(g, c)
    assert out["verdict"][:c["m"]].tolist() == verdicts, name   # the verdicts derived by hand
    oc.check_model(c, out, counts, name)


def test_constants_agree():
    assert (g.OPEN_NA, g.OPEN_OOR, g.OPEN_SHORT, g.OPEN_CLOSED_DROP, g.OPEN_CLOSED_RST, g.OPEN_CLOSED_RST_ACK,
            g.OPEN_LATER, g.OPEN_FULL, g.OPEN_DROP, g.OPEN_RST, g.OPEN_BADOPT, g.OPEN_ACCEPT) == tuple(range(12))
    assert (g.OPENC_SEGS, g.OPENC_SEGSKIP, g.OPENC_NOSPACE, g.OPENC_NR) == (oc.C_SEGS, oc.C_SEGSKIP, oc.C_NOSPACE,
                                                                           oc.C_NR)
    assert g.CTL_SYNACK == oc.K_SYNACK and g.TCP_LISTEN_DTYPE == oc.LISTEN and g.TCP_OPEN_DTYPE == oc.OPEN
    assert g.TCP_STATE_SYN_RECEIVED == 1 and g.OPEN_MAX_LISTEN == 4096


def test_miss_rst_seq_by_hand():
    c, _ = HAND["miss_len"]
    out, _ = oc.run_host(g, c)
    # seq + payload; SYN and FIN not counted, seq M32 + 2 wraps; off 15 with no options: 20 - 60 = -40;
    # off 0: the whole 27 bytes behind the IP header count
    assert out["rst_seq"][:4].tolist() == [103, 1, (10 - 40) & oc.M32, 10 + 27]
    assert out["seg_kind"][:6].tolist() == [oc.K_RST_ACK] * 6
    d = out["desc"][2]
    assert (int(d["seq"]), int(d["ack"]), int(d["tcp_flags"]), int(d["win"])) == (0, (10 - 40) & oc.M32, 0x14, 0)
    c, _ = HAND["miss"]
    out, _ = oc.run_host(g, c)
    assert out["rst_seq"][:5].tolist() == [0, 777, 0, 100, 100]
    d = out["desc"][0]   # the RST of the ACK: seq = the segment's ack, from the packet's own daddr
    assert (int(d["seq"]), int(d["ack"]), int(d["tcp_flags"]), int(d["lip"]), int(d["rip"]), int(d["lport"]),
            int(d["rport"])) == (777, 0, 0x04, oc.LIP, oc.RIP, 80, 40000)


@pytest.mark.parametrize("name", sorted(oc.OPTION_SHAPES))
def test_option_shape_by_hand(name):
    ob, res = oc.OPTION_SHAPES[name]
    c, _ = HAND["opt_" + name]
    out, _ = oc.run_host(g, c)
    if res is None:
        assert out["totals"][0] == 0 and out["seg_totals"][0] == 0
        return
    en, mss, ws = res
    r0, r1 = out["open"][0], out["open"][1]
    assert (int(r0["opt_en"]), int(r0["snd_mss"]), int(r0["snd_wscale"])) == (en, mss, ws), name
    assert (int(r1["opt_en"]), int(r1["snd_mss"]), int(r1["snd_wscale"])) == (en, mss, ws), name
    # listener 0: winmax 2^20, rcv_wscale 5; listener 1: winmax 40000, rcv_wscale 0
    if en & oc.OPT_WSCALE:
        assert (int(r0["rcv_wnd"]), int(r0["winmax"]), int(r0["rcv_wscale"])) == (1 << 20, 1 << 20, 5)
        assert int(out["desc"][0]["win"]) == (1 << 20) >> 5
    else:
        assert (int(r0["rcv_wnd"]), int(r0["winmax"]), int(r0["rcv_wscale"])) == (65535, 65535, 0)
        assert int(out["desc"][0]["win"]) == 65535
    assert (int(r1["rcv_wnd"]), int(r1["winmax"]), int(r1["rcv_wscale"])) == (40000, 40000, 0)
    assert int(out["desc"][1]["win"]) == 40000
    want = ([1, 3, 3, 5] if en & oc.OPT_WSCALE else []) + ([2, 4, 0x05, 0xB4] if en & oc.OPT_MSS else [])
    fo = oc.TX_BASE
    assert oc.tx(out)[fo + 54:fo + 54 + len(want)].tolist() == want
    assert int(out["desc"][0]["tcp_off"]) == 5 + len(want) // 4 and int(out["desc"][0]["tcp_flags"]) == 0x12
    assert (int(r0["irs"]), int(r0["rcv_nxt"]), int(r0["iss"]), int(r0["snd_una"]), int(r0["snd_nxt"]),
            int(r0["state"])) == (1000, 1001, 0x10007, 0x10007, 0x10008, 1)


@pytest.mark.parametrize("seed,m", [(1, 1), (2, 63), (3, 64), (4, 65), (5, 300), (6, 4097), (7, 500), (9, 257)])
def test_random_lists_match_model(seed, m):
    c = oc.random_case(seed, m, nlisten=1 + seed % 5, hash_slots=0 if seed % 2 else 1 << (2 * m - 1).bit_length(),
                       lead=seed % 4, caps=seed > 6)
    out, counts = oc.run_host(g, c)
    w = oc.check_model(c, out, counts, seed)
    if m >= 300:
        assert all(w["counts"][v] > 0 for v in range(oc.NR_VERDICTS)), w["counts"]


def test_identity_order_and_counts_null():
    c = oc.random_case(11, 200, with_order=False)
    out, _ = oc.run_host(g, c, counts=False)
    oc.check_model(c, out, None, "identity")


def test_blocks_is_checked_and_otherwise_ignored():
    c = oc.random_case(12, 100)
    a, _ = oc.run_host(g, c)
    b, _ = oc.run_host(g, c, blocks=7)
    oc.same(a, b, "blocks")


def test_m_zero_is_a_noop():
    c = oc.case([], [oc.listener()])
    out, counts = oc.run_host(g, c)
    assert counts == [0] * oc.C_NR
    for f, a in out.items():
        assert (a.view(np.uint8) == oc.SENTINEL).all(), f


def _refused(c, **kw):
    with pytest.raises(OSError) as e:
        oc.run_host(g, c, **kw)
    assert e.value.errno == errno.EINVAL


def test_refusals():
    c = oc.random_case(13, 40, n=50)
    _refused(c, blocks=g.OPEN_MAX_BLOCKS + 1)
    for hs in (100, 64, 3):          # not a power of two; below 2 * m; both
        _refused(dict(c, hash_slots=hs))
    _refused(c, frame_stride=61)
    _refused(dict(c, order=None))     # order == NULL with m != n


def _structs(c, out, **over):
    args = dict(frames=c["frames"], n=c["n"], stride=0, offs=c["offs"], pkt_len=c["pkt_len"], frames_len=None,
                m=c["m"], order=c["order"], sock=c["sock"], l4_status=c["l4_status"], listen=c["listen"],
                nlisten=len(c["listen"]), listen_base=oc.LISTEN_BASE, iss=c["iss"], seg_cap=c["seg_cap"],
                open_cap=c["open_cap"], frame_base=oc.TX_BASE, frame_stride=oc.TX_STRIDE, tx_frames=oc.tx(out),
                tx_frames_len=None, blocks=0, hash_slots=0, out={k: v for k, v in out.items() if k != "tx_all"},
                counts=None)
    args.update(over)
    return g._tcpopen_structs(**args)


def test_refusals_of_pointers_size_and_alignment():
    c = oc.random_case(14, 20)
    out = oc.blank(c)
    call = lambda b, i, o, s, cnt=None: g.lib.gcl_tcp_rx_open_host(
        None if b is None else ctypes.byref(b), None if i is None else ctypes.byref(i),
        None if o is None else ctypes.byref(o), None if s is None else ctypes.byref(s), cnt)
    b, i, o, s = _structs(c, out)
    assert call(b, i, o, s) == 0
    for k in range(4):
        a = [b, i, o, s]
        a[k] = None
        assert call(*a) == -errno.EINVAL
    b, i, o, s = _structs(c, out)
    i.size -= 1
    assert call(b, i, o, s) == -errno.EINVAL
    for f in ("sock", "iss", "listen", "tx_frames"):
        b, i, o, s = _structs(c, out)
        setattr(i, f, None)
        assert call(b, i, o, s) == -errno.EINVAL, f
    for f in ("verdict", "later_of", "rst_seq", "open", "backlog_out", "totals"):
        b, i, o, s = _structs(c, out)
        setattr(o, f, None)
        assert call(b, i, o, s) == -errno.EINVAL, f
    for f in ("desc", "frame_off", "seg_conn", "seg_kind", "seg_src", "totals"):
        b, i, o, s = _structs(c, out)
        setattr(s, f, None)
        assert call(b, i, o, s) == -errno.EINVAL, f
    for st, f, al in (("i", "order", 4), ("i", "sock", 4), ("i", "listen", 16), ("i", "iss", 4), ("o", "later_of", 4),
                      ("o", "rst_seq", 4), ("o", "open", 16), ("o", "backlog_out", 4), ("o", "totals", 8),
                      ("s", "desc", 16), ("s", "frame_off", 8), ("s", "seg_conn", 4), ("s", "seg_src", 4),
                      ("s", "totals", 8)):
        b, i, o, s = _structs(c, out)
        t = {"i": i, "o": o, "s": s}[st]
        setattr(t, f, getattr(t, f) + al // 2)
        assert call(b, i, o, s) == -errno.EINVAL, (f, "misaligned")
    b, i, o, s = _structs(c, out)
    assert call(b, i, o, s, out["totals"].ctypes.data + 4) == -errno.EINVAL   # counts misaligned
    for f, v in (("seg_cap", (1 << 31) + 1), ("open_cap", (1 << 31) + 1), ("m", (1 << 31) + 1), ("nlisten", 4097),
                 ("frame_stride", 0)):
        b, i, o, s = _structs(c, out)
        setattr(i, f, v)
        assert call(b, i, o, s) == -errno.EINVAL, f
    b, i, o, s = _structs(c, out)
    b.pkt_len = None
    assert call(b, i, o, s) == -errno.EINVAL
    b, i, o, s = _structs(c, out)
    b.frames = None
    assert call(b, i, o, s) == -errno.EINVAL


def test_workspace_refusals():
    need = ctypes.c_size_t()
    ws = lambda *a: g.lib.gcl_tcp_rx_open_workspace(*a, ctypes.byref(need))
    assert ws(100, 16, 0, 0) == 0 and need.value > 0
    assert g.lib.gcl_tcp_rx_open_workspace(100, 16, 0, 0, None) == -errno.EINVAL
    assert ws((1 << 31) + 1, 16, 0, 0) == -errno.EINVAL
    assert ws(100, 4097, 0, 0) == -errno.EINVAL
    assert ws(100, 16, 1025, 0) == -errno.EINVAL
    assert ws(100, 16, 0, 128) == -errno.EINVAL and ws(100, 16, 0, 300) == -errno.EINVAL
    assert ws(100, 16, 0, 256) == 0
