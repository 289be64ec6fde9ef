"""gcl_udp_rx_host (include/gcl_host.h) against the independent Python model of
udp_conn_recv and udp_par_recv and the hand-derived outputs of
tests/udprxcases.py: every verdict, sockets that enter full or with negative
words, POLLIN, the socket flags, zero-length datagrams, what is no datagram,
cookies outside the socket range, order, align, empty calls, the counters, the
chain into gcl_copy_batch_host and every refusal.  No GPU."""
import ctypes
import errno

import numpy as np
import pytest

from caladan_amd import gclassify as g
from tests import udprxcases as uc

HAND = uc.hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    c, want = HAND[name]
    out, counts = uc.run_host(g, c)
    uc.check_hand(c, want, out, name)          # the outputs derived by hand
    uc.check_model(c, out, counts, name)


def test_constants_agree():
    assert (g.UDPRX_QUEUED, g.UDPRX_SPAWN, g.UDPRX_FULL, g.UDPRX_CLOSED, g.UDPRX_NOSOCK, g.UDPRX_NA) == \
        (uc.QUEUED, uc.SPAWN, uc.FULL, uc.CLOSED, uc.NOSOCK, uc.NA)
    assert (g.UDPRXC_BYTES, g.UDPRXC_POLLINS, g.UDPRXC_NR) == (uc.C_BYTES, uc.C_POLLINS, uc.C_NR)
    assert (g.UDPS_SHUTDOWN, g.UDPS_ERR, g.UDPS_SPAWNER, g.UDPRX_SF_POLLIN) == (uc.SHUTDOWN, uc.ERR, uc.SPAWNER,
                                                                              uc.POLLIN)
    assert g.UDP_SOCK_DTYPE == uc.USOCK and g.UDP_SOCK_OUT_DTYPE == uc.USOCK_OUT and g.UDP_REC_DTYPE == uc.REC
    assert g.UDPRX_MAX_BLOCKS == 1024 and g.UDPRX_MAX_SOCK == 1 << 20 and g.lib.gcl_abi_version() == 6


@pytest.mark.parametrize("seed,m", [(1, 1), (2, 63), (3, 64), (4, 65), (5, 300), (6, 4097), (7, 500), (9, 257)])
def test_random_lists_match_model(seed, m):
    c = uc.random_case(seed, m, nsock=seed if seed < 5 else 5 + seed % 3, lead=seed % 4, sock_base=0 if seed == 7 else uc.SOCK_BASE)
    out, counts = uc.run_host(g, c)
    w = uc.check_model(c, out, counts, seed)
    if m >= 300:
        assert all(w["counts"][v] > 0 for v in range(uc.NR_VERDICTS)), w["counts"]
        assert w["counts"][uc.C_POLLINS] > 0


def test_identity_order_and_counts_null():
    c = uc.random_case(11, 200, with_order=False)
    out, _ = uc.run_host(g, c, counts=False)
    uc.check_model(c, out, None, "identity")


def test_counts_accumulate():
    c = uc.random_case(15, 120)
    cnt = np.zeros(uc.C_NR, dtype=np.uint64)
    uc.run_host(g, c, counts=cnt)
    uc.run_host(g, c, counts=cnt)
    assert cnt.tolist() == [2 * x for x in uc.model(c)["counts"]]


def test_blocks_is_checked_and_otherwise_ignored():
    c = uc.random_case(12, 100)
    a, _ = uc.run_host(g, c)
    b, _ = uc.run_host(g, c, blocks=7)
    uc.same(a, b, "blocks")


def test_chain_payload_rx_copy():
    """l4_payload_host -> udp_rx_host -> copy_batch_host: every socket's region holds exactly its taken
    payloads in arrival order, each at its padded place, and nothing of a dropped datagram"""
    c = uc.chain_case()
    out, dst, pay = uc.host_chain(g, c)
    ns, m = len(c["usock"]), c["m"]
    want = np.full(len(dst), uc.SENTINEL, dtype=np.uint8)
    v = out["verdict"][:m]
    assert all((v == x).any() for x in (uc.QUEUED, uc.SPAWN, uc.FULL, uc.CLOSED, uc.NOSOCK))
    for s in range(ns):
        at = int(out["sock_off"][s])
        k = int(out["rec_off"][s])
        for j in range(m):
            if int(c["sock"][j]) - uc.SOCK_BASE == s and v[j] in (uc.QUEUED, uc.SPAWN):
                ln = int(pay["len"][j])
                src = int(pay["src_off"][j])
                want[at:at + ln] = c["frames"][src:src + ln]
                r = out["rec"][k]
                assert (int(r["dst_off"]), int(r["len"]), int(r["rport"])) == (at, ln, 2000 + j)
                assert int(out["rec_idx"][j]) == k and int(out["dst_off"][j]) == at
                at += uc.pad(ln, c["align"])
                k += 1
        assert at == int(out["sock_off"][s + 1]) and k == int(out["rec_off"][s + 1])
    assert dst.tobytes() == want.tobytes()


def _refused(c, **kw):
    with pytest.raises(OSError) as e:
        uc.run_host(g, c, **kw)
    assert e.value.errno == errno.EINVAL


def test_refusals():
    c = uc.random_case(13, 40, n=50)
    _refused(c, blocks=g.UDPRX_MAX_BLOCKS + 1)
    for al in (3, 512, 96):
        _refused(c, align=al)
    _refused(dict(c, order=None))     # order == NULL with m != n


def _structs(c, out, **over):
    args = dict(frames=c["frames"], n=c["n"], stride=0, offs=c["offs"], pkt_len=c["pkt_len"], frames_len=None,
                m=c["m"], order=c["order"], sock=c["sock"], l4_status=c["l4_status"], usock=c["usock"],
                nsock=len(c["usock"]), sock_base=c["sock_base"], align=c["align"], blocks=0, out=out, counts=None)
    args.update(over)
    return g._udprx_structs(**args)


def test_refusals_of_pointers_size_and_alignment():
    c = uc.random_case(14, 20)
    out = uc.blank(c)
    call = lambda b, i, o, cnt=None: g.lib.gcl_udp_rx_host(
        None if b is None else ctypes.byref(b), None if i is None else ctypes.byref(i),
        None if o is None else ctypes.byref(o), cnt)
    b, i, o = _structs(c, out)
    assert call(b, i, o) == 0
    for k in range(3):
        a = [b, i, o]
        a[k] = None
        assert call(*a) == -errno.EINVAL
    b, i, o = _structs(c, out)
    i.size -= 1
    assert call(b, i, o) == -errno.EINVAL
    for f in ("sock", "usock"):
        b, i, o = _structs(c, out)
        setattr(i, f, None)
        assert call(b, i, o) == -errno.EINVAL, f
    for f in uc_fields():
        b, i, o = _structs(c, out)
        setattr(o, f, None)
        assert call(b, i, o) == -errno.EINVAL, f
    for st, f, al in (("i", "order", 4), ("i", "sock", 4), ("i", "usock", 16), ("o", "copy_len", 2),
                      ("o", "dst_off", 8), ("o", "rec_idx", 4), ("o", "rec", 16), ("o", "out_sock", 16),
                      ("o", "rec_off", 4), ("o", "sock_off", 8)):
        b, i, o = _structs(c, out)
        t = {"i": i, "o": o}[st]
        setattr(t, f, getattr(t, f) + al // 2)
        assert call(b, i, o) == -errno.EINVAL, (f, "misaligned")
    b, i, o = _structs(c, out)
    assert call(b, i, o, out["sock_off"].ctypes.data + 4) == -errno.EINVAL   # counts misaligned
    for f, v in (("m", (1 << 31) + 1), ("nsock", (1 << 20) + 1), ("blocks", 1025), ("align", 48)):
        b, i, o = _structs(c, out)
        setattr(i, f, v)
        assert call(b, i, o) == -errno.EINVAL, f
    for f in ("pkt_len", "frames"):
        b, i, o = _structs(c, out)
        setattr(b, f, None)
        assert call(b, i, o) == -errno.EINVAL, f
    b, i, o = _structs(c, out)
    b.offs, b.stride = None, 100      # what gcl_l4_payload refuses of a batch: a stride that is no multiple of 16
    assert call(b, i, o) == -errno.EINVAL
    # with m == 0 the per-entry arrays may be NULL; with nsock == 0 usock and out_sock
    c0 = uc.case([], [uc.usock()])
    b, i, o = _structs(c0, uc.blank(c0))
    for f in uc.ENTRY:
        setattr(o, f[0], None)
    o.rec = None
    assert call(b, i, o) == 0
    c1 = uc.case([(uc.frame(3), uc.S0)], [])
    b, i, o = _structs(c1, uc.blank(c1))
    i.usock, o.out_sock = None, None
    assert call(b, i, o) == 0


def uc_fields():
    return g.UDPRX_OUT_FIELDS


def test_workspace_refusals():
    need = ctypes.c_size_t()
    ws = lambda *a: g.lib.gcl_udp_rx_workspace(*a, ctypes.byref(need))
    assert ws(100, 16, 0) == 0 and need.value > 0
    assert g.lib.gcl_udp_rx_workspace(100, 16, 0, None) == -errno.EINVAL
    assert ws((1 << 31) + 1, 16, 0) == -errno.EINVAL
    assert ws(100, (1 << 20) + 1, 0) == -errno.EINVAL
    assert ws(100, 16, 1025) == -errno.EINVAL
    assert ws(0, 0, 0) == 0 and ws(100, 1 << 20, 1024) == 0
