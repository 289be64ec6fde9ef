"""CPU: gcl_tx_hdr_host and the neighbour table object (include/gcl_host.h)
against the model of tests/txhcases.py: exact equality of the whole frame
region with its guard bands, of every output array with its sentinel guard and
of the counters; then the produced frames through the pinned checksum and
payload code, the command words field by field, the table's own behaviour and
the error returns."""
import ctypes
import errno

import numpy as np
import pytest

from tests import txhcases as tc


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def table_of(g, case):
    t = g.NeighTable(hash_bits=case["hash_bits"])
    t.set(case["neigh"])
    return t


def blank_outputs(m, with_hash=True):
    out = {f: np.full(m + tc.OUT_GUARD, tc.OUT_SENTINEL[f], dtype=dt) for f, dt in tc.OUT_DTYPE.items()}
    if not with_hash:
        out["hash"] = None
    return out


def compare(got, want, m, what):
    for f in tc.OUT_DTYPE:
        if got[f] is None:
            continue
        a = np.asarray(got[f])
        assert a[:m].tolist() == want[f].tolist(), (what, f)
        assert (a[m:] == tc.OUT_SENTINEL[f]).all(), (what, f, "guard")


def run_host(g, case, table=None, shift=0, with_hash=True, counts=True):
    m = len(case["desc"])
    flen = case["frames_len"]
    buf = np.full(shift + tc.GUARD + flen + tc.GUARD, tc.SENTINEL, dtype=np.uint8)
    out = blank_outputs(m, with_hash)
    cnt = np.full(g.TXHC_NR, 5, dtype=np.uint64) if counts else None
    table = table or table_of(g, case)
    got = g.tx_hdr_host(case["desc"], case["frame_off"], buf[shift + tc.GUARD:], g.txh_net(**case["net"]),
                        table=table, m=m, frames_len=flen, shm_base=case["shm_base"], cap=case["cap"],
                        out=out, counts=cnt)
    return got, buf[shift:], cnt


@pytest.fixture(scope="module")
def models():
    assert sorted(tc.models()) == sorted(tc.CASE_NAMES)
    return tc.models()


def test_cases_cover_every_status(models):
    for name in ("big", f"big_bits{tc.BIG_HASH_BITS}"):
        cnt = models[name][1]["counts"]
        assert all(int(cnt[i]) > 100 for i in range(5)), (name, cnt)
    cnt = models["route"][1]["counts"]
    assert all(int(cnt[i]) > 0 for i in (0, 1, 2, 4)), cnt
    assert int(models["refuse"][1]["counts"][3]) == 9
    assert 1000 <= len(models["grid"][0]["desc"]) <= 2000
    assert int(models["grid"][1]["counts"][0]) == len(models["grid"][0]["desc"])


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_host_equals_model(g, models, name):
    case, want = models[name]
    m = len(case["desc"])
    for shift, with_hash, counts in ((0, True, True), (3, False, False)):
        got, buf, cnt = run_host(g, case, shift=shift, with_hash=with_hash, counts=counts)
        compare(got, want, m, name)
        assert np.array_equal(buf, want["frames"]), name
        if counts:
            assert (cnt - 5).tolist() == want["counts"].tolist()
            assert int(want["counts"][:4].sum()) == m


def test_local_hash_is_the_references_toeplitz(g, models):
    from oracle import orc
    case, want = models["big"]
    n = case["net"]
    loc = np.nonzero(want["tx_olflags"] & g.TXFLAG_LOCAL_HINT)[0]
    assert len(loc) > 100
    got, _, _ = run_host(g, case)
    for j in loc[:400].tolist():
        d = case["desc"][j]
        nh = int(want["cmd"][j]) & 0xFFFFFFFF
        assert int(got["hash"][j]) == orc.do_toeplitz(tc.RSS_KEY, n["addr"], nh, int(d["lport"]), int(d["rport"]))
        assert int(got["hash"][j]) == g.toeplitz(tc.RSS_KEY, n["addr"].to_bytes(4, "big") + nh.to_bytes(4, "big") +
                                                int(d["lport"]).to_bytes(2, "big") +
                                                int(d["rport"]).to_bytes(2, "big"))


def test_cmd_and_payload_decode(g, models):
    case, _ = models["route_localgw"]
    got, _, _ = run_host(g, case)
    m = len(case["desc"])
    seen_local = seen_remote = 0
    for j in range(m):
        cmd, pay, st = int(got["cmd"][j]), int(got["payload"][j]), int(got["status"][j])
        if st != g.TXH_OK:
            assert cmd == 0 and pay == 0
            continue
        fl = int(got["tx_olflags"][j])
        assert cmd >> 63 == 0 and cmd >> 56 == 0            # txcmd = TXPKT_NET_XMIT
        assert cmd >> 48 & 0xFF == fl
        assert cmd >> 32 & 0xFFFF == int(got["pkt_len"][j])
        assert pay & (1 << 48) - 1 == case["shm_base"] + int(case["frame_off"][j])
        assert pay >> 48 == int(got["hash"][j]) & 0xFFFF == g.lib.gcl_txpkt_rss(pay)
        if fl & g.TXFLAG_LOCAL:
            assert fl & g.TXFLAG_LOCAL_HINT and cmd & 0xFFFFFFFF in (tc.LOCAL_IP, tc.GATEWAY)
            seen_local += 1
        else:
            assert cmd & 0xFFFFFFFF == 0 and int(got["hash"][j]) == 0
            seen_remote += 1
    assert seen_local and seen_remote


@pytest.mark.parametrize("ipcsum", [0, 1])
def test_round_trip_through_checksum_and_payload(g, models, ipcsum):
    """The frames gcl_tx_hdr_host built, through gcl_l4_csum_host FILL and
    VERIFY, gcl_rx_csum_flags and gcl_l4_payload_host.  The runtime asks the
    NIC for no UDP checksum (tx_olflags has no TCP_CHKSUM bit for UDP), so
    with the produced tx_olflags a UDP datagram stays NONE; a FILL of every
    packet (tx_olflags NULL) makes it GOOD as well."""
    case = dict(models["grid"][0])
    case["net"] = dict(case["net"], flags=g.TXH_IP_CSUM if ipcsum else 0)
    m = len(case["desc"])
    got, buf, _ = run_host(g, case)
    frames = buf[tc.GUARD:tc.GUARD + case["frames_len"]]
    # the caller's part: option bytes (NOPs) and payload
    for j in range(m):
        d = case["desc"][j]
        o = int(case["frame_off"][j])
        hl = 4 * int(d["tcp_off"]) if d["proto"] == 6 else 8
        frames[o + 54:o + 34 + hl] = 1
        frames[o + 34 + hl:o + 34 + hl + int(d["paylen"])] = np.arange(int(d["paylen"]), dtype=np.uint8) ^ (j & 0xFF)
    offs, pl, fl = case["frame_off"], got["pkt_len"][:m].copy(), got["tx_olflags"][:m].copy()
    ok = got["status"][:m] == g.TXH_OK
    tcp = case["desc"]["proto"] == 6
    assert ok.all()
    st = g.l4_csum_host(frames, pl, mode=g.L4_VERIFY, offs=offs, n=m)
    assert (st[:m][~tcp] == g.L4_NONE).all()
    if ipcsum:
        for j in range(0, m, 7):
            o = int(offs[j])
            assert g.rx_csum_flags(bytes(frames[o:o + int(pl[j])]), 0) & g.F_IP_CKSUM_MASK == g.F_IP_CKSUM_GOOD
    g.l4_csum_host(frames, pl, mode=g.L4_FILL, offs=offs, n=m, tx_olflags=fl)
    st = g.l4_csum_host(frames, pl, mode=g.L4_VERIFY, offs=offs, n=m)
    assert (st[:m][tcp] == g.L4_GOOD).all() and (st[:m][~tcp] == g.L4_NONE).all()
    for j in range(0, m, 7):
        o = int(offs[j])
        assert g.rx_csum_flags(bytes(frames[o:o + int(pl[j])]), 0) & g.F_IP_CKSUM_MASK == g.F_IP_CKSUM_GOOD
    g.l4_csum_host(frames, pl, mode=g.L4_FILL, offs=offs, n=m)
    st = g.l4_csum_host(frames, pl, mode=g.L4_VERIFY, offs=offs, n=m)
    assert (st[:m] == g.L4_GOOD).all()
    pay = g.l4_payload_host(frames, pl, offs=offs, n=m, l4_status=st)
    d = case["desc"]
    hl = np.where(tcp, 4 * d["tcp_off"].astype(np.uint64), 8).astype(np.uint64)
    assert pay["src_off"][:m].tolist() == (offs + 34 + hl).tolist()
    assert pay["len"][:m].tolist() == d["paylen"].tolist()
    assert pay["kind"][:m].tolist() == np.where(tcp, g.PAY_TCP, g.PAY_UDP).tolist()
    meta = pay["meta"][:m]
    saddr = np.where(d["lip"] == 0, tc.ADDR, d["lip"])
    assert meta["rip"].tolist() == saddr.tolist() and meta["rport"].tolist() == d["lport"].tolist()
    assert meta["proto"].tolist() == d["proto"].tolist()
    assert meta["tcp_flags"].tolist() == np.where(tcp, d["tcp_flags"], 0).tolist()
    assert meta["seq"].tolist() == np.where(tcp, d["seq"], 0).tolist()
    assert meta["ack"].tolist() == np.where(tcp, d["ack"], 0).tolist()


def test_neigh_table_set_replace_clear_and_errors(g):
    t = g.NeighTable()
    assert len(t) == 0 and t.lookup(tc.GATEWAY) is None
    t.set(tc.BASE_NEIGH)
    assert len(t) == len(tc.BASE_NEIGH)
    for a, mac in tc.BASE_NEIGH:
        assert t.lookup(a) == mac
    assert t.lookup(tc.OFF_LINK) is None and t.lookup(0) is None
    t.set([(0, b"\x02\0\0\0\0\x09"), (tc.OFF_LINK, b"\x02\0\0\0\0\x0a")])   # address 0 is a key like any other
    assert len(t) == 2 and t.lookup(0) == b"\x02\0\0\0\0\x09" and t.lookup(tc.GATEWAY) is None
    with pytest.raises(OSError) as e:
        t.set([(5, tc.MAC), (6, tc.MAC), (5, tc.MAC)])
    assert e.value.errno == errno.EEXIST
    big = np.zeros(g.NEIGH_MAX_ENTRIES + 1, dtype=g.NEIGH_ENTRY_DTYPE)
    big["ip"] = np.arange(len(big)) + 100
    with pytest.raises(OSError) as e:
        t.set(big)
    assert e.value.errno == errno.ENOSPC
    assert g.lib.gcl_neigh_tbl_set(t._tbl, None, 3) == -errno.EINVAL
    assert g.lib.gcl_neigh_tbl_set(None, None, 0) == -errno.EINVAL
    assert g.lib.gcl_neigh_tbl_hash_bits(t._tbl, 0) == -errno.EINVAL
    assert g.lib.gcl_neigh_tbl_hash_bits(t._tbl, 33) == -errno.EINVAL
    # every error left the previous set in place
    assert len(t) == 2 and t.lookup(0) == b"\x02\0\0\0\0\x09" and t.lookup(5) is None
    t.set(big[:-1])                                                        # the full table
    assert len(t) == g.NEIGH_MAX_ENTRIES
    assert t.lookup(100) == bytes(6) and t.lookup(100 + g.NEIGH_MAX_ENTRIES) is None
    t.set([])
    assert len(t) == 0 and t.lookup(100) is None


@pytest.mark.parametrize("bits", [32, tc.BIG_HASH_BITS])
def test_neigh_table_finds_every_key_and_no_other(g, bits):
    neigh = tc.big_neigh()
    t = g.NeighTable(hash_bits=bits)
    t.set(neigh)
    have = dict(neigh)
    for a, mac in neigh:
        assert t.lookup(a) == mac
    rng = np.random.default_rng(3)
    for a in rng.integers(0, 2 ** 32, 5000).tolist() + [a + 1 for a, _ in neigh[:2000]]:
        assert t.lookup(a) == have.get(a)


def test_neigh_table_placement_failure_keeps_the_set(g):
    t = g.NeighTable()
    t.set(tc.BASE_NEIGH)
    t.hash_bits(1)      # two home hashes: at most eight slots can be reached
    with pytest.raises(OSError) as e:
        t.set([(1000 + i, tc.MAC) for i in range(64)])
    assert e.value.errno == errno.ENOSPC
    assert len(t) == len(tc.BASE_NEIGH) and t.lookup(tc.GATEWAY) == tc.mac_of(tc.GATEWAY)
    assert t.lookup(1000) is None


def test_einval(g):
    case = tc.route()[0]
    m = len(case["desc"])
    buf = np.zeros(case["frames_len"], dtype=np.uint8)
    out = blank_outputs(m)
    net = g.txh_net(**case["net"])

    def call(tin_kw=None, out_kw=None, key=tc.RSS_KEY):
        o = dict(out, **(out_kw or {}))
        kw = dict(size=ctypes.sizeof(g.GclTxhIn), desc=case["desc"].ctypes.data,
                  frame_off=case["frame_off"].ctypes.data, m=m, frames=buf.ctypes.data, frames_len=len(buf),
                  net=net)
        kw.update(tin_kw or {})
        tin = g.GclTxhIn(**kw)
        tout = g.GclTxhOut(**{f: (None if o[f] is None else o[f].ctypes.data) for f in g.TXH_OUT_FIELDS})
        return g.lib.gcl_tx_hdr_host(None, key, ctypes.byref(tin), ctypes.byref(tout), None)

    assert call() == 0
    assert call(out_kw=dict(hash=None)) == 0
    assert call(dict(m=0, desc=None, frames=None)) == 0
    for kw in (dict(size=80), dict(desc=None), dict(frame_off=None), dict(frames=None), dict(m=2 ** 31 + 1),
               dict(frames_len=2 ** 64 - 1)):
        assert call(kw) == -errno.EINVAL, kw
    for f in ("cmd", "payload", "pkt_len", "tx_olflags", "status"):
        assert call(out_kw={f: None}) == -errno.EINVAL, f
    assert call(key=None) == -errno.EINVAL
    assert g.lib.gcl_tx_hdr_host(None, tc.RSS_KEY, None, None, None) == -errno.EINVAL
