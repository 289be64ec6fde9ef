"""CPU: the host-only socket table (gcl_sock_tbl_*, include/gcl_host.h), which
runs the table build and the probe the GPU kernel shares (csrc/gcl_sock.h),
against the plain-Python definition of tests/sockcases.py and the
hand-derived fixture tests/golden/sock_cases.json."""
import numpy as np
import pytest

from tests import sockcases as sc

EINVAL, ENOSPC, EADDRINUSE = 22, 28, 98


@pytest.fixture(scope="module")
def g():
    from caladan_amd import gclassify
    return gclassify


def lookup(g, tbl, frames, raw, vbytes, tb=0, R=16, offs=None, frames_len=None, stride=64):
    region = np.ascontiguousarray(frames).reshape(-1)
    n = len(raw)
    return tbl.lookup(region, n, sc.pack_verdicts(raw, vbytes), vbytes, tb, R, stride=stride,
                      offs=offs, frames_len=frames_len)


def check(g, tbl, tables, frames, raw, vbytes, tb=0, R=16, what=""):
    region = np.ascontiguousarray(frames).reshape(-1)
    n = len(raw)
    want, wcnt = sc.expected(tables, region, len(region), np.arange(n, dtype=np.uint64) * 64, raw,
                             vbytes, tb, R)
    got, cnt = lookup(g, tbl, frames, raw, vbytes, tb, R)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"{what}: {len(bad)} of {n} differ, first at {bad[0]}: " \
                         f"{got[bad[0]]:#x} != {want[bad[0]]:#x}"
    assert cnt.tolist() == wcnt.tolist() and int(cnt.sum()) == n, what
    return want, wcnt


def test_constants_and_entry_layout(g):
    assert g.SOCK_ENTRY_DTYPE == sc.ENTRY and sc.ENTRY.itemsize == 20
    import ctypes
    assert ctypes.sizeof(g.GclSockEntry) == 20
    assert (g.SOCK_NA, g.SOCK_MISS, g.SOCK_MULTI, g.SOCK_COOKIE_MAX) == (sc.NA, sc.MISS, sc.MULTI, sc.COOKIE_MAX)
    assert (g.SOCK_HIT5, g.SOCK_HIT3, g.SOCK_HIT3_ANY, g.SOCK_N_MULTI, g.SOCK_N_MISS, g.SOCK_N_NA,
            g.SOCK_NR) == (sc.HIT5, sc.HIT3, sc.HIT3_ANY, sc.N_MULTI, sc.N_MISS, sc.N_NA, sc.NR)


@pytest.mark.parametrize("s", sc.golden_scenarios(), ids=lambda s: s["name"])
def test_golden_scenarios(g, s):
    """The hand-derived answers, through the library and through the Python
    definition (which the other tests then stand on)."""
    tbl = g.SockTable()
    for u, e in s["sets"].items():
        tbl.set(u, e)
    R = s["max_runtimes"]
    got, cnt = lookup(g, tbl, s["frames"], s["raw4"], 4, 0, R)
    for i, cite in enumerate(s["cites"]):
        assert got[i] == s["expect"][i], (s["name"], i, hex(got[i]), cite)
    assert cnt.tolist() == np.bincount(s["klass"], minlength=sc.NR).tolist()
    n = len(got)
    want, wcnt = sc.expected(sc.make_tables(s["sets"]), s["frames"].reshape(-1), n * 64,
                             np.arange(n, dtype=np.uint64) * 64, s["raw4"], 4, 0, R)
    assert want.tolist() == s["expect"].tolist() and wcnt.tolist() == cnt.tolist()


@pytest.mark.parametrize("vb,R,tb", [(8, 16, 0), (4, 4096, 0), (2, 64, 4), (2, 16, 8), (1, 16, 3), (1, 128, 0)])
def test_random_sets_every_verdict_width(g, vb, R, tb):
    rng = np.random.default_rng(1000 + vb + R)
    us = sorted(rng.choice(R, size=min(R, 12), replace=False).tolist())
    sets = sc.random_sets(rng, us[:-2], 60)  # two runtimes with no entries
    tbl = g.SockTable()
    for u, e in sets.items():
        tbl.set(u, e)
    n = 6000
    frames, u, kind = sc.traffic(rng, sets, n, us)
    raw = sc.verdicts_for(rng, u, vb, tb)
    _, cnt = check(g, tbl, sc.make_tables(sets), frames, raw, vb, tb, R, f"vb={vb}")
    assert cnt[:sc.N_NA + 1].min() > 0, cnt  # no class vacuously right
    # random verdict bytes: never out of bounds, equal to the definition
    check(g, tbl, sc.make_tables(sets), frames, sc.garbage_verdicts(rng, n, vb), vb, tb, R, "garbage")


def test_frames_cut_by_frames_len_offsets_and_alignment(g):
    """Offsets of every alignment, frames cut at every byte of [12, 38) by
    frames_len, offsets at and past it; the region goes on past frames_len
    with the bytes that would make the cut frame hit."""
    rng = np.random.default_rng(7)
    sets = sc.random_sets(rng, [3], 8)
    tbl = g.SockTable()
    tbl.set(3, sets[3])
    tables = sc.make_tables(sets)
    e = sets[3][sets[3]["match"] == sc.M5][0]
    f = sc.build_frames(rng, *(np.array([int(e[k])]) for k in ("proto", "lip", "lport", "rip", "rport")))[0]
    flen = 1000
    for k in range(0, 48):
        region = rng.integers(0, 256, size=flen + 128, dtype=np.uint8)
        region[flen - k:flen - k + 64] = f
        region[101:165] = f
        offs = np.array([flen - k, 101, flen, flen + 5, 1 << 40, (1 << 64) - 1, 0], dtype=np.uint64)
        raw = np.full(len(offs), 3, dtype=np.uint64)
        want, _ = sc.expected(tables, region, flen, offs, raw, 4, 0, 16)
        got, _ = tbl.lookup(region, len(offs), sc.pack_verdicts(raw, 4), 4, 0, 16, offs=offs, frames_len=flen)
        assert got.tolist() == want.tolist(), k
        assert want[1] == e["cookie"] and (want[0] == e["cookie"]) == (k >= 38), k
        assert (want[2:6] == sc.NA).all()


def test_set_error_returns_and_previous_set_survives(g):
    tbl = g.SockTable()
    ok = [(0x0A000001, 80, 6, 3, 7), (0x0A000001, 80, 6, 5, 8, 0x01020304, 99)]
    assert tbl.set(2, ok) == 0
    frames = sc.build_frames(np.random.default_rng(0), np.array([6, 6]), np.array([0x0A000001] * 2),
                             np.array([80, 80]), np.array([0x01020304, 5]), np.array([99, 99]))
    raw = np.array([2, 2], dtype=np.uint64)

    def answers():
        return lookup(g, tbl, frames, raw, 4)[0].tolist()

    assert answers() == [8, 7]
    bad = {
        "lport 0": ([(1, 0, 6, 3, 1)], EINVAL),
        "match 4": ([(1, 1, 6, 4, 1)], EINVAL),
        "match 0": ([(1, 1, 6, 0, 1)], EINVAL),
        "proto 1": ([(1, 1, 1, 3, 1)], EINVAL),
        "cookie past max": ([(1, 1, 6, 3, sc.COOKIE_MAX + 1)], EINVAL),
        "cookie MULTI": ([(1, 1, 6, 3, sc.MULTI)], EINVAL),
        "bad entry last": (ok + [(1, 0, 17, 5, 1, 2, 3)], EINVAL),
        "5-tuple twice": ([(9, 9, 17, 5, 1, 2, 3), (9, 9, 17, 3, 4), (9, 9, 17, 5, 5, 2, 3)], EADDRINUSE),
    }
    for what, (entries, err) in bad.items():
        with pytest.raises(OSError) as ei:
            tbl.set(2, entries)
        assert ei.value.errno == err, what
        assert answers() == [8, 7], what  # the previous set is still there
    with pytest.raises(OSError) as ei:
        tbl.set(4096, ok)
    assert ei.value.errno == EINVAL
    assert g.lib.gcl_sock_tbl_set(None, 0, None, 0) == -EINVAL
    assert g.lib.gcl_sock_tbl_set(tbl._tbl, 0, None, 1) == -EINVAL
    # the same 5-tuple in two runtimes is no conflict; the same 3-tuple twice is MULTI
    assert tbl.set(3, ok + [ok[0]]) == 0
    raw3 = np.array([3, 3], dtype=np.uint64)
    assert lookup(g, tbl, frames, raw3, 4)[0].tolist() == [8, sc.MULTI]
    assert answers() == [8, 7]
    # n == 0 clears, del drops, both leave the other runtime alone
    assert tbl.set(2, []) == 0
    assert answers() == [sc.MISS, sc.MISS]
    assert tbl.delete(3) == 0 and tbl.delete(3) == 0
    assert lookup(g, tbl, frames, raw3, 4)[0].tolist() == [sc.MISS, sc.MISS]
    with pytest.raises(OSError):
        tbl.delete(4096)


def test_more_than_max_entries_is_enospc(g):
    tbl = g.SockTable()
    e = np.zeros(g.SOCK_MAX_ENTRIES + 1, dtype=sc.ENTRY)
    e["lport"], e["proto"], e["match"] = 1, 6, sc.M3
    assert tbl.set(1, e[:5]) == 0
    with pytest.raises(OSError) as ei:
        tbl.set(2, e)                       # one set past the limit
    assert ei.value.errno == ENOSPC
    with pytest.raises(OSError) as ei:
        tbl.set(2, e[:g.SOCK_MAX_ENTRIES - 4])  # the context as a whole past it
    assert ei.value.errno == ENOSPC
    assert tbl.set(1, e[:1]) == 0


def test_lookup_error_returns(g):
    import ctypes
    tbl = g.SockTable()
    fr = np.zeros(640, dtype=np.uint8)
    v = np.zeros(10, dtype=np.uint32)
    out = np.full(10, 0x5A5A5A5A, dtype=np.uint32)

    def call(t=tbl._tbl, vb=4, tb=0, frames=fr.ctypes.data, frames_len=640, stride=64, nn=10,
             vv=v.ctypes.data, o=out.ctypes.data, batch=True):
        b = g.GclBatch(frames=frames, frames_len=frames_len, stride=stride, n=nn)
        return g.lib.gcl_sock_tbl_lookup_host(t, vb, tb, 16, ctypes.byref(b) if batch else None, vv, o, None)

    assert call(t=None) == -EINVAL and call(batch=False) == -EINVAL
    assert call(vv=None) == -EINVAL and call(o=None) == -EINVAL
    for vb in (0, 3, 5, 16):
        assert call(vb=vb) == -EINVAL
    assert call(tb=9) == -EINVAL
    assert call(frames=None) == -EINVAL and call(frames_len=(1 << 64) - 1) == -EINVAL
    assert call(nn=(1 << 40) + 1) == -EINVAL
    for stride in (0, 8, 24, (1 << 20) + 16):
        assert call(stride=stride) == -EINVAL
    assert (out == 0x5A5A5A5A).all()
    assert call(nn=0, frames=None) == 0 and (out == 0x5A5A5A5A).all()
    assert call() == 0 and (out == sc.NA).all()


def test_collision_knob_never_a_wrong_answer(g):
    """With the internal hash cut to a few bits every key falls into a few
    home buckets: the sets that can be placed are placed through long kick
    chains and every entry is found; the others are refused with -ENOSPC and
    the previous set stays.  200 entries at 2 bits (at most 16 slots in
    reach) cannot be placed."""
    rng = np.random.default_rng(21)
    placed_under_pressure = 0
    for bits in (2, 3, 4, 6):
        for n in (1, 2, 4, 7, 8, 12, 16, 24, 48, 200):
            tbl = g.SockTable(hash_bits=bits)
            keep = [(0x0A000001, 9, 6, 3, 77)]
            tbl.set(1, keep)
            e = np.zeros(n, dtype=sc.ENTRY)
            e["lip"], e["lport"] = 0x0A000005, 1 + rng.choice(65535, size=n, replace=False)
            e["proto"], e["match"] = 17, sc.M3
            e["cookie"] = np.arange(n) + 1000
            frames = sc.build_frames(rng, e["proto"].astype(np.int64), e["lip"].astype(np.int64),
                                     e["lport"].astype(np.int64), np.full(n, 5), np.full(n, 5))
            raw = np.full(n, 5, dtype=np.uint64)
            try:
                tbl.set(5, e)
            except OSError as err:
                assert err.errno == ENOSPC, (bits, n)
                assert (lookup(g, tbl, frames, raw, 4)[0] == sc.MISS).all(), (bits, n)
            else:
                assert lookup(g, tbl, frames, raw, 4)[0].tolist() == e["cookie"].tolist(), (bits, n)
                placed_under_pressure += n >= 2 ** bits
                assert (bits, n) != (2, 200)
            k = sc.build_frames(rng, np.array([6]), np.array([0x0A000001]), np.array([9]), np.array([1]), np.array([1]))
            assert lookup(g, tbl, k, np.array([1], dtype=np.uint64), 4)[0].tolist() == [77], (bits, n)
    assert placed_under_pressure >= 3
    with pytest.raises(OSError):
        g.SockTable(hash_bits=0)
    with pytest.raises(OSError):
        g.SockTable(hash_bits=33)


def test_hundred_thousand_entries_all_found(g):
    rng = np.random.default_rng(33)
    us = list(range(16))
    sets = sc.random_sets(rng, us, 100_000 // 16 + 200)
    assert sum(len(e) for e in sets.values()) >= 100_000
    tbl = g.SockTable()
    for u, e in sets.items():
        tbl.set(u, e)
    tables = sc.make_tables(sets)
    for u, e in sets.items():  # every entry, by a packet cut from it
        five = e["match"] == sc.M5
        lip = np.where(e["lip"] == 0, 0x0B000000 + u, e["lip"]).astype(np.int64)
        frames = sc.build_frames(rng, e["proto"].astype(np.int64), lip, e["lport"].astype(np.int64),
                                 np.where(five, e["rip"], 1).astype(np.int64),
                                 np.where(five, e["rport"], 1).astype(np.int64))
        raw = np.full(len(e), u, dtype=np.uint64)
        want, cnt = check(g, tbl, tables, frames, raw, 4, 0, 16, f"runtime {u}")
        assert (want[five] == e["cookie"][five]).all() and cnt[sc.N_MISS] == 0 and cnt[sc.N_NA] == 0
    # and a batch of mixed traffic over all of them
    frames, u, _ = sc.traffic(rng, sets, 20000)
    _, cnt = check(g, tbl, tables, frames, sc.verdicts_for(rng, u, 1, 3), 1, 3, 16, "mixed")
    assert cnt[:sc.N_NA + 1].min() > 0
    tbl.delete(7)
    sets.pop(7)
    check(g, tbl, sc.make_tables(sets), frames, sc.verdicts_for(rng, u, 4, 0), 4, 0, 16, "after del")
