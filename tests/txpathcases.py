"""tests/golden/txpath_ref.json (tests/golden/make_txpath_ref.py: the
reference's own tcp_push_tcphdr, chksum.h routines, net_push_iphdr and
net_get_ip_route, compiled in place) turned into the inputs of gcl_tx_hdr,
gcl_l4_csum and gcl_rx_csum, and the checks the CPU and GPU tests share.
Nothing here computes an expected byte: every one is read from the fixture.

Where the product's interface differs from the reference's on purpose, the
mapping is made here, once:
  gcl_txh_desc.win is the window as it goes on the wire (include/gclassify.h,
    struct gcl_txh_desc: "already scaled"), so win = (win >> wscale) & 0xFFFF
    of the recorded pcb values;
  gcl_txh_desc.ecn carries has_ecn in bit 7 and the codepoint in bits 0-1
    (the same struct), so ecn = has_ecn << 7 | (aux.ecn & 0x7F): bits 2-6 of
    the reference's ecn byte go along and must be ignored as IPTOS_ECN_MASK
    ignores them; no aux is ecn 0.
"""
import functools
import json
import os

import numpy as np

from caladan_amd import gclassify as G
from tests import l4cases as lc
from tests import txhcases as tc

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "txpath_ref.json")
TCP, UDP = 6, 17
MAC = tc.MAC


@functools.lru_cache(maxsize=None)
def load():
    with open(PATH) as f:
        return json.load(f)


def gen_payload(formula, n, a, b, c):
    return eval(formula, {"__builtins__": {}, "bytes": bytes, "range": range, "n": n, "a": a, "b": b, "c": c})


@functools.lru_cache(maxsize=None)
def payloads():
    """the payload bytes of every "l4" record, in order"""
    d = load()
    out = []
    for r in d["l4"]:
        p = bytes.fromhex(r["hex"]) if "hex" in r else gen_payload(d["payload_formula"], r["paylen"], *r["gen"])
        assert len(p) == r["paylen"]
        out.append(p)
    return out


def desc_ecn(aux):
    return 0 if aux is None else (0x80 if aux[0] else 0) | (aux[1] & 0x7F)


def l4_row(r):
    return dict(lip=r["lip"], rip=r["rip"], lport=r["lport"], rport=r["rport"], proto=r["proto"],
                tcp_flags=r["flags"], tcp_off=r["off"], ecn=desc_ecn(r["aux"]), seq=r["seq"], ack=r["ack"],
                win=(r["win"] >> r["wscale"]) & 0xFFFF, paylen=r["paylen"], pad=0xFEED0000)


def ip_row(i, r):
    return dict(lip=r["lip"], rip=r["daddr"], lport=3000 + i, rport=4000 + 3 * i, proto=r["proto"],
                tcp_flags=0x10, tcp_off=5, ecn=desc_ecn(r["aux"]), seq=i, ack=2 * i, win=i, paylen=r["paylen"],
                pad=i)


def net_of(n, flags=0):
    return dict(addr=n["addr"], netmask=n["netmask"], gateway=n["gateway"], mac=MAC, min_pkt_size=0, flags=flags)


def _place(lens):
    """frame i at the next free offset that is i mod 16"""
    offs, cur = [], 0
    for i, ln in enumerate(lens):
        cur += (i - cur) % 16
        offs.append(cur)
        cur += ln
    return offs, cur + 16


def _frame_len(proto, paylen):
    return 14 + 20 + (20 if proto == TCP else 8) + paylen


@functools.lru_cache(maxsize=None)
def txh_case(ip_csum):
    """(a txhcases case over every "l4" and "ip" record under the fixture's
    net, expect): expect[j] = (the recorded bytes from frame byte 14 on, the
    recorded next hop).  @ip_csum: GCL_TXH_IP_CSUM, netcfg.no_tx_offloads."""
    d = load()
    rows = [l4_row(r) for r in d["l4"]] + [ip_row(i, r) for i, r in enumerate(d["ip"])]
    key = "full" if ip_csum else "offload"
    expect = [(bytes.fromhex(r["iphdr_" + key]) + bytes.fromhex(r["l4hdr_offload"]), r["nh"]) for r in d["l4"]]
    expect += [(bytes.fromhex(r["hdr_" + key]), r["nh"]) for r in d["ip"]]
    offs, flen = _place([_frame_len(r["proto"], r["paylen"]) for r in rows])
    hops = sorted({nh for _, nh in expect})
    neigh = [(nh, tc.mac_of(nh)) for nh in hops]
    return tc.case(f"txpath_ipcsum{int(ip_csum)}", rows, offs, flen, neigh,
                   net_of(d["net"], G.TXH_IP_CSUM if ip_csum else 0)), expect


@functools.lru_cache(maxsize=None)
def route_cases():
    """[(a case of one net configuration: a UDP datagram to every recorded
    daddr, with a neighbour entry for every address that could be the next
    hop, the recorded next hops)]"""
    d = load()
    groups = {}
    for r in d["route"]:
        groups.setdefault((r["addr"], r["netmask"], r["gateway"]), []).append(r)
    out = []
    for (addr, mask, gw), recs in groups.items():
        rows = [dict(lip=0, rip=r["daddr"], lport=5000 + i, rport=53, proto=UDP, paylen=3) for i, r in enumerate(recs)]
        offs, flen = _place([_frame_len(UDP, 3)] * len(rows))
        cand = sorted({r["daddr"] for r in recs} | {gw})
        neigh = [(a, tc.mac_of(a)) for a in cand]
        n = dict(addr=addr, netmask=mask, gateway=gw, mac=MAC, min_pkt_size=0, flags=0)
        out.append((tc.case(f"txpath_route_{mask:#x}_{gw:#x}", rows, offs, flen, neigh, n), [r["nh"] for r in recs]))
    return out


def check_txh(case, expect, buf, out, what):
    """@buf: the frame region from its front guard on; @out: the outputs.
    Bytes 14.. of every frame are the recorded IP and L4 header; an entry that
    is sent (GCL_TXH_OK) carries the mac of the recorded next hop; one that is
    not is the runtime's own address or loopback (GCL_TXH_SELF: the reference
    hands those to net_tx_local_loopback before it routes, core.c:705-706)."""
    n = case["net"]
    sent = 0
    for j, (want, nh) in enumerate(expect):
        o = tc.GUARD + int(case["frame_off"][j])
        got = bytes(buf[o + 14:o + 14 + len(want)])
        assert got == want, (what, j, got.hex(), want.hex())
        rip = int(case["desc"]["rip"][j])
        if rip == n["addr"] or rip == tc.LOOPBACK:
            assert out["status"][j] == G.TXH_SELF, (what, j)
            continue
        assert out["status"][j] == G.TXH_OK, (what, j)
        assert bytes(buf[o:o + 14]) == tc.mac_of(nh) + MAC + b"\x08\x00", (what, j, hex(nh))
        sent += 1
    assert sent > len(expect) // 2


def check_route(case, hops, buf, out, what):
    n = case["net"]
    sent = 0
    for j, nh in enumerate(hops):
        o = tc.GUARD + int(case["frame_off"][j])
        rip = int(case["desc"]["rip"][j])
        if rip == n["addr"] or rip == tc.LOOPBACK:
            assert out["status"][j] == G.TXH_SELF, (what, j)
            continue
        assert out["status"][j] == G.TXH_OK, (what, j)
        assert bytes(buf[o:o + 6]) == tc.mac_of(nh), (what, j, hex(rip), hex(nh))
        sent += 1
    assert sent >= len(hops) - 1


# --- gcl_l4_csum ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def l4_frames(full=False):
    """Every "l4" record as a frame: an Ethernet header (type only), the
    recorded IP header, the recorded L4 header and the payload: as
    net_tx_ip leaves them for the NIC (@full False), or with every checksum
    the reference writes when netcfg.no_tx_offloads is set (@full True; a UDP
    record gets the recorded ipv4_udptcp_cksum, stored as the reference stores
    a sum: value & 0xFF, value >> 8)."""
    d = load()
    out = []
    for r, p in zip(d["l4"], payloads()):
        if not full:
            hdr = bytes.fromhex(r["iphdr_offload"]) + bytes.fromhex(r["l4hdr_offload"])
        elif r["proto"] == TCP:
            hdr = bytes.fromhex(r["iphdr_full"]) + bytes.fromhex(r["l4hdr_full"])
        else:
            u = bytes.fromhex(r["l4hdr_offload"])
            hdr = bytes.fromhex(r["iphdr_full"]) + u[:6] + bytes([r["cksum"] & 0xFF, r["cksum"] >> 8])
        f = np.frombuffer(bytes(12) + b"\x08\x00" + hdr + p, dtype=np.uint8).copy()
        f.setflags(write=False)
        out.append(f)
    return out


def l4_slots(frs):
    stride = -(-max(len(f) for f in frs) // 16) * 16
    return lc.slots(frs, stride)


def l4_packed(frs):
    """frame i at an offset that is i mod 16"""
    return lc.layout(frs, aligns=[i % 16 for i in range(len(frs))])


def check_filled(case, frames, status, what):
    """@frames after GCL_L4_FILL of the as-left-for-the-NIC frames: every
    frame equals the reference's no_tx_offloads = 1 bytes."""
    want = l4_frames(full=True)
    for i, w in enumerate(want):
        o = lc.start(case, i)
        got = frames[o:o + len(w)]
        assert status[i] == lc.FILLED_IP | lc.FILLED_L4, (what, i, status[i])
        bad = np.nonzero(got != w)[0]
        assert not len(bad), (what, load()["l4"][i]["name"], "first differing frame byte", int(bad[0]),
                              bytes(got[14:54]).hex(), bytes(w[14:54]).hex())


def flip_positions(f):
    """the first, a middle and the last L4 byte of frame @f outside the sum field"""
    proto, l4len = int(f[23]), len(f) - 34
    fo = 50 if proto == TCP else 40
    cov = [j for j in range(34, 34 + l4len) if j not in (fo, fo + 1)] if l4len < 64 else None
    if cov is not None:
        return cov[0], cov[len(cov) // 2], cov[-1]
    return 34, 34 + l4len // 2, 34 + l4len - 1    # a long frame: the middle and the end are payload


@functools.lru_cache(maxsize=None)
def flipped_frames(seed=0x51F7):
    """every full frame three times, one bit flipped (fixed seed) in its
    first, a middle and its last covered byte"""
    rng = np.random.default_rng(seed)
    out = []
    for f in l4_frames(full=True):
        for j in flip_positions(f):
            g = f.copy()
            g[j] ^= 1 << int(rng.integers(0, 8))
            out.append(g)
    return out


# --- gcl_rx_csum --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def rx_frames(seed=0x1C5):
    """(64-B frames, want_good): every recorded IP header carrying the
    reference's ipv4_cksum, then each again with one bit of its 20 bytes
    flipped (fixed seed), then each with one bit of the sum field flipped"""
    d = load()
    rng = np.random.default_rng(seed)
    hdrs = [bytes.fromhex(r["hdr_full"]) for r in d["ip"]] + [bytes.fromhex(r["iphdr_full"]) for r in d["l4"]]
    n = len(hdrs)
    fr = np.zeros((3 * n, 64), dtype=np.uint8)
    fr[:, 12] = 0x08
    for k in range(3):
        fr[k * n:(k + 1) * n, 14:34] = np.frombuffer(b"".join(hdrs), dtype=np.uint8).reshape(n, 20)
    for i in range(n):
        fr[n + i, 14 + int(rng.integers(0, 20))] ^= 1 << int(rng.integers(0, 8))
        fr[2 * n + i, 24 + int(rng.integers(0, 2))] ^= 1 << int(rng.integers(0, 8))
    return fr, np.arange(3 * n) < n
