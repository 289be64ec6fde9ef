"""Generate tests/golden/txpath_ref.json from the REFERENCE's own transmit
path: tcp_push_tcphdr (runtime/net/tcp_out.c:54-87), the checksum routines of
inc/net/chksum.h, and net_push_iphdr / net_get_ip_route
(runtime/net/core.c:592-626), compiled in place into
oracle/_ref/libtcpout_ref.so and libcore_ref.so by oracle/Makefile
(oracle/ref_tcpout.c, oracle/ref_core.c).

Run where /root/reference exists (after `make -C oracle ref`):
    python tests/golden/make_txpath_ref.py

The file holds inputs and the reference's outputs only.  tests/txpathcases.py
reads it; tests/test_txpath_ref.py calls build() where oracle/_ref is built
and requires the result equal to the committed file.

"l4": TCP segments and UDP datagrams.  Inputs: the tuple, seq, ack, win and
wscale (pcb.rcv_nxt_wnd = win << 32 | ack, pcb.rcv_wscale), flags, off, the
payload ("hex", or "gen": [a, b, c] for "payload_formula"), aux (null, or
[has_ecn, ecn]).  Outputs: "l4hdr_offload"/"l4hdr_full", the TCP header with
netcfg.no_tx_offloads 0/1; "phdr" and "cksum", ipv4_phdr_cksum and
ipv4_udptcp_cksum over the header (sum field 0) and payload, as the uint16_t
returned (in memory: value & 0xFF, value >> 8); "iphdr_offload"/"iphdr_full",
net_push_iphdr in front of it; "nh", net_get_ip_route(rip) under "net".  A UDP
record's "l4hdr_offload" is an INPUT: udp_send_raw (udp.c:24-40) is not
compiled, its four fields are written here.
"ip": net_push_iphdr alone: every ecn byte, the cases without aux.  "lip" is
the descriptor's address and "saddr" what net_tx_ip (core.c:693-698) makes of
it; that rule is not compiled (net_tx_ip needs ARP), it stays pinned to the
model only, and net_push_iphdr is recorded with the saddr it yields.
"route": net_get_ip_route under each record's own addr/netmask/gateway.
"raw": raw_cksum over "buf".
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402

OUT = os.path.join(HERE, "txpath_ref.json")
SEED = 0x7C9A
TCP, UDP = 6, 17
FORMULA = "bytes((a * i + b * (i >> 8) + c) & 0xFF for i in range(n))"
STORE_MAX = 1472            # longer payloads are "gen" only
MAX_TCP_PAY = 65535 - 14 - 20 - 20


def ip(a, b, c, d):
    return a << 24 | b << 16 | c << 8 | d


NET = {"addr": ip(10, 0, 0, 5), "netmask": 0xFFFFFF00, "gateway": ip(10, 0, 0, 1)}
LOOPBACK = ip(127, 0, 0, 1)
DESTS = [ip(10, 0, 0, 20), ip(10, 0, 0, 21), ip(192, 168, 7, 9), ip(10, 0, 0, 22), NET["gateway"],
         ip(10, 0, 0, 23), ip(8, 8, 8, 8)]
TCP_LENS = [0, 1, 2, 3, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 257, 535, 536, 1459, 1460, 8960]
UDP_LENS = [0, 1, 1471, 1472]
EDGE32 = [0, 2 ** 32 - 1, 2 ** 31 - 1, 2 ** 31]


def gen_payload(n, a, b, c):
    return eval(FORMULA, {"__builtins__": {}, "bytes": bytes, "range": range, "n": n, "a": a, "b": b, "c": c})


def le_words(b):
    """the exact sum of @b's 16-bit words as raw_cksum reads them"""
    b = bytes(b) + (b"\0" if len(b) & 1 else b"")
    return sum(b[i] | b[i + 1] << 8 for i in range(0, len(b), 2))


class Gen:
    def __init__(self):
        self.t = orc.ref_tcpout()
        self.x = orc.ref_txip()
        if self.t is None or self.x is None:
            raise SystemExit("oracle/_ref/libtcpout_ref.so or libcore_ref.so not built (make -C oracle ref)")
        self.rnd = random.Random(SEED)
        self.l4 = []

    def udp_hdr(self, lport, rport, paylen):
        return lport.to_bytes(2, "big") + rport.to_bytes(2, "big") + (paylen + 8).to_bytes(2, "big") + b"\0\0"

    def add(self, name, proto, payload=None, gen=None, paylen=None, **kw):
        """one "l4" record; payload bytes, or gen (a, b, c) with paylen"""
        rnd, i = self.rnd, len(self.l4)
        r = {"name": name, "proto": proto,
             "lip": kw.get("lip", ip(10, 0, 0, 5 + i % 2)), "lport": kw.get("lport", rnd.getrandbits(16)),
             "rip": kw.get("rip", DESTS[i % len(DESTS)]), "rport": kw.get("rport", rnd.getrandbits(16)),
             "seq": kw.get("seq", rnd.getrandbits(32)), "ack": kw.get("ack", rnd.getrandbits(32)),
             "win": kw.get("win", rnd.getrandbits(16)), "wscale": kw.get("wscale", 0),
             "flags": kw.get("flags", 0x18 if i & 1 else 0x10), "off": 5,
             "aux": kw.get("aux", [None, [1, i % 4], [0, 3]][i % 3])}
        if proto == UDP:
            r.update(seq=0, ack=0, win=0, wscale=0, flags=0, off=0)
        if gen is not None:
            payload = gen_payload(paylen, *gen)
            r["gen"] = list(gen)
        else:
            payload = bytes(payload)
            assert len(payload) <= STORE_MAX
            r["hex"] = payload.hex()
        r["paylen"] = len(payload)
        if proto == TCP:
            args = (r["lip"], r["lport"], r["rip"], r["rport"], r["seq"], r["ack"], r["win"], r["wscale"],
                    r["flags"], r["off"], payload)
            off_hdr, full_hdr = self.t.tcphdr(0, *args), self.t.tcphdr(1, *args)
            r["l4hdr_offload"], r["l4hdr_full"] = off_hdr.hex(), full_hdr.hex()
            l4 = full_hdr[:16] + b"\0\0" + full_hdr[18:] + payload
        else:
            l4 = self.udp_hdr(r["lport"], r["rport"], len(payload)) + payload
            r["l4hdr_offload"] = l4[:8].hex()
        r["phdr"] = self.t.ipv4_phdr_cksum(proto, r["lip"], r["rip"], len(l4))
        r["cksum"] = self.t.ipv4_udptcp_cksum(proto, r["lip"], r["rip"], l4)
        if proto == TCP:    # two outputs of the reference that must agree
            assert full_hdr[16] | full_hdr[17] << 8 == r["cksum"] and off_hdr[16] | off_hdr[17] << 8 == r["phdr"]
        iphdr, route = self.x
        aux = None if r["aux"] is None else tuple(r["aux"])
        r["iphdr_offload"] = iphdr(0, proto, r["rip"], r["lip"], len(l4), aux).hex()
        r["iphdr_full"] = iphdr(1, proto, r["rip"], r["lip"], len(l4), aux).hex()
        r["nh"] = route(NET["addr"], NET["netmask"], NET["gateway"], r["rip"])
        self.l4.append(r)
        return r

    def solved(self, name, proto, target=None, paylen=64, **kw):
        """A payload whose last word is solved for.  @target None: the
        complemented checksum is 0 (the reference returns 0xFFFF); else the
        exact sum of the L4 bytes' 16-bit words (field 0) is @target."""
        rnd = self.rnd
        lport, rport = (1, 2) if target else (rnd.getrandbits(16), rnd.getrandbits(16))
        lip, rip = kw.pop("lip", ip(10, 0, 0, 5)), kw.pop("rip", ip(10, 0, 0, 20))
        seq, ack, win = (1, 2, 3) if target else (rnd.getrandbits(32), rnd.getrandbits(32), rnd.getrandbits(16))
        if proto == TCP:
            hdr = self.t.tcphdr(1, lip, lport, rip, rport, seq, ack, win, 0, 0x10, 5, b"")
            hdr = hdr[:16] + b"\0\0" + hdr[18:]
        else:
            hdr = self.udp_hdr(lport, rport, paylen)
        if target is None:
            body = bytes(rnd.getrandbits(8) for _ in range(paylen - 2))
            c = self.t.ipv4_udptcp_cksum(proto, lip, rip, hdr + body + b"\0\0")
            last = c       # adding the complement of the sum so far brings it to 0xFFFF
        else:
            body = b""
            while target - le_words(hdr + body) > 0xFFFF:
                body += b"\xff\xff"
            body = body.ljust(paylen - 2, b"\0")
            last = target - le_words(hdr + body)
            assert 0 <= last <= 0xFFFF and len(body) == paylen - 2
        payload = body + bytes([last & 0xFF, last >> 8])
        r = self.add(name, proto, payload, lip=lip, rip=rip, lport=lport, rport=rport, seq=seq, ack=ack,
                     win=win, flags=0x10, **kw)
        if target is None:
            assert r["cksum"] == 0xFFFF and self.t.raw_cksum(hdr + payload) + r["phdr"] in (0xFFFF, 0x1FFFE)
        return r


def build():
    g = Gen()
    rnd = g.rnd

    def rand(n):
        return bytes(rnd.getrandbits(8) for _ in range(n))

    for n in TCP_LENS:
        if n <= STORE_MAX:
            g.add(f"tcp_len{n}", TCP, rand(n))
        else:
            g.add(f"tcp_len{n}", TCP, gen=(rnd.getrandbits(8) | 1, rnd.getrandbits(8), rnd.getrandbits(8)), paylen=n)
    for k, (s, a) in enumerate(zip(EDGE32, EDGE32[1:] + EDGE32[:1])):
        g.add(f"tcp_seq{s:#x}_ack{a:#x}", TCP, rand(12 + k), seq=s, ack=a)
    for win, ws in ((0, 0), (0xFFFF, 0), (0xFFFF << 7, 7), (0x7FFFFFFF, 14), (0x12345678, 3), (0x8000, 15)):
        g.add(f"tcp_win{win:#x}_ws{ws}", TCP, rand(9), win=win, wscale=ws)
    for fl in (0x10, 0x18, 0xFF, 0x02, 0x11):
        g.add(f"tcp_flags{fl:#x}", TCP, rand(5), flags=fl)
    g.add("tcp_max", TCP, gen=(167, 13, 101), paylen=MAX_TCP_PAY)
    for n in UDP_LENS:
        g.add(f"udp_len{n}", UDP, rand(n))
    for proto, nm in ((TCP, "tcp"), (UDP, "udp")):
        g.add(f"{nm}_zeros", proto, gen=(0, 0, 0), paylen=64)
        g.add(f"{nm}_ff_odd", proto, gen=(0, 0, 0xFF), paylen=1459)
        g.add(f"{nm}_ff_even", proto, gen=(0, 0, 0xFF), paylen=1460)
        g.add(f"{nm}_ff_big_odd", proto, gen=(0, 0, 0xFF), paylen=8959)
        g.add(f"{nm}_ff_big_even", proto, gen=(0, 0, 0xFF), paylen=8960)
        g.solved(f"{nm}_zero_result", proto)
    # the exact word sum of the L4 bytes: one and two carries over 0xFFFE
    g.solved("udp_sum_1fffe", UDP, target=0x1FFFE, paylen=16)
    g.solved("udp_sum_2fffe", UDP, target=0x2FFFE, paylen=16)
    g.solved("tcp_sum_2fffe", TCP, target=0x2FFFE, paylen=32)
    # raw_cksum(l4) and the pseudo-header sum both 0xFFFF: ipv4_udptcp_cksum's own sum is
    # 0x1FFFE before its one carry, and the result is the 0 that becomes 0xFFFF
    rip = ip(10, 0, 0, 20)
    lip = next(a for a in range(ip(10, 0, 0, 0), ip(10, 1, 0, 0))
               if g.t.ipv4_phdr_cksum(UDP, a, rip, 24) == 0xFFFF)
    r = g.solved("udp_total_1fffe", UDP, target=0xFFFF, paylen=16, lip=lip, rip=rip)
    assert r["phdr"] == 0xFFFF and r["cksum"] == 0xFFFF

    iphdr, route = g.x
    ips = []

    def add_ip(proto, daddr, lip, paylen, aux):
        saddr = lip if lip else (LOOPBACK if daddr == LOOPBACK else NET["addr"])   # core.c:693-698, not compiled
        l4bytes = (20 if proto == TCP else 8) + paylen
        a = None if aux is None else tuple(aux)
        off_hdr, full = iphdr(0, proto, daddr, saddr, l4bytes, a), iphdr(1, proto, daddr, saddr, l4bytes, a)
        ips.append({"proto": proto, "daddr": daddr, "lip": lip, "saddr": saddr, "paylen": paylen,
                    "l4bytes": l4bytes, "aux": aux, "hdr_offload": off_hdr.hex(), "hdr_full": full.hex(),
                    "cksum": g.t.ipv4_cksum(off_hdr),
                    "nh": route(NET["addr"], NET["netmask"], NET["gateway"], daddr)})

    for e in range(256):
        add_ip(TCP if e & 4 else UDP, DESTS[e % len(DESTS)], ip(10, 0, 0, 5 + e % 3), (e * 3) % 200, [1, e])
    for e in (0, 1, 2, 3, 0x80, 0x83, 0xFF):
        add_ip(TCP if e & 1 else UDP, DESTS[e % len(DESTS)], ip(10, 0, 0, 6), 10 + e % 7, [0, e])
    for k in range(4):
        add_ip(TCP if k & 1 else UDP, DESTS[k], ip(10, 0, 0, 5), 30 + k, None)
    for proto in (TCP, UDP):
        for daddr in (LOOPBACK, ip(10, 0, 0, 20), ip(192, 168, 7, 9), NET["addr"]):
            add_ip(proto, daddr, 0, 11, None)
    add_ip(TCP, ip(255, 255, 255, 255), ip(255, 255, 255, 255), 65535 - 14 - 20 - 20, [1, 3])
    add_ip(UDP, ip(10, 0, 0, 20), ip(10, 0, 0, 5), 0, None)

    routes = []
    addr, gw = ip(10, 0, 0, 5), ip(10, 0, 0, 1)
    for mask in (0, 0xFFFFFF00, 0xFFFFFFFF, 0xFFFF0000, 0x80000000):
        for daddr in (ip(10, 0, 0, 20), ip(10, 0, 1, 20), ip(192, 168, 7, 9), gw, addr, 0, 0xFFFFFFFF,
                      ip(10, 0, 0, 255), ip(138, 0, 0, 5)):
            routes.append({"addr": addr, "netmask": mask, "gateway": gw, "daddr": daddr,
                           "nh": route(addr, mask, gw, daddr)})
    # a gateway outside the subnet, and one that is the runtime's own address
    for gw2 in (ip(172, 16, 0, 1), addr):
        for daddr in (ip(10, 0, 0, 20), ip(192, 168, 7, 9), gw2):
            routes.append({"addr": addr, "netmask": 0xFFFFFF00, "gateway": gw2, "daddr": daddr,
                           "nh": route(addr, 0xFFFFFF00, gw2, daddr)})

    raws = []
    for buf in [b"", b"\x01", b"\x01\x02", b"\x01\x02\x03", rand(7), rand(8), rand(9), rand(20), rand(21),
                b"\xff" * 20, b"\xff" * 21, b"\xff\xff" + b"\x01\x00", b"\xff" * 1472, b"\xff" * 1473]:
        raws.append({"buf": buf.hex(), "sum": g.t.raw_cksum(buf)})

    return {"source": "reference tcp_push_tcphdr (runtime/net/tcp_out.c:54-87), inc/net/chksum.h, net_push_iphdr "
                      "and net_get_ip_route (runtime/net/core.c:592-626) via oracle/_ref/libtcpout_ref.so and "
                      "libcore_ref.so; a record with \"gen\": [a, b, c] has the payload payload_formula makes for "
                      "n = paylen; the saddr of a record whose lip is 0 follows net_tx_ip (core.c:693-698), which "
                      "is not compiled: that rule is pinned to the model only; a UDP l4hdr_offload is an input",
            "payload_formula": FORMULA, "seed": SEED, "net": NET, "l4": g.l4, "ip": ips, "route": routes,
            "raw": raws}


def dumps(d):
    """one record per line"""
    out = ["{"]
    keys = list(d)
    for k in keys:
        end = "" if k == keys[-1] else ","
        if isinstance(d[k], list):
            out.append(f"{json.dumps(k)}: [")
            out += [json.dumps(r) + ("," if j + 1 < len(d[k]) else "") for j, r in enumerate(d[k])]
            out.append("]" + end)
        else:
            out.append(f"{json.dumps(k)}: {json.dumps(d[k])}{end}")
    out.append("}")
    return "\n".join(out) + "\n"


def main():
    d = build()
    text = dumps(d)
    assert json.loads(text) == d
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{len(d['l4'])} l4, {len(d['ip'])} ip, {len(d['route'])} route, {len(d['raw'])} raw vectors, "
          f"{len(text)} bytes")


if __name__ == "__main__":
    main()
