"""Generate tests/golden/tcpfin_ref.json from the REFERENCE's own
tcp_push_tcphdr (runtime/net/tcp_out.c:54-87, compiled in place into
oracle/_ref/libtcpout_ref.so by oracle/Makefile, oracle/ref_tcpout.c): the 20
TCP header bytes of the FIN tcp_tx_ctl(c, TCP_FIN | TCP_ACK, NULL) sends
(tcp_out.c:264-295) for every tuple of tests/shutcases.py golden_inputs():
flags 0x11, off 5, no payload, seg_seq = snd_nxt, pcb.rcv_nxt_wnd = rcv_wnd <<
32 | rcv_nxt, pcb.rcv_wscale, once with netcfg.no_tx_offloads 0 (the sum field
holds the pseudo-header sum, as the NIC wants it) and once with 1 (the whole
checksum).

Run where the reference tree is mounted (after `make -C oracle ref`):
    python tests/golden/make_tcpfin_ref.py

The file holds inputs and the reference's outputs only.
tests/test_shut_ref.py calls build() where oracle/_ref is built and requires the
result equal to the committed file; it and tests/test_gpu_shut.py hold the bytes
gcl_tx_hdr and gcl_l4_csum FILL make of gcl_tcp_shut's FIN descriptors to it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from tests import shutcases as sc  # noqa: E402

OUT = os.path.join(HERE, "tcpfin_ref.json")
TCP_FIN_ACK = 0x11


def build():
    t = orc.ref_tcpout()
    if t is None:
        raise SystemExit("oracle/_ref/libtcpout_ref.so not built (make -C oracle ref)")
    segs = []
    for r in sc.golden_inputs():
        hdr = [t.tcphdr(full, r["lip"], r["lport"], r["rip"], r["rport"], r["seq"], r["ack"], r["rcv_wnd"],
                        r["wscale"], TCP_FIN_ACK, 5, b"") for full in (0, 1)]
        segs.append(dict(r, hdr_offload=hdr[0].hex(), hdr_full=hdr[1].hex()))
    return {"source": "reference tcp_push_tcphdr (runtime/net/tcp_out.c:54-87) via oracle/_ref/libtcpout_ref.so, "
                      "called as tcp_tx_ctl(c, TCP_FIN | TCP_ACK, NULL) calls it (tcp_out.c:264-295): flags 0x11, "
                      "off 5, no payload; hdr_offload with netcfg.no_tx_offloads 0, hdr_full with 1; rcv_wnd is "
                      "the window before the shift by wscale",
            "segs": segs}


def dumps(d):
    """one record per line"""
    out = ["{", f"\"source\": {json.dumps(d['source'])},", "\"segs\": ["]
    out += [json.dumps(r) + ("," if j + 1 < len(d["segs"]) else "") for j, r in enumerate(d["segs"])]
    out += ["]", "}"]
    return "\n".join(out) + "\n"


def main():
    d = build()
    text = dumps(d)
    assert json.loads(text) == d
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{len(d['segs'])} segments, {len(text)} bytes")


if __name__ == "__main__":
    main()
