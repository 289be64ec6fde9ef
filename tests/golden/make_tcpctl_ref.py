"""Generate tests/golden/tcpctl_ref.json from the REFERENCE's own
tcp_push_tcphdr (runtime/net/tcp_out.c:54-87, compiled in place into
oracle/_ref/libtcpout_ref.so by oracle/Makefile, oracle/ref_tcpout.c): the 20
TCP header bytes of every ACK and window probe the named cases of
tests/tcptmrcases.py send, as tcp_tx_ack and tcp_tx_probe_window
(tcp_out.c:178-228) call it: flags TCP_ACK, off 5, no payload, seg_seq =
snd_nxt or snd_una - 1, pcb.rcv_nxt_wnd = rcv_wnd << 32 | rcv_nxt,
pcb.rcv_wscale.

Run where the reference tree is mounted (after `make -C oracle ref`):
    python tests/golden/make_tcpctl_ref.py

The file holds inputs and the reference's outputs only.
tests/test_tcptmr_host.py calls build() where oracle/_ref is built and requires
the result equal to the committed file; it and tests/test_gpu_tcptmr.py hold
gcl_tx_hdr's bytes over the sweep's descriptors to it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from tests import tcptmrcases as tm  # noqa: E402

OUT = os.path.join(HERE, "tcpctl_ref.json")
TCP_ACK = 0x10


def build():
    t = orc.ref_tcpout()
    if t is None:
        raise SystemExit("oracle/_ref/libtcpout_ref.so not built (make -C oracle ref)")
    segs = []
    for r in tm.golden_inputs():
        hdr = t.tcphdr(0, r["lip"], r["lport"], r["rip"], r["rport"], r["seq"], r["ack"], r["rcv_wnd"], r["wscale"],
                       TCP_ACK, 5, b"")
        segs.append(dict(r, tcphdr=hdr.hex()))
    return {"source": "reference tcp_push_tcphdr (runtime/net/tcp_out.c:54-87) via oracle/_ref/libtcpout_ref.so, "
                      "called as tcp_tx_ack and tcp_tx_probe_window call it (tcp_out.c:178-228) with "
                      "netcfg.no_tx_offloads 0; kind 0 is an ACK, 1 a window probe; rcv_wnd is the window before "
                      "the shift by wscale",
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
