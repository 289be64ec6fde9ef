"""Generate tests/golden/txq_ref.json from the REFERENCE's own
tcp_push_tcphdr (runtime/net/tcp_out.c:54-87, compiled in place into
oracle/_ref/libtcpout_ref.so by oracle/Makefile, oracle/ref_tcpout.c): the 20
TCP header bytes of every tcp_off 5 segment the named cases of
tests/txqcases.py retransmit, as tcp_tx_retransmit_one (tcp_out.c:434-437)
calls it: the entry's flags, off 5, m->seg_seq after the partial-ACK pull of
:430-432, the payload that the pull left, pcb.rcv_nxt_wnd = rcv_wnd << 32 |
rcv_nxt as the connection has it now, pcb.rcv_wscale.  l4len is the length of
the trimmed payload: the first departure of include/gclassify.h.

Run where the reference tree is mounted (after `make -C oracle ref`):
    python tests/golden/make_txq_ref.py

The file holds inputs and the reference's outputs only.
tests/test_txq_chain.py calls build() where oracle/_ref is built and requires
the result equal to the committed file; it and tests/test_gpu_txq_chain.py hold
the frames that gcl_tcp_txq -> gcl_copy_batch -> gcl_tx_hdr leave to it.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from tests import txqcases as tq  # noqa: E402

OUT = os.path.join(HERE, "txq_ref.json")


def build():
    t = orc.ref_tcpout()
    if t is None:
        raise SystemExit("oracle/_ref/libtcpout_ref.so not built (make -C oracle ref)")
    segs = []
    for name in sorted(tq.cases()):
        case = tq.cases()[name]
        reg = tq.region(tq.region_size(case))
        for r in tq.sent_segments(case):
            if not tq.in_golden(r):
                continue
            at = r["old"] + tq.HDR + r["trim"]
            hdr = t.tcphdr(0, r["lip"], r["lport"], r["rip"], r["rport"], r["seq"], r["ack"], r["rcv_wnd"],
                           r["wscale"], r["flags"], 5, reg[at:at + r["paylen"]].tobytes())
            segs.append(dict(case=name, **{f: r[f] for f in tq.GOLDEN_KEYS}, tcphdr=hdr.hex()))
    return {"source": "reference tcp_push_tcphdr (runtime/net/tcp_out.c:54-87) via oracle/_ref/libtcpout_ref.so, "
                      "called as tcp_tx_retransmit_one calls it (tcp_out.c:434-437) with netcfg.no_tx_offloads 0; "
                      "seq is m->seg_seq after the pull of trim bytes, paylen the payload left, rcv_wnd the window "
                      "before the shift by wscale",
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
