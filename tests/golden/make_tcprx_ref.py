"""Generate tests/golden/tcprx_ref.json from the REFERENCE's own tcp_rx_conn,
__tcp_rx_conn, is_acceptable, tcp_rx_text and tcp_rx_append_text
(runtime/net/tcp_in.c, compiled in place into oracle/_ref/libtcpin_ref.so by
oracle/Makefile behind the driver of oracle/ref_tcpin.c): what the reference
did with every segment of every connection of every named case of
tests/tcprxcases.py, tests/tcprxfcases.py and tests/tcprxocases.py, and of the
small random streams tests/tcprxrefcases.py lists (one of each file's
generator; of the out-of-order one a stream with reordering and loss and one
with overlapping retransmits).  The driver applies no rule of the product: a
connection's segments all go through tcp_rx_conn, in list order; only the
entries that never reach it (not TCP, or no connection) are left out.

Run where the reference tree is mounted (after `make -C oracle ref`):
    python tests/golden/make_tcprx_ref.py

The file holds the cases by name and the reference's outputs only; the case
files regenerate the frames.  One record per case: per connection 'c' that has
segments or a queue, 'segs' with one row per segment: 't' the words WORDS of
tests/tcprxrefcases.py after the call (the PCB words, rxq_ooo_len, whether
ack_ts was rewritten, and the calls of tcp_timer_update ('slow'), tcp_conn_ack,
tcp_tx_ack, POLLIN, POLLOUT, tcp_tx_fast_retransmit_start and the frees), and
where not empty 'f' the mbufs freed, 'l' the mbufs newly linked at the tail of
c->rxq as (id, bytes pulled from the front, length), 'q' rxq_ooo after the
call where it changed, 'x' the arguments of tcp_conn_fail, tcp_conn_set_state
and tcp_tx_raw_rst / _rst_ack; 'qfinal' is rxq_ooo after the last segment as
(seq, end, id).  An id is k for the connection's segment k, -1 - i for entry i
of its input queue.  rcv_nxt, rcv_wnd and rxq_ooo_len before a call are those
after the call before it (the generator checks that) and are not stored twice.
tests/test_tcprx_ref.py calls build() where oracle/_ref is built and requires
the result equal to the committed file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from tests import tcprxrefcases as rr  # noqa: E402

OUT = os.path.join(HERE, "tcprx_ref.json")


def build():
    ref = orc.ref_tcpin()
    if ref is None:
        raise SystemExit("oracle/_ref/libtcpin_ref.so not built (make -C oracle ref)")
    return {"source": "reference tcp_rx_conn (runtime/net/tcp_in.c:172-296) with __tcp_rx_conn, is_acceptable, "
                      "tcp_rx_text and tcp_rx_append_text via oracle/_ref/libtcpin_ref.so; a connection is in "
                      "TCP_STATE_ESTABLISHED when its flags have GCL_TCPC_ELIGIBLE or GCL_TCPC_ESTABLISHED, else in "
                      "CLOSE_WAIT; tx_exclusive 0; rxq holds one mbuf when GCL_TCPC_RXQ is set; rxq_ooo is the "
                      "case's input queue",
            "words": list(rr.WORDS),
            "cases": [rr.record(ref, name) for name in rr.names()]}


def dumps(d):
    """one record per line"""
    out = ["{", f"\"source\": {json.dumps(d['source'])},", f"\"words\": {json.dumps(d['words'])},", "\"cases\": ["]
    out += [json.dumps(r, separators=(",", ":")) + ("," if j + 1 < len(d["cases"]) else "")
            for j, r in enumerate(d["cases"])]
    out += ["]", "}"]
    return "\n".join(out) + "\n"


def main():
    d = build()
    text = dumps(d)
    assert json.loads(text) == d
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{len(d['cases'])} cases, {sum(len(c['segs']) for r in d['cases'] for c in r['conns'])} segments, "
          f"{len(text)} bytes")


if __name__ == "__main__":
    main()
