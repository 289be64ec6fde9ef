"""Generate tests/golden/tcprxs_ref.json from the REFERENCE's own tcp_rx_conn,
__tcp_rx_conn, is_acceptable, tcp_rx_text and tcp_rx_append_text
(runtime/net/tcp_in.c, compiled in place into oracle/_ref/libtcpin_ref.so by
oracle/Makefile behind the driver of oracle/ref_tcpin.c): what the reference
did with every segment of every connection of every named case of
tests/tcprxscases.py and of the thinned random stream tests/tcprxsrefcases.py
lists, each connection started in the case's state word.  A connection in
SYN_SENT or in no state of enum tcp state is not fed: gcl_tcp_rx_states does
not walk it.

Run where the reference tree is mounted (after `make -C oracle ref`):
    python tests/golden/make_tcprxs_ref.py

The file holds the cases by name and the reference's trace only, in the layout
of tests/golden/tcprx_ref.json ('t' the words WORDS, 'f' the mbufs freed, 'l'
the mbufs linked into c->rxq as (id, bytes pulled, length), 'q' rxq_ooo where
it changed, 'x' fail_err, new_state, rst_kind, rst_seq and rst_ack); the case
file regenerates the frames.  tests/test_tcprxs_host.py calls build() where
oracle/_ref is built and requires the result equal to the committed file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from tests import tcprxsrefcases as sr  # noqa: E402

OUT = os.path.join(HERE, "tcprxs_ref.json")


def build():
    ref = orc.ref_tcpin()
    if ref is None:
        raise SystemExit("oracle/_ref/libtcpin_ref.so not built (make -C oracle ref)")
    return {"source": "reference tcp_rx_conn (runtime/net/tcp_in.c:172-296) with __tcp_rx_conn, is_acceptable, "
                      "tcp_rx_text and tcp_rx_append_text via oracle/_ref/libtcpin_ref.so; a connection starts in "
                      "the case's state word (without one: ESTABLISHED when its flags have GCL_TCPC_ELIGIBLE or "
                      "GCL_TCPC_ESTABLISHED); tx_exclusive 0; rxq holds one mbuf when GCL_TCPC_RXQ is set; rxq_ooo "
                      "is the case's input queue",
            "words": list(sr.WORDS), "extra": list(sr.EXTRA),
            "cases": [sr.record(ref, name) for name in sr.names()]}


def dumps(d):
    """one record per line"""
    out = ["{", f"\"source\": {json.dumps(d['source'])},", f"\"words\": {json.dumps(d['words'])},",
           f"\"extra\": {json.dumps(d['extra'])},", "\"cases\": ["]
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
