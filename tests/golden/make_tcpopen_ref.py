"""Generate tests/golden/tcpopen_ref.json from the REFERENCE's own
tcp_parse_options (runtime/net/tcp_in.c:298-348, compiled in place into
oracle/_ref/libtcpin_ref.so by oracle/Makefile behind the driver of
oracle/ref_tcpin.c).  The driver reaches it when a connection enters in
SYN_SENT: a SYN|ACK with win 1 and ack 1 on a connection with snd_una 0 and
snd_nxt 1 takes it to ESTABLISHED with snd_wnd = 1 << snd_wscale, and rcv_wnd
falls to 0 exactly when no WSCALE option counted (the driver's winmax is 0).
That pair is recorded for every option shape of tests/tcpopencases.py EXCEPT
those with a length byte of 0: the reference does not return from them, so
they are never fed to it.

Run where the reference tree is mounted (after `make -C oracle ref`):
    python tests/golden/make_tcpopen_ref.py
tests/test_tcpopen_ref.py calls build() where oracle/_ref is built and requires
the result equal to the committed file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import orc  # noqa: E402
from tests import tcpopencases as oc  # noqa: E402

OUT = os.path.join(HERE, "tcpopen_ref.json")


def shapes():
    """the option shapes the reference can be given: (name, option bytes padded to whole words with EOL)"""
    res = []
    for name in sorted(oc.OPTION_SHAPES):
        ob, want = oc.OPTION_SHAPES[name]
        if want is None:
            continue            # a length byte of 0: tcp_parse_options loops forever
        assert oc.parse_options(list(ob)) is not None and len(ob) % 4 == 0
        res.append((name, ob))
    return res


def record(ref, name, ob):
    f = oc.frame(oc.SYN | oc.TACK, seq=5000, ack=1, opts=ob)
    f = f[:48] + b"\x00\x01" + f[50:]          # win = 1
    conn = dict.fromkeys(ref.CONN, 0)
    conn.update(snd_una=0, snd_nxt=1, rcv_nxt=0, rcv_wnd=4096, rcv_mss=1460, state=0)
    trace, _ = ref.run(conn, [], f, [14], [len(f) - 14])
    t = trace[0]
    return {"name": name, "opts": ob.hex(), "state": t["state"], "snd_wnd": t["snd_wnd"], "rcv_wnd": t["rcv_wnd"]}


def build():
    ref = orc.ref_tcpin()
    if ref is None:
        raise SystemExit("oracle/_ref/libtcpin_ref.so not built (make -C oracle ref)")
    return {"source": "reference tcp_parse_options (runtime/net/tcp_in.c:298-348) reached through __tcp_rx_conn in "
                      "SYN_SENT via oracle/_ref/libtcpin_ref.so: a SYN|ACK with win 1 and ack 1, snd_una 0, snd_nxt "
                      "1, winmax 0; snd_wnd = 1 << snd_wscale, rcv_wnd 0 exactly when no WSCALE option counted",
            "cases": [record(ref, name, ob) for name, ob in shapes()]}


def dumps(d):
    out = ["{", f"\"source\": {json.dumps(d['source'])},", "\"cases\": ["]
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
    print(f"{len(d['cases'])} cases, {len(text)} bytes")


if __name__ == "__main__":
    main()
