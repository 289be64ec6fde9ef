"""gcl_tcp_rx_open_host's option walk against what the REFERENCE's own
tcp_parse_options did (tests/golden/tcpopen_ref.json, recorded by
tests/golden/make_tcpopen_ref.py from runtime/net/tcp_in.c compiled in place):
snd_wscale and the WSCALE bit of every option shape but those with a length
byte of 0, which the reference does not return from and is never given.
snd_mss is not visible through that driver; it rests on the model and the hand
cases of tests/tcpopencases.py.  The committed fixture is always checked; where
oracle/_ref is built the generator's result must equal it.  No GPU."""
import importlib.util
import json
import os

import pytest

from caladan_amd import gclassify as g
from tests import tcpopencases as oc

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcpopen_ref.json")
with open(PATH) as f:
    REF = json.load(f)


def _generator():
    spec = importlib.util.spec_from_file_location("make_tcpopen_ref", os.path.join(os.path.dirname(PATH),
                                                                                    "make_tcpopen_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_fixture_is_what_the_reference_gives():
    from oracle import orc
    if orc.ref_tcpin() is None:
        pytest.skip("oracle/_ref/libtcpin_ref.so not built (no reference tree)")
    gen = _generator()
    fresh = gen.build()
    assert json.loads(gen.dumps(fresh)) == REF


def test_fixture_holds_every_shape_the_reference_returns_from():
    names = {r["name"] for r in REF["cases"]}
    assert names == {n for n, (_, want) in oc.OPTION_SHAPES.items() if want is not None}
    for r in REF["cases"]:
        assert bytes.fromhex(r["opts"]) == oc.OPTION_SHAPES[r["name"]][0]
        assert oc.parse_options(list(bytes.fromhex(r["opts"]))) is not None   # no length byte of 0 was ever fed
        assert r["state"] == g.TCP_STATE_ESTABLISHED
    assert sum(r["rcv_wnd"] != 0 for r in REF["cases"]) >= 6 and sum(r["rcv_wnd"] == 0 for r in REF["cases"]) >= 6


@pytest.mark.parametrize("rec", REF["cases"], ids=[r["name"] for r in REF["cases"]])
def test_twin_and_model_agree_with_the_reference(rec):
    ob = bytes.fromhex(rec["opts"])
    c = oc.case([(oc.syn(opts=ob), oc.L0)], [oc.listener()])
    out, _ = oc.run_host(g, c)
    assert int(out["verdict"][0]) == oc.ACCEPT
    r = out["open"][0]
    assert 1 << int(r["snd_wscale"]) == rec["snd_wnd"]
    assert bool(int(r["opt_en"]) & oc.OPT_WSCALE) == (rec["rcv_wnd"] != 0)
    en, _, ws = oc.parse_options(list(ob))
    assert 1 << ws == rec["snd_wnd"] and bool(en & oc.OPT_WSCALE) == (rec["rcv_wnd"] != 0)
