"""CPU: gcl_tcp_rx_states_host (csrc/gcl_host.c with the rule of
csrc/gcl_tcprxs.h) against what the REFERENCE's own tcp_rx_conn did in every
state (tests/golden/tcprxs_ref.json), against the hand-derived values of the
named cases and the plain Python transcription of tests/tcprxscases.py, and
byte for byte against gcl_tcp_rx_ooo_host where the two calls must agree."""
import errno
import importlib.util
import os

import numpy as np
import pytest

from tests import tcprxcases as rc
from tests import tcprxocases as oc
from tests import tcprxscases as sc
from tests import tcprxsrefcases as sr
from tests.tcprxcases import TCP_FIN, TCP_RST, TCP_SYN, TCP_URG


@pytest.fixture(scope="module")
def g():
    import caladan_amd.gclassify as g
    return g


def _generator():
    path = os.path.join(os.path.dirname(sr.PATH), "make_tcprxs_ref.py")
    spec = importlib.util.spec_from_file_location("make_tcprxs_ref", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_committed_traces_are_what_the_reference_gives():
    """Where oracle/_ref is built, the generator's result in memory equals
    the committed file, text and all."""
    from oracle import orc
    if orc.ref_tcpin() is None:
        pytest.skip("oracle/_ref/libtcpin_ref.so not built: the reference tree is not here")
    gen = _generator()
    with open(sr.PATH) as f:
        assert gen.dumps(gen.build()) == f.read()


def test_fixture_holds_every_named_case_and_stays_small():
    assert os.path.getsize(sr.PATH) <= 144 * 1024
    d = sr.load()
    assert [r["case"] for r in d["cases"]] == sr.names()
    seen = set()
    for r in d["cases"]:
        for cr in r["conns"]:
            for row in cr["segs"]:
                x = dict(zip(sr.EXTRA, row.get("x", [0] * 5)))
                if x["new_state"]:
                    seen.add(("state", x["new_state"] - 1))
                if x["rst_kind"]:
                    seen.add(("rst", x["rst_kind"]))
                if x["fail_err"]:
                    seen.add("fail")
    # every transition of :462-473, :530-542 and :581-590, both RSTs and tcp_conn_fail were recorded
    assert seen >= {("state", s) for s in (sc.ESTABLISHED, sc.FIN_WAIT2, sc.TIME_WAIT, sc.CLOSED, sc.CLOSE_WAIT,
                                            sc.CLOSING)} | {("rst", 1), ("rst", 2), "fail"}


@pytest.mark.parametrize("name", sorted(sc.cases()))
def test_named_case(g, name):
    """the hand-derived values, the transcription and the host twin agree, byte for byte and inside the guards"""
    case, exp = sc.cases()[name]
    want = sc.model(case)
    sc.check_expected(want, exp, "model " + name)
    got, cnt = sc.run_host(g, case)
    sc.compare(got, want, case, name)
    assert cnt.tolist() == want["counts"].tolist()


def test_host_twin_gives_what_the_reference_did(g):
    total = 0
    for name in sr.names():
        got, _ = sc.run_host(g, sr.case_of(name))
        total += sr.check(got, name, "host")
    assert total == sr.comparable() and total > 250


def test_transcription_gives_what_the_reference_did():
    for name in sr.names():
        sr.check(sc.model(sr.case_of(name)), name, "model")


@pytest.mark.parametrize("name", sorted(sc.STREAMS))
def test_random_lifetimes(g, name):
    case = sc.stream(name)
    want = sc.model(case)
    if name != "small_windows":
        sc.check_mix(want)
    got, cnt = sc.run_host(g, case)
    sc.compare(got, want, case, name)
    assert cnt.tolist() == want["counts"].tolist()


def _plain(case):
    """no FIN, RST, SYN or URG anywhere, and only connections gcl_tcp_rx_ooo calls ESTABLISHED or leaves alone"""
    n = len(case["pkt_len"])
    for i in range(n):
        o = int(case["offs"][i]) if case["offs"] is not None else i * case["stride"]
        if o + 48 <= case["frames_len"] and int(case["frames"][o + 47]) & (TCP_FIN | TCP_RST | TCP_SYN | TCP_URG):
            return False
    q = case.get("q")
    return q is None or not any(int(e["flags"]) & TCP_FIN for e in q)


def test_parity_with_tcp_rx_ooo(g):
    """on every case of tests/tcprxocases.py without FIN, RST, SYN or URG the shared outputs are byte-equal"""
    names = [n for n in sorted(oc.cases()) if _plain(oc.case_of(n))]
    assert len(names) >= 15
    for name in names + [0, 1, 2]:
        case = oc.stream(name) if isinstance(name, int) else oc.case_of(name)
        if isinstance(name, int) and not _plain(case):
            continue
        want, wcnt = oc.run_host(g, case)
        got, cnt = sc.run_host(g, case)
        oc.compare(got, want, case, f"parity {name}")
        assert cnt[:oc.NR].tolist() == wcnt.tolist() and cnt[oc.NR:].tolist() == [0, 0, 0, 0]
        assert not got["ev"][:len(got["ev"]) - sc.GUARD].any()


def test_einval(g):
    """what the C twin itself refuses: buffers that pass the binding's size checks"""
    case = sc.case_of("established_fin_without_text")
    z = oc.sizes(case)

    def call(**kw):
        out = sc.blank(case)
        out.update(kw.pop("out", {}))
        args = dict(stride=case["stride"], offs=case["offs"], frames_len=case["frames_len"], m=z["m"],
                    nconn=z["nconn"], q_out_cap=z["cap"], nq=0, out=out)
        conn = kw.pop("conn", case["conn"])
        args.update(kw)
        return g.tcp_rx_states_host(case["frames"], case["pkt_len"], case["sock"], conn, **args)

    def refused(**kw):
        with pytest.raises(OSError) as e:
            call(**kw)
        assert e.value.errno == errno.EINVAL, kw

    call()
    for f in ("ev", "rst_seq", "state_after", "state_out", "oflags", "skip", "verdict", "sflags", "rcv_nxt_after",
              "copy_len", "dst_off", "out_conn", "conn_off", "out_ext", "qout_off", "totals"):
        refused(out={f: None})
    odd = np.zeros(4 * z["m"] + 64, dtype=np.uint8)
    refused(out={"rst_seq": odd[1:]})
    refused(out={"skip": odd[1:]})
    refused(nconn=(1 << 20) + 1, conn=np.zeros((1 << 20) + 1, dtype=case["conn"].dtype),
            out={"out_conn": np.zeros(48 * ((1 << 20) + 1), dtype=np.uint8),
                 "out_ext": np.zeros(16 * ((1 << 20) + 1), dtype=np.uint8),
                 "conn_off": np.zeros((1 << 20) + 2, dtype=np.uint64),
                 "qout_off": np.zeros((1 << 20) + 2, dtype=np.uint32),
                 "state_out": np.zeros((1 << 20) + 1, dtype=np.uint8)})
    refused(align=3)
    refused(blocks=rc.MAX_BLOCKS + 1)
    refused(q_out_cap=4, out={"qout": None})
