"""GPU: gcl_tcp_txq -> gcl_copy_batch -> gcl_tx_hdr on one stream over a tx
region on the device, for every named case of tests/txqcases.py that
retransmits: each frame, in place and by copy, holds the reference's own
tcp_push_tcphdr bytes (tests/golden/txq_ref.json) in front of the payload bytes
that stay, and no other byte of the region changed."""
import numpy as np
import pytest
import torch

from tests import txqcases as tq
from tests.test_gpu_tcprx import dev
from tests.test_gpu_txq import rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from caladan_amd import gclassify
    return gclassify


@pytest.fixture(scope="module")
def clf(g):
    c = g.Classifier(0, 16, g.HASH_JENKINS)
    yield c
    c.close()


def test_chain_leaves_the_references_headers_in_front_of_the_payload(g, clf):
    segs = tq.load_golden()["segs"]
    net = g.txh_net(tq.NET["addr"], tq.NET["netmask"], tq.NET["gateway"], tq.NET["mac"])
    sent = 0
    for name in sorted(tq.cases()):
        case = tq.cases()[name]
        k = int(tq.model(case)["totals"][1])
        if k == 0:
            continue
        nconn, nent = len(case["conn"]), len(case["ent"])
        reg = dev(tq.region(tq.region_size(case)))
        want = dev(case["want"]) if case.get("want") is not None else None
        out = clf.tcp_txq(case["now"], dev(case["qoff"]), rec(case["ent"], 16), rec(case["cold"], 16), nent,
                          rec(case["conn"], 48), rec(case["addr"], 16), nconn, case["seg_cap"], want=want,
                          frame_stride=case["frame_stride"], frame_base=case["frame_base"])
        clf.copy_batch(reg, out["src_off"], out["len"], k, reg, dst_off=out["dst_off"], olflags=False, rss=False)
        hdr = clf.tx_hdr(out["desc"], out["frame_off"], k, reg, net)
        torch.cuda.synchronize()
        got = dict(totals=out["totals"].cpu().numpy().view(np.uint64),
                   frame_off=out["frame_off"].cpu().numpy().view(np.uint64),
                   len=out["len"].cpu().numpy().view(np.uint16))
        refused = (hdr["status"].cpu().numpy()[:k] == g.TXH_REFUSED).tolist()
        sent += tq.check_chain(name, case, got, reg.cpu().numpy(), [r for r in segs if r["case"] == name], refused)
    assert sent > 100
