"""bench.py as its callers run it: a plain `--gpus 1 --steps K --warmup W` run
prints the headline line and nothing that takes runs of its own (--full), and
--dump-outputs writes what the last timed step computed, the same from run to
run and equal to the oracle's classification of the same packets.  A small
batch (--scaling strong --total-pkts) keeps the runs short."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.rxcases import to_verdict1

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS, WARMUP = 2 * 65536, 3, 1
FULL_ONLY = ("group", "group_node", "secondary", "e2e", "cpu_baseline", "e2e_multi")


def run_bench(out_dir):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {**os.environ, "GCL_BENCH_DETAIL": str(out_dir / "detail.json")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--scaling", "strong", "--total-pkts", str(N),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-800:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {k: np.load(out_dir / f"{k}.npy") for k in ("verdicts", "counts", "stats")}


@pytest.fixture(scope="module")
def first(tmp_path_factory):
    return run_bench(tmp_path_factory.mktemp("dump_a"))


def test_gpu_bench_plain_line(first):
    line, _ = first
    assert line["unit"] == "Mpkt/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value is the packets of the timed steps over their wall time, ms_per_step that time per step
    assert abs(line["value"] - N / (line["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * line["value"] + 0.1
    assert line["counts_check"] == "ok"
    assert not [k for k in FULL_ONLY if k in line]
    assert "frac" in line["roofline"] and "ceiling_ms" not in line["roofline"]


def test_gpu_bench_dump_matches_oracle(first, orc):
    import bench
    from caladan_amd import gclassify as g
    _, out = first
    _, _, stride, R, T, _ = bench.WORKLOADS["udp64"]
    assert out["verdicts"].dtype == np.float32 and out["verdicts"].shape == (N, bench.VERDICT_BYTES)
    assert out["counts"].dtype == np.float64 and out["counts"].shape == (R,)
    assert out["stats"].dtype == np.float64 and out["stats"].shape == (g.NR_STATS,)
    frames, _, _ = orc.generate(g.WL_UDP64, N, stride, R, seed=bench.SEED)
    t = orc.Tables(R, g.HASH_JENKINS, 0, g.F_RSS_HASH | g.F_IP_CKSUM_GOOD)
    bench.setup_tables(t, R, T)
    ve, ce, se = t.classify(frames, N, stride)
    want = to_verdict1(ve, {r: T for r in range(R)}, g.thread_bits_for(R, T))
    assert (out["verdicts"][:, 0] == want.astype(np.float32)).all()
    # the last step's own counts, not the sum over warmup, settle and timed steps
    assert (out["counts"] == ce.astype(np.float64)).all()
    assert (out["stats"] == se.astype(np.float64)).all()


def test_gpu_bench_dump_is_repeatable(first, tmp_path):
    _, a = first
    _, b = run_bench(tmp_path)
    for k in a:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), k
