"""bench.py's command line on the GPU: a plain run's result line and --dump-outputs.

One plain run of the default workload (the Roman-empire stand-in, Jaccard + ApproxER)
with --blas-threads 1, the OpenBLAS order the reference's golden vectors were made in:
the arrays it dumps are the timed path's own outputs, so they equal the reference's
scores of tests/golden/roman_full.npz bit for bit.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, bits_equal, load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bench") / "dump")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--blas-threads", "1", "--dump-outputs", out],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out


def test_plain_line_has_the_headline_only(plain_run):
    d, _ = plain_run
    assert d["metric"] == "scored edges/sec (Jaccard+ApproxER)"
    assert d["unit"] == "scored edges/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0
    # value = E * steps / elapsed and ms_per_step = elapsed / steps, both rounded
    assert d["value"] == pytest.approx(65_854 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    # the secondary measurements belong to --full
    for key in ("cpu_baseline", "box_blas_order", "kernels", "dropin_numpy_tie_break"):
        assert key not in d
    assert d.get("roofline") is None


def test_dumped_outputs_are_the_reference_scores(plain_run):
    _, out = plain_run
    assert sorted(os.listdir(out)) == ["approx_er.npy", "jaccard.npy"]
    g = load_golden("roman_full")
    for name in ("jaccard", "approx_er"):
        a = np.load(os.path.join(out, f"{name}.npy"))
        assert a.dtype == np.float64
        assert bits_equal(a, g[f"scores_{name}"]), name
