"""bench.py's plain run: exactly K timed steps, ONE JSON line with the headline fields and none of the --full legs, and
--dump-outputs writing the iterates after the last timed step -- the same arrays from run to run, since the inputs are."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import ROOT

pytestmark = pytest.mark.gpu


def _bench(*flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "10", *flags],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_k_steps_and_dumps_the_iterates(tmp_path):
    runs = [_bench("--dump-outputs", str(tmp_path / str(k))) for k in range(2)]
    for d in runs:
        assert d["steps"] == 40 and d["warmup"] == 10 and d["n_gpus"] == 1
        assert d["metric"].startswith("ms/RBCD-iteration") and d["unit"] == "ms" and d["dtype"] == "f64"
        assert d["higher_is_better"] is False and d["value"] == d["ms_per_step"] and 0 < d["ms_per_step"] < 1.0
        assert not {"roofline", "convergence", "cpu_baseline", "timing", "counters"} & set(d)
    a, b = ({k: np.load(str(tmp_path / str(r) / (k + ".npy"))) for k in ("X", "Y", "V", "cost")} for r in range(2))
    n = 2500  # sphere2500, r = 5: 5 x 4 doubles per pose
    for k in ("X", "Y", "V"):
        assert a[k].dtype == np.float64 and a[k].shape == (5 * 4 * n,) and np.isfinite(a[k]).all()
        assert np.abs(a[k] - b[k]).max() <= 1e-9 * max(1.0, np.abs(b[k]).max()), k
    assert a["cost"].shape == (1,) and 0 < a["cost"][0] and abs(a["cost"][0] - b["cost"][0]) <= 1e-9 * b["cost"][0]
