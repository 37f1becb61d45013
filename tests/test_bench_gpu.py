"""A plain `bench.py` run on the device: the headline alone, its record and its dumped outputs, within 30 s of its timed steps."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_bench_run(tmp_path):
    steps, warmup = 10, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    c = json.loads(lines[0])
    assert c["unit"] == "edges/s" and c["higher_is_better"] is True and c["dtype"] == "f64" and c["value"] > 0 and c["ms_per_step"] > 0
    assert c["config"]["lm_iterations_done"] == 20 and c["config"]["system_edges"] > 0
    assert not c.get("roofline") and not c.get("cpu_baseline") and not c.get("secondary") and not c.get("c4_1gpu")
    assert wall - (steps + warmup) * c["ms_per_step"] * 1e-3 < 30.0, wall
    d = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in ("poses", "edge_error", "edge_used", "chi2")}
    assert d["poses"].shape == (1000, 12) and len(d["edge_used"]) == 5000 and len(d["edge_error"]) == int(d["edge_used"].sum())
    assert all(np.isfinite(v).all() for v in d.values()) and d["chi2"][1] < d["chi2"][0]
