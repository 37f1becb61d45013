"""The small-graph PCG launches of a one-graph pass carry the hierarchy copy they apply BY VALUE (csrc/pgo_types.hpp: PcgArgs; the host
predicts it with lm_pass_ix, csrc/pgo_lm.hpp) and hold it against the LM state on the device.  A wrong prediction must cost time and
nothing else: the kernels do no work, the pass ends as anomaly 4, the host-driven loop solves the graph from its start poses - to the
bits of an undisturbed solve.  UZL_LM_WRONG_IX=1 (diagnostic build only) makes every prediction wrong."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DIAG = os.path.join(os.path.dirname(HERE), "uzliti_slam_amd", "libuzl_mi355x_diag.so")


def _run(n, e, its, **env):
    assert os.path.exists(DIAG), "the diagnostic library is built by `make` beside the product"
    e_ = dict(os.environ, UZL_LIB=DIAG, **env)
    out = subprocess.run([sys.executable, os.path.join(HERE, "_wrong_ix_worker.py"), str(n), str(e), str(its)], env=e_, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("n,e,its", [(1000, 5000, 12), (300, 1200, 7)])
def test_wrong_copy_ends_in_the_fallback_with_the_same_poses(n, e, its):
    good = _run(n, e, its)
    bad = _run(n, e, its, UZL_LM_WRONG_IX="1")
    assert not good["anomaly_lines"], good["anomaly_lines"]
    for hist in ("0", "1"):
        for k in range(3):
            a, b = good["runs"][hist][k], bad["runs"][hist][k]
            assert a["stats"]["status"] == 0 and b["stats"]["status"] == 0
            assert a["stats"]["lm_passes"] > 0, a                  # the device-resident loop solved it ...
            assert b["stats"]["lm_passes"] == 0, b                 # ... and here the host-driven loop did, after the anomaly
            for f in ("iterations_done", "lm_trials", "pcg_iterations", "chi2_final", "lambda_final"):
                assert a["stats"][f] == b["stats"][f], (hist, k, f, a, b)
            assert a["poses"] == b["poses"], (hist, k)
    # every disturbed solve went through the anomaly route, with the code of this check
    assert len(bad["anomaly_lines"]) == 6 and all("anomaly 4" in ln for ln in bad["anomaly_lines"]), bad["anomaly_lines"]
    # pass_history 0 and 1: equal results, disturbed or not
    for runs in (good["runs"], bad["runs"]):
        for k in range(3):
            assert runs["0"][k]["poses"] == runs["1"][k]["poses"]
            for f in ("iterations_done", "lm_trials", "pcg_iterations", "chi2_final", "lambda_final"):
                assert runs["0"][k]["stats"][f] == runs["1"][k]["stats"][f], (k, f)
