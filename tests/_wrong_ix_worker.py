"""Helper of tests/test_pcg_args_gpu.py: solves config 2's graph three times per pass_history setting on the device-resident loop and prints
stats, pose digests and what the verbose log said about anomalies.  UZL_LM_WRONG_IX (diagnostic build) is read once per process, hence a
subprocess."""
import contextlib
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uzliti_slam_amd import capi, synth  # noqa: E402

n, e, its = (int(v) for v in sys.argv[1:4])
g = synth.make_pose_graph(n, e, seed=77)
out = {"runs": {}, "anomaly_lines": []}
with tempfile.TemporaryFile(mode="w+") as log:
    # the library writes its verbose log to the C stderr
    saved = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        for hist in (0, 1):
            p = capi.Pgo(lm_loop=0, pass_history=hist, verbose=1)
            p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
            runs = []
            for _ in range(3):
                p.reset()
                st = p.optimize(its)
                poses = np.ascontiguousarray(p.store()[0])
                runs.append(dict(stats={k: st[k] for k in ("status", "lm_passes", "iterations_done", "lm_trials", "pcg_iterations", "chi2_final", "lambda_final")},
                                 poses=hashlib.sha256(poses.tobytes()).hexdigest()))
            p.close()
            out["runs"][str(hist)] = runs
    finally:
        os.dup2(saved, 2)
        os.close(saved)
    log.seek(0)
    out["anomaly_lines"] = [ln.strip() for ln in log if "anomaly" in ln]
print(json.dumps(out))
