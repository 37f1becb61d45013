"""Helper of tests/test_ransac_geometry_gpu.py: runs every case of tests/ransac_cases.py through uzl_ransac_points, in the LDS tile
and in HBM scratch, and prints one digest per (case, placement).  The vote switch (UZL_VOTE_VALU) is read once per process and
only by the diagnostic library (UZL_LIB), hence a subprocess."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_cases as RC  # noqa: E402
from uzliti_slam_amd import capi  # noqa: E402

m = capi.Match(seed=RC.SEED)
print(json.dumps(RC.device_digests(m)))
m.close()
