"""Helper of tests/test_pgo_hierarchy_gpu.py: one case of that module in a process of its own, for the switches the diagnostic library
reads once per process (UZL_ML_NO_COMP4: the walked hierarchy).  Prints one JSON line: the class the hook reported and the worst ratio
per stage."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import test_pgo_hierarchy_gpu as T  # noqa: E402
from uzliti_slam_amd import capi  # noqa: E402

case = sys.argv[1]
if case == "walked":
    want = dict(cl=0, agg=4, mult=0, cg_variant=T.CG_PLAIN4)
    h = T.run_case(capi, 10000, 50000, 4, T.NO_SCHUR, want, "C4 walked", after=5)
    T.run_steady(capi, 10000, 50000, 4, {}, want, "C4 walked")
else:
    raise SystemExit("unknown case " + case)
print(json.dumps(dict(levels=h["levels"], cl=h["cl"], agg=h["agg"], mult=h["mult"], cg_variant=h["cg_variant"], measured=T.MEASURED)))
