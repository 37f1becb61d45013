#!/usr/bin/env python3
"""Records tests/golden/lm_pass_counts.json on an MI355X (run from the repo root: python tests/golden/make_lm_pass_counts.py [out.json]).

The file holds what the device-resident LM loop did on the cases of tests/lm_pass_cases.py AT THE COMMIT IT WAS RECORDED AT: passes,
trials, PCG iterations and LM iterations of every optimize.  Record it at the parent of a change to the host's pass planner
(csrc/pgo_lm_pass.hpp), twice - a case whose counts differ between two runs of the same commit is no fixture and is left out by hand -
and tests/test_lm_pass_counts_gpu.py then says whether the change enqueues the passes the parent did.  Numbers only: a fixture."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(HERE))

import lm_pass_cases as LC               # noqa: E402
from uzliti_slam_amd import capi         # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lm_pass_counts.json")
    rec = {name: run(capi) for name, run in LC.CASES.items()}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded", len(rec), "cases to", out)
