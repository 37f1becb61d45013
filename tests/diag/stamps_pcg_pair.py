#!/usr/bin/env python3
"""Diagnostic: the small-graph PCG pair's time from kernel entry to "every operand load sent" (s_memrealtime stamps of workgroup 0,
-DUZL_STAMPS build of pgo_ml_kernels.hip: STAMP(16) in ml_spmv, STAMP(32) in ml_cg_comp), and ml_spmv's later phases.
tests/diag/stamps_pgo.sh builds build/stb/libuzl_stamps.so (and prints the large-graph kernels' stamps); then, on the GPU box:

    UZL_LIB=$PWD/build/stb/libuzl_stamps.so python tests/diag/stamps_pcg_pair.py [nodes=1000] [edges=5000]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from uzliti_slam_amd import capi, synth    # noqa: E402

L = capi.lib()
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
e = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
g = synth.make_pose_graph(n, e)
p = capi.Pgo()
p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
p.optimize(20)
out = (C.c_ulonglong * 64)()
L.uzl_debug_read_stamps(out, 1)
for _ in range(3):
    p.reset()
    st = p.optimize(20)
L.uzl_debug_read_stamps(out, 0)
ns, nc = max(out[47], 1), max(out[46], 1)
print("n %d e %d pcg %d; ml_spmv launches stamped %d, ml_cg_comp %d (100 MHz ticks -> us)" % (n, e, st["pcg_iterations"], ns, nc))
for i, nm in enumerate(["prefetch issue", "r.z reduction", "row products + folds", "restriction + stores"]):
    print("  ml_spmv    %-32s %7.3f us" % (nm, out[16 + i] / ns / 100.0))
print("  ml_cg_comp %-32s %7.3f us" % ("prefetch issue", out[32] / nc / 100.0))
