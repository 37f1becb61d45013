"""What shrinking the resident graph in place saves: wall time of (a) uzl_pgo_rewrite_graph against (b) the path without it,
uzl_pgo_add_graph of the host-rewritten arrays on the same handle (capi.Pgo.add_graph, its host packing included; the host rewrite
itself - apply_merge_plan and the like - is NOT counted), on synth.make_pose_graph at 1k / 5k, 10k / 50k and 20k / 100k nodes / edges.
Two workloads per graph: one merge (the first pair uzl_merge_search finds with gates widened to the graph's spacing, rewritten by
merge.pgo_rewrite_of_plan) and a scope drop of 5 % of the nodes (a contiguous stretch in the middle).
Wall time = host clock around the call, which ends in the stream synchronise of the graph-entry path.  Before every timed call the
handle is given the full graph again (untimed); (a) and (b) alternate in one process, UZL_REWRITE_TIMING_REPS of each (default 20)
after two warm-up rounds; median, min, max.  Also: structure_ms of the optimize that follows either (the structure is rebuilt both
ways, so the two should agree; 3 calls each), and the event time of the two kernels of (a) beside the bytes they move,
2 * 608 * E_new + 2 * 64 * N_new.  One JSON line per graph and workload, to stdout and to UZL_REWRITE_TIMING_LOG (default
profiles/rewrite_timing.log); no threshold, not a test."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

REPS = int(os.environ.get("UZL_REWRITE_TIMING_REPS", "20"))
LOG = os.environ.get("UZL_REWRITE_TIMING_LOG", os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "rewrite_timing.log"))
GRAPHS = [("1k/5k", 1000, 5000), ("10k/50k", 10000, 50000), ("20k/100k", 20000, 100000)]
FAR = np.array([1.0e6, 0.0, 0.0])


def spread(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def main():
    import rewrite_reference as R
    from uzliti_slam_amd import capi, synth
    from uzliti_slam_amd.merge import pgo_rewrite_of_drops, pgo_rewrite_of_plan
    lines = []
    for name, n, e in GRAPHS:
        g = synth.make_pose_graph(n, e, seed=12345)
        P, F, ed = g["nodes_pose"], g["nodes_fixed"], g["edges"]
        with capi.Merge(max_distance=1.0, max_rotation_deg=45.0) as m:
            m.set_graph(P, capi.gate_edges(ed["from"], ed["to"], ed["type"], valid=ed["valid"]))
            keep, drop, _ = m.search(1, FAR, 0.0)
            assert keep >= 0, "no pair to merge"
            plan = m.plan(keep, drop, 1, 1)
        for workload, rw in (("merge", pgo_rewrite_of_plan(plan)), ("scope drop 5 %", pgo_rewrite_of_drops(np.arange(n // 2, n // 2 + n // 20)))):
            want = R.rewrite_arrays(P, F, ed, rw["drop_nodes"], rw.get("pose_nodes", ()), rw.get("poses"), rw.get("xf"), rw.get("ops", ()))
            n_new, e_new = len(want[0]), len(want[2]["from"])
            p = capi.Pgo()
            wall = dict(a=[], b=[]); structure = dict(a=[], b=[])
            for rep in range(-2, REPS):
                for which in ("a", "b"):
                    p.add_graph(P, F, ed)                                     # the resident graph, as before the shrink (untimed)
                    t = time.perf_counter()
                    if which == "a":
                        p.rewrite_graph(**rw)
                    else:
                        p.add_graph(want[0], want[1], want[2])
                    dt = 1e3 * (time.perf_counter() - t)
                    if rep >= 0:
                        wall[which].append(dt)
                    if 0 <= rep < 3:
                        structure[which].append(p.optimize(1)["structure_ms"])
            assert (p.n, p.e_in) == (n_new, e_new)
            # the kernels of (a) by their dispatch timestamps
            p.set_profiling(True)
            for _ in range(5):
                p.add_graph(P, F, ed)
                p.rewrite_graph(**rw)
            kt = p.kernel_times()
            p.close()
            moved = 2 * 608 * e_new + 2 * 64 * n_new
            kernel_us = {k: 1e3 * kt[k]["ms"] / kt[k]["launches"] for k in ("rewrite_edges", "rewrite_nodes") if k in kt}
            both_us = sum(kernel_us.values())
            lines.append(json.dumps(dict(graph=name, workload=workload, nodes=n, edges=e, nodes_after=n_new, edges_after=e_new, reps=REPS,
                                         rewrite_graph_ms=spread(wall["a"]), add_graph_rewritten_ms=spread(wall["b"]),
                                         ratio_of_medians=float(np.median(wall["a"]) / np.median(wall["b"])),
                                         structure_ms_after_rewrite=spread(structure["a"]), structure_ms_after_add_graph=spread(structure["b"]),
                                         kernel_us=kernel_us, bytes_moved=moved, kernels_GBps=(moved / (both_us * 1e-6) / 1e9) if both_us > 0 else None)))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
