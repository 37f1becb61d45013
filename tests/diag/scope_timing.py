"""Wall time of one uzl_scope_reevaluate(-1) on the online loop's graphs (synth.make_pose_graph at 1k / 5k, 10k / 50k and 20k / 100k nodes /
edges) and on a 1,500-node chain-like graph (1,530 edges), each with the pass's barrier rounds and whether its distances lived in LDS,
and of uzl_scope_request at 20k nodes, beside the time the heapq restatement (tests/scope_reference.py) takes for the same call on the
same host.  Wall time = host clock around the call (it ends in a device synchronise), median of UZL_SCOPE_TIMING_REPS calls after a
warm-up that also builds the CSR (a pass after set_valid / add pays that rebuild once more: printed as first_call_ms).  Prints one JSON
line per graph; no threshold, not a test."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_SCOPE_TIMING_REPS", "7"))
GRAPHS = [("online 1k/5k", 1000, 5000, 12345), ("online 10k/50k", 10000, 50000, 12345), ("online 20k/100k", 20000, 100000, 12345),
          ("chain-like 1500/1530", 1500, 1530, 4040)]


def median_ms(fn):
    wall = []
    for _ in range(REPS):
        t = time.perf_counter(); fn(); wall.append(time.perf_counter() - t)
    return 1e3 * float(np.median(wall))


def main():
    from scope_reference import ScopeReference
    from uzliti_slam_amd import capi, synth
    for name, n, e, seed in GRAPHS:
        g = synth.make_pose_graph(n, e, seed=seed)
        ed = g["edges"]
        E = capi.gate_edges(ed["from"], ed["to"], ed["type"], valid=ed["valid"])
        h = capi.Scope(); r = ScopeReference()
        h.set_graph(g["nodes_pose"], None, E); r.set_graph(g["nodes_pose"], None, E)
        t = time.perf_counter(); h.reevaluate(); first = 1e3 * (time.perf_counter() - t)
        ms = median_ms(h.reevaluate)
        t = time.perf_counter(); r.reevaluate(); cpu = 1e3 * (time.perf_counter() - t)
        same = bool(np.array_equal(h.uncertainty().view(np.uint64), r.uncertainty().view(np.uint64)))
        print(json.dumps(dict(graph=name, nodes=n, edges=e, reevaluate_ms=ms, first_call_ms=first, restatement_ms=cpu, bit_equal=same,
                              reps=REPS, **h.stats())), flush=True)
        if n == 20000:
            cur = n - 1
            rq = median_ms(lambda: h.request(cur))
            t = time.perf_counter(); want = r.request(cur); cpu = 1e3 * (time.perf_counter() - t)
            radius, ids = h.request(cur)
            print(json.dumps(dict(graph=name, call="request", nodes=n, request_ms=rq, restatement_ms=cpu, radius=radius, out_of_scope=len(ids),
                                  equal=bool(radius == want[0] and np.array_equal(ids, want[1])), reps=REPS)), flush=True)
        h.close()


if __name__ == "__main__":
    main()
