"""Wall time of one uzl_merge_partners and one uzl_merge_search on the online loop's graphs (synth.make_pose_graph at 1k / 5k, 10k / 50k
and 20k / 100k nodes / edges) and on a 1,500-node chain-like graph (1,530 edges), each with the starts the search walked from and the
nodes those walks marked, beside the time the NumPy / plain-Python restatement (tests/merge_reference.py) takes for the same table on
the same host.  Each graph runs twice: with the reference's gates (0.25 m, 15 degrees: consecutive poses of these graphs lie 0.3 m
apart, so only revisited places have a geometric candidate) and with gates widened to the spacing of the graphs
(UZL_MERGE_TIMING_DISTANCE, default 1.0 m, and 45 degrees), where every node has a candidate and is walked from - the most a search
can cost.  Every node is a start (the scope centre is far away).
Wall time = host clock around the call (it ends in a device synchronise), median of UZL_MERGE_TIMING_REPS calls after a warm-up that
also builds the CSR (printed as first_call_ms).  Prints one JSON line per graph; no threshold, not a test."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_MERGE_TIMING_REPS", "7"))
DIST = float(os.environ.get("UZL_MERGE_TIMING_DISTANCE", "1.0"))
GRAPHS = [("online 1k/5k", 1000, 5000, 12345), ("online 10k/50k", 10000, 50000, 12345), ("online 20k/100k", 20000, 100000, 12345),
            ("chain-like 1500/1530", 1500, 1530, 4040)]
FAR = np.array([1.0e6, 0.0, 0.0])


def median_ms(fn):
    wall = []
    for _ in range(REPS):
        t = time.perf_counter(); fn(); wall.append(time.perf_counter() - t)
    return 1e3 * float(np.median(wall))


def main():
    from merge_reference import MergeReference
    from uzliti_slam_amd import capi, synth
    for name, n, e, seed in GRAPHS:
        for cfg in (dict(max_distance=0.25, max_rotation_deg=15.0), dict(max_distance=DIST, max_rotation_deg=45.0)):
            g = synth.make_pose_graph(n, e, seed=seed)
            ed = g["edges"]
            E = capi.gate_edges(ed["from"], ed["to"], ed["type"], valid=ed["valid"])
            h = capi.Merge(**cfg); r = MergeReference(**cfg)
            h.set_graph(g["nodes_pose"], E); r.set_graph(g["nodes_pose"], E)
            t = time.perf_counter(); table = h.partners(FAR, 0.0); first = 1e3 * (time.perf_counter() - t)
            partners_ms = median_ms(lambda: h.partners(FAR, 0.0))
            st = h.stats()
            search_ms = median_ms(lambda: h.search(1, FAR, 0.0))
            tick = h.search(1, FAR, 0.0)
            t = time.perf_counter(); want = r.partners(FAR, 0.0); cpu = 1e3 * (time.perf_counter() - t)
            t = time.perf_counter(); want_tick = r.search(1, FAR, 0.0); cpu_tick = 1e3 * (time.perf_counter() - t)
            print(json.dumps(dict(graph=name, nodes=n, edges=e, max_distance=cfg["max_distance"], partners_ms=partners_ms, search_ms=search_ms, first_call_ms=first,
                                  restatement_partners_ms=cpu, restatement_search_ms=cpu_tick, with_partner=int((table >= 0).sum()),
                                  equal=bool(np.array_equal(table, want) and tick == want_tick), tick=list(tick), reps=REPS, **st)), flush=True)
            h.close()


if __name__ == "__main__":
    main()
