"""Kernel and wall time of occupancy-grid builds (uzl_grid_*) at the deployed point (720 beams of pi/360, range_max 6 m, 5 cm
cells, UZL_GRID_TIMING_DENSE=1: every beam returns): a full build and a 256-node extend at 2k and 20k nodes of make_pose_graph's trajectory, ray-cast room scans.  Wall time =
host clock around the call (it ends in a device synchronise); kernel time: run under rocprofv3 --kernel-trace --stats with
UZL_GRID_TIMING_REPS=1 and read grid_tile_kernel / grid_stats_kernel there.  Prints one JSON line per size."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import grid_scenes as GS  # noqa: E402
from uzliti_slam_amd import capi  # noqa: E402

REPS = int(os.environ.get("UZL_GRID_TIMING_REPS", "10"))


def main():
    sizes = [int(x) for x in (sys.argv[1:] or ["2000", "20000"])]
    for n in sizes:
        poses, scans = GS.scene(n, seed=5)
        if os.environ.get("UZL_GRID_TIMING_DENSE"):                        # every beam returns: ranges uniform in [0.5, 6)
            rng = np.random.default_rng(n)
            for s in scans:
                s["ranges"] = rng.uniform(0.5, 5.99, len(s["ranges"])).astype(np.float32)
        g = capi.Grid(range_max=GS.DEPLOYED["range_max"], resolution=GS.DEPLOYED["resolution"])
        t = time.perf_counter(); g.add_scans(scans); t_add = time.perf_counter() - t
        k = n - 256
        g.build(poses)                                                         # warm-up
        full, ext, read = [], [], []
        for _ in range(REPS):
            t = time.perf_counter(); info = g.build(poses); full.append(time.perf_counter() - t)
            g.build(poses[:k])
            t = time.perf_counter(); g.extend(poses, k); ext.append(time.perf_counter() - t)
            t = time.perf_counter(); g.read(); read.append(time.perf_counter() - t)
        info = g.build(poses)
        print(json.dumps(dict(nodes=n, beams=int(sum(len(s["ranges"]) for s in scans)), width=info["width"], height=info["height"],
                              valid_beams=info["valid_beams"], add_scans_ms=1e3 * t_add, build_ms=1e3 * float(np.median(full)),
                              extend256_ms=1e3 * float(np.median(ext)), read_ms=1e3 * float(np.median(read)), reps=REPS)), flush=True)
        g.close()


if __name__ == "__main__":
    main()
