"""Wall time of uzl_laser_estimate for 1, 64 and 1,024 pairs of 720-beam scans (the room, corridor and invalid-beam scenes of
tests/laser_scenes.py with their three first guesses, repeated) at the default config, in microseconds per pair, beside the time
the NumPy restatement (tests/laser_reference.py) takes per pair on the same host, and the ratio of one call of 1,024 pairs to
1,024 calls' worth of the single-pair time.  Wall time = host clock around the call (it ends in a device synchronise), median of
UZL_LASER_TIMING_REPS calls after a warm-up.  Kernel time: run under rocprofv3 --kernel-trace --stats with
UZL_LASER_TIMING_REPS=1 and read laser_icp_kernel there.  Prints one JSON line per size and one summary line; no threshold, not a
test."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_LASER_TIMING_REPS", "5"))


def main():
    import laser_reference as LR
    import laser_scenes as LS
    from uzliti_slam_amd import capi
    sizes = [int(x) for x in sys.argv[1:] if not x.startswith("--")] or [1, 64, 1024]
    scenes = LS.scenes()
    names = ["room", "corridor", "room_invalid"]
    h = capi.Laser()
    for n in names:
        h.add_scans([scenes[n]["scan_from"], scenes[n]["scan_to"]])
    base = [(2 * k, 2 * k + 1, LS.displaced(scenes[n]["true"], *g)) for k, n in enumerate(names) for g in LS.GUESSES]
    t = time.perf_counter()
    ref = [LR.estimate(scenes[n]["scan_from"], scenes[n]["scan_to"], LS.displaced(scenes[n]["true"], *g)) for n in names for g in LS.GUESSES]
    cpu_us = 1e6 * (time.perf_counter() - t) / len(ref)
    per_pair = {}
    for n in sizes:
        pairs = capi.Laser.pack_pairs([base[k % len(base)] for k in range(n)])
        out = h.estimate(pairs)                                              # warm-up: code object, buffers
        wall = []
        for _ in range(REPS):
            t = time.perf_counter(); h.estimate(pairs); wall.append(time.perf_counter() - t)
        per_pair[n] = 1e6 * float(np.median(wall)) / n
        print(json.dumps(dict(pairs=n, beams=720, call_ms=1e3 * float(np.median(wall)), us_per_pair=per_pair[n],
                              iterations_mean=float(out["iterations"].mean()), ok=int((out["status"] == 0).sum()), reps=REPS)), flush=True)
    h.close()
    summary = dict(restatement_cpu_us_per_pair=cpu_us)
    if 1 in per_pair and 1024 in per_pair:
        summary.update(one_call_of_1024_over_1024_single_calls=per_pair[1024] / per_pair[1])
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
