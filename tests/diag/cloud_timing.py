"""Wall time of uzl_cloud_add_images and uzl_cloud_estimate for 64 pairs of 640 x 480 image pairs (the room corner of
tests/cloud_scenes.py rendered at VGA from 64 different displacements, first guesses 0.03 m / 1 degree off): the 128 images in one
add, the 64 pairs in one estimate against 64 single-pair calls, beside the time the NumPy restatement (tests/cloud_reference.py)
takes for one pair on the same host.  Wall time = host clock around the call (it ends in a device synchronise), median of
UZL_CLOUD_TIMING_REPS calls after a warm-up.  Kernel times: run under rocprofv3 --kernel-trace --stats with
UZL_CLOUD_TIMING_REPS=1.  Prints one JSON line per measurement; no threshold, not a test."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_CLOUD_TIMING_REPS", "5"))


def main():
    import cloud_reference as LR
    import cloud_scenes as CS
    from uzliti_slam_amd import capi
    n_pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    cam = dict(w=640, h=480, fx=580.0, fy=580.0, cx=319.5, cy=239.5)
    rng = np.random.default_rng(0)
    images, colors, true = [], [], []
    for k in range(n_pairs):
        B = CS.pose(rng.uniform(-0.08, 0.08, 3), np.radians(rng.uniform(-2.5, 2.5, 3)))
        true.append(B)
        for T in (np.eye(3, 4), B):
            depth, bgr = CS.render(T, seed=k, **cam)
            images.append(dict(depth=depth, fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], camera_transform=np.eye(3, 4)))
            colors.append(bgr)
    wall = []
    for r in range(REPS + 1):                                                # the first is the warm-up: code objects, buffers
        h = capi.Cloud()
        t = time.perf_counter(); h.add_images(images, colors); wall.append(time.perf_counter() - t)
        if r < REPS:
            h.close()
    points = [h.point_count(i) for i in range(2 * n_pairs)]
    print(json.dumps(dict(what="add_images", images=2 * n_pairs, call_ms=1e3 * float(np.median(wall[1:])), points_mean=float(np.mean(points)),
                          points_max=int(max(points)), reps=REPS)), flush=True)
    pairs = [(2 * k, 2 * k + 1, CS.displaced(true[k], 0.03, 1.0)) for k in range(n_pairs)]
    out = h.estimate(pairs)
    wall = []
    for _ in range(REPS):
        t = time.perf_counter(); h.estimate(pairs); wall.append(time.perf_counter() - t)
    one_call = float(np.median(wall))
    wall = []
    for _ in range(REPS):
        t = time.perf_counter()
        for p in pairs:
            h.estimate([p])
        wall.append(time.perf_counter() - t)
    singles = float(np.median(wall))
    err = [CS.pose_errors(out[k]["transform"], true[k]) for k in range(n_pairs)]
    print(json.dumps(dict(what="estimate", pairs=n_pairs, one_call_ms=1e3 * one_call, ms_per_pair=1e3 * one_call / n_pairs,
                          single_calls_ms=1e3 * singles, single_ms_per_pair=1e3 * singles / n_pairs, iterations_mean=float(out["iterations"].mean()),
                          ok=int((out["status"] == 0).sum()), worst_m=max(e[0] for e in err), worst_rad=max(e[1] for e in err), reps=REPS)), flush=True)
    got = [h.read(i) for i in (0, 1)]
    h.close()
    if "--no-restatement" not in sys.argv:
        t = time.perf_counter()
        a = LR.make_cloud(*LR.voxel_grid(*LR.cloud_from_images(images[0]["depth"], colors[0], cam["fx"], cam["fy"], cam["cx"], cam["cy"])))
        b = LR.make_cloud(*LR.voxel_grid(*LR.cloud_from_images(images[1]["depth"], colors[1], cam["fx"], cam["fy"], cam["cx"], cam["cy"])))
        t_add = time.perf_counter() - t
        t = time.perf_counter()
        w = LR.estimate(a, b, pairs[0][2])
        t_est = time.perf_counter() - t
        same = all(np.array_equal(g["xyz"], c["xyz"]) and np.array_equal(g["lab"], c["lab"]) for g, c in zip(got, (a, b)))
        print(json.dumps(dict(what="restatement", add_s_per_pair=t_add, estimate_s_per_pair=t_est, clouds_equal=bool(same),
                              integers_equal=bool(w["num_corr_iter"] == out[0]["num_corr_iter"][:len(w["num_corr_iter"])].tolist()),
                              transform_diff=float(np.abs(w["transform"] - out[0]["transform"].reshape(3, 4)).max()))), flush=True)


if __name__ == "__main__":
    main()
