"""Wall time of uzl_orb_extract with GIST from host memory for 64 mono8 images of 640 x 480 (four distinct rectangle scenes repeated),
beside the NumPy restatement's time per image on the same host.  Wall time = host clock around the call (it ends in a device
synchronise), median of UZL_ORB_TIMING_REPS calls after a warm-up.  Kernel times: run under rocprofv3 --kernel-trace --stats with
UZL_ORB_TIMING_REPS=1; with --kernel-stats FILE [images] [extracts] this script reads rocprofv3's kernel-stats CSV and prints, per
kernel, the time per extract and the bytes it has to move (BYTES below: what the kernel must read plus write per image when every
operand is touched once) as a rate against the 6.3 TB/s a copy reaches on this part.  Prints JSON lines; no threshold, not a test."""
import csv
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_ORB_TIMING_REPS", "5"))
W, H = 640, 480
HBM_TB_S = 6.3
L1 = 533 * 400                                  # level 1 of the whole image
C0, C1 = 4 * 320 * 240, 4 * 267 * 200           # the four cells' levels
KP = 320                                        # keypoints per image, about
BYTES = {                                       # per image, defaults (2 x 2 cells, 2 levels)
    "orb_resize_kernel": (W * H + L1) + (C0 + C1),          # cells and whole image: level 0 read, level 1 written
    "orb_gist_resize_kernel": 63 * 63 * 5,                  # four taps read, one pixel written
    "orb_fast_kernel": 4 * (258 * 178 + 205 * 138),         # the region the border leaves, read once
    "orb_cut_kernel": 8 * 256 * 4,
    "orb_orient_kernel": 2800 * 9 + 2 * KP * 709,           # candidates, and the kept ones' patches (L2)
    "orb_order_kernel": 2 * KP * 20,
    "orb_blur_kernel": 2 * (W * H + L1 + 63 * 63),
    "orb_describe_kernel": KP * (20 + 512 + 32),
}


def kernel_stats(path, images, extracts):
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        m = re.search(r"orb_\w+_kernel", name)
        if not m:
            continue
        calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
        out = dict(kernel=m.group(0), calls=calls, total_ms=total_ns * 1e-6, us_per_extract=total_ns / extracts * 1e-3)
        if images:
            b = BYTES[m.group(0)] * images
            out.update(bytes_per_extract=b, tb_per_s=b * extracts / (total_ns * 1e-9) / 1e12,
                       share_of_hbm=b * extracts / (total_ns * 1e-9) / 1e12 / HBM_TB_S)
        print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--kernel-stats":
        return kernel_stats(args[1], int(args[2]) if len(args) > 2 else 0, int(args[3]) if len(args) > 3 else 2)
    import orb_reference as R
    import orb_scenes as S
    from uzliti_slam_amd import capi
    n = int(args[0]) if args else 64
    pattern = S.pattern()
    base = [S.rectangles(W, H, seed=1000 + W + k) for k in range(4)]
    t = time.perf_counter()
    want = R.extract(base[0], pattern)
    want_gist = R.gist(base[0], 12.5, pattern)
    numpy_s = time.perf_counter() - t
    images = [base[k % 4] for k in range(n)]
    angles = [12.5] * n
    h = capi.Orb(pattern)
    h.extract(images, gist_angles=angles)                                     # warm-up: code objects, staging and HBM buffers
    got = h.read(0)
    assert np.array_equal(got["desc"], want["desc"]) and np.array_equal(got["u"], want["u"]) and np.array_equal(h.gist(0), want_gist)
    arr, keep = capi.DepthFilter.pack_guides(images)
    ang = np.asarray(angles, np.float32)
    import ctypes as C
    times = []
    for _ in range(REPS):
        t = time.perf_counter()
        rc = capi.lib().uzl_orb_extract(h._h, C.c_int32(n), arr, None, ang.ctypes.data_as(C.POINTER(C.c_float)))
        times.append(time.perf_counter() - t)
        assert rc == 0
    kps = sum(h.count(k) for k in range(n))
    h.close()
    print(json.dumps(dict(images=n, keypoints=kps, extract_ms=1e3 * float(np.median(times)), ms_per_image=1e3 * float(np.median(times)) / n,
                          numpy_ms_per_image=1e3 * numpy_s, reps=REPS)), flush=True)


if __name__ == "__main__":
    main()
