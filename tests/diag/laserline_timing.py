"""Wall time of uzl_laserline_extract from host memory for 1, 64 and 2,000 depth images of 640 x 480 f32 (the room scene, four distinct
images repeated), beside the bare copy of the same bytes from pinned host memory (hipMemcpy through torch), and the bytes per second
both amount to.  Wall time = host clock around the call (it ends in a device synchronise), median of UZL_LASERLINE_TIMING_REPS
calls after a warm-up.  Kernel time: run under rocprofv3 --kernel-trace --stats with UZL_LASERLINE_TIMING_REPS=1 and read
laser_bin_kernel / laser_finish_kernel there (the bin kernel reads the chunk the copy has put into HBM, so its dispatch time is its
time with the images resident); with --kernel-stats FILE this script reads rocprofv3's kernel-stats CSV and prints pixel bytes over
the bin kernel's total time against the achievable streaming rate.  Prints one JSON line per size; no threshold, not a test."""
import csv
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_LASERLINE_TIMING_REPS", "5"))
STREAM_TBS = 6.3                      # achievable HBM streaming rate of the MI355X, TB/s
IMAGE_BYTES = 640 * 480 * 4


def kernel_stats(path, images):
    """rocprofv3 kernel-stats CSV of a run with `images` images extracted (warm-up + 1 rep = 2 extracts)"""
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        if "laser_" not in name:
            continue
        calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
        out = dict(kernel=re.search(r"laser_\w+", name).group(0), calls=calls, total_ms=total_ns * 1e-6, mean_us=total_ns / calls * 1e-3)
        if "bin" in name and images:
            tbs = 2 * images * IMAGE_BYTES / (total_ns * 1e-9) / 1e12
            out.update(pixel_tb_per_s=tbs, share_of_streaming_rate=tbs / STREAM_TBS)
        print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--kernel-stats":
        return kernel_stats(args[1], int(args[2]) if len(args) > 2 else 0)
    bare = "--no-copy" not in args
    if bare:                                                                  # torch owns the device before the library touches it
        import torch
        torch.cuda.synchronize()
    import laserline_scenes as LS
    from uzliti_slam_amd import capi
    sizes = [int(x) for x in args if not x.startswith("--")] or [1, 64, 2000]
    base = [LS.image(LS.room(seed=30 + k), LS.camera_transform(yaw=40.0 + 90.0 * k, pitch=5.0 * k)) for k in range(4)]
    for n in sizes:
        images = capi.Laserline.pack_images([dict(base[k % 4], group=k) for k in range(n)])
        h = capi.Laserline()
        r, _, _ = h.extract(images)                                           # warm-up: code objects, staging and HBM buffers
        wall = []
        for _ in range(REPS):
            t = time.perf_counter(); h.extract(images); wall.append(time.perf_counter() - t)
        h.close()
        out = dict(images=n, bytes=n * IMAGE_BYTES, beams_hit=int((r < 6).sum()), extract_ms=1e3 * float(np.median(wall)),
                   extract_gb_per_s=n * IMAGE_BYTES / float(np.median(wall)) / 1e9, reps=REPS)
        if bare:
            src = torch.empty(min(n * IMAGE_BYTES, 1 << 30), dtype=torch.uint8).pin_memory()   # at most 1 GiB pinned; larger sizes copy it again
            dst = torch.empty_like(src, device="cuda")
            times = []
            for _ in range(REPS + 1):
                torch.cuda.synchronize()
                t = time.perf_counter()
                left = n * IMAGE_BYTES
                while left > 0:
                    k = min(left, src.numel())
                    dst[:k].copy_(src[:k], non_blocking=True)
                    left -= k
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t)
            copy = float(np.median(times[1:]))
            out.update(pinned_copy_ms=1e3 * copy, pinned_copy_gb_per_s=n * IMAGE_BYTES / copy / 1e9)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
