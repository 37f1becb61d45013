"""Wall time of uzl_depthfilter_refine from host memory, and of refine -> uzl_depthfilter_to_laserline, for 64 images of 640 x 480 f32
with their mono8 guides (the room scene under the block guide, four distinct images repeated), beside two yardsticks taken in the
same run: a device-to-device copy that moves the bytes the refine kernel reads plus writes (4 + 1 read and 4 written per pixel, so
a copy of 4.5 bytes per pixel: the memory bound, timed with device events), and the NumPy restatement per image.  Wall time = host
clock around the call (it ends in a device synchronise), median of UZL_DEPTHFILTER_TIMING_REPS calls after a warm-up.  Kernel time:
run under rocprofv3 --kernel-trace --stats with UZL_DEPTHFILTER_TIMING_REPS=1 and read depth_refine_kernel there (it reads the
chunk the copy has put into HBM, so its dispatch time is its time with the images resident); with --kernel-stats FILE this script
reads rocprofv3's kernel-stats CSV and prints the kernel's bytes per second.  Prints JSON lines; no threshold, not a test."""
import csv
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

REPS = int(os.environ.get("UZL_DEPTHFILTER_TIMING_REPS", "5"))
PIXELS = 640 * 480
KERNEL_BYTES = PIXELS * 9             # per image: depth f32 and guide u8 read, refined f32 written


def kernel_stats(path, images, refines=3):
    """rocprofv3 kernel-stats CSV of a run with `images` images and UZL_DEPTHFILTER_TIMING_REPS=1: three refines (the warm-up, one
    alone, one before to_laserline), each of one launch per staging chunk"""
    for row in csv.DictReader(open(path)):
        name = row.get("Name", "")
        if "depth_" not in name and "laser_" not in name:
            continue
        calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
        out = dict(kernel=re.search(r"(depth|laser)_\w+", name).group(0), calls=calls, total_ms=total_ns * 1e-6, mean_us=total_ns / calls * 1e-3)
        if "depth_refine" in name and images:
            out.update(us_per_refine=total_ns / refines * 1e-3, tb_per_s=refines * images * KERNEL_BYTES / (total_ns * 1e-9) / 1e12)
        print(json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--kernel-stats":
        return kernel_stats(args[1], int(args[2]) if len(args) > 2 else 0)
    bare = "--no-copy" not in args
    if bare:                                                                  # torch owns the device before the library touches it
        import torch
        torch.cuda.synchronize()
    import depthfilter_reference as DR
    import depthfilter_scenes as DS
    import laserline_scenes as LS
    from uzliti_slam_amd import capi
    sizes = [int(x) for x in args if not x.startswith("--")] or [64]
    base = [DS.scene(seed=30 + k, T=LS.camera_transform(yaw=40.0 + 90.0 * k, pitch=5.0 * k)) for k in range(4)]
    t = time.perf_counter()
    want = DR.refine(base[0][0]["depth"], base[0][1])
    numpy_s = time.perf_counter() - t
    for n in sizes:
        images = [dict(base[k % 4][0], group=k) for k in range(n)]
        guides = [base[k % 4][1] for k in range(n)]
        h, line = capi.DepthFilter(), capi.Laserline()
        h.refine(images, guides)                                              # warm-up: code objects, staging and HBM buffers
        assert np.array_equal(h.read(0).view(np.uint32), want.view(np.uint32))
        h.to_laserline(line)
        refine, both = [], []
        for _ in range(REPS):
            t = time.perf_counter(); h.refine(images, guides); refine.append(time.perf_counter() - t)
        for _ in range(REPS):
            t = time.perf_counter(); h.refine(images, guides); r, _, _ = h.to_laserline(line); both.append(time.perf_counter() - t)
        h.close(); line.close()
        out = dict(images=n, kernel_bytes=n * KERNEL_BYTES, beams_hit=int((r < 6).sum()), refine_ms=1e3 * float(np.median(refine)),
                   refine_to_laserline_ms=1e3 * float(np.median(both)), numpy_ms_per_image=1e3 * numpy_s, reps=REPS)
        if bare:
            src = torch.empty(n * KERNEL_BYTES // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            times = []
            for _ in range(REPS + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); dst.copy_(src); b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b))
            copy_ms = float(np.median(times[1:]))
            out.update(device_copy_ms=copy_ms, device_copy_tb_per_s=n * KERNEL_BYTES / (copy_ms * 1e-3) / 1e12)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
