"""GPU test of the CloudTransformationEstimator mirror in uzliti_slam_amd/adapter/ (adapter_selftest `cloud`): nodes with one depth
and colour image each, queued pair by pair as GraphSlamNode queues them; the edges the worker thread delivers equal, bit for bit,
what uzl_cloud_add_images + uzl_cloud_estimate give for the same images with T_diff = from.pose^-1 to.pose."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cloud_scenes as CS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTER = os.path.join(ROOT, "uzliti_slam_amd", "adapter")


def test_the_cloud_estimator_mirror(capi, tmp_path):
    exe = os.path.join(ADAPTER, "adapter_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", ADAPTER])
    s = CS.scenes()["corner"]
    world = CS.pose([1.0, -0.5, 0.2], [0.1, -0.2, 0.3])                      # node 0 somewhere in the map, node 1 by odometry
    poses = [world, CS.mul(world, CS.displaced(s["true"], 0.03, 1.0))]
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<i", 2))
        for side, T in zip(("from", "to"), poses):
            d = s["depth_" + side]
            f.write(struct.pack("<ii4d", d.shape[1], d.shape[0], s["fx"], s["fy"], s["cx"], s["cy"]))
            f.write(T.astype("<f8").tobytes()); f.write(np.ascontiguousarray(d, "<f4").tobytes()); f.write(np.ascontiguousarray(s["bgr_" + side]).tobytes())
    r = subprocess.run([exe, "cloud", str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "CLOUD_OK 2 pairs" in r.stdout, (r.returncode, r.stdout, r.stderr)
    raw = open(out, "rb").read()
    rec = np.dtype([("type", "<i4"), ("sensors", "<i4"), ("score", "<f8"), ("transform", "<f8", (12,)), ("information", "<f8", (36,))])
    got = np.frombuffer(raw[:2 * rec.itemsize], rec)
    iterations, num_corr = struct.unpack("<ii", raw[2 * rec.itemsize:])
    h = capi.Cloud()
    im = lambda side: dict(depth=s["depth_" + side], fx=s["fx"], fy=s["fy"], cx=s["cx"], cy=s["cy"], camera_transform=np.eye(3, 4))
    assert h.add_images([im("from"), im("to")], [s["bgr_from"], s["bgr_to"]]) == 0

    def mul(A, B):                                                           # the mirror's order of operations
        C = np.zeros((3, 4))
        for r_ in range(3):
            for c in range(4):
                C[r_, c] = A[r_, 0] * B[0, c] + A[r_, 1] * B[1, c] + A[r_, 2] * B[2, c]
            C[r_, 3] += A[r_, 3]
        return C

    def inv(A):
        B = np.zeros((3, 4))
        B[:, :3] = A[:, :3].T
        for r_ in range(3):
            B[r_, 3] = -(A[0, r_] * A[0, 3] + A[1, r_] * A[1, 3] + A[2, r_] * A[2, 3])
        return B

    I = np.eye(3, 4)
    guess = lambda a, b: mul(mul(mul(inv(I), inv(I)), mul(inv(poses[a]), poses[b])), mul(I, I))
    want = h.estimate([(0, 1, guess(0, 1)), (1, 0, guess(1, 0))])
    h.close()
    for g, w in zip(got, want):
        assert w["status"] == capi.CLOUD_OK and g["type"] == 1 and g["sensors"] == 1 and g["score"] == 1.0
        assert g["transform"].tobytes() == w["transform"].tobytes() and g["information"].tobytes() == w["information"].tobytes()
    assert CS.pose_errors(got[0]["transform"], s["true"])[0] < 1e-3
    assert (iterations, num_corr) == (int(want[0]["iterations"]), int(want[0]["num_corr"]))
