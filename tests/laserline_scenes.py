"""Seeded depth-image scenes for the laser-line tests and tests/diag/laserline_timing.py: a camera looking into a room of random
depth with holes, and the base <- camera transforms the tests put it through."""
import math

import numpy as np

FX = FY = 525.0


def rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


# optical frame (x right, y down, z forward) -> base frame (x forward, y left, z up)
OPTICAL = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])


def camera_transform(yaw=0.0, pitch=0.0, roll=0.0, height=0.6, x=0.0, y=0.0):
    """base <- camera, 3x4: the camera `height` up, yawed, pitched (down is positive) and rolled, in degrees"""
    T = np.zeros((3, 4))
    T[:, :3] = rot("z", yaw) @ rot("y", pitch) @ rot("x", roll) @ OPTICAL
    T[:, 3] = [x, y, height]
    return T


def room(width=640, height=480, seed=0, lo=1.5, hi=4.0, holes=0.1, u16=False):
    """random depth lo..hi m with a share of holes (0, and NaN for f32) -> float32 metres or uint16 millimetres"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(lo, hi, (height, width)).astype(np.float32)
    hole = rng.random((height, width)) < holes
    if u16:
        out = np.round(d.astype(np.float64) * 1000.0).astype(np.uint16)
        out[hole] = 0
        return out
    d[hole] = np.where(rng.random(int(hole.sum())) < 0.5, np.float32(0), np.float32(np.nan))
    return d


def image(depth, T=None, group=None, fx=None, fy=None):
    """the dict Laserline.extract and the restatement take; the focal lengths default to a 640-pixel-wide camera's field of view"""
    h, w = depth.shape
    fx = FX * max(w, 1) / 640.0 if fx is None else fx
    fy = fx if fy is None else fy
    im = dict(depth=depth, fx=fx, fy=fy, cx=(w - 1) / 2.0, cy=(h - 1) / 2.0,
              camera_transform=camera_transform(yaw=40.0) if T is None else T)
    if group is not None:
        im["group"] = group
    return im


def circle_points(n, seed=0):
    """base-frame points spread over the full circle, 0.3 .. 6 m out -> (qx, qy) float32"""
    rng = np.random.default_rng(seed)
    a, r = rng.uniform(-math.pi, math.pi, n), rng.uniform(0.3, 6.0, n)
    return (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)
