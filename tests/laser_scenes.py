"""Synthetic laser scans for the scan matcher's tests: exact 2-D ray casts against polygons from two known sensor poses, so every
scene has a known true relative pose (T_true: `to`'s frame in `from`'s).  A scan is the dict capi.Laser.add_scans and
laser_reference take: values (f32), angle_min, angle_increment, range_min, range_max."""
import math

import numpy as np

F32 = np.float32
ROOM = [(0.0, 0.0), (6.0, 0.0), (6.0, 4.0), (0.0, 4.0)]                                  # 6 x 4 m
CORRIDOR = [(0.0, 0.0), (7.0, 0.0), (7.0, 5.0), (5.2, 5.0), (5.2, 1.6), (0.0, 1.6)]      # L-shaped, 1.6 / 1.8 m wide
CLOSET = [(0.0, 0.0), (2.2, 0.0), (2.2, 1.6), (0.0, 1.6)]                                # small enough for a 5-degree grid
RANGE_MIN, RANGE_MAX = 0.05, 12.0


def cast_rays(polygon, x, y, d):
    """t >= 0 at which the ray (x, y) + t d[k] leaves the polygon (inf: never), for direction vectors d (n, 2) of any length"""
    P = np.asarray(polygon, np.float64)
    r = np.full(len(d), np.inf)
    for k in range(len(P)):
        p0, e = P[k], P[(k + 1) % len(P)] - P[k]
        den = d[:, 0] * e[1] - d[:, 1] * e[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((p0[0] - x) * e[1] - (p0[1] - y) * e[0]) / den
            u = ((p0[0] - x) * d[:, 1] - (p0[1] - y) * d[:, 0]) / den
        hit = (np.abs(den) > 1e-14) & (t > 0) & (u >= 0) & (u <= 1)
        r = np.where(hit & (t < r), t, r)
    return r


def cast(polygon, pose, n, angle_min, angle_increment):
    """ranges (f32) of n beams from pose = (x, y, theta) inside the polygon; the beam angles are the f64 values of the f32 grid"""
    x, y, th = pose
    amin, inc = float(F32(angle_min)), float(F32(angle_increment))
    a = th + amin + inc * np.arange(n)
    return cast_rays(polygon, x, y, np.stack([np.cos(a), np.sin(a)], 1)).astype(F32)


def depth_image(polygon, pose, width, height, fx, cx):
    """32FC1 depth image of the polygon's (vertical) walls from a level camera at pose = (x, y, yaw): the optical axis is the
    base frame's x, column u looks along (1, -(u - cx) / fx), and depth is the distance along the axis - the same in every row"""
    x, y, th = pose
    c, s = math.cos(th), math.sin(th)
    lat = -(np.arange(width) - cx) / fx
    d = np.stack([c - s * lat, s + c * lat], 1)
    return np.repeat(cast_rays(polygon, x, y, d).astype(F32)[None, :], height, 0)


def scan(values, angle_min, angle_increment):
    return dict(values=np.ascontiguousarray(values, F32), angle_min=float(F32(angle_min)), angle_increment=float(F32(angle_increment)),
                range_min=RANGE_MIN, range_max=RANGE_MAX)


def pose_matrix(x, y, th):
    return np.array([[math.cos(th), -math.sin(th), 0, x], [math.sin(th), math.cos(th), 0, y], [0, 0, 1, 0]], np.float64)


def relative(pose_from, pose_to):
    """T_true = pose_from^-1 pose_to as (x, y, theta)"""
    xf, yf, tf = pose_from
    dx, dy = pose_to[0] - xf, pose_to[1] - yf
    c, s = math.cos(tf), math.sin(tf)
    return (c * dx + s * dy, -s * dx + c * dy, pose_to[2] - tf)


def displaced(true, dx, dy, dth_deg):
    """a first guess (3x4): the true relative pose moved by (dx, dy) m and dth_deg degrees"""
    return pose_matrix(true[0] + dx, true[1] + dy, true[2] + math.radians(dth_deg))


GUESSES = [(0.3, 0.0, 10.0), (-0.2, 0.2, -10.0), (0.1, -0.15, 5.0)]                      # up to 0.3 m and 10 degrees off


def make(name, polygon, pose_from, pose_to, n, angle_min, angle_increment, invalid=0.0, seed=0):
    f = cast(polygon, pose_from, n, angle_min, angle_increment)
    t = cast(polygon, pose_to, n, angle_min, angle_increment)
    if invalid > 0.0:                                        # out of range below and above, and NaN, a third each
        rng = np.random.RandomState(seed)
        for v in (f, t):
            bad = rng.permutation(n)[:int(round(invalid * n))]
            v[bad[0::3]] = F32(0.0)
            v[bad[1::3]] = F32(40.0)
            v[bad[2::3]] = F32(np.nan)
    return dict(name=name, scan_from=scan(f, angle_min, angle_increment), scan_to=scan(t, angle_min, angle_increment),
                true=relative(pose_from, pose_to), n=n)


def scenes():
    """name -> scene; every scene with at least 37 beams converges to its true pose from GUESSES"""
    full = (-math.pi, math.pi / 360)                         # the laser line's default grid: 720 beams over 360 degrees
    a, b = (2.0, 1.5, 0.1), (2.6, 1.9, 0.45)
    out = [make("room", ROOM, a, b, 720, *full),
           make("corridor", CORRIDOR, (6.0, 1.0, 0.5), (6.2, 2.0, 1.0), 720, *full),
           make("room_invalid", ROOM, a, b, 720, *full, invalid=0.30, seed=5),
           make("closet37", CLOSET, (0.9, 0.7, 0.2), (1.1, 0.8, 0.4), 37, -math.pi / 2, math.pi / 36),
           make("room8", ROOM, a, (2.1, 1.55, 0.15), 8, -math.pi, math.pi / 4)]
    return {s["name"]: s for s in out}


def empty_scan(n=720):
    """no valid beam"""
    return scan(np.zeros(n, F32), -math.pi, math.pi / 360)
