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


MIRROR_ROOM = [(-2.0, -1.5), (4.0, -1.5), (4.0, 1.5), (-2.0, 1.5)]                       # symmetric about the x axis
MIRROR_GRID = (-100 * 2.0 ** -5, 2.0 ** -5)              # 201 beams: every angle exact, beam 100 at 0, so the table is symmetric
MIRROR_X = (0.17, 0.0, 0.0)                              # the stage estimate: c = 1 and s = 0 exactly
# (outliers_max_perc, outliers_adaptive_order, outliers_adaptive_mult) settings -> correspondences the restatement leaves on `mirror`
MIRROR_TRIMS = [(dict(), 154), (dict(outliers_max_perc=0.0), 2), (dict(outliers_max_perc=1.0, outliers_adaptive_mult=1.0), 134),
                (dict(outliers_adaptive_order=0.0), 2), (dict(outliers_adaptive_mult=0.0), 0),
                (dict(outliers_max_perc=1.0, outliers_adaptive_order=1.0), 191)]
STRIP_COUNTS = [9, 63, 64, 65, 255, 256, 257, 511, 512, 513]                             # beside 64, 256 and 512: lane t owns t, t + 256, ...
STRIP_PAIRS = [(257, 255), (255, 257), (256, 256), (513, 64), (512, 63), (65, 511), (9, 257)]   # (from, to) beam counts
STRIP_POSES = ((2.0, 1.5, 0.1), (2.2, 1.6, 0.2))
STRIP_GUESS = (0.1, -0.05, 4.0)
RANGE_EDGE_AT = 300                                      # first of the eight edited readings of `range_edges`
RANGE_EDGE_VALID = [1, 0, 1, 0, 0, 0, 0, 0]
# configurations on the stock `room` with GUESSES[0] -> what the restatement gives (status by name, then the fields that are pinned)
STATUS_CONFIGS = [(dict(min_valid_fraction=0.9), "FEW_MATCHES", dict()),
                  (dict(max_iterations=1), "OK", dict(iterations=1, nvalid=310)),
                  (dict(max_iterations=2), "OK", dict(iterations=2, nvalid=501)),
                  (dict(epsilon_xy=0.0, epsilon_theta=0.0, max_iterations=6), "OK", dict(iterations=6)),
                  (dict(max_angular_correction_deg=5.0), "TOO_FAR", dict()),
                  (dict(fail_fraction=0.9), "FEW_CORR", dict(iterations=0)),
                  (dict(max_correspondence_dist=0.0), "FEW_CORR", dict(iterations=0))]


def range_edge_values():
    """f32(range_min), the f32 below it, f32(range_max), the f32 above it, +inf, -inf, -0.0, NaN"""
    lo, hi = F32(RANGE_MIN), F32(RANGE_MAX)
    return np.array([lo, np.nextafter(lo, F32(0)), hi, np.nextafter(hi, F32(np.inf)), np.inf, -np.inf, -0.0, np.nan], F32)


def edge(name, scan_from, scan_to, true, x=None, guess=None, **cfg):
    """a scene of edge_scenes(): `x` = (tx, ty, theta) is where the stage entry is evaluated, `guess` the 3x4 first guess of a
    solve; by default both are the true pose displaced by STRIP_GUESS.  `cfg`: the settings the scene's stage is evaluated under."""
    if guess is None:
        guess = pose_matrix(*x) if x is not None else displaced(true, *STRIP_GUESS)
    if x is None:
        x = (float(guess[0, 3]), float(guess[1, 3]), math.atan2(guess[1, 0], guess[0, 0]))
    return dict(name=name, scan_from=scan_from, scan_to=scan_to, true=true, x=tuple(x), guess=guess, n=len(scan_to["values"]),
                n_from=len(scan_from["values"]), cfg=cfg)


def edge_scenes():
    """name -> scene for the rules the ray-cast scenes of scenes() never reach: exact ties by symmetry (mirror*), clockwise and
    zero-increment grids (coincident, reach), beam counts beside the strip width (strip_<from>_<to>), four grids of one length
    (grid_*), readings at the range limits, and a pair that converges further from its first guess than step 10 allows (far64)"""
    out = []
    amin, inc = MIRROR_GRID
    mf = cast(MIRROR_ROOM, (0.0, 0.0, 0.0), 201, amin, inc)
    mt = cast(MIRROR_ROOM, (0.1, 0.0, 0.0), 201, amin, inc)
    for v in (mf, mt):
        v[:100] = v[101:][::-1]                              # bit-equal readings left and right of beam 100
    true = (0.1, 0.0, 0.0)

    def mirror(name, edit_from=(), edit_to=()):
        f, t = mf.copy(), mt.copy()
        for sl, val in edit_from:
            f[sl] = val
        for sl, val in edit_to:
            t[sl] = val
        out.append(edge(name, scan(f, amin, inc), scan(t, amin, inc), true, x=MIRROR_X))

    nan = F32(np.nan)
    mirror("mirror")
    mirror("mirror_hole", [(slice(100, 101), nan)])
    mirror("mirror_updown", [(slice(99, 102), np.array([nan, 3.9, nan], F32))])
    mirror("mirror_doubles", [(slice(97, 100), nan), (slice(101, 104), nan)], [(slice(100, 101), nan)])
    # the same `from` points stored clockwise (the solve starts off the axis: a symmetric second iteration is summation noise)
    out.append(edge("clockwise", scan(mf[::-1], -amin, -inc), scan(mt, amin, inc), true, x=MIRROR_X, guess=displaced(true, *STRIP_GUESS)))
    a, b = STRIP_POSES
    rel = relative(a, b)
    room = {n: (scan(cast(ROOM, a, n, -math.pi, 2 * math.pi / n), -math.pi, 2 * math.pi / n),
                scan(cast(ROOM, b, n, -math.pi, 2 * math.pi / n), -math.pi, 2 * math.pi / n)) for n in STRIP_COUNTS}
    i257 = 2 * math.pi / 257
    grids = dict(A=(-math.pi, i257), B=(-math.pi + 0.3, i257), C=(-math.pi, 0.9 * i257), D=(math.pi, -i257))
    out.append(edge("clockwise257", room[257][0], scan(cast(ROOM, b, 257, *grids["D"]), *grids["D"]), rel))
    # every point of a scan on one ray
    out.append(edge("coincident", scan([1, 1, 1.5, 2, 2, 2.5, 3, 3, 3.5, 4, 4, 4.5], 0.25, 0.0),
                    scan([1.02, 1.2, 1.5, 1.9, 2.05, 2.4, 2.9, 3.1, 3.5, 3.9, 4.1, 4.4], 0.25, 0.0), (0.0, 0.0, 0.0), x=(0.01, 0.02, 0.01)))
    # one ray at angle 0 (c = 1, s = 0), identity estimate, max_correspondence_dist = 2^-2: five beams of `to` lie exactly that far
    # from their j1 (squared distance 2^-4 on both sides of the comparison), one lies twice as far, two lie on their j1
    out.append(edge("reach", scan([1, 2, 3, 4, 5, 6, 7, 8], 0.0, 0.0), scan([1.25, 2.25, 3.5, 4.0, 4.75, 6.25, 7.0, 8.25], 0.0, 0.0),
                    (0.0, 0.0, 0.0), x=(0.0, 0.0, 0.0), max_correspondence_dist=0.25))
    for nf, nt in STRIP_PAIRS:
        out.append(edge("strip_%d_%d" % (nf, nt), room[nf][0], room[nt][1], rel))
    for g in "ABCD":
        out.append(edge("grid_" + g, room[257][0], scan(cast(ROOM, b, 257, *grids[g]), *grids[g]), rel))
    # a 0.9 x 0.6 m room: every point stays within max_correspondence_dist under a first guess 33 degrees off, so the solve
    # converges and step 10 rejects it at the default limits (1.5 x 33 > 45)
    tiny, ta, tb = [(0.15 * px, 0.15 * py) for px, py in ROOM], (0.45, 0.3, 0.1), (0.465, 0.315, 0.2)
    i64 = 2 * math.pi / 64
    out.append(edge("far64", scan(cast(tiny, ta, 64, -math.pi, i64), -math.pi, i64), scan(cast(tiny, tb, 64, -math.pi, i64), -math.pi, i64),
                    relative(ta, tb), guess=displaced(relative(ta, tb), 0.0, 0.0, 33.0)))
    stock = scenes()["room"]
    v = stock["scan_to"]["values"].copy()
    v[RANGE_EDGE_AT:RANGE_EDGE_AT + 8] = range_edge_values()
    out.append(edge("range_edges", stock["scan_from"], scan(v, -math.pi, math.pi / 360), stock["true"],
                    guess=displaced(stock["true"], *GUESSES[0])))
    return {s["name"]: s for s in out}


def empty_scan(n=720):
    """no valid beam"""
    return scan(np.zeros(n, F32), -math.pi, math.pi / 360)
