"""NumPy restatement of the laser-line contract in include/uzl_mi355x.h ("Laser line from depth images"), written from the contract
alone: every f32 / f64 cast explicit, and the bin of a point found by the definition of step 6 itself - all n + 1 boundaries
tested for every point - so that it shares no shortcut with the kernel.  `extract` mirrors uzl_laserline_extract; the other
functions are the contract's steps, and two of the reference's own formulas (its atan2f bin and its sequential nearest / farthest
update) for the tests that compare against them."""
import functools
import math

import numpy as np

DEFAULTS = dict(min_height=0.0, max_height=1.0, angle_increment=math.pi / 360.0, range_min=0.45, range_max=5.0, depth_scale=1.0)
F32, F64 = np.float32, np.float64
CHUNK = 16384                         # points per (points x boundaries) block of the bin test


def angular_grid(angle_increment):
    """step 1 -> (amin, amax, inc) as float32 and n"""
    amin, amax, inc = F32(-math.pi), F32(math.pi), F32(angle_increment)
    return amin, amax, inc, int(np.uint32(np.ceil((amax - amin) / inc)))


@functools.lru_cache(maxsize=16)
def _trig(amin, inc, n):
    th = [amin + float(k) * inc for k in range(n + 1)]
    return np.array([math.cos(t) for t in th], F64), np.array([math.sin(t) for t in th], F64)


def trig_table(amin, inc, n):
    """step 1: (c_k, s_k), k = 0..n, theta_k = (double)amin + (double)k (double)inc, the host's libm (math, not np)"""
    return _trig(float(amin), float(inc), int(n))


def depth_values(depth, depth_scale=1.0):
    """step 2 -> (d as float32, used)"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        d = (depth.astype(F64) * 0.001).astype(F32)
    else:
        assert depth.dtype == F32
        d = depth.copy()
    if depth_scale != 1.0:
        d = (d.astype(F64) * float(depth_scale)).astype(F32)
    with np.errstate(invalid="ignore"):
        return d, (d > 0) & np.isfinite(d)


def base_points(d, u, v, fx, fy, cx, cy, T):
    """steps 3-4 for depths d at columns u, rows v (arrays of one shape) -> (qx, qy, qz) float32"""
    d = np.asarray(d, F32)
    dd = d.astype(F64)
    with np.errstate(all="ignore"):
        x = (((np.asarray(u, F64) - float(cx)) * dd) / float(fx)).astype(F32)
        y = (((np.asarray(v, F64) - float(cy)) * dd) / float(fy)).astype(F32)
        T = np.asarray(T, F64).reshape(12).astype(F32)
        q = [((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * d) + T[4 * a + 3] for a in range(3)]
    assert all(c.dtype == F32 for c in q)
    return q


def height_ok(qz, min_height, max_height):
    """step 5"""
    z = qz.astype(F64)
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(qz) | (z < float(min_height)) | (z > float(max_height)))


def bins(qx, qy, c, s):
    """step 6 by its definition -> bin per point, -1 = dropped"""
    n = len(c) - 1
    qx, qy = np.asarray(qx, F32).reshape(-1), np.asarray(qy, F32).reshape(-1)
    out = np.full(len(qx), -1, np.int64)
    for o in range(0, len(qx), CHUNK):
        X, Y = qx[o:o + CHUNK].astype(F64)[:, None], qy[o:o + CHUNK].astype(F64)[:, None]
        with np.errstate(all="ignore"):
            holds = ((c[None, :] * X + s[None, :] * Y) > 0) & ((c[None, :] * Y) >= (s[None, :] * X))
        below = Y[:, 0] < 0                                   # below the x axis: the smallest k that holds while k + 1 does not
        cand = holds[:, :n] & ~holds[:, 1:]
        first = np.where(cand.any(1), cand.argmax(1), -1)
        last = np.where(holds[:, :n].any(1), n - 1 - holds[:, n - 1::-1].argmax(1), -1)   # else: the largest k that holds
        out[o:o + CHUNK] = np.where(below, first, last)
    return out


def nearest_farthest(b, qx, qy, n, range_max):
    """step 7 over the points with bin b >= 0 -> (ranges, intensities) float32"""
    keep = b >= 0
    b, qx, qy = b[keep], qx[keep], qy[keep]
    with np.errstate(over="ignore"):
        s = qx * qx + qy * qy
    assert s.dtype == F32
    mn, mx = np.full(n, np.inf, F32), np.zeros(n, F32)
    np.minimum.at(mn, b, s)
    np.maximum.at(mx, b, s)
    hi = F32(range_max) + F32(1.0)
    return np.where(mn < hi * hi, np.sqrt(mn), hi).astype(F32), np.where(mx > 0, np.sqrt(mx), F32(0)).astype(F32)


def image_scan(image, cfg):
    """steps 2-7 of one image -> (ranges, intensities)"""
    amin, _, inc, n = angular_grid(cfg["angle_increment"])
    c, s = trig_table(amin, inc, n)
    depth = np.asarray(image["depth"])
    if depth.size == 0:
        return nearest_farthest(np.zeros(0, np.int64), np.zeros(0, F32), np.zeros(0, F32), n, cfg["range_max"])
    d, used = depth_values(depth, cfg["depth_scale"])
    v, u = np.nonzero(used)
    qx, qy, qz = base_points(d[used], u, v, image["fx"], image["fy"], image["cx"], image["cy"], image["camera_transform"])
    ok = height_ok(qz, cfg["min_height"], cfg["max_height"])
    qx, qy = qx[ok], qy[ok]
    return nearest_farthest(bins(qx, qy, c, s), qx, qy, n, cfg["range_max"])


def merge(scan, b, range_min, range_max):
    """step 8: (ranges, intensities) of b merged into those of scan"""
    lo, hi0 = F32(range_min), F32(range_max)
    out = []
    with np.errstate(invalid="ignore"):
        for which, (a, r) in enumerate(zip(scan, b)):
            skip = np.isnan(r) | (r < lo) | ((r > hi0) if which == 0 else False)
            take = np.isnan(a) | (a == 0) | (a > hi0)
            close = np.abs(a - r) < F32(0.1)
            far = F32(0) if which == 0 else np.where(a > r, F32(0), a)
            new = np.where(take, r, np.where(close, F32(0.5) * (a + r), far))
            out.append(np.where(skip, a, new).astype(F32))
    return out[0], out[1]


def scan_center(ranges, c, s, range_min, range_max):
    """step 9"""
    lo, hi0 = F32(range_min), F32(range_max)
    sx = sy = 0.0
    count = 0
    for k, r in enumerate(ranges):
        if np.isnan(r) or not r > lo or not r <= hi0:
            continue
        sx += float(c[k]) * float(r)
        sy += float(s[k]) * float(r)
        count += 1
    if count == 0:
        return np.zeros(3)
    return np.array([float(F32(sx / float(count))), float(F32(sy / float(count))), 0.0])


def extract(images, **cfg):
    """uzl_laserline_extract: images = dicts with depth, fx, fy, cx, cy, camera_transform and optionally group (default: the index)
    -> (ranges, intensities: float32 (n_scans, n); scan centres: float64 (n_scans, 3))"""
    cfg = dict(DEFAULTS, **cfg)
    amin, _, inc, n = angular_grid(cfg["angle_increment"])
    c, s = trig_table(amin, inc, n)
    scans, group = [], None
    for i, im in enumerate(images):
        one = image_scan(im, cfg)
        g = im.get("group", i)
        if scans and g == group:
            scans[-1] = merge(scans[-1], one, cfg["range_min"], cfg["range_max"])
        else:
            scans.append(one)
        group = g
    ranges = np.array([r for r, _ in scans], F32).reshape(len(scans), n)
    intens = np.array([i for _, i in scans], F32).reshape(len(scans), n)
    centres = np.array([scan_center(r, c, s, cfg["range_min"], cfg["range_max"]) for r in ranges], F64).reshape(len(scans), 3)
    return ranges, intens, centres


def grid_scans(ranges, nodes, **cfg):
    """the scans of an extract as uzl_grid_add_scans / uzl_laserline_to_grid store them"""
    cfg = dict(DEFAULTS, **cfg)
    amin, _, inc, _ = angular_grid(cfg["angle_increment"])
    return [dict(node=int(nd), ranges=r, angle_min=float(amin), angle_increment=float(inc), range_min=float(F32(cfg["range_min"])))
            for nd, r in zip(nodes, ranges)]


# ------------------------------------------------------------------------------------- the reference's own formulas
def atan2f_bins(qx, qy, amin, inc):
    """graph_grid_mapper.cpp:452-458: (int)((-atan2(-y, x) - angle_min) / angle_increment), float throughout"""
    qx, qy = np.asarray(qx, F32), np.asarray(qy, F32)
    angle = -np.arctan2(-qy, qx)
    assert angle.dtype == F32
    return ((angle - F32(amin)) / F32(inc)).astype(np.int64)


def sequential_nearest_farthest(s_values, range_max):
    """graph_grid_mapper.cpp:459-465 on one bin: the squared ranges in the order given -> (range, intensity)"""
    rng, far = F32(range_max) + F32(1.0), F32(0)
    for s in s_values:
        s = F32(s)
        if s < rng * rng:
            rng = np.sqrt(s)
        if s > far * far:
            far = np.sqrt(s)
    return F32(rng), F32(far)
