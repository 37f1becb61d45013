"""Planted scenes for the laser-line edge tests (test_laserline_edges_reference.py on the CPU, test_laserline_edges_gpu.py on the
device): points of exact f32 coordinates beside bin boundaries, at the +-pi seam, on the axes and where an atan2f guess misses;
height and depth limits; images whose columns walk through the bins row by row, with the restated lane walk that says which rows
one lane of the bin kernel visits in order; and the merge / centre truth table.  Everything is seeded and built from
laserline_reference alone; the expected values of a scene are computed once and shared (expected())."""
import collections
import functools
import itertools
import math

import numpy as np

import laserline_reference as LR

F32, F64 = np.float32, np.float64
GRIDS = {720: math.pi / 360, 1257: 0.005, 1440: math.pi / 720, 4096: 6.2831855 / 4095.5}       # the grids of test_laserline_gpu.py
DENORM = np.nextafter(F32(0), F32(1))
FLT_MAX = np.finfo(F32).max
RADII = (0.5, 3.0, 1e3)


def table(n):
    """grid n -> (amin, inc, c, s)"""
    amin, _, inc, m = LR.angular_grid(GRIDS[n])
    assert m == n
    return (amin, inc) + LR.trig_table(amin, inc, n)


def ulps(x, k):
    """the f32 k steps above x (below for k < 0), +0 and -0 counted as one value"""
    i = np.asarray(x, F32).view(np.int32).astype(np.int64)
    i = np.where(i < 0, -(i & 0x7fffffff), i) + k
    return np.where(i < 0, (-i) | 0x80000000, i).astype(np.uint32).view(F32)


def is_neg_zero(v):
    return bool(v == 0 and np.signbit(v))


# ------------------------------------------------------------------------------------------------------ 1. exact planted points
def point_image(X, Y, Z=0.5, group=None):
    """A 1 x 1 f32 image of depth 1 whose base-frame point is (X, Y, Z) bit for bit: the rotation part is zero, so
    q_a = ((0 x + 0 y) + 0 d) + T[a][3].  fx = fy = -1 make x = y = -0, and a coordinate that is to be -0 gets the row
    (0, 0, -0, -0): every term of its sum is then -0; any other row ends in +0 + V = V."""
    rows = [[0.0, 0.0, -0.0, -0.0] if is_neg_zero(v) else [0.0, 0.0, 0.0, float(v)] for v in (F32(X), F32(Y), F32(Z))]
    im = dict(depth=np.ones((1, 1), F32), fx=-1.0, fy=-1.0, cx=0.0, cy=0.0, camera_transform=np.array(rows, F64))
    if group is not None:
        im["group"] = group
    return im


def point_images(points):
    """(X, Y[, Z]) per point -> one image and one scan each"""
    return [point_image(*p) for p in points]


def image_points(images):
    """the base-frame points of images of one pixel each, by the reference's steps 2-4 -> (qx, qy, qz) float32"""
    q = []
    for im in images:
        d, _ = LR.depth_values(im["depth"])
        q.append([c[0] for c in LR.base_points(d.reshape(-1)[:1], [0], [0], im["fx"], im["fy"], im["cx"], im["cy"], im["camera_transform"])])
    return tuple(np.array(c, F32) for c in zip(*q))


def boundary_ks(n):
    """the boundaries the issue names and a seeded handful more"""
    rng = np.random.default_rng(n)
    return [0, 1, n // 4, n // 2 - 1, n // 2, n // 2 + 1, 3 * n // 4, n - 2, n - 1, n] + sorted(int(k) for k in rng.integers(2, n - 2, 6))


def boundary_clusters(n):
    """-> [(k, r, X[5], Y[5])]: the f32 point nearest to r (c_k, s_k) and its neighbours at -2 .. 2 ulp in Y, or in X where
    |s_k| > |c_k|"""
    _, _, c, s = table(n)
    out = []
    for k in boundary_ks(n):
        for r in RADII:
            X, Y = np.full(5, F32(r * c[k])), np.full(5, F32(r * s[k]))
            steps = np.arange(-2, 3)
            if abs(s[k]) > abs(c[k]):
                X = ulps(X, steps)
            else:
                Y = ulps(Y, steps)
            out.append((k, r, X, Y))
    return out


def seam_points(n):
    """X < 0 with Y = +-0, +- the smallest denormal, +- the f32 around |X| 8.74e-8 (the tangent of amin + pi) and the f32 either
    side of X tan(theta_0) and X tan(theta_n), mirrored below the axis too -> (X, Y)"""
    _, _, c, s = table(n)
    xs, ys = [], []
    for X in (F32(-0.5), F32(-3.0), F32(-1e3)):
        Y = [F32(0.0), F32(-0.0), DENORM, -DENORM]
        base = [F32(abs(float(X)) * 8.74e-8), F32(float(X) * s[0] / c[0]), F32(float(X) * s[n] / c[n])]
        for b in base:
            for k in range(-2, 3):
                Y += [ulps(b, k)[()], -ulps(b, k)[()]]
        xs += [X] * len(Y)
        ys += Y
    return np.array(xs, F32), np.array(ys, F32)


def axis_points():
    """(+-r, +-0), (+-0, +-r), denormal coordinates and 3e38 in each coordinate -> (X, Y); the origins are origin_points()"""
    z, big = [F32(0.0), F32(-0.0)], F32(3e38)
    pts = []
    for r in (F32(0.5), F32(3.0), DENORM, F32(1e-40), big):
        pts += [(sr, z0) for sr in (r, -r) for z0 in z] + [(z0, sr) for sr in (r, -r) for z0 in z]
    for a in (DENORM, F32(-1e-40), big, -big):
        pts += [(a, DENORM), (a, -DENORM), (DENORM, a), (-DENORM, a), (a, F32(1.0)), (F32(-1.0), a), (a, a), (a, -a)]
    X, Y = zip(*pts)
    return np.array(X, F32), np.array(Y, F32)


def origin_points():
    return np.array([0.0, -0.0, 0.0, -0.0], F32), np.array([0.0, 0.0, -0.0, -0.0], F32)


@functools.lru_cache(maxsize=None)
def guess_misses(n, want=40, batch=1500):
    """Seeded points beside boundaries where the reference's own atan2f bin (LR.atan2f_bins) differs from step 6's, and points whose
    guess leaves [0, n) before the clamp -> (X, Y, clamped: how many of them are of the second kind).  The search runs batch by
    batch until `want` points are found."""
    amin, inc, c, s = table(n)
    rng = np.random.default_rng(1000 + n)
    found, clamp = [], []
    for _ in range(20):
        k = rng.integers(0, n + 1, batch)
        r = rng.uniform(0.3, 6.0, batch)
        X, Y = (r * c[k]).astype(F32), (r * s[k]).astype(F32)
        step = rng.integers(-2, 3, batch)
        in_x = np.abs(s[k]) > np.abs(c[k])
        X, Y = np.where(in_x, ulps(X, step), X), np.where(in_x, Y, ulps(Y, step))
        # the seam's share: on and just above the negative x axis, where the f32 angle is pi
        m = batch // 10
        X[:m] = -r[:m].astype(F32)
        Y[:m] = np.where(rng.random(m) < 0.3, F32(0), (r[:m] * rng.uniform(0, 2e-7, m)).astype(F32))
        mine, guess = LR.bins(X, Y, c, s), LR.atan2f_bins(X, Y, amin, inc)
        for i in np.nonzero((mine != guess) & (mine >= 0))[0]:
            (clamp if guess[i] < 0 or guess[i] >= n else found).append((X[i], Y[i]))
        if len(found) >= want:
            break
    pts = found[:want] + clamp[:10]
    return np.array([p[0] for p in pts], F32), np.array([p[1] for p in pts], F32), len(clamp[:10])


@functools.lru_cache(maxsize=None)
def planted(n):
    """every family of exact points for grid n -> {family: (X, Y)}"""
    cl = boundary_clusters(n)
    return dict(boundary=(np.concatenate([x for _, _, x, _ in cl]), np.concatenate([y for _, _, _, y in cl])),
                seam=seam_points(n), axes=axis_points(), origin=origin_points(), misses=guess_misses(n)[:2])


def planted_images(n):
    return [point_image(x, y) for X, Y in planted(n).values() for x, y in zip(X, Y)]


# non-finite coordinates from finite inputs: fx = fy = 1e-38 and u - cx = v - cy = 3 give x = y = 3e38, a coefficient of +-2 sends
# a sum to +-inf, a pair (2, -2) to inf - inf = NaN, and u - cx = 12 makes x itself infinite, so that a zero coefficient gives NaN
def _overflow_image(rx, ry, rz, cx=-3.0):
    return dict(depth=np.ones((1, 1), F32), fx=1e-38, fy=1e-38, cx=cx, cy=-3.0, camera_transform=np.array([rx, ry, rz], F64))


NONFINITE = {                                      # name -> image; the CPU test asserts which coordinates come out infinite or NaN
    "qx=+inf": _overflow_image([2, 0, 0, 0], [0, 0, 0, 1.5], [0, 0, 0, 0.5]),
    "qx=-inf": _overflow_image([-2, 0, 0, 0], [0, 0, 0, 1.5], [0, 0, 0, 0.5]),
    "qx=+inf, qy<0": _overflow_image([2, 0, 0, 0], [0, 0, 0, -1.5], [0, 0, 0, 0.5]),
    "qx=-inf, qy<0": _overflow_image([-2, 0, 0, 0], [0, 0, 0, -1.5], [0, 0, 0, 0.5]),
    "qy=+inf": _overflow_image([0, 0, 0, 1.5], [0, 2, 0, 0], [0, 0, 0, 0.5]),
    "qy=-inf": _overflow_image([0, 0, 0, 1.5], [0, -2, 0, 0], [0, 0, 0, 0.5]),
    "qy=+inf, qx<0": _overflow_image([0, 0, 0, -1.5], [0, 2, 0, 0], [0, 0, 0, 0.5]),
    "qy=-inf, qx<0": _overflow_image([0, 0, 0, -1.5], [0, -2, 0, 0], [0, 0, 0, 0.5]),
    "both inf": _overflow_image([2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 0, 0.5]),
    "qx=inf-inf": _overflow_image([2, -2, 0, 0], [0, 0, 0, 1.5], [0, 0, 0, 0.5]),
    "qy=inf-inf": _overflow_image([0, 0, 0, 1.5], [2, -2, 0, 0], [0, 0, 0, 0.5]),
    "qz=inf-inf": _overflow_image([0, 0, 0, 1.5], [0, 0, 0, 1.5], [2, -2, 0, 0.5]),
    "x=inf, qx=inf 0": _overflow_image([0, 0, 0, 1.5], [0, 0, 0, 1.5], [0, 0, 0, 0.5], cx=-12.0),
    "x=inf, qy=qz=inf 0": _overflow_image([1, 0, 0, 0], [0, 0, 0, 1.5], [0, 0, 0, 0.5], cx=-12.0),
}

# heights: (min_height, max_height) -> [(Z, kept)], and whether comparing in f32 ((float)min_height, (float)max_height) would keep
# another set.  0.1 and 0.7 are the issue's; 0.7 as a minimum and 1.1, 0.3 as maxima are the limits that round the other way, so
# that a narrowed comparison keeps the f32 the double comparison drops.
def _around(v):
    """the f32 either side of the double v; v itself between them where it is an f32"""
    if float(F32(v)) == v:
        return [np.nextafter(F32(v), F32(-np.inf)), F32(v), np.nextafter(F32(v), F32(np.inf))]
    lo = F32(v) if float(F32(v)) < v else np.nextafter(F32(v), F32(-np.inf))
    return [lo, np.nextafter(lo, F32(np.inf))]


HEIGHTS = {
    (0.1, 0.7): list(zip(_around(0.1) + _around(0.7), [False, True, True, False])),
    (0.5, 0.5): list(zip(_around(0.5), [False, True, False])),
    (0.0, 1.0): [(F32(0.0), True), (F32(-0.0), True), (-DENORM, False), (F32(1.0), True), (np.nextafter(F32(1), F32(2)), False)],
    (0.7, 1.1): list(zip(_around(0.7) + _around(1.1), [False, True, True, False])),
    (0.3, 0.3): list(zip(_around(0.3), [False, False])),
}


def height_images(limits):
    return [point_image(2.0, 1.0, z) for z, _ in HEIGHTS[limits]]


def level_camera(height=0.5):
    """looks along +x, level: q_x = d, q_y = -x, q_z = -y + height"""
    return np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, height]], F64)


def depth_validity_images():
    """1 x 1 and 1 x 5 images of the pixel values at the ends of both encodings -> {"f32": images, "u16": images}"""
    f = np.array([-0.0, DENORM, FLT_MAX, np.inf, np.nan, 1.0, 2.5, 1e-30, 3e4], F32)
    u = np.array([0, 1, 65535, 1000, 2500], np.uint16)
    out = {}
    for name, vals in (("f32", f), ("u16", u)):
        ims = [dict(depth=vals[i:i + 1].reshape(1, 1).copy(), fx=300.0, fy=300.0, cx=0.0, cy=0.0, camera_transform=level_camera())
               for i in range(len(vals))]
        for i in range(len(vals)):
            row = np.roll(vals, -i)[:5].reshape(1, 5).copy()
            ims.append(dict(depth=row, fx=300.0, fy=300.0, cx=2.0, cy=0.0, camera_transform=level_camera()))
        out[name] = ims
    return out


DEPTH_SCALES = {"f32": (1.0, 1e300, 0.001, 1000.0), "u16": (1.0, 1e-46, 0.001, 1000.0)}


# ------------------------------------------------------------------------------------------------------------- 2. column walks
BLOCK, VEC = 256, 4                       # kLaserBlock, kLaserVec (laserline_types.hpp)


def lanes_for(nvec):
    """uzl_laserline.hip, lanes_for:
        for (int passes = 1; passes <= 8; passes++) {
            const int lanes = (nvec + passes - 1) / passes;
            if (lanes < 1 || lanes > kLaserBlock) continue;
            const double use = (double)nvec / ((double)passes * lanes) * (double)(lanes * (kLaserBlock / lanes)) / kLaserBlock;
            if (use > best_use) { best_use = use; best = lanes; }
        }
        return best_use > 0. ? best : kLaserBlock;"""
    best, best_use = 1, 0.0
    for passes in range(1, 9):
        lanes = (nvec + passes - 1) // passes
        if lanes < 1 or lanes > BLOCK:
            continue
        use = float(nvec) / (float(passes) * lanes) * float(lanes * (BLOCK // lanes)) / BLOCK
        if use > best_use:
            best_use, best = use, lanes
    return best if best_use > 0 else BLOCK


def band_rows(rows_in_chunk):
    """uzl_laserline.hip, launch_bin: a.band_rows = min(max((rows + 2047) / 2048, 8), 64)"""
    return min(max((rows_in_chunk + 2047) // 2048, 8), 64)


def lane_visits(width, height, rows_in_chunk):
    """laserline_kernels.hip, bin_band: thread t of a band's workgroup takes the vectors cv = t % lanes, + lanes, ... and in each the
    rows r0 + t / lanes, + side, ... (side = kLaserBlock / lanes), with a fresh Column per vector
    -> [(band, lane, column, rows in the order visited)], one entry per Column the kernel opens"""
    nvec = (width + VEC - 1) // VEC
    lanes = lanes_for(nvec)
    side, rows_per_band = BLOCK // lanes, band_rows(rows_in_chunk)
    out = []
    for band, r0 in enumerate(range(0, height, rows_per_band)):
        r1 = min(r0 + rows_per_band, height)
        for t in range(lanes * side):
            rows = list(range(r0 + t // lanes, r1, side))
            for cv in range(t % lanes, nvec, lanes):
                out += [(band, t, u, rows) for u in range(cv * VEC, min(cv * VEC + VEC, width))]
    return out


FY = 344.0                                # one row is 1 / 344 rad: a third of a bin of pi / 360
WINDOW = dict(min_height=-8.0, max_height=8.0)     # keeps every pixel of depth <= 4; a depth of 60 leaves it beyond 46 columns from cx
OUT_DEPTH = 60.0


def walk_camera(forward=False, offset=0.0):
    """rolled by 90 degrees: q_x = -d (+d: forward) + offset, q_y = y, q_z = x.  Without the offset the angle of a pixel is a
    function of its row alone, with the +-pi seam across the rows at v = cy; with it the angle also moves with the depth, so that a
    column can come back to a bin it left."""
    return np.array([[0, 0, 1.0 if forward else -1.0, offset], [0, 1, 0, 0], [1, 0, 0, 0]], F64)


def walk_depth(width, height, seed, u16, pad=0, cy=0.0, ramp=True):
    """Seeded depths in [1, 4] that differ in every pixel: a ramp down the rows (up them for an odd seed) plus noise of less than a
    third of the ramp's step, so that the rows of a bin are ordered by depth and the nearest and the farthest point of every bin lie
    in its first and its last row - a boundary row put into the neighbouring bin moves that bin's range or intensity, however many
    pixels the bin has.  Rows (never the seam's, v = cy, nor its neighbours), pixels and short vertical streaks of 0 (dropped);
    beyond 47 columns from the middle also pixels of OUT_DEPTH, which the height window drops."""
    rng = np.random.default_rng(seed)
    down = np.linspace(0.0, 1.0, height)[:, None]
    step = 2.9 / max(height - 1, 1)
    d = 1.05 + 2.9 * (1.0 - down if seed % 2 else down) + step * rng.uniform(-0.3, 0.3, (height, width))
    if not ramp:                                                         # unordered: with the offset camera the angle jumps with the depth
        d = rng.uniform(1.0, 4.0, (height, width))
    outer = np.abs(np.arange(width) - (width - 1) / 2.0) > 47.0
    d[rng.random((height, width)) < 0.06] = 0.0
    d[(rng.random((height, width)) < 0.06) & outer[None, :]] = OUT_DEPTH
    rows = rng.random(height) < 0.08
    rows[max(int(cy) - 1, 0):int(cy) + 2] = False
    d[rows] = 0.0
    for u in np.nonzero(rng.random(width) < 0.3)[0]:
        r = int(rng.integers(0, height))
        d[r:r + int(rng.integers(3, 7)), u] = OUT_DEPTH if outer[u] and rng.random() < 0.5 else 0.0
    full = np.full((height, width + pad), 1500 if u16 else 1.5, np.uint16 if u16 else F32)       # the padding is never read
    full[:, :width] = np.round(d * 1000.0).astype(np.uint16) if u16 else d.astype(F32)
    return full[:, :width]


def walk_image(width, height, seed, u16, cy, fy=FY, forward=False, offset=0.0, pad=0):
    return dict(depth=walk_depth(width, height, seed, u16, pad, cy, ramp=offset == 0.0), fx=FY, fy=fy, cx=(width - 1) / 2.0, cy=cy,
                camera_transform=walk_camera(forward, offset))


# Sizes whose lanes walk several rows of a column in a band of 8 (lanes_for gives 256 lanes side by side for 256 vectors and 127 for
# 127: side = 1 and 2), a last band of 4 and of 7 rows, a ragged last vector, and a padded step that is no multiple of 16 bytes.
# For each: the seam going down the rows, going up them (fy < 0) with the offset camera, and the forward camera.
WALKING = {(1024, 16): 12.0, (1021, 20): 18.0, (508, 23): 11.5}        # (width, height) -> cy
# The issue's sizes.  lanes_for makes side >= 8 for all of them, so in a band of 8 rows each lane sees one row: controls.
CONTROLS = {(640, 48): 20.0, (516, 48): 23.5, (132, 24): 12.0, (160, 24): 11.5, (8, 64): 30.0, (3, 64): 31.5}


@functools.lru_cache(maxsize=None)
def walk_scenes(u16):
    """-> {name: image}"""
    out = {}
    for i, ((w, h), cy) in enumerate(WALKING.items()):
        # rows of 1029 pixels: a step of 4116 / 2058 bytes, no multiple of a 16- / 8-byte load; rows of 1024 pixels around 1021
        pad = {(1024, 16): 5, (1021, 20): 3}.get((w, h), 0)
        out["%dx%d down" % (w, h)] = walk_image(w, h, 100 + i, u16, cy, pad=pad)
        out["%dx%d up, offset" % (w, h)] = walk_image(w, h, 110 + i, u16, cy, fy=-FY, offset=0.3)
        out["%dx%d forward" % (w, h)] = walk_image(w, h, 120 + i, u16, cy, forward=True, offset=0.3 if i == 1 else 0.0)
    for i, ((w, h), cy) in enumerate(CONTROLS.items()):
        kind = (i + int(u16)) % 3
        out["%dx%d control" % (w, h)] = walk_image(w, h, 130 + i, u16, cy, fy=-FY if kind == 1 else FY, forward=kind == 2,
                                                   offset=0.3 if i % 2 else 0.0, pad=11 if (w, h) == (160, 24) else 0)
    return out


@functools.lru_cache(maxsize=None)
def plane_scenes():
    """q_y = y + 0.05 d under a focal length of 1e6: the angle is atan(0.05) for every depth, all pixels of an image lie in one inner
    bin -> {name: image}"""
    out = {}
    for i, (w, h) in enumerate(((640, 48), (1024, 16))):
        im = walk_image(w, h, 140 + i, False, cy=(h - 1) / 2.0, forward=True)
        out["%dx%d plane" % (w, h)] = dict(im, fx=1e6, fy=1e6, camera_transform=np.array([[0, 0, 1, 0], [0, 1, 0.05, 0], [1, 0, 0, 0]], F64))
    return out


def pixel_bins(im, n=720, **cfg):
    """the bin of every pixel by the reference's steps 2-6 -> int (height, width), -1 = dropped"""
    cfg = dict(LR.DEFAULTS, **cfg)
    _, _, c, s = table(n)
    d, used = LR.depth_values(im["depth"], cfg["depth_scale"])
    v, u = np.nonzero(used)
    qx, qy, qz = LR.base_points(d[used], u, v, im["fx"], im["fy"], im["cx"], im["cy"], im["camera_transform"])
    ok = LR.height_ok(qz, cfg["min_height"], cfg["max_height"])
    out = np.full(d.shape, -1, np.int64)
    out[v[ok], u[ok]] = LR.bins(qx[ok], qy[ok], c, s)
    return out


TRANSITIONS = ("same inner bin", "neighbouring bin", "jump of 2 or more", "inner to bin 0", "inner to bin n-1", "seam n-1 to 0",
               "seam 0 to n-1", "dropped between two of one bin", "return to a bin left earlier")


def count_transitions(binmap, visits, n, rows_per_band=8):
    """over the consecutive kept pixels of each Column of `visits` -> Counter of TRANSITIONS, of "whole band in one inner bin" and
    "band ends inside a run", and "longest walk" (rows one Column visits)"""
    cnt = collections.Counter()
    for _, _, u, rows in visits:
        cnt["longest walk"] = max(cnt["longest walk"], len(rows))
        seq = binmap[rows, u].tolist()
        prev, gap, left = -1, False, set()
        for b in seq:
            if b < 0:
                gap = True
                continue
            if prev >= 0:
                inner = 0 < prev < n - 1
                if b == prev:
                    cnt["same inner bin"] += inner
                    cnt["dropped between two of one bin"] += gap
                else:
                    seam = {b, prev} == {0, n - 1}
                    cnt["neighbouring bin"] += abs(b - prev) == 1
                    cnt["jump of 2 or more"] += abs(b - prev) >= 2 and not seam
                    cnt["inner to bin 0"] += inner and b == 0
                    cnt["inner to bin n-1"] += inner and b == n - 1
                    cnt["seam n-1 to 0"] += prev == n - 1 and b == 0
                    cnt["seam 0 to n-1"] += prev == 0 and b == n - 1
                    left.add(prev)
                    cnt["return to a bin left earlier"] += b in left
            prev, gap = b, False
        if len(seq) == rows_per_band and len(set(seq)) == 1 and 0 < seq[0] < n - 1:
            cnt["whole band in one inner bin"] += 1
        if len(seq) >= 2 and seq[-1] == seq[-2] and 0 < seq[-1] < n - 1:
            cnt["band ends inside a run"] += 1
    return cnt


BAND9 = (132, 420, 40)                    # 40 copies of a 132 x 420 u16 image: 16,800 rows in one chunk, band_rows = 9


@functools.lru_cache(maxsize=None)
def band9_image():
    w, h, _ = BAND9
    return walk_image(w, h, 150, True, cy=200.0, offset=0.3)


@functools.lru_cache(maxsize=None)
def expected(kind, name=None, u16=False):
    """LR.extract of one walk / plane / band-9 image under WINDOW, computed once"""
    im = {"walk": lambda: walk_scenes(u16)[name], "plane": lambda: plane_scenes()[name], "band9": band9_image}[kind]()
    return LR.extract([im], **WINDOW)


# --------------------------------------------------------------------------------------------- 3. merge and centre truth table
def pair_image(near, far, group):
    """A 1 x 2 f32 image of depths (near, far) whose points are (near, +0) and (far, +0): q_x = d, q_y = 0.  sqrtf(fl(d d)) = d, so
    the image's range in the bin of the +x axis is `near` and its intensity `far`, bit for bit (3e38 as far: the intensity is inf).
    near = far = 0: an empty scan."""
    T = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 0, 0.5]], F64)
    return dict(depth=np.array([[near, far]], F32), fx=1.0, fy=1.0, cx=0.0, cy=0.0, camera_transform=T, group=group)


def up(x):
    return np.nextafter(F32(x), F32(np.inf))


def down(x):
    return np.nextafter(F32(x), F32(-np.inf))


MERGE_CFG = dict(range_min=0.45, range_max=5.0)
CLOSE_CFG = dict(range_min=0.01, range_max=5.0)
# fabsf(a - r) on 0.1f and on its two neighbours: below 0.125 both a and a - 0.1f are multiples of the ulp of 0.1f, so
# r = a - 0.1f is exact, and one ulp of a moves the difference by exactly one ulp of 0.1f
CLOSE_A = (down(0.12), F32(0.12), up(0.12))
CLOSE_R = F32(0.12) - F32(0.1)


def merge_groups():
    """-> [(cfg, [cameras (near, far) in order])]: one group each"""
    lo, hi0 = F32(0.45), F32(5.0)
    big = F32(3e38)
    a_states = {"empty": [(0, 0)], "zero range, intensity kept": [(2.0, 2.0), (3.0, 3.0)], "both zero": [(3.0, 3.0), (2.0, 2.0)],
                "above hi0": [(5.5, 5.5)], "inf intensity": [(2.0, big)], "in range": [(2.0, 2.0)], "near and far": [(1.0, 3.0)]}
    r_states = {"below lo": (down(lo), down(lo)), "lo": (lo, lo), "hi0": (hi0, hi0), "above hi0": (up(hi0), up(hi0)), "empty": (0, 0),
                "inf intensity": (2.05, big), "close": (2.05, 2.05), "far above": (3.0, 3.0), "far below": (1.0, 1.0),
                "near below lo, far in range": (0.3, 2.05), "near close, far above hi0": (1.95, 5.5)}
    groups = [(MERGE_CFG, a + [r]) for a in a_states.values() for r in r_states.values()]
    for a in CLOSE_A:                                                    # both orders of the two cameras
        groups += [(CLOSE_CFG, [(a, a), (CLOSE_R, CLOSE_R)]), (CLOSE_CFG, [(CLOSE_R, CLOSE_R), (a, a)])]
    groups += [(MERGE_CFG, [(2.0, 2.0), (F32(2.0) + F32(0.1), F32(2.0) + F32(0.1))]), (MERGE_CFG, [(2.0, 2.0), (down(1.9), up(2.1))])]
    groups += [(MERGE_CFG, [(2.0, 2.0), (2.05, 2.05), (3.0, 3.0)]), (MERGE_CFG, [(2.0, 2.0), (3.0, 3.0), (2.5, 2.5)]),
               (MERGE_CFG, [(3.0, 3.0), (2.0, 2.0), (2.5, 2.5), (2.52, 2.52)])]
    groups += [(MERGE_CFG, list(p)) for p in itertools.permutations([(2.0, 2.0), (2.05, 2.05), (3.0, 3.0)])]
    # the ends check_cfg admits: range_min = 0 (nothing is below lo, a 0.0 is retaken), range_max = range_min (only r = lo merges)
    for cfg in (dict(range_min=0.0, range_max=5.0), dict(range_min=2.0, range_max=2.0)):
        groups += [(cfg, [a, r]) for a in ((0, 0), (2.0, 2.0), (1.0, 3.0)) for r in ((2.0, 2.0), (0.05, 0.05), (2.05, 2.05), (1e-30, 3.0), (0, 0))]
    return groups


def merge_images(cfg):
    """the groups of one cfg as the images of one call -> (images, the cameras of each group)"""
    mine = [cams for c, cams in merge_groups() if c == cfg]
    return [pair_image(near, far, g) for g, cams in enumerate(mine) for near, far in cams], mine


def merge_cfgs():
    seen = []
    for cfg, _ in merge_groups():
        if cfg not in seen:
            seen.append(cfg)
    return seen


def merge_branch(a, r, lo, hi0, intensity):
    """the branch of step 8 that (a, r) takes"""
    a, r, lo, hi0 = F32(a), F32(r), F32(lo), F32(hi0)
    if np.isnan(r):
        return "skip: r NaN"
    if r < lo:
        return "skip: r < lo"
    if not intensity and r > hi0:
        return "skip: r > hi0"
    if np.isnan(a):
        return "take: a NaN"
    if a == 0:
        return "take: a == 0"
    if a > hi0:
        return "take: a > hi0"
    with np.errstate(invalid="ignore"):
        if np.abs(a - r) < F32(0.1):
            return "mean"
    if not intensity:
        return "zero"
    return "zero: a > r" if a > r else "keep: a <= r"


# every branch finite inputs can reach (a range or an intensity is never NaN)
RANGE_BRANCHES = ("skip: r < lo", "skip: r > hi0", "take: a == 0", "take: a > hi0", "mean", "zero")
INTENSITY_BRANCHES = ("skip: r < lo", "take: a == 0", "take: a > hi0", "mean", "zero: a > r", "keep: a <= r")


def bin_centre_point(n, k, r):
    """the f32 point at radius r a quarter of the way into bin k (where n inc > 2 pi the upper half of bin n - 1 is bin 0's)"""
    amin, inc, _, _ = table(n)
    th = float(amin) + (k + 0.25) * float(inc)
    return F32(r * math.cos(th)), F32(r * math.sin(th))


def grouped(lists):
    """lists of images -> one list, list g as group g"""
    return [dict(im, group=g) for g, ims in enumerate(lists) for im in ims]


CENTRE_CFG = dict(range_min=0.45, range_max=5.0)


def centre_groups(n=720):
    """-> {name: images of one group}: ranges equal to lo, just above it, equal to hi0, just above it (on the four half-axes, where
    the range is the coordinate bit for bit), a 0.0 from a merge and ordinary beams; exactly one counted beam; none"""
    lo, hi0 = F32(0.45), F32(5.0)
    edge = [point_image(lo, 0.0), point_image(0.0, up(lo)), point_image(-hi0, 0.0), point_image(0.0, -up(hi0))]
    zero = [point_image(*bin_centre_point(n, 100, 2.0)), point_image(*bin_centre_point(n, 100, 3.0))]
    plain = [point_image(*bin_centre_point(n, k, 1.0 + 0.004 * k)) for k in (7, 250, 400, 650)]
    # the range above hi0 comes first: as r of a merge it would be skipped
    return {"edges": edge[::-1] + zero + plain, "one beam": [edge[3], edge[0], zero[0], zero[1], plain[1]], "no beam": [edge[3], edge[0]] + zero,
            "empty": [point_image(0.0, 0.0)]}


@functools.lru_cache(maxsize=None)
def every_beam(n=4096):
    """4096 images of one pixel and one group, one in the middle of each bin at a seeded radius in [1, 4]
    -> (images, LR.extract of them)"""
    rng = np.random.default_rng(n)
    order = rng.permutation(n)
    images = [point_image(*bin_centre_point(n, int(k), float(rng.uniform(1.0, 4.0))), group=0) for k in order]
    return images, LR.extract(images, angle_increment=GRIDS[n])
