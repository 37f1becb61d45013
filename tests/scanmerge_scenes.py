"""Scenes for the scan-merge tests: (keep scan, drop scan, keep_displacement, drop_displacement) tuples, built once.  Seeded; nothing
here depends on the code under test.  tests/test_scanmerge_reference.py checks on the CPU that each scene reaches the case it is
named for; tests/test_scanmerge_gpu.py holds the device to the restatement on them."""
import functools
import math

import numpy as np

import laserline_reference as LR
import scanmerge_reference as R

F32, F64 = np.float32, np.float64
EYE = np.eye(3, 4)
LO, HI = 0.45, 5.0


@functools.lru_cache(maxsize=None)
def inc_for(n):
    """an angle_increment whose laser-line grid (step 1) has exactly n beams"""
    for up in range(0, 64):
        inc = float(np.nextafter(F32(2.0 * math.pi / n), F32(10.0)) if up == 0 else F32(2.0 * math.pi / n) * F32(1.0 + up * 1e-6))
        if LR.angular_grid(inc)[3] == n:
            return inc
    raise AssertionError(n)


def planar(tx, ty, th):
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, -s, 0, tx], [s, c, 0, ty], [0, 0, 1, 0]], F64)


def line_scan(n, ranges, intensities=None, lo=LO, hi=HI, displacement=None, stamp_ns=0):
    """a scan on the laser-line grid of n beams"""
    amin, _, inc, m = LR.angular_grid(inc_for(n))
    assert m == n
    r = np.broadcast_to(np.asarray(ranges, F32), (n,)).copy()
    it = r + F32(0.5) if intensities is None else np.broadcast_to(np.asarray(intensities, F32), (n,)).copy()
    return R.scan(r, it, amin, inc, lo, hi, displacement, stamp_ns)


def room(rng, n, lo=LO, hi=HI, holes=0.1, **kw):
    """a seeded scan of a rough room: smooth walls 1 - 4 m away with noise, a share of beams without a return"""
    th = np.linspace(-math.pi, math.pi, n, endpoint=False)
    base = 2.5 + 1.2 * np.sin(2 * th + rng.uniform(0, 6)) + 0.3 * np.sin(7 * th + rng.uniform(0, 6))
    r = (base + rng.normal(0, 0.02, n)).astype(F32)
    r[rng.random(n) < holes] = F32(hi + 1.0)
    it = (r + rng.uniform(0.0, 0.6, n)).astype(F32)
    it[rng.random(n) < holes] = F32(0.0)
    return line_scan(n, r, it, lo, hi, **kw)


def generic(rng):
    """a displacement of the size a merge produces: translation up to 0.12 m, rotation up to 0.13 rad"""
    return planar(rng.uniform(-0.12, 0.12), rng.uniform(-0.12, 0.12), rng.uniform(-0.13, 0.13))


def sized(n_a, n_b, seed, b_stamp=1):
    rng = np.random.default_rng(seed)
    return (room(rng, n_a, stamp_ns=5, displacement=generic(rng)), room(rng, n_b, stamp_ns=5 + b_stamp, displacement=generic(rng)),
            generic(rng), generic(rng))


def finer_b(b_stamp):
    """64 bins, a third of them without a point of a; b with 4096 beams puts about 64 points into every bin"""
    rng = np.random.default_rng(11)
    a = room(rng, 64, holes=0.35, stamp_ns=10)
    b = room(rng, 4096, holes=0.05, stamp_ns=10 + b_stamp)
    return a, b, planar(0.01, -0.02, 0.4 * inc_for(64)), generic(rng)


def readings():
    """NaN, +-inf and readings exactly at, just below and just above each limit, in ranges and intensities of both scans"""
    lo, hi = F32(LO), F32(HI)
    special = np.array([np.nan, np.inf, -np.inf, lo, np.nextafter(lo, F32(0)), np.nextafter(lo, F32(9)), hi, np.nextafter(hi, F32(0)),
                        np.nextafter(hi, F32(9)), 0.0, -1.0, 2.0], F32)
    n = 64
    r = np.resize(special, n)
    a = line_scan(n, r, np.roll(r, 3), stamp_ns=1)
    b = line_scan(n, np.roll(r, 5), np.roll(r, 7), stamp_ns=2)
    half = planar(0, 0, 0.5 * inc_for(n))
    return a, b, half, half


def at_limits(which):
    """every reading of a at a.range_min (which = 0) or a.range_max (1): half a bin of rotation puts beam i in the middle of a bin
    with rho within an ulp of the limit - below it, on it and above it over the beams - and b's points 0.5 m away meet it there"""
    n = 720
    v = F32(LO) if which == 0 else F32(HI)
    half = planar(0, 0, 0.5 * inc_for(n))
    a = line_scan(n, v, v, stamp_ns=3)
    b = line_scan(n, 2.0, 2.0, stamp_ns=4 if which == 0 else 2)
    return a, b, half, half


def near_tenth():
    """b's points 0.1f away from a's, a few ulps to either side of it, nearer and farther"""
    n = 720
    half = planar(0, 0, 0.5 * inc_for(n))
    ra = np.full(n, 2.0, F32)
    k = np.arange(n)
    step = F32(2.0 ** -22)                                   # the spacing of f32 in [2, 4); in [1, 2) two of these steps differ
    rb = np.where(k % 2 == 0, ra + (F32(419430) + (k // 2 % 5 - 2).astype(F32)) * step, ra - (F32(419430) + (k // 2 % 5 - 2).astype(F32)) * step)
    a = line_scan(n, ra, ra + F32(1.0), stamp_ns=9)
    b = line_scan(n, rb.astype(F32), (rb + F32(1.0)).astype(F32), stamp_ns=8)
    return a, b, half, half


def seam(neg_zero):
    """b's beam 0 looks along +x (angle_min = 0: c = 1, s = 0 exactly) and a half turn puts its point on the negative x axis with
    q_y = +0, or -0 when every term of the row is -0; a reading of 0 with range_min = 0 is a point at the origin"""
    n = 64
    rng = np.random.default_rng(5)
    a = room(rng, n, stamp_ns=1)
    rb = np.full(16, 2.0, F32)
    rb[3] = F32(0.0)
    b = R.scan(rb, rb, 0.0, 0.05, 0.0, HI, None, 2)
    z = -0.0 if neg_zero else 0.0
    turn = np.array([[-1.0, z, z, z], [z, -1.0, z, z], [0, 0, 1, 0]], F64)
    return a, b, EYE.copy(), turn


def identity():
    rng = np.random.default_rng(21)
    return room(rng, 720, stamp_ns=1), room(rng, 720, stamp_ns=2), EYE.copy(), EYE.copy()


def crowded(b_stamp):
    """three or more points of b in every bin of a, ranges within and beyond 0.1 of each other: the fold's order matters"""
    rng = np.random.default_rng(31 + b_stamp)
    a = room(rng, 64, holes=0.2, stamp_ns=10)
    th = np.linspace(-math.pi, math.pi, 360, endpoint=False)
    r = (2.5 + 1.2 * np.sin(2 * th + 1.0) + rng.choice([0.0, 0.04, 0.09, 0.15, 0.3], 360)).astype(F32)
    b = line_scan(360, r, r + F32(0.07), stamp_ns=10 + b_stamp)
    return a, b, planar(0.02, 0.01, 0.3 * inc_for(64)), planar(-0.03, 0.02, 0.01)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (a, b, keep_displacement, drop_displacement)"""
    s = {}
    for n in (8, 63, 64, 65):
        s["n%d" % n] = sized(n, n, 100 + n)
    s["n720"] = sized(720, 720, 720)
    s["n4096"] = sized(4096, 4096, 4096)
    s["n720_b65"] = sized(720, 65, 1)
    s["n65_b720"] = sized(65, 720, 2, b_stamp=-1)
    s["finer_b_newer"] = finer_b(1)
    s["finer_b_older"] = finer_b(-1)
    s["readings"] = readings()
    s["cur_at_range_min"] = at_limits(0)
    s["cur_at_range_max"] = at_limits(1)
    s["near_tenth"] = near_tenth()
    s["seam_pos_zero"] = seam(False)
    s["seam_neg_zero"] = seam(True)
    s["identity"] = identity()
    for name, st in (("newer", 1), ("older", -1), ("same", 0)):
        s["crowded_" + name] = crowded(st)
    return s


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's result for a scene, computed once (read-only: the tests share it)"""
    trace = []
    out = R.merge(*scenes()[name], trace=trace)
    out["trace"] = trace
    for v in (out["ranges"], out["intensities"], out["center"], *out["bin"], *out["rho"]):
        v.setflags(write=False)
    return out
