"""CPU tests (no GPU needed) of the laser-line contract's NumPy restatement tests/laserline_reference.py: hand-checked cases per step,
the order-independence step 7 claims for the reference's sequential update, and the restated bin rule against the reference's own
atan2f formula (at most 1 point in 5,000 differs, never by more than one bin)."""
import math

import numpy as np
import pytest

import laserline_reference as LR
import laserline_scenes as LS

F32 = np.float32
I34 = np.eye(3, 4)
INCREMENTS = [math.pi / 360, 0.005, math.pi / 720]


def grid(inc=math.pi / 360):
    amin, amax, inc, n = LR.angular_grid(inc)
    return amin, inc, n, LR.trig_table(amin, inc, n)


def test_angular_grid():
    amin, amax, inc, n = LR.angular_grid(math.pi / 360)
    assert (amin, amax, n) == (F32(-math.pi), F32(math.pi), 720) and inc == F32(math.pi / 360)
    assert LR.angular_grid(0.005)[3] == 1257 and LR.angular_grid(math.pi / 720)[3] == 1440
    c, s = LR.trig_table(amin, inc, n)
    assert len(c) == len(s) == n + 1
    assert c[360] == math.cos(float(amin) + 360.0 * float(inc)) and s[7] == math.sin(float(amin) + 7.0 * float(inc))


def test_depth_of_a_pixel():
    d, used = LR.depth_values(np.array([[0.0, -1.0, np.nan, np.inf, 2.5, 1e-30]], F32))
    assert used.tolist() == [[False, False, False, False, True, True]]
    d, used = LR.depth_values(np.array([[0, 1, 1234, 65535]], np.uint16))
    assert used.tolist() == [[False, True, True, True]]
    assert d[0, 2] == F32(1234 * 0.001) and d[0, 3] == F32(65535 * 0.001) and d.dtype == F32
    d, _ = LR.depth_values(np.array([[3.0]], F32), depth_scale=0.5)
    assert d[0, 0] == F32(1.5)
    d, _ = LR.depth_values(np.array([[1001]], np.uint16), depth_scale=0.3)
    assert d[0, 0] == F32(float(F32(1001 * 0.001)) * 0.3)


def test_camera_and_base_point():
    # on the optical axis: x = y = 0, z = d; the transform's translation carries through
    T = np.array([[0, 0, 1, 0.1], [-1, 0, 0, 0.2], [0, -1, 0, 0.6]], float)
    qx, qy, qz = LR.base_points(np.array([2.0], F32), [319.5], [239.5], 525.0, 525.0, 319.5, 239.5, T)
    assert (qx[0], qy[0], qz[0]) == (F32(2.0) + F32(0.1), F32(0.2), F32(0.6))
    # off axis, by hand: x = (float)(((u - cx) d) / fx), the sums in f32 in the written order
    d, u, v = F32(1.7), 100.0, 400.0
    x, y = F32(((u - 319.5) * float(d)) / 525.0), F32(((v - 239.5) * float(d)) / 520.0)
    Tf = T.astype(F32)
    qx, qy, qz = LR.base_points(np.array([d]), [u], [v], 525.0, 520.0, 319.5, 239.5, T)
    assert qx[0] == F32(F32(F32(Tf[0, 0] * x) + F32(Tf[0, 1] * y)) + F32(Tf[0, 2] * d)) + Tf[0, 3]
    assert qz[0] == F32(F32(F32(Tf[2, 0] * x) + F32(Tf[2, 1] * y)) + F32(Tf[2, 2] * d)) + Tf[2, 3]
    assert qy[0] == F32(F32(F32(Tf[1, 0] * x) + F32(Tf[1, 1] * y)) + F32(Tf[1, 2] * d)) + Tf[1, 3]


def test_height_limits_are_inclusive():
    z = np.array([0.0, -0.0, np.nextafter(F32(0), F32(-1)), 1.0, np.nextafter(F32(1), F32(2)), np.nan, 0.5], F32)
    assert LR.height_ok(z, 0.0, 1.0).tolist() == [True, True, False, True, False, False, True]
    assert LR.height_ok(np.array([0.3], F32), 0.3, 0.3).tolist() == [False]       # (double)0.3f > 0.3


def test_bins_by_hand():
    amin, inc, n, (c, s) = grid()
    # well inside bins
    for k in (0, 1, 100, 359, 360, 361, 718, 719):
        th = float(amin) + (k + 0.5) * float(inc)
        assert LR.bins([F32(2 * math.cos(th))], [F32(2 * math.sin(th))], c, s)[0] == k
    # the axes: +x is the lower edge of bin 360 up to the rounding of amin, +y and -y a quarter turn away
    assert LR.bins([1.0, 0.0, 0.0], [0.0, 1.0, -1.0], c, s).tolist() == [360, 540, 180]
    # the negative x axis goes to bin n - 1 for y = +0 and for y = -0; just below it is bin 0, just above it bin n - 1
    assert LR.bins([-1.0, -1.0, -1.0, -1.0], [0.0, -0.0, -1e-6, 1e-6], c, s).tolist() == [n - 1, n - 1, 0, n - 1]
    # the origin and non-finite coordinates are dropped
    assert LR.bins([0.0, -0.0, np.nan, 1.0], [0.0, 0.0, 1.0, np.nan], c, s).tolist() == [-1, -1, -1, -1]


def test_a_point_exactly_on_a_boundary_direction():
    """a point whose direction is boundary k bit for bit is at-or-past k (>=) and not past k + 1: bin k"""
    amin, inc, n, (c, s) = grid()
    # directions that are exact in f32: k = 360 + 180 is +y up to the table's rounding; build exact ones from the table itself
    for k in (3, 200, 360, 500, 719):
        # a point on boundary k in f64 would need f64 coordinates; in f32 take the nearest point and check it against the rule
        X, Y = float(F32(c[k] * 3)), float(F32(s[k] * 3))
        at_or_past = c[k] * Y >= s[k] * X
        b = LR.bins([F32(X)], [F32(Y)], c, s)[0]
        assert b == (k if at_or_past else k - 1)
    # an exact tie: c_k Y == s_k X holds for (X, Y) = (c_k, s_k) scaled by a power of two whenever both are f32 values
    ks = [k for k in range(n) if F32(c[k]) == c[k] and F32(s[k]) == s[k]]
    for k in ks:
        assert LR.bins([F32(c[k] * 2)], [F32(s[k] * 2)], c, s)[0] == k


def test_overlap_of_the_last_bin_goes_to_bin_zero():
    """n inc > 2 pi (0.005: n = 1257): boundary n lies past the seam, a point between boundary 0 and boundary n is the reference's
    bin 0"""
    amin, inc, n, (c, s) = grid(0.005)
    th = -math.pi + 0.0009
    assert float(amin) + n * float(inc) - math.pi > 0.0018
    q = ([F32(2 * math.cos(th))], [F32(2 * math.sin(th))])
    assert LR.bins(*q, c, s)[0] == 0 == LR.atan2f_bins(*q, amin, inc)[0]
    th = math.pi - 0.001
    q = ([F32(2 * math.cos(th))], [F32(2 * math.sin(th))])
    assert LR.bins(*q, c, s)[0] == n - 1 == LR.atan2f_bins(*q, amin, inc)[0]


def test_nearest_farthest_and_empty_bins():
    b = np.array([5, 5, 5, 9, -1])
    qx = np.array([3.0, 1.0, 2.0, 7.0, 0.1], F32)
    qy = np.array([0.0, 1.0, 0.0, 0.0, 0.1], F32)
    r, i = LR.nearest_farthest(b, qx, qy, 16, 5.0)
    assert r[5] == np.sqrt(F32(2)) and i[5] == F32(3) and r.dtype == i.dtype == F32
    assert r[9] == F32(6) and i[9] == F32(7)                 # 49 >= hi hi = 36: the range keeps hi, the intensity is the far point
    assert r[0] == F32(6) and i[0] == F32(0)                 # an empty bin


@pytest.mark.parametrize("seed", range(4))
def test_sequential_update_equals_min_and_max(seed):
    """step 7's claim: the reference's sequential update (compare against the square of an already rounded square root) gives
    sqrtf(min s) and sqrtf(max s) for every order - random values, and values clustered within 5 ulps of each other"""
    rng = np.random.default_rng(seed)
    hi = F32(5.0) + F32(1.0)
    for trial in range(500):
        if trial % 2:
            s = rng.uniform(0.01, 50.0, 200).astype(F32)
        else:
            base = F32(rng.uniform(0.05, 40.0))
            s = (base.view(np.uint32) + rng.integers(-5, 6, 200).astype(np.int64)).astype(np.uint32).view(F32)
        rng.shuffle(s)
        r, i = LR.sequential_nearest_farthest(s, 5.0)
        mn, mx = s.min(), s.max()
        assert r == (np.sqrt(mn) if mn < hi * hi else hi)
        assert i == np.sqrt(mx)


def test_merge_branches():
    lo, hi0 = 0.45, 5.0
    nan = np.nan
    #                skip: NaN, < lo, > hi0 | a NaN, a == 0, a > hi0 -> r | close -> mean | far apart -> 0
    a = np.array([1.0, 1.0, 1.0, nan, 0.0, 6.0, 2.0, 2.0, 2.0], F32)
    r = np.array([nan, 0.4, 5.5, 2.0, 2.0, 2.0, 2.05, 2.2, 0.45], F32)
    want = [1.0, 1.0, 1.0, 2.0, 2.0, 2.0, float(F32(0.5) * (F32(2.0) + F32(2.05))), 0.0, 0.0]
    got, _ = LR.merge((a, a), (r, np.full(9, nan, F32)), lo, hi0)
    assert got.tolist() == [float(F32(w)) for w in want]
    # intensities: no upper test on r; far apart: 0 only when a > r, else unchanged
    a = np.array([1.0, 1.0, 1.0, nan, 0.0, 6.0, 2.0, 2.0, 2.0, 2.0], F32)
    r = np.array([nan, 0.4, 5.5, 2.0, 2.0, 2.0, 2.05, 2.2, 1.0, 7.0], F32)
    want = [1.0, 1.0, 1.0, 2.0, 2.0, 2.0, float(F32(0.5) * (F32(2.0) + F32(2.05))), 2.0, 0.0, 2.0]
    want[2] = 1.0                                            # |1 - 5.5| >= 0.1 and a < r: unchanged
    _, got = LR.merge((a, a), (np.full(10, nan, F32), r), lo, hi0)
    assert got.tolist() == [float(F32(w)) for w in want]
    # the boundary of "close": |a - r| < 0.1f in f32
    a, r = np.array([1.0], F32), np.array([F32(1.0) + F32(0.1)], F32)
    got, _ = LR.merge((a, a), (r, r), lo, hi0)
    assert got[0] == (F32(0.5) * (a[0] + r[0]) if abs(a[0] - r[0]) < F32(0.1) else 0)


def test_scan_center_uses_strict_lower_and_inclusive_upper_bound():
    amin, inc, n, (c, s) = grid()
    lo, hi0 = 0.45, 5.0
    r = np.full(n, 6.0, F32)
    assert LR.scan_center(r, c, s, lo, hi0).tolist() == [0.0, 0.0, 0.0]
    r[10], r[20], r[30], r[40] = F32(lo), F32(hi0), np.nan, 2.0     # r = lo does not count (the merge's r >= lo would take it), r = hi0 does
    got = LR.scan_center(r, c, s, lo, hi0)
    sx = c[20] * float(F32(hi0)) + c[40] * 2.0
    sy = s[20] * float(F32(hi0)) + s[40] * 2.0
    assert got.tolist() == [float(F32(sx / 2.0)), float(F32(sy / 2.0)), 0.0]
    a = np.array([0.0], F32)
    assert LR.merge((a, a), (np.array([lo], F32),) * 2, lo, hi0)[0][0] == F32(lo)


def test_extract_merges_groups_in_order_and_handles_empty_images():
    ims = [LS.image(LS.room(32, 24, seed=i), LS.camera_transform(yaw=30.0 * i), group=g) for i, g in enumerate([0, 0, 1, 2, 2, 2])]
    ims.append(dict(LS.image(np.zeros((0, 0), F32)), group=3))
    r, i, ce = LR.extract(ims)
    assert r.shape == i.shape == (4, 720) and ce.shape == (4, 3)
    assert (r[3] == F32(6)).all() and (i[3] == 0).all() and ce[3].tolist() == [0, 0, 0]
    cfg = dict(LR.DEFAULTS)
    two = LR.merge(LR.image_scan(ims[0], cfg), LR.image_scan(ims[1], cfg), cfg["range_min"], cfg["range_max"])
    assert np.array_equal(r[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(i[0].view(np.uint32), two[1].view(np.uint32))
    one = LR.image_scan(ims[2], cfg)
    assert np.array_equal(r[1].view(np.uint32), one[0].view(np.uint32))
    assert (r[1] < 6).sum() > 20                             # the scene reaches the scan


@pytest.mark.parametrize("inc", INCREMENTS)
def test_bin_rule_against_the_reference_formula(inc):
    """the restated bin and the reference's (int)((-atan2f(-y, x) - amin) / inc) differ for at most 1 point in 5,000 and never by more
    than one bin: on the room scene (640 x 480, depth 1.5-4 m, 10 % holes, camera 0.6 m up, yawed 40 degrees) and over the circle"""
    amin, inc32, n, (c, s) = grid(inc)
    d, used = LR.depth_values(LS.room(seed=1))
    v, u = np.nonzero(used)
    im = LS.image(d)
    qx, qy, qz = LR.base_points(d[used], u, v, im["fx"], im["fy"], im["cx"], im["cy"], im["camera_transform"])
    ok = LR.height_ok(qz, 0.0, 1.0)
    scenes = {"room": (qx[ok], qy[ok]), "circle": LS.circle_points(400000, seed=2)}
    for name, (qx, qy) in scenes.items():
        assert len(qx) > 100000
        mine, ref = LR.bins(qx, qy, c, s), LR.atan2f_bins(qx, qy, amin, inc32)
        diff = np.abs(mine - ref)
        print("%s, increment %.6f: %d points, %d dropped, %d differ (%.2e), largest difference %d bins"
              % (name, inc, len(qx), (mine < 0).sum(), (diff != 0).sum(), (diff != 0).mean(), diff.max()))
        assert (mine >= 0).all()
        assert (diff != 0).sum() * 5000 <= len(qx)
        assert diff.max() <= 1
    assert len(np.unique(LR.bins(*scenes["circle"], c, s))) == n     # every bin is reachable
