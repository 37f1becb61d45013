"""CPU tests of tests/depthfilter_reference.py, the NumPy restatement the depth-filter kernels are held to: against an independent
scalar version (one pixel at a time, np.float32 scalars, OpenCV's own border loops), and the properties the contract in
include/uzl_mi355x.h states - a plane survives, every output is 0 or an original value of its disc, a non-finite pixel erases
exactly its 7 x 7 square, an edge the guide shares survives, a flat guide blurs yet the snap restores the input, the tables are exp
to an ulp, the lift equals a scalar loop."""
import math

import numpy as np
import pytest

import depthfilter_reference as DR
import depthfilter_scenes as DS
import laserline_scenes as LS

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def border_interpolate(p, n, reflect):
    """cv::borderInterpolate for BORDER_REPLICATE / BORDER_REFLECT_101, as OpenCV loops"""
    if 0 <= p < n:
        return p
    if not reflect:
        return 0 if p < 0 else n - 1
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else n - 1 - (p - n) - 1
    return p


def scalar_pass(src, guide, cw, sw, R, axis):
    h, w = src.shape
    out = np.zeros((h, w), F32)
    zero = F32(0.0)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                t, ws = F32(0.0), F32(0.0)
                g0 = int(guide[y, x])
                for k in range(-R, R + 1):
                    yy = border_interpolate(y + k, h, False) if axis == 0 else y
                    xx = border_interpolate(x + k, w, False) if axis == 1 else x
                    wk = F32(sw[k + R] * cw[abs(int(guide[yy, xx]) - g0)])
                    t = F32(t + F32(wk * src[yy, xx]))
                    ws = F32(ws + wk)
                wk = F32(zero * cw[0])
                t = F32(t + F32(wk * src[y, x]))
                ws = F32(ws + wk)
                out[y, x] = F32(t / ws)
    return out


def scalar_snap(filtered, before, P):
    h, w = before.shape
    out = np.zeros((h, w), F32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                minv, best = F32(DR.FLT_MAX), F32(0.0)
                for i in range(-P, P + 1):
                    for j in range(-P, P + 1):
                        if math.sqrt(float(i * i + j * j)) > P:
                            continue
                        b = before[border_interpolate(y + i, h, True), border_interpolate(x + j, w, True)]
                        a = F32(abs(F32(b - filtered[y, x])))
                        if a < minv:
                            minv, best = a, b
                out[y, x] = best
    return out


def scalar_refine(depth, guide, radius=3, nearest_radius=2, sigma_space=3.0, sigma_color=5.0, depth_scale=1.0):
    d = DR.depth_values(depth, depth_scale)
    cw, sw = DR.tables(radius, sigma_space, sigma_color)
    hor = scalar_pass(d, guide, cw, sw, radius, 1)
    ver = scalar_pass(hor, guide, cw, sw, radius, 0)
    return ver, scalar_snap(ver, d, nearest_radius)


@pytest.mark.parametrize("size", [(37, 53), (1, 1), (3, 5), (5, 3)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_the_restatement_equals_a_scalar_loop(size, u16):
    w, h = size
    im, g = DS.scene(w, h, seed=w + h, u16=u16, kind="blocks" if w > 5 else "noise")
    for cfg in (dict(), dict(radius=1, nearest_radius=1, sigma_color=30.0, depth_scale=0.5), dict(radius=0, nearest_radius=0)):
        st = DR.stages(im["depth"], g, **cfg)
        ver, snapped = scalar_refine(im["depth"], g, **cfg)
        assert np.array_equal(st["vertical"], ver, equal_nan=True)
        assert np.array_equal(bits(st["snapped"]), bits(snapped))
        assert np.array_equal(bits(DR.refine(im["depth"], g, **cfg)), bits(snapped))
        assert not np.isnan(snapped).any()


def test_reflect101_equals_the_border_loop():
    for n in (1, 2, 3, 4, 7):
        p = np.arange(-9, n + 9)
        assert DR.reflect101(p, n).tolist() == [border_interpolate(int(q), n, True) for q in p]


def test_the_disc_of_the_default_radius_has_13_taps():
    assert len(DR.disc(2)) == 13 and DR.disc(0) == [(0, 0)] and len(DR.disc(1)) == 5 and len(DR.disc(7)) == 149
    assert DR.disc(2)[:4] == [(-2, 0), (-1, -1), (-1, 0), (-1, 1)]


def test_a_plane_under_a_random_guide_comes_back_with_identical_bits():
    for value in (2.345, 0.001, 9.75):
        d = np.full((40, 56), value, F32)
        out = DR.refine(d, DS.guide(56, 40, seed=1, kind="noise"))
        assert np.array_equal(bits(out), bits(d))


def test_every_output_is_zero_or_an_original_value_of_its_disc():
    im, g = DS.scene(61, 47, seed=4)
    d = DR.depth_values(im["depth"])
    out = DR.refine(im["depth"], g)
    h, w = d.shape
    member = out.view(np.uint32) == 0
    for i, j in DR.disc(2):
        b = d[DR.reflect101(np.arange(h) + i, h)[:, None], DR.reflect101(np.arange(w) + j, w)[None, :]]
        member |= bits(out) == bits(b)
    assert member.all()
    assert (out != 0).sum() > 0.5 * out.size


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_pixel_erases_exactly_its_7x7_square(bad):
    rng = np.random.default_rng(3)
    d = rng.uniform(1.0, 4.0, (40, 48)).astype(F32)
    spots = [(12, 15), (30, 40), (2, 1)]                                    # the last one: its square is cut by the border
    for y, x in spots:
        d[y, x] = bad
    out = DR.refine(d, DS.guide(48, 40, seed=2))
    want = np.zeros(d.shape, bool)
    for y, x in spots:
        want[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = True
    assert np.array_equal(out == 0, want)
    assert np.isfinite(out).all()


def step_scene():
    d = np.full((32, 48), 1.0, F32); d[:, 24:] = 3.0
    g = np.full((32, 48), 40, np.uint8); g[:, 24:] = 200
    return d, g


def test_a_depth_step_on_a_guide_step_comes_back_unchanged():
    d, g = step_scene()
    st = DR.stages(d, g)
    assert np.array_equal(bits(st["snapped"]), bits(d))
    assert np.abs(st["vertical"] - d).max() < 1e-6                          # cw[160] is 0 in f32: nothing crosses the edge


def test_a_flat_guide_blurs_and_the_snap_restores_the_input():
    d, _ = step_scene()
    st = DR.stages(d, DS.guide(48, 32, kind="flat"))
    assert np.abs(st["vertical"] - d).max() > 0.5
    assert np.array_equal(bits(st["snapped"]), bits(d))


def test_the_tables_are_exp_to_one_ulp():
    for R, ss, sc in ((3, 3.0, 5.0), (15, 7.5, 30.0), (0, 1.0, 1.0), (2, 0.0, -1.0)):
        cw, sw = DR.tables(R, ss, sc)
        assert cw.dtype == F32 and sw.dtype == F32 and len(cw) == 256 and len(sw) == 2 * R + 1
        ss, sc = (ss if ss > 0 else 1.0), (sc if sc > 0 else 1.0)             # sigma <= 0 becomes 1
        i = np.arange(256, dtype=np.float64)
        k = np.abs(np.arange(-R, R + 1, dtype=np.float64))
        for got, want in ((cw, np.exp(i * i * (-0.5 / (sc * sc)))), (sw, np.exp(k * k * (-0.5 / (ss * ss))))):
            want32 = want.astype(F32)
            assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.maximum(want32, np.finfo(F32).tiny)).astype(np.float64))
        assert cw[0] == 1 and sw[R] == 1 and np.array_equal(sw, sw[::-1])
    cw, _ = DR.tables(3, 3.0, 5.0)
    assert cw[160] == 0 and cw[255] == 0 and cw[10] > 0


def test_the_lift_equals_a_scalar_loop():
    im, g = DS.scene(33, 21, seed=9)
    image = DR.refine(im["depth"], g)
    image[5, 7] = np.nan; image[6, 8] = 0.0; image[7, 9] = np.inf
    rng = np.random.default_rng(9)
    u = np.concatenate([rng.integers(-5, 40, 200), [7, 8, 9]]).astype(np.int32)
    v = np.concatenate([rng.integers(-5, 30, 200), [5, 6, 7]]).astype(np.int32)
    fx, fy, cx, cy = im["fx"], 1.1 * im["fy"], im["cx"], im["cy"] + 0.25
    for max_depth in (0.0, 2.5, 100.0):
        pos, valid = DR.lift(image, u, v, fx, fy, cx, cy, max_depth)
        assert pos.shape == (3, 203) and pos.dtype == np.float64 and valid.dtype == np.uint8
        for k in range(len(u)):
            uu, vv = min(max(int(u[k]), 0), 32), min(max(int(v[k]), 0), 20)
            d = float(image[vv, uu])
            if d != 0 and not math.isnan(d) and (max_depth == 0.0 or d <= max_depth):
                want = ((uu - cx) * d / fx, (vv - cy) * d / fy, d)
                assert valid[k] == 1
            else:
                want = (0.0, 0.0, -1.0)
                assert valid[k] == 0
            assert pos[:, k].tolist() == list(want)
        assert valid[-3] == 0 and valid[-2] == 0 and valid[-1] == (1 if max_depth == 0.0 else 0)
    assert 0 < DR.lift(image, u, v, fx, fy, cx, cy, 2.5)[1].sum() < DR.lift(image, u, v, fx, fy, cx, cy, 0.0)[1].sum()
    pos, valid = DR.lift(image, [], [], fx, fy, cx, cy)
    assert pos.shape == (3, 0) and valid.shape == (0,)
