"""CPU tests (no GPU): the NumPy restatement of the ORB contract (tests/orb_reference.py) against facts it does not itself encode -
the FAST score against the arc min / max formula, the resize against the identity and float bilinear interpolation, the blur weights
against the Gaussian they come from, the umax table and the per-level split against the reference's formulas, fastAtan2 and the
cos / sin recipe against libm, the tie rule of the cuts and the totality of the output order."""
import math

import numpy as np
import pytest

import orb_reference as R
import orb_scenes as S

F32 = np.float32


def arc_score(patch):
    """the score of the centre of a 7 x 7 patch from the minima / maxima of the 16 arcs of 9"""
    p = int(patch[3, 3])
    d = [int(patch[3 + dy, 3 + dx]) - p for dx, dy in R.CIRCLE]
    best = 0
    for k in range(16):
        arc = [d[(k + i) % 16] for i in range(9)]
        best = max(best, min(arc), -max(arc))
    return max(best - 1, 0)


def test_fast_score_by_definition_equals_the_arc_formula():
    rng = np.random.default_rng(1)
    seen = set()
    for k in range(400):
        patch = rng.integers(0, 256, (7, 7))
        if k % 4:                                   # an arc of random length brighter or darker than the centre by a random margin
            c, n, start = int(rng.integers(0, 256)), int(rng.integers(7, 17)), int(rng.integers(0, 16))
            patch[3, 3] = c
            side = 1 if rng.random() < 0.5 else -1
            for i in range(n):
                dx, dy = R.CIRCLE[(start + i) % 16]
                patch[3 + dy, 3 + dx] = np.clip(c + side * int(rng.integers(1, 256)), 0, 255)
        patch = patch.astype(np.uint8)
        got = int(R.fast_scores(patch)[3, 3])
        assert got == arc_score(patch), (k, patch.tolist())
        seen.add(got)
    assert len(seen) > 50 and 0 in seen             # the patches span many scores, none included


def test_fast_extremes():
    dot = np.zeros((7, 7), np.uint8); dot[3, 3] = 255
    assert R.fast_scores(dot)[3, 3] == 254 and R.fast_scores(255 - dot)[3, 3] == 254
    assert not R.fast_scores(np.full((9, 9), 77, np.uint8)).any()
    assert not R.fast_scores(np.zeros((6, 20), np.uint8)).any()


def test_resize_at_equal_size_is_the_identity():
    img = S.rectangles(37, 29, seed=2)
    assert np.array_equal(R.resize(img, 37, 29), img)


@pytest.mark.parametrize("dw,dh", [(67, 63), (63, 63), (31, 90), (136, 131)])
def test_resize_is_within_one_grey_level_of_float_bilinear(dw, dh):
    img = S.rectangles(80, 76, seed=3)
    sh, sw = img.shape

    def axis(dn, sn):
        f = (np.arange(dn) + 0.5) * (sn / dn) - 0.5
        s = np.floor(f)
        f = f - s
        f[s < 0] = 0; s[s < 0] = 0
        f[s >= sn - 1] = 0; s[s >= sn - 1] = sn - 1
        s = s.astype(int)
        return s, np.minimum(s + 1, sn - 1), f

    x0, x1, fx = axis(dw, sw)
    y0, y1, fy = axis(dh, sh)
    I = img.astype(np.float64)
    top = I[y0][:, x0] * (1 - fx) + I[y0][:, x1] * fx
    bot = I[y1][:, x0] * (1 - fx) + I[y1][:, x1] * fx
    want = top * (1 - fy)[:, None] + bot * fy[:, None]
    err = np.abs(R.resize(img, dw, dh).astype(np.float64) - want).max()
    print("largest difference from float bilinear: %.3f grey levels" % err)
    assert err <= 1.0


def test_blur_weights_and_their_sum():
    g = np.exp(-((np.arange(7) - 3.0) ** 2) / (2.0 * 2.0 * 2.0))
    k = (g / g.sum()).astype(F32)
    assert [int(v) for v in R.rnd(k * F32(256))] == R.BLUR_K == [18, 34, 49, 55, 49, 34, 18]
    assert sum(R.BLUR_K) == 257


def test_blur_of_a_constant_image():
    """Step 10 does not renormalise its weights (sum 257), so a constant c comes back as sat_u8((c * 257 * 257 + 32768) >> 16): c
    itself for c <= 31, where the excess c * 1025 / 65536 stays below one half, and for 255, where it saturates; c + 1 from 32 to
    95, and so on up to 254 -> 255.  Every constant is checked against that closed form, on an image larger than the kernel and on
    a single pixel (every tap reflected onto it)."""
    for c in range(256):
        want = min((c * 257 * 257 + 32768) >> 16, 255)
        assert np.array_equal(R.blur(np.full((9, 13), c, np.uint8)), np.full((9, 13), want, np.uint8)), c
        assert R.blur(np.full((1, 1), c, np.uint8))[0, 0] == want
        assert want == c or 32 <= c <= 254
    assert R.blur(np.full((5, 4), 255, np.uint8)).min() == 255 and R.blur(np.full((5, 4), 31, np.uint8)).max() == 31


def test_umax_table_and_the_level_split():
    half = 15                                       # aorb.cpp:639-654
    umax = [0] * (half + 1)
    vmax = int(math.floor(half * math.sqrt(2.0) / 2 + 1))
    vmin = int(math.ceil(half * math.sqrt(2.0) / 2))
    for v in range(vmax + 1):
        umax[v] = int(round(math.sqrt(half * half - v * v)))
    v0 = 0
    for v in range(half, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    assert umax == R.UMAX
    assert R.n_per_level(600, 1.2, 2) == [327, 273]
    assert R.n_per_level(600, 1.2, 1) == [600]
    assert sum(R.n_per_level(600, 1.2, 8)) == 600


def test_fast_atan2_is_within_its_documented_accuracy():
    worst = 0.0
    vals = list(range(-60, 61, 3)) + [-100000, -2551, 2551, 100000, 1, -1]
    for m01 in vals:
        for m10 in vals:
            got = float(R.fast_atan2(F32(m01), F32(m10)))
            want = math.degrees(math.atan2(m01, m10)) % 360.0
            err = abs(got - want)
            worst = max(worst, min(err, 360.0 - err))
    print("largest fastAtan2 error: %.4f degrees" % worst)
    assert worst <= 0.3
    assert float(R.fast_atan2(F32(0), F32(0))) == 0.0


def test_cos_sin_recipe_is_within_1e_14_of_libm():
    worst = 0.0
    rng = np.random.default_rng(4)
    angles = [0.0, 90.0, 359.9, -17.5, 720.25, 45.0, 135.0, 180.0, 270.0, -360.0] + list(rng.uniform(-4000.0, 4000.0, 3000))
    for deg in angles:
        x = float(F32(deg) * F32(math.pi / 180.0))
        c, s = R.cos_sin(x)
        worst = max(worst, abs(c - math.cos(x)), abs(s - math.sin(x)))
    print("largest cos / sin error: %.3g" % worst)
    assert worst <= 1e-14


def test_a_level_keeps_all_ties_at_the_cut():
    r = np.array([9, 7, 7, 7, 7, 5, 3], F32)
    assert R.retain_best(r, 3).tolist() == [True, True, True, True, True, False, False]
    assert R.retain_best(r, 7).all() and R.retain_best(r, 8).all()
    assert R.retain_best(r, 1).tolist() == [True] + [False] * 6
    assert not R.retain_best(r, 0).any()


def test_the_output_order_is_total():
    o = R.extract(S.rectangles(320, 240, seed=5), S.pattern())
    n = len(o["u"])
    assert n > 100
    keys = list(zip(o["octave"].tolist(), (-o["response"]).tolist(), o["v"].tolist(), o["u"].tolist()))
    assert len(set(keys)) == n and keys == sorted(keys)
    assert set(o["octave"].tolist()) == {0, 1}
