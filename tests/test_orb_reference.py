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


# ------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/orb_cases.py: what each one exercises is a property of the restatement, shown here; the GPU tests
# (test_orb_configs_gpu.py, test_orb_stages_gpu.py) rely on it only because it is asserted here.
import orb_cases as K


def octaves(o, n_levels):
    return np.bincount(o["octave"], minlength=n_levels).tolist()


@pytest.mark.parametrize("inverse", [False, True])
def test_threshold_254_and_253_on_dots(inverse):
    """the largest admitted threshold keeps exactly the dots that score 254: score >= threshold, not >; one less doubles them"""
    pre = "inverse_dots" if inverse else "dots"
    img = K.CASES[pre + "_t254"]["img"]
    h, w = img.shape
    inner = S.dots(w, h)[19:h - 19, 19:w - 19]
    n255, n254 = int((inner == 255).sum()), int((inner == 254).sum())
    assert n255 >= 20 and n255 == n254
    top, _ = K.reference(pre + "_t254")
    assert len(top["u"]) == n255 and set(top["response"].tolist()) == {254.0}
    assert (S.dots(w, h)[top["v"].astype(int), top["u"].astype(int)] == 255).all()
    both, _ = K.reference(pre + "_t253")
    assert len(both["u"]) == n255 + n254 == 2 * len(top["u"]) and set(both["response"].tolist()) == {253.0, 254.0}


def test_thresholds_1_5_and_40():
    t1, t5, t40 = (K.reference("rect160_t%d" % t)[0] for t in (1, 5, 40))
    assert len(t1["u"]) > len(t5["u"]) > len(t40["u"]) > 0
    assert t1["response"].min() < 5 <= t5["response"].min() and t40["response"].min() >= 40


def test_scale_2_fills_three_octaves_and_exceeds_both_cuts():
    o, info = K.reference("scale2")
    assert all(n > 0 for n in octaves(o, 3))
    assert any(n > n_l for _, n, n_l in info["level_candidates"])
    assert len(info["cell_candidates"]) == 4 and all(n > share for n, share in info["cell_candidates"])
    assert R.level_size(200, 180, 2.0, 1) == (100, 90) and R.level_size(200, 180, 2.0, 2) == (50, 45)
    x0, x1, a0, a1 = R.resize_taps(100, 200)                              # exact half-pixel taps
    assert a0.tolist() == [1024] * 100 and a1.tolist() == [1024] * 100 and x0.tolist() == list(range(0, 200, 2))


def test_scale_1_05_fills_eight_octaves():
    o, _ = K.reference("scale105")
    assert all(n > 0 for n in octaves(o, 8))


def test_scale_1_5_loses_its_last_level_to_the_border():
    o, info = K.reference("scale15")
    oc = octaves(o, 4)
    assert all(n > 0 for n in oc[:3]) and oc[3] == 0
    for cell_w in (101, 102):
        w3, h3 = R.level_size(cell_w, 187, 1.5, 3)
        assert w3 <= 38 < h3                                             # too narrow for an edge of 19, though not too low
        assert min(R.level_size(cell_w, 187, 1.5, 2)) > 38
    assert all(n == 0 for l, n, _ in info["level_candidates"] if l == 3)


def test_grid_8_by_8_and_a_share_of_zero():
    o, info = K.reference("grid8")
    h, w = K.CASES["grid8"]["img"].shape
    ws = set((j + 1) * w // 8 - j * w // 8 for j in range(8)); hs = set((i + 1) * h // 8 - i * h // 8 for i in range(8))
    assert len(hs) > 1 and min(ws | hs) >= 44                            # unequal cells, each with room inside an edge of 19
    assert len(info["cell_candidates"]) == 64 and sum(1 for n, _ in info["cell_candidates"] if n > 0) >= 16
    assert len(o["u"]) > 0
    none, info0 = K.reference("grid8_share0")
    assert all(share == 0 for _, share in info0["cell_candidates"]) and sum(n for n, _ in info0["cell_candidates"]) > 0
    assert len(none["u"]) == 0
    assert set(c for s in info0["stages"] for c in s["cut"]) == {0, 256}   # 256 where a cell has something to drop, 0 where not


def test_a_last_level_whose_share_is_zero():
    """n_per_level[-1] == 0 does exist in the admitted range: scale_factor 2, 3 levels and number_of_features 1 split 2 features
    as rnd(1.14) + rnd(0.57) + max(2 - 2, 0) = 1 + 1 + 0.  The last level then keeps nothing though it has candidates."""
    cfg = K.CASES["last_level0"]["cfg"]
    assert R.n_per_level(2, 2.0, 3) == [1, 1, 0]
    o, info = K.reference("last_level0")
    assert [n for l, n, _ in info["level_candidates"]][2] > 0 and info["stages"][0]["cut"][2] == 256
    assert len(o["u"]) >= 1 and 2 not in o["octave"].tolist() and cfg["n_levels"] == 3


def test_pattern_15_reads_outside_a_level_0_image():
    o, info = K.reference("pattern15")
    assert set(o["octave"].tolist()) == {0} and len(info["outside"]) == len(o["u"]) > 100
    assert sum(1 for n in info["outside"] if n > 0) >= 1
    p = K.CASES["pattern15"]["pattern"]
    assert p.min() == -15 and p.max() == 15 and p.shape == (512, 2)
    o13, info13 = K.reference("pattern13")
    assert len(o13["u"]) == len(o["u"]) and not any(info13["outside"])
    assert (o13["desc"] != o["desc"]).any()
    # the frame of noise leaves keypoints and angles as they are without it ...
    img = K.CASES["pattern15"]["img"]
    plain = R.extract(K.scene(163, 157), S.pattern(), **K.CASES["pattern13"]["cfg"])
    assert all(np.array_equal(plain[f], o13[f]) for f in ("u", "v", "response", "angle", "octave")) and not np.array_equal(K.scene(163, 157), img)
    # ... and makes the outside reads tell: with the outside points clamped to the border instead of reflected, descriptors change
    blurred, (H, W), changed = R.blur(img), img.shape, 0
    for k in np.nonzero(np.array(info["outside"]) > 0)[0]:
        row, col = R.pattern_reads(int(R.rnd(o["u"][k])), int(R.rnd(o["v"][k])), o["angle"][k], p)
        inside = (row >= 0) & (row < H) & (col >= 0) & (col < W)
        assert (~inside).sum() == info["outside"][k]
        val = np.where(inside, blurred[np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)], img[np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)]).astype(int)
        clamped = np.packbits((val[0::2] < val[1::2]).astype(np.uint8).reshape(32, 8), axis=1, bitorder="little").reshape(32)
        changed += int((clamped != o["desc"][k]).any())
    assert changed >= 1


def test_satellites_give_the_exact_angles():
    img, where = S.satellites()
    o, _ = K.reference("satellites")
    assert len(o["u"]) == len(where) == 10
    got = {(int(u), int(v)): a for u, v, a in zip(o["u"], o["v"], o["angle"])}
    by_offset = {off: got[(x, y)] for x, y, off in where}                # one keypoint per dot, none elsewhere
    assert all(a.dtype == F32 for a in by_offset.values())
    assert [float(by_offset[k]) for k in (None, (10, 0), (0, 10), (-10, 0), (0, -10))] == [0.0, 0.0, 90.0, 180.0, 270.0]
    assert sorted(o["angle"].tolist()).count(0.0) == 2
    d = float(R.fast_atan2(F32(1), F32(1)))                              # the ax == ay branch: c is exactly 1
    assert 44.9 < d < 45.1
    diag = [by_offset[k] for k in ((7, 7), (-7, 7), (-7, -7), (7, -7))]
    assert [float(a) for a in diag] == [float(F32(d)), float(F32(180) - F32(d)), float(F32(360) - (F32(180) - F32(d))), float(F32(360) - F32(d))]
    assert [int(a // 90) for a in diag] == [0, 1, 2, 3]
    assert 0.0 < float(by_offset[(12, 5)]) < 45.0 and float(by_offset[(12, 5)]) != float(F32(d))


def test_fine_masks_resize_to_what_no_nearest_rule_gives():
    """Bilinear interpolation stays between its taps, so the upper levels of the {0, 1} mask hold 0 and 1 only - but not where a
    nearest-neighbour pick puts them; the same fields with 200 in place of 1 hold values in between as well."""
    results = {}
    for name in ("fine_mask", "fine_mask200", "half_mask3", "no_mask3"):
        results[name] = K.reference(name)
    for name, hi in (("fine_mask", 1), ("fine_mask200", 200)):
        o, info = results[name]
        assert set(np.unique(K.CASES[name]["mask"]).tolist()) == {0, hi}
        mixed = 0
        for st in info["stages"]:
            for l in (1, 2):
                m, m0 = st["masks"][l], st["masks"][0]
                v = set(np.unique(m).tolist())
                if 0 in v and len(v) > 1:
                    mixed += 1
                    ys = np.minimum((np.arange(m.shape[0]) * m0.shape[0]) // m.shape[0], m0.shape[0] - 1)
                    xs = np.minimum((np.arange(m.shape[1]) * m0.shape[1]) // m.shape[1], m0.shape[1] - 1)
                    assert ((m != 0) != (m0[ys][:, xs] != 0)).any()
                    if hi > 1:
                        assert v - {0, hi}
        assert mixed >= 2
        oc = octaves(o, 3)
        assert oc[0] > 0 and oc[1] > 0
        keys = lambda r: set(zip(r["octave"].tolist(), r["u"].tolist(), r["v"].tolist()))
        assert keys(o) != keys(results["no_mask3"][0]) and keys(o) != keys(results["half_mask3"][0])
    assert any((a != b).any() for sa, sb in zip(results["fine_mask"][1]["stages"], results["fine_mask200"][1]["stages"])
               for a, b in zip(sa["masks"][1:], sb["masks"][1:]) if a is not None and ((a != 0) != (b != 0)).any())


def test_stage_reports_against_what_they_do_not_encode():
    name = "scale2"
    case, (o, info) = K.CASES[name], K.reference(name)
    cfg = dict(R.DEFAULTS, **case["cfg"])
    img = case["img"]
    h, w = img.shape
    n_l = R.n_per_level(2 * cfg["number_of_features"], cfg["scale_factor"], cfg["n_levels"])
    assert len(info["stages"]) == 4 and len(info["pyramid"]) == len(info["blurred"]) == 3
    for ci, st in enumerate(info["stages"]):
        i, j = divmod(ci, 2)
        cell = img[i * h // 2:(i + 1) * h // 2, j * w // 2:(j + 1) * w // 2]
        assert np.array_equal(st["levels"][0], cell)
        kept = []
        for l in range(3):
            lv = st["levels"][l]
            lh, lw = lv.shape
            assert (lw, lh) == R.level_size(cell.shape[1], cell.shape[0], 2.0, l)
            x, y, s = R.fast_keypoints(lv, None, cfg["fast_threshold"])
            inside = (x >= 19) & (x < lw - 19) & (y >= 19) & (y < lh - 19)
            want = sorted(zip(x[inside].tolist(), y[inside].tolist(), s[inside].tolist()))
            assert sorted(zip(*(a.tolist() for a in st["candidates"][l]))) == want and len(want) > 0
            kept.append(s[inside][R.retain_best(s[inside], n_l[l])])
        # the cut is the smallest response that passes retain_best twice
        union = np.concatenate(kept)
        final = [k[np.isin(k, union[R.retain_best(union, cfg["number_of_features"] // 4)])] for k in kept]
        twice = np.concatenate(final)
        assert 0 < len(twice) < len(union) and min(st["cut"]) in twice.tolist()   # the cut is itself a kept response
        for l in range(3):
            s = st["candidates"][l][2]
            assert sorted(s[s >= st["cut"][l]].tolist()) == sorted(final[l].tolist())
    assert sum(len(s[2][s[2] >= c]) for st in info["stages"] for s, c in zip(st["candidates"], st["cut"])) >= len(o["u"]) > 0
    assert R.cut([9, 7, 7, 5], 2) == 7 and R.cut([9, 7], 2) == 0 and R.cut([9], 0) == 256 and R.cut([], 0) == 0
    # the blurred level of a constant image: the closed form of test_blur_of_a_constant_image
    info = {}
    R.extract(np.full((90, 100), 77, np.uint8), S.pattern(), info=info, n_levels=2, scale_factor=1.5)
    want = min((77 * 257 * 257 + 32768) >> 16, 255)
    assert [b.shape for b in info["blurred"]] == [(90, 100), (60, 67)] and all((b == want).all() for b in info["blurred"])
    assert all((p == 77).all() for p in info["pyramid"]) and info["outside"] == []
