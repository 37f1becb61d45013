"""CPU tests (no GPU needed) of the planted laser-line scenes in tests/laserline_edge_scenes.py, which test_laserline_edges_gpu.py
sends through the device: every family asserts on the reference (tests/laserline_reference.py) that the edge it is planted for
really occurs - both bins beside a boundary, both seam bins, atan2f guesses that miss, kept and dropped heights and depths, each
kind of transition between the consecutive rows one lane of the bin kernel visits, every reachable merge branch, counted and
uncounted beams of the centre - so that an empty or degenerate plant fails here instead of passing silently on the device."""
import collections
import itertools

import numpy as np
import pytest

import laserline_edge_scenes as ES
import laserline_reference as LR

F32 = np.float32
GRID_IDS = [str(n) for n in ES.GRIDS]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_point_images_carry_their_coordinates_bit_for_bit():
    pts = [(1.5, -2.25, 0.5), (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), (-0.0, -0.0, 0.5), (ES.DENORM, -ES.DENORM, 1e-40), (3e38, -3e38, 0.1),
           (F32(0.1), ES.ulps(F32(0.1), 1)[()], ES.ulps(F32(0.1), -1)[()])]
    q = ES.image_points(ES.point_images(pts))
    for a, col in enumerate(q):
        assert np.array_equal(bits(col), bits([p[a] for p in pts]))
    assert ES.ulps(F32(0), -1)[()] == -ES.DENORM and ES.ulps(-ES.DENORM, 2)[()] == ES.DENORM and ES.ulps(F32(1), 1)[()] == np.nextafter(F32(1), F32(2))


@pytest.mark.parametrize("n", ES.GRIDS, ids=GRID_IDS)
def test_boundary_clusters_hold_both_bins(n):
    """Each cluster of five points around boundary k = 1 .. n - 1 holds points of bin k - 1 and of bin k.  Boundaries 0 and n part no
    bins under step 6: boundary 0 lies 8.7e-8 rad above the negative x axis, where bin n - 1 has every point on or above the axis,
    and boundary n lies there too (n inc = 2 pi) or below the axis inside bin 0 (n inc > 2 pi); their clusters stay planted and
    must lie in one of those two bins.  The bin change at the seam is the x axis itself: test_seam_points."""
    _, _, c, s = ES.table(n)
    clusters = ES.boundary_clusters(n)
    assert len(clusters) == 16 * 3 and {0, 1, n // 4, n // 2, n - 1, n} <= {k for k, _, _, _ in clusters}
    both = 0
    for k, r, X, Y in clusters:
        assert len(X) == 5 and len(set(zip(bits(X).tolist(), bits(Y).tolist()))) == 5
        b = set(LR.bins(X, Y, c, s).tolist())
        if 0 < k < n:
            assert b == {k - 1, k}, (k, r, b)
            both += 1
        else:
            assert len(b) == 1 and b <= {0, n - 1}, (k, r, b)
    assert both == 14 * 3


@pytest.mark.parametrize("n", ES.GRIDS, ids=GRID_IDS)
def test_seam_points(n):
    _, _, c, s = ES.table(n)
    X, Y = ES.seam_points(n)
    b = LR.bins(X, Y, c, s)
    assert (X < 0).all() and (b >= 0).all()
    assert (b == 0).sum() >= 10 and (b == n - 1).sum() >= 10
    zero = Y == 0
    assert zero.sum() == 6 and np.signbit(Y[zero]).sum() == 3 and (b[zero] == n - 1).all()
    assert (b[Y < 0] == 0).all()                                           # below the axis bin 0 wins wherever both claim the point
    tiny = np.abs(Y) == ES.DENORM
    assert tiny.sum() == 6 and set(b[tiny].tolist()) == {0, n - 1}


@pytest.mark.parametrize("n", ES.GRIDS, ids=GRID_IDS)
def test_axes_origin_and_extreme_coordinates(n):
    _, _, c, s = ES.table(n)
    X, Y = ES.axis_points()
    b = LR.bins(X, Y, c, s)
    assert (b >= 0).all() and len(np.unique(b)) >= 8
    assert (LR.bins(*ES.origin_points(), c, s) == -1).all() and np.signbit(ES.origin_points()[1]).sum() == 2
    cfg = dict(angle_increment=ES.GRIDS[n])
    r, i, ce = LR.extract(ES.point_images(zip(*ES.origin_points())), **cfg)
    assert (r == F32(6)).all() and (i == 0).all() and (ce == 0).all()    # dropped: the scans are empty
    # a denormal point: s underflows to 0, the range is 0.0 and the intensity 0; 3e38: s overflows, range hi and intensity inf
    r, i, _ = LR.extract(ES.point_images([(ES.DENORM, -ES.DENORM), (3e38, 1.0), (-1.0, -3e38)]), **cfg)
    assert (r[0] == 0).sum() == 1 and (i[0] == 0).all()
    assert (r[1:] == F32(6)).all() and np.isinf(i[1]).sum() == 1 and np.isinf(i[2]).sum() == 1


def test_non_finite_coordinates_from_finite_inputs():
    _, _, c, s = ES.table(720)
    names, images = list(ES.NONFINITE), list(ES.NONFINITE.values())
    qx, qy, qz = ES.image_points(images)
    q = dict(zip(names, zip(qx, qy, qz)))
    assert q["qx=+inf"][0] == np.inf and q["qx=-inf"][0] == -np.inf and q["qx=+inf"][1] == F32(1.5) and q["qx=-inf, qy<0"][1] == F32(-1.5)
    assert q["qy=+inf"][1] == np.inf and q["qy=-inf, qx<0"][1] == -np.inf and q["qy=-inf, qx<0"][0] == F32(-1.5)
    assert np.isinf(q["both inf"][0]) and np.isinf(q["both inf"][1])
    assert np.isnan(q["qx=inf-inf"][0]) and np.isfinite(q["qx=inf-inf"][1:]).all()
    assert np.isnan(q["qy=inf-inf"][1]) and np.isfinite(q["qy=inf-inf"][0]) and np.isfinite(q["qy=inf-inf"][2])
    assert np.isnan(q["qz=inf-inf"][2]) and np.isfinite(q["qz=inf-inf"][:2]).all()
    assert np.isnan(q["x=inf, qx=inf 0"]).all()                             # inf 0 = NaN in every row
    assert q["x=inf, qy=qz=inf 0"][0] == np.inf and np.isnan(q["x=inf, qy=qz=inf 0"][1:]).all()
    r, i, ce = LR.extract(images)
    b = LR.bins(qx, qy, c, s)
    kept = 0
    for k, name in enumerate(names):
        assert (r[k] == F32(6)).all() and (ce[k] == 0).all(), name          # s = inf is not below hi hi: the range stays hi
        infinite = np.isinf([qx[k], qy[k]]).any() and not np.isnan([qx[k], qy[k], qz[k]]).any()
        print("%-20s q = (%g, %g, %g): bin %d" % (name, qx[k], qy[k], qz[k], b[k]))
        if infinite:
            assert b[k] >= 0 and np.isinf(i[k, b[k]]) and (np.delete(i[k], b[k]) == 0).all(), name
            kept += 1
        else:
            assert (i[k] == 0).all() and (b[k] == -1 or np.isnan(qz[k])), name
    assert kept == 9


@pytest.mark.parametrize("n", ES.GRIDS, ids=GRID_IDS)
def test_guess_misses(n):
    amin, inc, c, s = ES.table(n)
    X, Y, clamped = ES.guess_misses(n)
    mine, guess = LR.bins(X, Y, c, s), LR.atan2f_bins(X, Y, amin, inc)
    outside = (guess < 0) | (guess >= n)
    print("grid %d: %d points where the atan2f bin misses, %d of them outside [0, n) before the clamp" % (n, len(X), outside.sum()))
    assert (mine >= 0).all() and (mine != guess).all() and len(X) >= 20 and outside.sum() == clamped
    assert (np.abs(mine - guess)[~outside] == 1).all()                      # one bin off: the neighbours the kernel tries
    if n in (720, 1440):                                                    # n inc = 2 pi in f32: the angle pi gives index n
        assert clamped >= 5 and (guess[outside] == n).all() and (mine[outside] == n - 1).all()


def test_height_limits_compare_in_double():
    differs = 0
    for (lo, hi), cases in ES.HEIGHTS.items():
        z = np.array([v for v, _ in cases], F32)
        kept = [k for _, k in cases]
        assert LR.height_ok(z, lo, hi).tolist() == kept, (lo, hi)
        narrowed = ~((z < F32(lo)) | (z > F32(hi)))
        differs += narrowed.tolist() != kept
        r, _, _ = LR.extract(ES.height_images((lo, hi)), min_height=lo, max_height=hi)
        assert ((r < F32(6)).sum(1) == np.array(kept)).all()
    assert differs >= 2 and sum(k for c in ES.HEIGHTS.values() for _, k in c) >= 6
    assert float(F32(0.1)) != 0.1 and float(F32(0.7)) != 0.7                              # doubles that are no f32 values
    z = [v for v, _ in ES.HEIGHTS[(0.1, 0.7)]]
    assert float(z[0]) < 0.1 < float(z[1]) and z[1] == np.nextafter(z[0], F32(1)) and float(z[2]) < 0.7 < float(z[3])
    assert [float(v) for v, _ in ES.HEIGHTS[(0.5, 0.5)]] == [float(np.nextafter(F32(0.5), F32(0))), 0.5, float(np.nextafter(F32(0.5), F32(1)))]


def test_depth_validity():
    sets = ES.depth_validity_images()
    f = [im["depth"][0, 0] for im in sets["f32"][:9]]
    assert np.signbit(f[0]) and f[0] == 0 and f[1] == ES.DENORM and f[2] == ES.FLT_MAX and np.isinf(f[3]) and np.isnan(f[4])
    used = [bool(LR.depth_values(im["depth"])[1][0, 0]) for im in sets["f32"][:9]]
    assert used == [False, True, True, False, False, True, True, True, True]
    u = [int(im["depth"][0, 0]) for im in sets["u16"][:5]]
    assert u[:3] == [0, 1, 65535] and [bool(LR.depth_values(im["depth"])[1][0, 0]) for im in sets["u16"][:5]] == [False, True, True, True, True]
    assert all(im["depth"].shape == (1, 5) for im in sets["f32"][9:]) and len(sets["u16"]) == 10
    # depth_scale 1e-46 on u16: 1 mm .. 1 m underflow to 0 and are dropped, 65.535 m stays a denormal and is used
    d, ok = LR.depth_values(np.array([[1, 1000, 2500, 65535]], np.uint16), 1e-46)
    assert d[0, :3].tolist() == [0, 0, 0] and ok.tolist() == [[False, False, False, True]] and 0 < d[0, 3] < np.finfo(F32).tiny
    # depth_scale 1e300 on f32: every used depth becomes inf and is dropped
    with np.errstate(over="ignore"):
        d, ok = LR.depth_values(np.array([[ES.DENORM, 1.0, ES.FLT_MAX, 0.0]], F32), 1e300)
    assert np.isinf(d[0, :3]).all() and not ok.any()
    kept = {}
    for enc, images in sets.items():
        for scale in ES.DEPTH_SCALES[enc]:
            with np.errstate(over="ignore"):
                r, i, _ = LR.extract(images, depth_scale=scale)
            kept[enc, scale] = int(((r != F32(6)) | (i > 0)).any(1).sum())       # a denormal depth gives s = 0: range 0.0, intensity 0
    print("scans that hold a point per (encoding, depth_scale):", kept)
    assert kept["f32", 1e300] == 0 and kept["f32", 1.0] >= 9 and kept["u16", 1e-46] >= 1 and kept["u16", 0.001] >= 5 and kept["f32", 1000.0] >= 5


# ----------------------------------------------------------------------------------------------------------------- column walks
def test_the_restated_lane_walk():
    assert [ES.lanes_for((w + 3) // 4) for w in (1024, 1021, 508, 640, 516, 132, 160, 8, 3)] == [256, 256, 127, 32, 17, 11, 8, 2, 1]
    assert ES.band_rows(1) == ES.band_rows(16384) == 8 and ES.band_rows(16385) == 9 and ES.band_rows(10 ** 6) == 64
    w, h, copies = ES.BAND9
    assert ES.band_rows(h * copies) == 9 and h % 9 != 0 and w * h * copies * 2 < 4.5e6
    for (w, h), rows_in_chunk in (((1021, 20), 20), ((508, 23), 500), ((132, 24), 24), ((3, 64), 64), ((132, 420), 16800)):
        seen = np.zeros((h, w), int)
        for band, lane, u, rows in ES.lane_visits(w, h, rows_in_chunk):
            assert 0 <= lane < 256 and all(band * ES.band_rows(rows_in_chunk) <= r < (band + 1) * ES.band_rows(rows_in_chunk) for r in rows)
            seen[rows, u] += 1
        assert (seen == 1).all()                                            # every pixel by exactly one Column
    longest = {size: max(len(rows) for *_, rows in ES.lane_visits(*size, size[1])) for size in list(ES.WALKING) + list(ES.CONTROLS)}
    assert [longest[s] for s in ES.WALKING] == [8, 8, 4]                    # a lane walks a whole band, or every other row of it
    assert all(longest[s] == 1 for s in ES.CONTROLS)                        # the controls: one row per lane and band
    assert [h % 8 for _, h in ES.WALKING] == [0, 4, 7]                      # whole bands, and last bands of 4 and 7 rows


@pytest.mark.parametrize("u16", [False, True], ids=["f32", "u16"])
def test_walks_meet_every_transition(u16):
    """per family of scenes (one per encoding): each kind of step between two consecutive kept pixels of one Column at least 10 times"""
    total = collections.Counter()
    scenes = ES.walk_scenes(u16)
    assert len(scenes) == 3 * len(ES.WALKING) + len(ES.CONTROLS)
    for name, im in scenes.items():
        assert im["depth"].dtype == (np.uint16 if u16 else F32)
        if name.endswith("control"):
            continue
        h, w = im["depth"].shape
        binmap = ES.pixel_bins(im, **ES.WINDOW)
        cnt = ES.count_transitions(binmap, ES.lane_visits(w, h, h), 720)
        print(name, dict(cnt))
        total += cnt
        d, used = LR.depth_values(im["depth"])
        assert (~used).mean() > 0.05 and (used & (binmap < 0)).mean() > 0.02          # zeros, and pixels the height window drops
        if name in ("1024x16 down", "1021x20 down"):                                    # the row v = cy: points on the axis itself, Y = +0
            assert im["cy"] == int(im["cy"]) and (binmap[int(im["cy"])] == 719).sum() >= 100 and (binmap[int(im["cy"]) - 1] == 0).sum() >= 100
    for kind in ES.TRANSITIONS:
        assert total[kind] >= 10, kind
    steps = {name: im["depth"].strides[0] for name, im in scenes.items()}
    item = 2 if u16 else 4
    assert steps["1024x16 down"] % (4 * item) != 0 and steps["1021x20 down"] % (4 * item) == 0 and steps["160x24 control"] % (4 * item) != 0


def test_plane_keeps_a_column_in_one_bin():
    scenes = ES.plane_scenes()
    for name, im in scenes.items():
        h, w = im["depth"].shape
        binmap = ES.pixel_bins(im, **ES.WINDOW)
        b = np.unique(binmap[binmap >= 0])
        assert len(b) == 1 and 0 < b[0] < 719 and (binmap < 0).mean() > 0.05
        cnt = ES.count_transitions(binmap, ES.lane_visits(w, h, h), 720)
        print(name, dict(cnt))
        if w == 1024:                                                       # 640 x 48 is a control: its lanes see one row per band
            assert cnt["whole band in one inner bin"] >= 10 and cnt["band ends inside a run"] >= 10
            assert cnt["dropped between two of one bin"] >= 10 and cnt["neighbouring bin"] == cnt["jump of 2 or more"] == 0


# -------------------------------------------------------------------------------------------------- merge and centre truth table
def replay(cfg, cams, kx):
    """the branches the cameras of one group take at the bin of the +x axis, and the merged (range, intensity)"""
    full = dict(LR.DEFAULTS, **cfg)
    scans = [LR.image_scan(ES.pair_image(near, far, 0), full) for near, far in cams]
    for (near, far), (r, i) in zip(cams, scans):                            # the image's scan is (near, far) itself
        hi = F32(full["range_max"]) + F32(1)
        near, far = F32(near), F32(far)
        if near > 1e-10:
            assert r[kx] == (near if near < hi else hi) and i[kx] == (far if far < 1e19 else np.inf)
        else:
            assert r[kx] == (hi if near == 0 else 0) and i[kx] == far       # no point at all, or one whose s underflows
    a, taken = (scans[0][0][kx:kx + 1], scans[0][1][kx:kx + 1]), []
    for r, i in scans[1:]:
        taken.append((ES.merge_branch(a[0][0], r[kx], cfg["range_min"], cfg["range_max"], False),
                      ES.merge_branch(a[1][0], i[kx], cfg["range_min"], cfg["range_max"], True)))
        a = LR.merge(a, (r[kx:kx + 1], i[kx:kx + 1]), cfg["range_min"], cfg["range_max"])
    return taken, (a[0][0], a[1][0])


def test_merge_table_takes_every_branch():
    _, _, c, s = ES.table(720)
    kx = int(LR.bins([1.0], [0.0], c, s)[0])
    assert kx == int(LR.bins([3e38], [0.0], c, s)[0]) == int(LR.bins([0.01], [0.0], c, s)[0])   # one bin for every radius
    ranges, intens, pairs = collections.Counter(), collections.Counter(), collections.Counter()
    results = {}
    for cfg, cams in ES.merge_groups():
        taken, out = replay(cfg, cams, kx)
        for br, bi in taken:
            ranges[br] += 1
            intens[bi] += 1
            pairs[br, bi] += 1
        results[tuple(sorted(cfg.items())), tuple(cams)] = out
    print("range branches:", dict(ranges))
    print("intensity branches:", dict(intens))
    assert set(ranges) == set(ES.RANGE_BRANCHES) and set(intens) == set(ES.INTENSITY_BRANCHES)
    assert min(ranges.values()) >= 3 and min(intens.values()) >= 3 and len(pairs) >= 15
    # |a - r| on 0.1f and on its two neighbours, in both orders
    lo, a, hi = ES.CLOSE_A
    r = ES.CLOSE_R
    tenth = F32(0.1)
    assert abs(lo - r) == np.nextafter(tenth, F32(0)) and abs(a - r) == tenth and abs(hi - r) == np.nextafter(tenth, F32(1))
    key = tuple(sorted(ES.CLOSE_CFG.items()))
    for x, close in ((lo, True), (a, False), (hi, False)):
        for cams in (((x, x), (r, r)), ((r, r), (x, x))):
            got = results[key, cams]
            assert got[0] == (F32(0.5) * (x + r) if close else 0), (x, cams)
        assert results[key, ((x, x), (r, r))][1] == (F32(0.5) * (x + r) if close else 0)       # a > r
        assert results[key, ((r, r), (x, x))][1] == (F32(0.5) * (x + r) if close else r)       # a <= r: kept
    # three cameras: the result depends on the order
    key = tuple(sorted(ES.MERGE_CFG.items()))
    perms = [results[key, p] for p in itertools.permutations([(2.0, 2.0), (2.05, 2.05), (3.0, 3.0)])]
    assert len({float(p[0]) for p in perms}) >= 2 and len({float(p[1]) for p in perms}) >= 2
    assert results[key, ((2.0, 2.0), (3.0, 3.0), (2.5, 2.5))][0] == F32(2.5)                   # the zero is retaken
    # the ends check_cfg admits
    zero_lo = tuple(sorted(dict(range_min=0.0, range_max=5.0).items()))
    assert results[zero_lo, ((2.0, 2.0), (1e-30, 3.0))] == (0, F32(2.0))                       # r = 0.0 is not below lo = 0: far apart
    assert results[zero_lo, ((0, 0), (1e-30, 3.0))] == (0, F32(3.0))
    same = tuple(sorted(dict(range_min=2.0, range_max=2.0).items()))
    assert results[same, ((2.0, 2.0), (2.05, 2.05))][0] == F32(2.0) and results[same, ((1.0, 3.0), (2.0, 2.0))][0] == F32(0)
    for cfg in ES.merge_cfgs():
        images, groups = ES.merge_images(cfg)
        assert len(images) == sum(len(g) for g in groups) and images[-1]["group"] == len(groups) - 1


def test_centre_scans_hold_counted_and_uncounted_beams():
    _, _, c, s = ES.table(720)
    lo, hi0 = F32(0.45), F32(5.0)
    groups = ES.centre_groups()
    r, i, ce = LR.extract(ES.grouped(groups.values()), **ES.CENTRE_CFG)
    scans = dict(zip(groups, r))
    finite = scans["edges"][scans["edges"] != F32(6)]
    assert sorted(finite.tolist())[:3] == [0.0, float(lo), float(ES.up(lo))] and hi0 in finite and ES.up(hi0) in finite and len(finite) == 9

    def counted(x):
        return int(((x > lo) & (x <= hi0)).sum())

    assert [counted(scans[k]) for k in groups] == [6, 1, 0, 0]
    assert (scans["no beam"] == 0).sum() == 1 and (scans["no beam"] == lo).sum() == 1 and (scans["no beam"] == ES.up(hi0)).sum() == 1
    assert (ce[2:] == 0).all() and (ce[:2, :2] != 0).all()
    k = int(np.nonzero((scans["one beam"] > lo) & (scans["one beam"] <= hi0))[0][0])
    x = float(scans["one beam"][k])
    assert ce[1].tolist() == [float(F32(c[k] * x)), float(F32(s[k] * x)), 0.0]
    # a shift of either bound by one ulp would change the count
    assert counted(scans["edges"]) != int(((scans["edges"] >= lo) & (scans["edges"] <= hi0)).sum())
    assert counted(scans["edges"]) != int(((scans["edges"] > lo) & (scans["edges"] < hi0)).sum())


def test_every_beam_of_4096_is_counted():
    images, (r, i, ce) = ES.every_beam()
    _, _, c, s = ES.table(4096)
    qx, qy, _ = ES.image_points(images)
    assert sorted(LR.bins(qx, qy, c, s).tolist()) == list(range(4096))
    assert len(images) == 4096 and r.shape == (1, 4096) and ((r > F32(0.45)) & (r <= F32(5))).all() and len(np.unique(r)) > 4000
    assert np.array_equal(ce[0], LR.scan_center(r[0], c, s, 0.45, 5.0)) and np.abs(ce[0, :2]).max() > 1e-3
