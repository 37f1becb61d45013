"""CPU tests of the NumPy restatement tests/cloud_reference.py, the pin of uzl_cloud_*, by independent means: SciPy's kd-tree for the
two searches, numpy.linalg.eigh for the normal, numpy.cbrt and libm's pow for the colour conversion, a dictionary for the voxel
grid, SciPy's BFGS for the inner step (the stated divergence of contract step 7), and the scenes' true displacements.  Nothing here
involves the code under test."""
import math

import numpy as np
import pytest
from scipy.optimize import minimize
from scipy.spatial import cKDTree

import cloud_reference as LR
import cloud_scenes as CS

SCENES = CS.scenes()
_clouds = {}

# Largest difference between the restatement's cube root and numpy.cbrt over every X, Y, Z a BGR8 colour can give (below), in
# units of the last place of f64.  The last Halley step rounds five times; numpy.cbrt is itself within 1.
CBRT_ULP_MEASURED = 3.0
# Largest pose difference (metres, radians) between the restatement's damped Gauss-Newton and SciPy's BFGS on the same f from the
# same start, over the first outer iteration of the SOLVE scenes at the second guess: DESIGN.md, "Cloud registration".
BFGS_MEASURED = (1.954e-7, 1.082e-7)
# step 4: a point is left out of the covariance comparison when its two smallest eigenvalues are closer than GAP times the largest
# (the normal is then not defined by the data); at most CAP of a scene's points may be
GAP, CAP = 1e-3, 0.02


def clouds(name):
    if name not in _clouds:
        s = SCENES[name]
        _clouds[name] = (LR.make_cloud(*s["cloud_from"]), LR.make_cloud(*s["cloud_to"]))
    return _clouds[name]


def ill_conditioned(xyz):
    idx, _ = LR.knn(xyz, LR.DEFAULTS["k"])
    w = np.linalg.eigvalsh(LR.full(LR.neighbour_cov(xyz, idx)))
    return (w[:, 1] - w[:, 0]) < GAP * w[:, 2]


def test_the_scenes_are_what_the_tests_need():
    for name, s in SCENES.items():
        for side in ("from", "to"):
            n = len(s["cloud_" + side][0])
            assert 1000 < n < 2500, (name, side, n)
    d = SCENES["corner_holes"]["depth_from"]
    assert np.isnan(d).any() and (d == 0).any() and (d > 5).any() and (d < 0).any()


def test_cloud_from_images_against_a_scalar_loop():
    s = SCENES["corner_holes"]
    xyz, bgr = LR.cloud_from_images(s["depth_from"], s["bgr_from"], s["fx"], s["fy"], s["cx"], s["cy"])
    want = []
    for v in range(s["depth_from"].shape[0]):
        for u in range(s["depth_from"].shape[1]):
            d = s["depth_from"][v, u]
            if d > 0 and not math.isnan(d):
                want.append((np.float32((u - s["cx"]) * float(d) / s["fx"]), np.float32((v - s["cy"]) * float(d) / s["fy"]), d,
                             *s["bgr_from"][v, u]))
    want = np.array(want, np.float64)
    assert np.array_equal(xyz.astype(np.float64), want[:, :3]) and np.array_equal(bgr, want[:, 3:].astype(np.uint8))


@pytest.mark.parametrize("name", ["small", "corner_holes"])
def test_voxel_grid_against_a_dictionary(name):
    s = SCENES[name]
    xyz, bgr = LR.cloud_from_images(s["depth_to"], s["bgr_to"], s["fx"], s["fy"], s["cx"], s["cy"])
    f32 = np.float32
    inv = f32(1.0) / f32(0.05)
    ok = [i for i in range(len(xyz)) if np.isfinite(xyz[i]).all() and f32(0) <= xyz[i, 2] <= f32(5)]
    lo = [math.floor(float(min(xyz[i, a] for i in ok) * inv)) for a in range(3)]
    hi = [math.floor(float(max(xyz[i, a] for i in ok) * inv)) for a in range(3)]
    dx, dy = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
    cells = {}
    for i in ok:                                                 # ascending pixel index
        ijk = [math.floor(float(xyz[i, a] * inv)) - lo[a] for a in range(3)]
        cells.setdefault(ijk[0] + ijk[1] * dx + ijk[2] * dx * dy, []).append(i)
    want_xyz, want_bgr = [], []
    for key in sorted(cells):
        acc = [f32(0)] * 6
        for i in cells[key]:
            for a, v in enumerate([xyz[i, 0], xyz[i, 1], xyz[i, 2], f32(bgr[i, 2]), f32(bgr[i, 1]), f32(bgr[i, 0])]):
                acc[a] = f32(acc[a] + v)
        c = [f32(a / f32(len(cells[key]))) for a in acc]
        want_xyz.append(c[:3])
        want_bgr.append([int(c[5]), int(c[4]), int(c[3])])
    got_xyz, got_bgr = LR.voxel_grid(xyz, bgr)
    assert np.array_equal(got_xyz.view(np.uint32), np.array(want_xyz, f32).view(np.uint32))
    assert np.array_equal(got_bgr, np.array(want_bgr, np.uint8))
    assert max(len(v) for v in cells.values()) > 1 and (len(ok) < len(xyz) or name == "small")
    keep, keys = LR.voxel_keys(xyz)
    assert keep.tolist() == ok and sorted(set(keys.tolist())) == sorted(cells)


def test_voxel_grid_edges():
    f32 = np.float32
    one = np.array([[0.01, 0.02, 1.0], [0.02, 0.01, 1.01]], f32)
    xyz, bgr = LR.voxel_grid(one, np.array([[10, 20, 30], [11, 21, 32]], np.uint8))
    assert len(xyz) == 1 and bgr.tolist() == [[10, 20, 31]]
    assert np.array_equal(xyz[0], (one[0] + one[1]) / f32(2))
    none = LR.voxel_grid(np.array([[0, 0, 6.0], [np.nan, 0, 1.0]], f32), np.zeros((2, 3), np.uint8))
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)
    assert LR.voxel_keys(np.array([[0, 0, 1.0], [4000.0, 4000.0, 5.0]], f32)) is None      # 80000 x 80000 x 81 cells
    assert LR.voxel_keys(np.array([[0, 0, 1.0], [100.0, 100.0, 5.0]], f32)) is not None


def test_cube_root_against_numpy_cbrt():
    """every value of every channel, the other two drawn at random"""
    rng = np.random.default_rng(0)
    cols = []
    for ch in range(3):
        a = rng.integers(0, 256, (256 * 64, 3)).astype(np.uint8)
        a[:, ch] = np.repeat(np.arange(256), 64)
        cols.append(a)
    bgr = np.concatenate(cols)
    t = LR.lin_table()
    B, G, R = t[bgr[:, 0]], t[bgr[:, 1]], t[bgr[:, 2]]
    x = np.concatenate([((R * 0.4124 + G * 0.3576) + B * 0.1805) / 0.95047, (R * 0.2126 + G * 0.7152) + B * 0.0722,
                        ((R * 0.0193 + G * 0.1192) + B * 0.9505) / 1.08883])
    x = x[x > 0.008856]
    assert x.min() < 0.0089 and x.max() > 0.98 and len(x) > 100000
    ulp = np.abs(LR.cbrt(x) - np.cbrt(x)) / np.spacing(np.cbrt(x))
    print("cube root: largest difference to numpy.cbrt %.1f ulp over %d values" % (ulp.max(), len(x)))
    assert ulp.max() <= CBRT_ULP_MEASURED
    # the seed is within a factor 1.75 of the root over the whole range, as the header says
    y0 = 0.35 + 0.7 * x
    assert (y0 / np.cbrt(x)).max() < 1.75 and (y0 / np.cbrt(x)).min() > 0.8


def _lab_pow(b, g, r):
    """gicp6d.cpp:44-110 as written, with libm's pow"""
    c = []
    for q in (r, g, b):
        q = q / 255.0
        c.append(math.pow((q + 0.055) / 1.055, 2.4) if q > 0.04045 else q / 12.92)
    R, G, B = c
    X = R * 0.4124 + G * 0.3576 + B * 0.1805
    Y = R * 0.2126 + G * 0.7152 + B * 0.0722
    Z = R * 0.0193 + G * 0.1192 + B * 0.9505
    X /= 0.95047
    Z /= 1.08883
    X, Y, Z = [math.pow(u, 1.0 / 3.0) if u > 0.008856 else 7.787 * u + 16.0 / 116.0 for u in (X, Y, Z)]
    return np.float32(116.0 * Y - 16.0), np.float32(500.0 * (X - Y)), np.float32(200.0 * (Y - Z))


def test_lab_against_the_reference_formula_with_pow():
    rng = np.random.default_rng(1)
    bgr = np.concatenate([rng.integers(0, 256, (6000, 3)), [[0, 0, 0], [255, 255, 255], [10, 10, 10], [11, 11, 11], [255, 0, 0], [0, 255, 0],
                                                           [0, 0, 255], [1, 2, 3]]]).astype(np.uint8)
    got = LR.lab(bgr)
    want = np.array([_lab_pow(*c) for c in bgr.tolist()], np.float32)
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print("CIELAB after the cast to f32: %d of %d values differ from pow's" % (differ, got.size))
    assert differ <= got.size // 1000                         # 3 ulp of f64 reach an f32 rounding boundary about once in 10^8
    assert np.abs(got - want).max() <= np.spacing(np.float32(128.0))
    assert abs(got[-7, 0] - 100.0) < 1e-3 and abs(got[-8, 0]) < 1e-6     # white, black
    assert (bgr == 10).all(1).any() and (bgr == 11).all(1).any()          # either side of 0.04045


@pytest.mark.parametrize("name", ["small", "corner_holes"])
def test_knn_against_a_kd_tree(name):
    xyz = SCENES[name]["cloud_from"][0]
    idx, dist = LR.knn(xyz, 20)
    d, want = cKDTree(xyz.astype(np.float64)).query(xyz.astype(np.float64), k=21)
    gaps = np.diff(d * d, axis=1) > 1e-5 * (d * d)[:, 1:]      # gaps[:, r]: ranks r and r + 1 are no near tie
    clear = gaps[:, :20] & np.concatenate([np.ones((len(xyz), 1), bool), gaps[:, :19]], 1)      # rank r is tied with neither side
    assert clear.mean() > 0.3
    assert np.array_equal(idx[clear], want[:, :20][clear])
    assert (idx[:, 0] == np.arange(len(xyz))).all() and (dist[:, 0] == 0).all() and (np.diff(dist, axis=1) >= 0).all()
    same_set = [set(a) == set(b) for a, b in zip(idx[gaps[:, 19]].tolist(), want[gaps[:, 19], :20].tolist())]
    assert all(same_set)


def test_knn_ties_go_to_the_lower_index():
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), [1.0]), -1).reshape(-1, 3).astype(np.float32)
    idx, dist = LR.knn(g, 5)
    for i in range(len(g)):
        d = ((g - g[i]) ** 2).sum(1)
        assert idx[i].tolist() == sorted(range(len(g)), key=lambda j: (d[j], j))[:5]


@pytest.mark.parametrize("name", ["small", "corner"])
def test_nn6_against_a_kd_tree(name):
    a, b = clouds(name)
    G = CS.displaced(SCENES[name]["true"], *CS.GUESSES[1])
    j, d2, kept = LR.correspondences(a, b, G, np.eye(3, 4))
    w = LR.DEFAULTS["lab_weight"]
    q = np.concatenate([a["xyz"], w * a["lab"]], 1).astype(np.float64)
    t = np.concatenate([LR.move32(b["xyz"], G), w * b["lab"]], 1).astype(np.float64)
    d, want = cKDTree(t).query(q, k=2)
    clear = (d[:, 1] ** 2 - d[:, 0] ** 2) > 1e-5 * d[:, 1] ** 2
    assert clear.mean() > 0.9
    assert np.array_equal(j[clear], want[clear, 0])
    assert np.allclose(d2, d[:, 0] ** 2, rtol=1e-5, atol=1e-12)
    assert np.array_equal(kept, (d2.astype(np.float64) < 0.2 * 0.2).astype(np.int32)) and 0 < kept.sum() < len(kept)


@pytest.mark.parametrize("name", list(SCENES))
def test_normals_against_eigh_and_the_cap_on_points_left_out(name):
    for xyz in (SCENES[name]["cloud_from"][0], SCENES[name]["cloud_to"][0]):
        idx, _ = LR.knn(xyz, 20)
        c6 = LR.neighbour_cov(xyz, idx)
        n = LR.normals(c6)
        w, V = np.linalg.eigh(LR.full(c6))
        out = ill_conditioned(xyz)
        assert out.mean() <= CAP, (name, out.mean())
        assert np.abs((n * V[:, :, 0]).sum(1))[~out].min() > 1 - 1e-9
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-15
        # C = I - (1 - eps) n n^T is PCL's U diag(1, 1, eps) U^T
        C = LR.full(LR.covariances(xyz))
        want = np.einsum("nij,j,nkj->nik", V, [0.001, 1.0, 1.0], V)
        assert np.abs(C - want)[~out].max() < 1e-8


def test_mahalanobis_is_the_inverse():
    a, b = clouds("small")
    s = SCENES["small"]
    G = CS.displaced(s["true"], *CS.GUESSES[2])
    T = CS.pose([0.01, -0.02, 0.005], [0.01, 0.02, -0.01])
    j, _, kept = LR.correspondences(a, b, G, T)
    k = np.flatnonzero(kept)
    M = LR.full(LR.mahalanobis(T, G, a["cov"][k], b["cov"][j[k]]))
    S = T[:, :3] @ LR.full(a["cov"][k]) @ T[:, :3].T + G[:, :3] @ LR.full(b["cov"][j[k]]) @ G[:, :3].T
    assert np.abs(M @ S - np.eye(3)).max() < 1e-9


def test_the_sums_are_the_derivatives_of_f():
    """H and g of contract step 7 against finite differences of f under T <- [dR(w) | v] T"""
    a, b = clouds("small")
    G = CS.displaced(SCENES["small"]["true"], *CS.GUESSES[1])
    T = CS.pose([0.01, -0.02, 0.005], [0.01, 0.02, -0.01])
    p, q, M, cnt = LR.problem(a, b, G, T)
    S = LR.evaluate(T, p, q, M)
    f = lambda d: LR.evaluate(LR.apply(T, d), p, q, M)[27]
    h = 1e-5
    E = np.eye(6)
    g = np.array([(f(h * E[k]) - f(-h * E[k])) / (2 * h) for k in range(6)])
    assert np.allclose(g, 2 * S[21:27], rtol=1e-5, atol=1e-6 * np.abs(S[21:27]).max())
    H = np.zeros((6, 6))
    H[np.triu_indices(3)] = S[:6]
    H[:3, 3:] = S[6:15].reshape(3, 3)
    H[3:, 3:][np.triu_indices(3)] = S[15:21]
    H = np.triu(H) + np.triu(H, 1).T
    for k in range(6):
        gk = np.array([(LR.evaluate(LR.apply(LR.apply(T, h * E[k]), h * E[m]), p, q, M)[27] - LR.evaluate(LR.apply(LR.apply(T, h * E[k]), -h * E[m]), p, q, M)[27]
                        - LR.evaluate(LR.apply(LR.apply(T, -h * E[k]), h * E[m]), p, q, M)[27] + LR.evaluate(LR.apply(LR.apply(T, -h * E[k]), -h * E[m]), p, q, M)[27])
                       / (4 * h * h) for m in range(6)])
        # Gauss-Newton's H leaves out the curvature of the rotation, which is of the size of the residual
        assert np.allclose(gk, 2 * H[k], rtol=0.1, atol=0.05 * np.abs(H).max()), k
    d = LR.solve(S, 0.0)
    assert np.allclose(H @ d, -S[21:27], rtol=1e-9, atol=1e-9 * np.abs(S[21:27]).max())
    Tn = LR.apply(T, d)
    assert abs(np.linalg.det(Tn[:, :3]) - 1) < 1e-12 and np.abs(Tn[:, :3] @ Tn[:, :3].T - np.eye(3)).max() < 1e-12


def test_solve_refuses_a_matrix_that_is_not_positive():
    S = np.zeros(28)
    S[[0, 3, 5, 15, 18, 20]] = [1, 1, 1, 1, 1, -1]
    assert LR.solve(S, 0.0) is None
    S[20] = 1
    S[21:27] = 1
    assert np.allclose(LR.solve(S, 0.0), -1) and np.allclose(LR.solve(S, 1.0), -0.5)


@pytest.mark.parametrize("name", CS.SOLVE)
def test_bfgs_reaches_the_same_minimiser(name):
    """the stated divergence of contract step 7: PCL's BFGS and this damped Gauss-Newton stop at the same stationary point of f"""
    a, b = clouds(name)
    G = CS.displaced(SCENES[name]["true"], *CS.GUESSES[1])
    p, q, M, cnt = LR.problem(a, b, G, np.eye(3, 4))
    T = LR.inner(np.eye(3, 4), p, q, M)

    def f(x):
        return LR.evaluate(CS.pose(x[3:], x[:3]), p, q, M)[27]

    r = minimize(f, np.zeros(6), method="BFGS", options=dict(gtol=1e-10))
    dt, dr = CS.pose_errors(T, CS.pose(r.x[3:], r.x[:3]))
    print("%s: BFGS %d iterations, f %.12g against %.12g, poses %.3e m %.3e rad apart" % (name, r.nit, r.fun, f(np.zeros(6)), dt, dr))
    assert LR.evaluate(T, p, q, M)[27] <= r.fun * (1 + 1e-9)
    assert dt <= 10 * BFGS_MEASURED[0] and dr <= 10 * BFGS_MEASURED[1]


@pytest.mark.parametrize("name", CS.SOLVE)
def test_the_solve_scenes_keep_the_pose_bound_in_the_restatement_alone(name):
    """cloud_scenes.SOLVE: the restatement alone ends within the project's pose bound of the true displacement"""
    a, b = clouds(name)
    s = SCENES[name]
    for g in CS.GUESSES:
        e = LR.estimate(a, b, CS.displaced(s["true"], *g))
        dt, dr = CS.pose_errors(e["transform"], s["true"])
        print("%s %s: %d iterations, %s, %.3e m %.3e rad from the truth" % (name, g, e["iterations"], e["num_corr_iter"], dt, dr))
        assert e["status"] == LR.OK and e["match_score"] > 0.8 and e["iterations"] < 20
        assert dt < 1e-3 and dr < 1e-4
        assert np.array_equal(e["information"], np.diag([1e4] * 3 + [1e6] * 3)) and e["matching_score"] == 1.0


def test_gates_in_the_restatement():
    a, b = clouds("small")
    s = SCENES["small"]
    far = CS.mul(s["true"], CS.pose([1.5, 0, 0], [0, 0, 0]))
    e = LR.estimate(a, b, far)
    assert e["status"] in (LR.NO_CORR, LR.LOW_SCORE) and e["matching_score"] == 0.0 and not e["information"].any()
    e = LR.estimate(a, b, s["true"], LR.config(max_translation=1e-6))
    assert e["status"] == LR.TOO_FAR
    e = LR.estimate(a, b, s["true"], LR.config(min_score=0.99))
    assert e["status"] == LR.LOW_SCORE
    with pytest.raises(ValueError):
        LR.make_cloud(a["xyz"][:19], a["bgr"][:19])
    assert LR.make_cloud(a["xyz"][:20], a["bgr"][:20])["n"] == 20
