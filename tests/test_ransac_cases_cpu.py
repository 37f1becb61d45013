"""The cases of tests/ransac_cases.py are what they claim to be: shown on the reference side alone (CPU oracle + NumPy), so that the
device test that replays them (tests/test_ransac_geometry_gpu.py) compares against inputs known to reach the degenerate branch,
the round edge or the collapse it is named after.  A class that is not reached fails here instead of silently testing something else."""
import numpy as np
import pytest

import np_reference as NP
import ransac_cases as RC

CASES = RC.all_cases()
BY_NAME = {c.name: c for c in CASES}
FLT_MIN = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def results(oracle):
    return {c.name: RC.run_on_oracle(oracle, c) for c in CASES}


def _votes(oracle, c):
    """Every hypothesis' consensus count (no early exit), through the oracle's own stages."""
    m = c.P.shape[1]
    out = np.zeros(c.iterations, np.int64)
    for i in range(c.iterations):
        s = oracle.sample3(RC.SEED, c.job_id, i, c.iterations, m, c.do_prosac)
        out[i] = oracle.consensus3d(c.P, c.Q, oracle.pose_svd(c.P, c.Q, list(s)), c.max_error)[0]
    return out


def _cov32(P, Q):
    """The float covariance the pose recipe accumulates for the whole cloud (same recurrence, NumPy float32)."""
    with np.errstate(all="ignore"):
        p = P.astype(np.float32); q = Q.astype(np.float32)
        cov = np.zeros((3, 3), np.float32); m1 = np.zeros(3, np.float32); m2 = np.zeros(3, np.float32)
        for k in range(P.shape[1]):
            alpha = np.float32(1) / np.float32(k + 1)
            d1 = p[:, k] - m1; d2 = q[:, k] - m2
            cov = (np.float32(1) - alpha) * (cov + alpha * np.outer(d2, d1))
            m1 = m1 + alpha * d1; m2 = m2 + alpha * d2
    return cov


def test_case_list():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    count = {k: len(f()) for k, f in RC.CLASSES.items()}
    assert count == dict(geometry=7, m_edge=10, offset=3, scale=8, nonfinite=3, threshold=7, break_pct=9, iterations=7, steered=9,
                         path_edge=3, odd_stride=1)
    assert [c.P.shape[1] for c in RC.m_edge_cases()] == [0, 1, 2, 3, 4, 15, 16, 17, 31, 33]
    assert [c.iterations for c in RC.iteration_cases()] == [1, 2, 255, 256, 257, 513, 4096]
    # the LDS tile holds 2716 points at 200 iterations: 16 + 800 + 57 n <= 152 KiB, points padded to even
    assert RC.lds_max_points(200) == 2716 and [c.P.shape[1] for c in RC.path_cases()] == [2716, 2717, 2718]
    for it in RC.ITERATIONS + (600,):
        n = RC.lds_max_points(it)
        assert 16 + 4 * ((it + 3) & ~3) + 57 * n <= RC.LDS_BUDGET < 16 + 4 * ((it + 3) & ~3) + 57 * (n + 2)
        assert RC.filler(it, False)[0].shape[1] == n and RC.filler(it, True)[0].shape[1] == n + 2


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_oracle_semantics(results, name):
    """mask = float64 recount of |T P - Q| < t outside a band of 1e-12 (scaled with the case), consensus = its sum, mse = mean
    inlier distance."""
    c, r = BY_NAME[name], results[name]
    scale = float(np.ldexp(1.0, RC.scale_exponent(c)))
    with np.errstate(all="ignore"):
        d = NP.point_distances(c.P, c.Q, r["T"])
        safe = ~(np.abs(d - c.max_error) <= 1e-12 * scale)
        assert np.array_equal(r["mask"][safe].astype(bool), (d < c.max_error)[safe])
    assert r["consensus"] == int(r["mask"].sum())
    if r["consensus"] > 0:
        want = d[r["mask"] == 1].mean()
        assert abs(r["mse"] - want) <= 1e-12 * scale or r["mse"] == want
    assert 0 <= r["iterations_run"] <= c.iterations
    if c.P.shape[1] < 3:
        assert r["iterations_run"] == 0 and r["consensus"] == 0 and np.array_equal(r["T"], np.eye(3, 4)) and r["mse"] == 0


WELL = ["base", "duplicates", "offset_1e+03", "scale_2^-20", "scale_2^-66", "scale_2^40"] + ["m_%d" % m for m in RC.M_EDGE]


@pytest.mark.parametrize("name", WELL)
def test_well_conditioned_pose_vs_kabsch(results, name):
    """The float recipe's refit against a float64 Kabsch fit of the same inlier set: 2e-4 and |det R - 1| < 1e-5, the numbers
    of test_pose_svd_vs_kabsch.  That test's clouds have coordinates of order 1; here the translation is compared in units of the
    case's coordinate scale (2^e, or the offset of an offset case: a float rotation's error of 1e-5 rad moves the translation of a
    cloud 1e3 away by 1e-2), the rotation as it is."""
    c, r = BY_NAME[name], results[name]
    m = c.P.shape[1]
    if m < 3:
        assert r["consensus"] == 0 and np.array_equal(r["T"], np.eye(3, 4))
        return
    assert r["consensus"] >= 3, "a well-conditioned case must find its consensus"
    assert r["consensus"] >= m - int(RC.OUTLIER_FRAC * m) - max(2, m // 20)
    e = RC.scale_exponent(c)
    P = np.ldexp(c.P, -e); Q = np.ldexp(c.Q, -e)                      # exact: powers of two
    T = r["T"].copy(); T[:, 3] = np.ldexp(T[:, 3], -e)
    unit = float(name.split("_")[1]) if name.startswith("offset_") else 1.0
    # the inlier set the refit used: the winning hypothesis' set.  The final mask is its recount; fit what the result describes
    sel = r["mask"] == 1
    K = NP.kabsch(P[:, sel], Q[:, sel])
    D = np.abs(T - K); D[:, 3] /= unit
    assert D.max() < 2e-4, D.max()
    assert abs(np.linalg.det(T[:, :3]) - 1) < 1e-5


@pytest.mark.parametrize("row", RC.STEERED, ids=lambda r: "%d_of_%d" % (r[1], r[0]))
def test_steered_stops(results, row):
    iters, want, j0, job = row
    r = results["steered_%d_of_%d" % (want, iters)]
    assert r["iterations_run"] == want and r["best_iteration"] == want - 1 and r["consensus"] > RC.STEER_BP * RC.STEER_M


def test_steered_list_covers_the_round_edges():
    got = sorted((it, w) for it, w, _, _ in RC.STEERED)
    assert [w for it, w in got if it == 600] == [255, 256, 257, 258, 512]
    assert [w for it, w in got if it == 257][-1] == 256 and [w for it, w in got if it == 513][-1] == 512
    assert [w for it, w in got if it == 257][0] < 256 and [w for it, w in got if it == 513][0] < 256


def test_geometry_classes_reached(oracle, results):
    def centred_sv(P):
        return np.linalg.svd(P - P.mean(1, keepdims=True), compute_uv=False)
    s = centred_sv(BY_NAME["coplanar"].P)
    assert s[1] > 1 and s[2] < 1e-12
    s = centred_sv(BY_NAME["collinear"].P)
    assert s[0] > 1 and s[1] < 1e-12
    c = BY_NAME["duplicates"]
    assert len(np.unique(np.concatenate([c.P, c.Q]).T, axis=0)) == 10 and c.P.shape[1] == 120
    c = BY_NAME["identical"]
    assert len(np.unique(c.P.T, axis=0)) == 1 and len(np.unique(c.Q.T, axis=0)) == 1
    assert results["identical"]["consensus"] == 120            # zero covariance -> R = I, t = q - p: everything agrees
    assert results["identical"]["iterations_run"] == 600 and results["collinear"]["iterations_run"] == 600
    assert results["collinear"]["consensus"] >= 100
    # mirrored: the unconstrained orthogonal fit of the inliers is a reflection
    c = BY_NAME["mirrored"]
    H = (c.Q - c.Q.mean(1, keepdims=True)) @ (c.P - c.P.mean(1, keepdims=True)).T
    U, _, Vt = np.linalg.svd(H)
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0
    assert abs(np.linalg.det(results["mirrored"]["T"][:, :3]) - 1) < 1e-5
    # noise-free: the maximum count is reached in more than one round and the first one wins
    c = BY_NAME["noise_free"]
    v = _votes(oracle, c)
    r = results["noise_free"]
    best = np.nonzero(v == v.max())[0]
    assert r["iterations_run"] == c.iterations and v.max() == 90
    assert best[0] < 256 and ((best >= 256) & (best < 512)).any() and (best >= 512).any()
    assert r["best_iteration"] == best[0]


def test_position_and_scale_classes_reached(results):
    # offset 1e6: the hypotheses find a consensus, the float refit loses it: recount 0, mse = 0 / 0, finite T
    r = results["offset_1e+06"]
    assert r["best_iteration"] >= 0, "no hypothesis reached a consensus of 3: the refit never ran"
    assert r["consensus"] == 0 and np.isnan(r["mse"]) and np.isfinite(r["T"]).all() and not np.array_equal(r["T"], np.eye(3, 4))
    assert not r["mask"].any()
    # 2^-66: the float covariance is denormal (and not zero); 2^-20: it is normal
    c = BY_NAME["scale_2^-66"]
    cov = np.abs(_cov32(c.P, c.Q))
    assert 0 < cov.max() < FLT_MIN
    assert np.abs(_cov32(BY_NAME["scale_2^-20"].P, BY_NAME["scale_2^-20"].Q)).max() > FLT_MIN
    # 2^-1040 / 2^-1070: the coordinates are f64 denormals, and zero as floats
    for e in (-1040, -1070):
        c = BY_NAME["scale_2^%d" % e]
        a = np.abs(c.P[c.P != 0])
        assert a.max() < np.finfo(np.float64).tiny and a.min() > 0 and not c.P.astype(np.float32).any()
        assert 0 < c.max_error < np.finfo(np.float64).tiny
    # 2^63 / 2^66: the casts are finite, the covariance overflows; 2^500: the cast overflows
    with np.errstate(all="ignore"):
        for e in (63, 66):
            c = BY_NAME["scale_2^%d" % e]
            assert np.isfinite(c.P.astype(np.float32)).all() and np.isfinite(c.Q.astype(np.float32)).all()
            assert not np.isfinite(_cov32(c.P, c.Q)).all()
        c = BY_NAME["scale_2^500"]
        assert np.isinf(c.P.astype(np.float32)).all()
    c = BY_NAME["scale_2^40"]
    assert np.isfinite(_cov32(c.P, c.Q)).all()


def test_nonfinite_and_threshold_classes_reached(results):
    assert np.isnan(BY_NAME["nan_in_P"].P).sum() == 1 and np.isinf(BY_NAME["inf_in_Q"].Q).sum() == 1
    c = BY_NAME["negative_zero"]
    assert np.signbit(c.P[:, ::3]).all() and not c.P[:, ::3].any()
    # the poisoned correspondence is never an inlier, the rest of the scene still is found
    assert results["nan_in_P"]["mask"][17] == 0 and results["inf_in_Q"]["mask"][40] == 0
    assert results["nan_in_P"]["consensus"] >= 80 and results["inf_in_Q"]["consensus"] >= 80
    for t in (0.0, -1.0, np.nan):
        r = results["threshold_%r" % t]
        assert r["consensus"] == 0 and r["iterations_run"] == RC.BASE_ITERS and r["best_iteration"] == -1
    for t in (np.inf, 1e200):                      # t * t overflows: every finite distance is below it
        r = results["threshold_%r" % t]
        assert r["consensus"] == RC.BASE_M and r["iterations_run"] == 1
    for t in (5e-324, 1e-170):                     # t * t underflows to zero: only an exact zero distance is below it
        assert t * t == 0.0
        assert results["threshold_%r" % t]["consensus"] == 0


def test_break_and_iteration_classes_reached(oracle, results):
    v = _votes(oracle, BY_NAME["break_0.0"])
    assert results["break_0.0"]["iterations_run"] == int(np.nonzero(v >= 3)[0][0]) + 1 > 1
    assert results["break_1.0"]["iterations_run"] == RC.BASE_ITERS and results["break_1.5"]["iterations_run"] == RC.BASE_ITERS
    for bp, m in RC.BREAK_EDGE:
        c, r = BY_NAME["break_%r_x_%d" % (bp, m)], results["break_%r_x_%d" % (bp, m)]
        k = int(round(bp * m))
        assert k >= 3 and abs(bp * m - k) <= 2 * np.spacing(float(k))
        v = _votes(oracle, c)
        assert v.max() == k and v[0] == k            # the hypotheses count exactly the integer next to bp * M
        if float(k) > bp * m:
            assert r["iterations_run"] == 1
        else:
            assert r["iterations_run"] == c.iterations
        assert r["consensus"] == k
    # a count equal to the integer stops the loop only where the product landed below it
    assert [float(np.sign(bp * m - round(bp * m))) for bp, m in RC.BREAK_EDGE] == [0, 0, 0, 0, 1, -1]
    assert [results["break_%r_x_%d" % (bp, m)]["iterations_run"] for bp, m in RC.BREAK_EDGE] == [600, 600, 600, 600, 600, 1]
    for it in RC.ITERATIONS:                       # break percentage 0.9 on a scene with 25 % outliers: no early stop
        assert results["iterations_%d" % it]["iterations_run"] == it
    # 513 iterations: the last round holds a single hypothesis; 257 likewise
    assert results["iterations_4096"]["consensus"] >= 85


def test_path_edge_cases(results):
    for m in RC.PATH_EDGE_M:
        r = results["path_%d" % m]
        assert r["iterations_run"] == RC.PATH_ITERS and r["consensus"] >= 0.7 * m


def test_estimate_offset_pairs_collapse(oracle):
    (f0, t0), (f1, t1) = RC.estimate_offset_pairs()
    r = RC.estimate_on_oracle(oracle, f0, t0, RC.ESTIMATE_JOBS[0])
    assert f0["desc"].shape[0] == 200 and r["ok"] == 1 and r["n_corr"] >= 100 and r["best_iteration"] >= 0
    assert r["consensus"] == 0 and np.isnan(r["mse"]) and np.isfinite(r["T"]).all() and np.array_equal(r["information"], np.eye(6))
    r = RC.estimate_on_oracle(oracle, f1, t1, RC.ESTIMATE_JOBS[1])
    assert r["ok"] == 1 and r["consensus"] >= 3 and r["mse"] > 0 and r["information"][0, 0] == 0.1 * r["consensus"] / r["mse"]
