"""CPU tests (no GPU) of tests/laser_reference.py, the NumPy restatement that pins the laser scan matching contract: it recovers
the true pose of every scene, its closed-form step is the constrained minimum, its doubles and trim equal a sequential version,
and its information block has the contract's trace, symmetry and placement."""
import math

import numpy as np
import pytest

import laser_reference as LR
import laser_scenes as LS

SCENES = LS.scenes()
CONVERGING = [n for n, s in SCENES.items() if s["n"] >= 37]
# Measured worst case of the restatement over CONVERGING x GUESSES (closet37, guess 1): 2.62e-4 m, 3.15e-4 rad - the last step
# below epsilon_xy / epsilon_theta ends the iteration, not a floor of the arithmetic (most cases end below 1e-5).  Asserted with a
# factor of two, which also covers libm differences between hosts.
BOUND_M, BOUND_RAD = 2 * 2.62e-4, 2 * 3.15e-4


def pose_error(r, true):
    x = r["x"]
    return math.hypot(x[0] - true[0], x[1] - true[1]), abs(math.atan2(math.sin(r["theta"] - true[2]), math.cos(r["theta"] - true[2])))


@pytest.mark.parametrize("guess", range(len(LS.GUESSES)))
@pytest.mark.parametrize("name", CONVERGING)
def test_recovers_the_true_pose(name, guess):
    """steps 1-10 from a first guess up to 0.3 m and 10 degrees off (measured worst case: 2.62e-4 m, 3.15e-4 rad; bound: twice that)"""
    s = SCENES[name]
    r = LR.estimate(s["scan_from"], s["scan_to"], LS.displaced(s["true"], *LS.GUESSES[guess]))
    et, er = pose_error(r, s["true"])
    print(name, guess, r["status"], r["iterations"], r["nvalid"], "%.3e m %.3e rad" % (et, er))
    assert r["status"] == LR.OK and r["matching_score"] == r["nvalid"] > 0.25 * r["scan_valid"]
    assert 1 <= r["iterations"] <= 10 and r["deg_count"] > 0
    assert et < BOUND_M and er < BOUND_RAD


def test_all_scenes_are_there():
    assert set(SCENES) == {"room", "corridor", "room_invalid", "closet37", "room8"}
    assert [SCENES[n]["n"] for n in ("room", "closet37", "room8")] == [720, 37, 8]
    v = LR.points(SCENES["room_invalid"]["scan_to"])[1]
    assert abs((~v).mean() - 0.30) < 0.01
    assert not LR.points(LS.empty_scan())[1].any()


def random_terms(rng, k, noise):
    """k random correspondences around a random true (t, theta): a, b, w of step 6"""
    th = rng.uniform(-math.pi, math.pi)
    t = rng.uniform(-1, 1, 2)
    R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    p = rng.uniform(-5, 5, (k, 2))
    q = p @ R.T + t + rng.normal(0, noise, (k, 2))
    ang = rng.uniform(0, 2 * math.pi, k)
    n = np.stack([np.cos(ang), np.sin(ang)], 1)
    a = np.stack([n[:, 0], n[:, 1], n[:, 0] * p[:, 0] + n[:, 1] * p[:, 1], n[:, 1] * p[:, 0] - n[:, 0] * p[:, 1]], 1)
    b = (n * q).sum(1)
    w = 1.0 / (np.linalg.norm(p, axis=1) ** 2 + 0.01)
    return a, b, w, (t[0], t[1], th)


@pytest.mark.parametrize("seed,k,noise", [(1, 200, 0.0), (2, 50, 0.05), (3, 12, 0.5), (4, 400, 2.0), (5, 4, 0.2)])
def test_step6_is_the_constrained_minimum(seed, k, noise):
    """step 6 against a dense search: cost(closed form) <= cost at 10^5 sampled (t, theta) - half of them over the whole range, half
    around the solution at scales 1e-3 .. 1e-1 - and |c^2 + s^2 - 1| < 1e-12"""
    rng = np.random.RandomState(seed)
    a, b, w, _ = random_terms(rng, k, noise)
    M, v, wbb = LR.sums(a, b, w)
    x = LR.solve(M, v)
    assert x is not None
    assert abs(x[2] * x[2] + x[3] * x[3] - 1.0) < 1e-12

    def costs(X):
        e = X @ a.T - b
        return (w * e * e).sum(1)

    best = costs(np.array([x]))[0]
    th0 = math.atan2(x[3], x[2])
    n = 50000
    tg = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)], 1)
    thg = rng.uniform(-math.pi, math.pi, n)
    scale = 10.0 ** rng.uniform(-3, -1, n)
    tl = np.array(x[:2]) + rng.normal(0, 1, (n, 2)) * scale[:, None]
    thl = th0 + rng.normal(0, 1, n) * scale
    lowest = math.inf
    for t, th in ((tg, thg), (tl, thl)):
        for i in range(0, n, 10000):
            X = np.concatenate([t[i:i + 10000], np.cos(th[i:i + 10000])[:, None], np.sin(th[i:i + 10000])[:, None]], 1)
            lowest = min(lowest, costs(X).min())
    assert best <= lowest
    assert abs(LR.cost(M, v, wbb, x) - best) <= 1e-9 * max(wbb, 1.0)


def sequential_doubles_and_trim(Q, W, j1, j2, cfg):
    """steps 3-4 one correspondence at a time, from step 2's j1 / j2"""
    nt = len(j1)
    d2 = [None] * nt
    for i in range(nt):
        if j1[i] >= 0:
            dx, dy = W[i, 0] - Q[j1[i], 0], W[i, 1] - Q[j1[i], 1]
            d2[i] = dx * dx + dy * dy
    left = []
    for i in range(nt):
        if j1[i] < 0:
            continue
        if any(j1[o] == j1[i] and d2[o] < d2[i] for o in range(nt) if o != i and j1[o] >= 0):
            continue
        left.append(i)
    d = {}
    for i in left:
        lx, ly = Q[j2[i], 0] - Q[j1[i], 0], Q[j2[i], 1] - Q[j1[i], 1]
        length = math.sqrt(lx * lx + ly * ly)
        nx, ny = -ly / length, lx / length
        d[i] = abs(nx * (W[i, 0] - Q[j1[i], 0]) + ny * (W[i, 1] - Q[j1[i], 1]))
    k = len(left)
    srt = sorted(d.values())
    valid = np.zeros(nt, np.int32); dist = np.zeros(nt)
    if k:
        l1 = srt[min(max(int(math.floor(k * cfg["outliers_max_perc"])), 0), k - 1)]
        l2 = cfg["outliers_adaptive_mult"] * srt[min(max(int(math.floor(k * cfg["outliers_adaptive_order"])), 0), k - 1)]
        for i in left:
            dist[i] = d[i]
            valid[i] = 0 if d[i] > min(l1, l2) else 1
    return valid, dist


@pytest.mark.parametrize("name", ["room_invalid", "closet37", "room8", "corridor"])
def test_steps_3_and_4_against_a_sequential_version(name):
    s = SCENES[name]
    F, T = LR.points(s["scan_from"]), LR.points(s["scan_to"])
    cfg = LR.config(max_correspondence_dist=0.5 if s["n"] < 37 else 0.3)
    dropped_double = dropped_trim = 0
    for g in LS.GUESSES:
        x = LR.guess_to_x(LS.displaced(s["true"], *g))
        j1, j2, valid, dist = LR.correspondences(F, T, x, cfg)
        W = LR.moved(T[0], x)
        want_valid, want_dist = sequential_doubles_and_trim(F[0], W, j1, j2, cfg)
        assert np.array_equal(valid, want_valid) and np.array_equal(dist, want_dist)
        assert ((j1 >= 0) == (j2 >= 0)).all() and (j1[j1 >= 0] != j2[j1 >= 0]).all() and not valid[j1 < 0].any()
        dropped_double += int(((j1 >= 0) & (dist == 0) & (valid == 0)).sum())
        dropped_trim += int(((dist > 0) & (valid == 0)).sum())
    if s["n"] >= 37:
        assert dropped_double > 0 and dropped_trim > 0                  # both steps had something to do


@pytest.mark.parametrize("name", CONVERGING)
def test_step9_information(name):
    s = SCENES[name]
    cfg = LR.config(goal_trace=10000.0, other_information=100.0)
    r = LR.estimate(s["scan_from"], s["scan_to"], LS.displaced(s["true"], *LS.GUESSES[0]), cfg)
    inf3, I = r["inf3"], r["information"]
    assert abs(np.trace(inf3) - cfg["goal_trace"]) <= 1e-9 * cfg["goal_trace"]
    assert np.array_equal(inf3, inf3.T) and np.linalg.eigvalsh(inf3).min() > 0
    want = np.eye(6) * 100.0
    want[:2, :2] = inf3[:2, :2]; want[5, 5] = inf3[2, 2]
    assert np.array_equal(I, want)
    T = r["transform"]
    assert np.array_equal(T[:, 3], [r["x"][0], r["x"][1], 0]) and T[1, 0] == r["x"][3] and T[0, 0] == r["x"][2]


def test_rejections():
    """steps 5, 8 and 10 each give their status"""
    s = SCENES["room"]
    c = SCENES["corridor"]                                   # (3 m along a wall of the rectangle still leaves that wall matched)
    far = LR.estimate(c["scan_from"], c["scan_to"], LS.displaced(c["true"], 3.0, 0.0, 0.0))
    assert far["status"] == LR.FEW_CORR and far["matching_score"] == 0
    none = LR.estimate(s["scan_from"], LS.empty_scan(), LS.displaced(s["true"], 0, 0, 0))
    assert none["status"] == LR.FEW_CORR and none["scan_valid"] == 0
    tight = LR.config(max_linear_correction=0.3)
    moved = LR.estimate(s["scan_from"], s["scan_to"], LS.displaced(s["true"], *LS.GUESSES[0]), tight)
    assert moved["status"] == LR.TOO_FAR and moved["matching_score"] == 0 and moved["nvalid"] > 0
    same = LR.estimate(s["scan_from"], s["scan_from"], np.eye(3, 4))
    assert same["status"] == LR.OK and same["iterations"] == 1 and same["nvalid"] == same["scan_valid"]
    assert max(abs(same["x"][0]), abs(same["x"][1]), abs(same["theta"])) < 1e-12
