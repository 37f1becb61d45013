"""CPU tests (no GPU) of tests/laser_reference.py, the NumPy restatement that pins the laser scan matching contract: it recovers
the true pose of every scene, its closed-form step is the constrained minimum, its nearest-neighbour search, doubles and trim equal
a sequential version, its information block has the contract's trace, symmetry and placement, and the edge scenes
(laser_scenes.edge_scenes) reach the ties, strip ends, grids and statuses the GPU tests use them for."""
import math

import numpy as np
import pytest

import laser_reference as LR
import laser_scenes as LS

SCENES = LS.scenes()
EDGES = LS.edge_scenes()
MIRRORS = ["mirror", "mirror_hole", "mirror_updown", "mirror_doubles"]
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


def stage_x(s):
    """an edge scene's stage estimate as (tx, ty, c, s)"""
    return (s["x"][0], s["x"][1], math.cos(s["x"][2]), math.sin(s["x"][2]))


@pytest.mark.parametrize("name", ["room_invalid", "closet37", "room8", "corridor"] + MIRRORS)
def test_steps_3_and_4_against_a_sequential_version(name):
    """the ray-cast scenes at every first guess; the mirror scenes (equal distances, equal minima of one j1, several at the limit)
    at their stage estimate under every trim configuration"""
    if name in MIRRORS:
        s = EDGES[name]
        runs = [(stage_x(s), LR.config(**kw)) for kw, _ in LS.MIRROR_TRIMS]
    else:
        s = SCENES[name]
        cfg = LR.config(max_correspondence_dist=0.5 if s["n"] < 37 else 0.3)
        runs = [(LR.guess_to_x(LS.displaced(s["true"], *g)), cfg) for g in LS.GUESSES]
    F, T = LR.points(s["scan_from"]), LR.points(s["scan_to"])
    dropped_double = dropped_trim = 0
    for x, cfg in runs:
        j1, j2, valid, dist = LR.correspondences(F, T, x, cfg)
        W = LR.moved(T[0], x)
        want_valid, want_dist = sequential_doubles_and_trim(F[0], W, j1, j2, cfg)
        assert np.array_equal(valid, want_valid) and np.array_equal(dist, want_dist)
        assert ((j1 >= 0) == (j2 >= 0)).all() and (j1[j1 >= 0] != j2[j1 >= 0]).all() and not valid[j1 < 0].any()
        dropped_double += int(((j1 >= 0) & (dist == 0) & (valid == 0)).sum())
        dropped_trim += int(((dist > 0) & (valid == 0)).sum())
    if s["n"] >= 37:
        assert dropped_double > 0 and dropped_trim > 0                  # both steps had something to do


def sequential_step2(F, T, x, cfg):
    """step 2 one beam at a time in Python floats -> j1, j2 (int32, -1: none) and, per beam of `to`, whether the smallest squared
    distance was reached by more than one beam of `from`, whether the beams above and below j1 were equally far, and whether the
    correspondence fell because points j1 and j2 coincide"""
    (Q, qv, _), (P, pv, _) = F, T
    tx, ty, c, s = x
    nt, nf = len(P), len(Q)
    q = [(float(Q[j, 0]), float(Q[j, 1])) if qv[j] else None for j in range(nf)]
    j1 = np.full(nt, -1, np.int32); j2 = np.full(nt, -1, np.int32)
    tie1 = np.zeros(nt, bool); tie2 = np.zeros(nt, bool); same = np.zeros(nt, bool)
    max_sq = cfg["max_correspondence_dist"] * cfg["max_correspondence_dist"]
    for i in range(nt):
        if not pv[i]:
            continue
        px, py = float(P[i, 0]), float(P[i, 1])
        wx, wy = (c * px - s * py) + tx, (s * px + c * py) + ty

        def sq(j):
            dx, dy = wx - q[j][0], wy - q[j][1]
            return dx * dx + dy * dy

        best, bd, times = -1, math.inf, 0
        for j in range(nf):
            if q[j] is None:
                continue
            d2 = sq(j)
            if d2 < bd:                                       # the first strict minimum: ties stay with the lowest index
                best, bd, times = j, d2, 1
            elif d2 == bd:
                times += 1
        if best < 0 or not bd <= max_sq:
            continue
        tie1[i] = times > 1
        up = next((j for j in range(best + 1, nf) if q[j] is not None), -1)
        down = next((j for j in range(best - 1, -1, -1) if q[j] is not None), -1)
        if up >= 0 and down >= 0:
            tie2[i] = sq(up) == sq(down)
            other = up if sq(up) <= sq(down) else down
        else:
            other = up if up >= 0 else down
        if other < 0:
            continue
        lx, ly = q[other][0] - q[best][0], q[other][1] - q[best][1]
        if not lx * lx + ly * ly > 0.0:
            same[i] = True
            continue
        j1[i], j2[i] = best, other
    return j1, j2, tie1, tie2, same


STEP2_CASES = [(n, 0) for n in MIRRORS + ["coincident", "clockwise", "reach"]] + [("room_invalid", g) for g in range(len(LS.GUESSES))]


@pytest.mark.parametrize("name,g", STEP2_CASES)
def test_step_2_against_a_sequential_version(name, g):
    if name in EDGES:
        s = EDGES[name]
        x = stage_x(s)
    else:
        s = SCENES[name]
        x = LR.guess_to_x(LS.displaced(s["true"], *LS.GUESSES[g]))
    cfg = LR.config(**s.get("cfg", {}))
    F, T = LR.points(s["scan_from"]), LR.points(s["scan_to"])
    j1, j2, _, _ = LR.correspondences(F, T, x, cfg)
    want1, want2, tie1, tie2, same = sequential_step2(F, T, x, cfg)
    assert np.array_equal(j1, want1) and np.array_equal(j2, want2)
    assert (j1 >= 0).sum() > 0
    if name == "room_invalid":
        assert (np.abs(j2 - j1)[j1 >= 0] > 1).sum() > 50 and not tie1.any() and not tie2.any()      # invalid beams are skipped; no tie
    if name == "mirror":
        assert tie2.tolist() == [i == 100 for i in range(201)] and not tie1.any()
    if name == "mirror_hole":
        assert tie1.tolist() == [i == 100 for i in range(201)]
    if name == "mirror_updown":
        assert tie2[100] and (np.abs(j2 - j1) > 1).sum() == 3
    if name == "mirror_doubles":
        assert not tie1.any() and not tie2.any()
    if name == "coincident":
        assert same.sum() == 8


def stage(name, **kw):
    s = EDGES[name]
    return LR.correspondences(s["scan_from"], s["scan_to"], stage_x(s), LR.config(**dict(s["cfg"], **kw)))


def stage_counts(j1, valid, dist):
    """(correspondences of step 2, dropped as doubles, left after step 3, left after step 4)"""
    have = j1 >= 0
    doubles = have & (dist == 0) & (valid == 0)
    return int(have.sum()), int(doubles.sum()), int((have & ~doubles).sum()), int(valid.sum())


def test_the_mirror_scenes_are_what_the_tests_need():
    """the restatement alone reaches every tie rule on them, with the counts the GPU tests rely on"""
    s = EDGES["mirror"]
    for sc in (s["scan_from"], s["scan_to"]):
        p = LR.points(sc)[0]
        assert np.array_equal(p[:100, 0], p[101:, 0][::-1]) and np.array_equal(p[:100, 1], -p[101:, 1][::-1]) and p[100, 1] == 0
    assert stage_x(s)[2:] == (1.0, 0.0)
    j1, j2, valid, dist = stage("mirror")
    assert stage_counts(j1, valid, dist) == (201, 10, 191, 154)
    d = dist[(j1 >= 0) & ~((dist == 0) & (valid == 0))]
    _, counts = np.unique(d, return_counts=True)
    assert (counts == 2).sum() == 95 and counts.max() == 2                 # 95 pairs of equal d (and the centre beam alone)
    limit = dist[valid == 1].max()
    assert (d == limit).sum() == 2 and valid[dist == limit].tolist() == [1, 1]   # d > limit with two d == limit: both kept
    assert (j1[100], j2[100]) == (100, 101)                                 # the up / down tie goes to the upper beam
    assert np.array_equal(valid, valid[::-1]) and np.array_equal(dist, dist[::-1])
    for kw, want in LS.MIRROR_TRIMS:
        j1, j2, valid, dist = stage("mirror", **kw)
        assert stage_counts(j1, valid, dist)[2:] == (191, want), kw
        assert np.array_equal(valid, valid[::-1])
    assert len(set(dist[stage("mirror", outliers_max_perc=0.0)[2] == 1])) == 1                         # the tied minimum
    # mirror_hole: beams 99 and 101 of `from` are equally near to beam 100 of `to`; the lower wins
    j1, j2, valid, dist = stage("mirror_hole")
    assert (j1[100], j2[100]) == (99, 101)                                  # (j2 skips the invalid beam 100)
    assert stage_counts(j1, valid, dist) == (201, 11, 190, 154)
    # mirror_updown: beams 98 and 102 of `from` are the neighbours of 100 and equally far; the upper wins
    j1, j2, valid, dist = stage("mirror_updown")
    assert (j1[100], j2[100]) == (100, 102) and (j1[99], j2[99]) == (98, 100) and (j1[101], j2[101]) == (102, 100)
    assert stage_counts(j1, valid, dist) == (201, 12, 189, 152)
    # mirror_doubles: beams 98, 99, 101, 102 of `to` all have j1 = 100; 99 and 101 at the same smallest distance, so both stay
    j1, j2, valid, dist = stage("mirror_doubles")
    assert j1[[98, 99, 101, 102]].tolist() == [100] * 4 and j1[100] == -1
    assert dist[99] == dist[101] and abs(dist[99] - 0.07000003) < 1e-8 and dist[98] == 0 and dist[102] == 0
    assert valid[[98, 99, 101, 102]].tolist() == [0] * 4                    # two as doubles, two by the trim
    assert stage_counts(j1, valid, dist) == (200, 14, 186, 150)
    for name, want in (("mirror", 154), ("mirror_doubles", 150)):           # one step: every integer comes from the first correspondences
        s = EDGES[name]
        r = LR.estimate(s["scan_from"], s["scan_to"], s["guess"], LR.config(max_iterations=1))
        assert (r["status"], r["iterations"], r["nvalid"], r["deg_count"]) == (LR.OK, 1, want, want)


def solved(name, **kw):
    s = EDGES[name]
    return LR.estimate(s["scan_from"], s["scan_to"], s["guess"], LR.config(**kw))


def test_the_grid_scenes_are_what_the_tests_need():
    """clockwise, zero-increment, strip-edge and equal-length grids in the restatement alone"""
    assert set(EDGES) == set(MIRRORS) | {"clockwise", "clockwise257", "coincident", "range_edges", "far64", "reach"} \
        | {"strip_%d_%d" % p for p in LS.STRIP_PAIRS} | {"grid_" + g for g in "ABCD"}
    assert max(max(s["n"], s["n_from"]) for n, s in EDGES.items() if n != "range_edges") == 513
    assert {c for p in LS.STRIP_PAIRS for c in p} == set(LS.STRIP_COUNTS)
    # clockwise: the same points as mirror's `from`, so the same correspondences with the indices reversed
    a, b = stage("mirror"), stage("clockwise")
    off = np.arange(201) != 100                               # ... but for the centre tie: the upper index is now the other point
    assert np.array_equal(b[0], 200 - a[0]) and np.array_equal(b[1][off], 200 - a[1][off]) and a[1][100] == b[1][100] == 101
    assert np.array_equal(b[2], a[2]) and np.array_equal(b[3], a[3])
    for name, deg in (("clockwise", -155), ("clockwise257", -195), ("grid_D", -195)):
        r = solved(name)
        assert (r["status"], r["deg_count"], r["matching_score"]) == (LR.VIEWPOINT, deg, 0.0) and r["nvalid"] > 0
        assert np.array_equal(r["information"], np.eye(6) * 100.0)
    # coincident: every point of a scan on one ray; a j1 whose upper neighbour is the same point gives nothing
    j1, j2, valid, dist = stage("coincident")
    assert j1.tolist() == [-1, -1, 2, -1, -1, 5, -1, -1, 8, -1, -1, 11] and j2.tolist() == [-1, -1, 3, -1, -1, 4, -1, -1, 9, -1, -1, 10]
    # reach: a squared distance equal to max_correspondence_dist^2 is kept; beam 2 is twice as far from both its neighbours
    j1, j2, valid, dist = stage("reach")
    assert j1.tolist() == [0, 1, -1, 3, 4, 5, 6, 7] and j2.tolist() == [1, 2, -1, 4, 3, 6, 7, 6] and valid.tolist() == [1, 1, 0, 1, 1, 1, 1, 1]
    assert stage("reach", max_correspondence_dist=0.2499)[2].tolist() == [0, 0, 0, 1, 0, 0, 1, 0]
    want = {(257, 255): (LR.OK, 2), (255, 257): (LR.OK, 2), (256, 256): (LR.OK, 2), (513, 64): (LR.OK, 2), (512, 63): (LR.OK, 2),
            (65, 511): (LR.FEW_MATCHES, 3), (9, 257): (LR.FEW_CORR, 0)}
    for p in LS.STRIP_PAIRS:
        s = EDGES["strip_%d_%d" % p]
        assert (s["n_from"], s["n"]) == p
        r = solved(s["name"])
        assert (r["status"], r["iterations"]) == want[p], p
    r = solved("strip_65_511")
    assert stage_counts(*[stage("strip_65_511")[k] for k in (0, 2, 3)])[1] == 436 and (r["nvalid"], r["scan_valid"]) == (53, 511)
    assert r["matching_score"] == 0 and r["information"][0, 0] != 100.0     # FEW_MATCHES carries the scaled block
    assert [solved("grid_" + g)["status"] for g in "ABCD"] == [LR.OK, LR.OK, LR.OK, LR.VIEWPOINT]
    keys = {(EDGES["grid_" + g]["scan_to"]["angle_min"], EDGES["grid_" + g]["scan_to"]["angle_increment"]) for g in "ABCD"}
    assert len(keys) == 4 and len({k[0] for k in keys}) == 3 and len({k[1] for k in keys}) == 3


def test_the_range_and_status_scenes_are_what_the_tests_need():
    s = EDGES["range_edges"]
    at = LS.RANGE_EDGE_AT
    v = s["scan_to"]["values"][at:at + 8]
    lo, hi = np.float32(LS.RANGE_MIN), np.float32(LS.RANGE_MAX)
    assert v[0] == lo and v[1] < lo and v[2] == hi and v[3] > hi and np.isposinf(v[4]) and np.isneginf(v[5])
    assert v[6] == 0 and np.signbit(v[6]) and np.isnan(v[7])
    assert float(v[1]) < LS.RANGE_MIN < float(v[0])                         # f64 range_min lies between: the comparison is in f32
    assert LR.points(s["scan_to"])[1][at:at + 8].astype(int).tolist() == LS.RANGE_EDGE_VALID
    r = solved("range_edges")
    assert (r["status"], r["scan_valid"]) == (LR.OK, 720 - 6)
    room = SCENES["room"]
    for kw, status, fields in LS.STATUS_CONFIGS:
        r = LR.estimate(room["scan_from"], room["scan_to"], LS.displaced(room["true"], *LS.GUESSES[0]), LR.config(**kw))
        assert r["status"] == getattr(LR, status), kw
        assert {k: r[k] for k in fields} == fields, kw
        assert (r["matching_score"] > 0) == (status == "OK")
        if status in ("FEW_MATCHES", "TOO_FAR"):
            assert r["nvalid"] > 0 and r["information"][0, 0] != 100.0
    # the two statuses no listed pair reaches at the defaults, for the mixed batch: TOO_FAR after convergence, DEGENERATE at once
    r = solved("far64")
    assert r["status"] == LR.TOO_FAR and abs(r["theta"] - EDGES["far64"]["true"][2]) < 1e-6 and r["iterations"] < 10
    s = SCENES["room8"]
    r = LR.estimate(s["scan_from"], s["scan_to"], LS.displaced(s["true"], *LS.GUESSES[0]))
    assert (r["status"], r["iterations"]) == (LR.DEGENERATE, 0)
    far = LR.estimate(room["scan_from"], room["scan_to"], LS.displaced(room["true"], *LS.GUESSES[0]), LR.config(max_angular_correction_deg=5.0))
    assert not LR.too_far(LS.displaced(room["true"], *LS.GUESSES[0]), far["x"], LR.config(max_angular_correction_deg=45.0))   # the angle alone


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
