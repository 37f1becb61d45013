"""Deterministic inputs for the estimator's RANSAC core (stages M6-M9) at degenerate geometry, extreme position / scale,
non-finite operands, exceptional thresholds and break percentages, and stops at the edges of the 256-hypothesis rounds.
Plain NumPy, fixed seeds.  tests/test_ransac_cases_cpu.py proves on the oracle alone that every case reaches the class it
is named after; tests/test_ransac_geometry_gpu.py runs them on the device.

A case is (name, P, Q, max_error, iterations, break_percentage, do_prosac, job_id) with P, Q of shape (3, M)."""
import hashlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name P Q max_error iterations break_percentage do_prosac job_id")

SEED = 777                    # the handle's seed (Match(seed=...)) and the oracle's

# base scene: 120 points in [-2, 2]^3, ~0.3 rad, 4 mm noise, 25 % outliers, threshold 0.05.  600 hypotheses = two full rounds of
# 256 and one of 88; at a break percentage of 0.9 a scene with 25 % outliers never stops early, so every vote counts for the maximum
BASE_M, BASE_THR, BASE_ITERS, BASE_BP = 120, 0.05, 600, 0.9
NOISE, OUTLIER_FRAC = 0.004, 0.25
ROTVEC = np.array([0.1, -0.2, 0.2])                     # |.| = 0.3 rad
TRANS = np.array([0.3, -0.1, 0.2])

# the LDS tile of estimate_kernel: 4 sort keys + one vote per iteration (padded to 4) + 57 bytes per point, points padded to even,
# within 152 KiB (uzl_match.hip: kLdsBudget, estimate_lds_bytes)
LDS_BUDGET = 152 * 1024


def lds_max_points(iterations):
    """Largest problem of a ransac_points call that still keeps every problem of the call in the LDS tile."""
    n = (LDS_BUDGET - 16 - 4 * ((iterations + 3) & ~3)) // 57
    n &= ~1
    while ((16 + 4 * ((iterations + 3) & ~3) + 57 * n + 15) & ~15) > LDS_BUDGET:
        n -= 2
    return n


def rot(v):
    """Rodrigues."""
    v = np.asarray(v, float)
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def scene(m=BASE_M, seed=0, noise=NOISE, outlier_frac=OUTLIER_FRAC, P=None):
    """(P, Q, outlier flags): Q = R P + t + noise, a fixed fraction of the correspondences displaced by ~1 m."""
    rng = np.random.default_rng(1000 + seed)
    if P is None:
        P = rng.uniform(-2, 2, (3, m))
    m = P.shape[1]
    Q = rot(ROTVEC) @ P + TRANS[:, None] + rng.normal(0, noise, (3, m))
    out = np.zeros(m, bool)
    n_out = int(outlier_frac * m)
    if n_out:
        out[rng.permutation(m)[:n_out]] = True
        Q[:, out] += rng.normal(0, 1.0, (3, n_out))
    return P, Q, out


def _case(name, P, Q, thr=BASE_THR, iters=BASE_ITERS, bp=BASE_BP, prosac=True, job=0):
    return Case(name, np.ascontiguousarray(P, np.float64), np.ascontiguousarray(Q, np.float64), float(thr), int(iters), float(bp),
                bool(prosac), int(job))


# ------------------------------------------------------------------------------------------------ geometry
def geometry_cases():
    out = []
    P, Q, _ = scene(seed=1)
    out.append(_case("base", P, Q, job=1))
    # coplanar: z = 0 before the motion; a quarter of the points displaced
    rng = np.random.default_rng(2)
    Pp = rng.uniform(-2, 2, (3, BASE_M)); Pp[2] = 0.
    P, Q, _ = scene(seed=2, P=Pp)
    out.append(_case("coplanar", P, Q, job=2))
    # collinear, 3 mm noise: every covariance has rank 1 up to the noise
    s = np.random.default_rng(3).uniform(-2, 2, BASE_M)
    Pl = np.outer(np.array([1., 2., -1.]) / np.sqrt(6.), s)
    P, Q, _ = scene(seed=3, P=Pl, noise=0.003, outlier_frac=0.)
    out.append(_case("collinear", P, Q, bp=1.0, job=3))          # break percentage 1: all 600 rank-1 hypotheses are computed
    # ten distinct correspondences, each twelve times: most samples hold a repeated point (rank <= 1 covariance)
    P10, Q10, _ = scene(m=10, seed=4, outlier_frac=0.2)
    out.append(_case("duplicates", np.tile(P10, 12), np.tile(Q10, 12), job=4))
    # all points identical: zero covariance
    p = np.array([[0.5], [-1.25], [0.75]])
    out.append(_case("identical", np.tile(p, BASE_M), np.tile(rot(ROTVEC) @ p + TRANS[:, None], BASE_M), bp=1.0, job=5))
    # noise-free: every all-inlier hypothesis gets the same count, ties run across the rounds (the first must win)
    P, Q, _ = scene(seed=6, noise=0.)
    out.append(_case("noise_free", P, Q, job=6))
    # mirrored cloud: the least-squares orthogonal map is a reflection, the determinant fix has to act
    P, Q, _ = scene(seed=7)
    out.append(_case("mirrored", P, Q * np.array([[1.], [1.], [-1.]]), job=7))
    return out


M_EDGE = (0, 1, 2, 3, 4, 15, 16, 17, 31, 33)            # the 16-point MFMA step and its clamped tail


def m_edge_cases():
    out = []
    for m in M_EDGE:
        P, Q, _ = scene(m=m, seed=20 + m)
        out.append(_case("m_%d" % m, P, Q, job=20 + m))
    return out


# ------------------------------------------------------------------------------------------------ position and scale
OFFSETS = (1e3, 1e6, 1e9)
SCALE_EXPONENTS = (-20, -66, -1040, -1070, 40, 63, 66, 500)


def offset_cases():
    out = []
    for k, off in enumerate(OFFSETS):
        P, Q, _ = scene(seed=40 + k)
        out.append(_case("offset_%.0e" % off, P + off, Q + off, job=40 + k))
    return out


def scale_cases():
    out = []
    for k, e in enumerate(SCALE_EXPONENTS):
        P, Q, _ = scene(seed=50 + k)
        out.append(_case("scale_2^%d" % e, np.ldexp(P, e), np.ldexp(Q, e), thr=float(np.ldexp(BASE_THR, e)), job=50 + k))
    return out


def scale_exponent(case):
    return int(case.name.split("^")[1]) if case.name.startswith("scale_2^") else 0


# ------------------------------------------------------------------------------------------------ non-finite and signed
def nonfinite_cases():
    out = []
    P, Q, _ = scene(seed=60)
    P = P.copy(); P[1, 17] = np.nan
    out.append(_case("nan_in_P", P, Q, job=60))
    P, Q, _ = scene(seed=61)
    Q = Q.copy(); Q[2, 40] = np.inf
    out.append(_case("inf_in_Q", P, Q, job=61))
    P = np.random.default_rng(62).uniform(-2, 2, (3, BASE_M)); P[:, ::3] = -0.0
    P, Q, _ = scene(seed=62, P=P)
    out.append(_case("negative_zero", P, Q, job=62))
    return out


# ------------------------------------------------------------------------------------------------ thresholds
THRESHOLDS = (0.0, -1.0, np.inf, np.nan, 5e-324, 1e-170, 1e200)


def threshold_cases():
    P, Q, _ = scene(seed=1)
    return [_case("threshold_%r" % t, P, Q, thr=t, job=70 + k) for k, t in enumerate(THRESHOLDS)]


# ------------------------------------------------------------------------------------------------ break percentage
BREAK_PCTS = (0.0, 1.0, 1.5)
# break_pct * M next to an integer.  The first four products round to the integer itself in float64 (3.0, 3.0, 7.0, 3.0), though none of
# the factors is exact; 7 / 25 * 25 = 7.000000000000001 and 13 / 23 * 23 = 12.999999999999998 land one ulp above and below
BREAK_EDGE = ((0.6, 5), (0.1, 30), (0.7, 10), (0.3, 10), (7 / 25, 25), (13 / 23, 23))


def break_edge_scene(bp, m, seed):
    """round(bp * M) exact correspondences first (PROSAC's first prefix), the rest far away: the all-inlier hypotheses count
    exactly round(bp * M), so whether they stop the loop is decided by the last bit of bp * M."""
    k = int(round(bp * m))
    rng = np.random.default_rng(seed)
    P = rng.uniform(-2, 2, (3, m))
    Q = rot(ROTVEC) @ P + TRANS[:, None]
    Q[:, k:] += rng.uniform(5, 9, (3, m - k))
    return P, Q, k


def break_cases():
    P, Q, _ = scene(seed=1)
    out = [_case("break_%r" % bp, P, Q, bp=bp, job=80 + k) for k, bp in enumerate(BREAK_PCTS)]
    for k, (bp, m) in enumerate(BREAK_EDGE):
        Pe, Qe, _ = break_edge_scene(bp, m, 90 + k)
        out.append(_case("break_%r_x_%d" % (bp, m), Pe, Qe, bp=bp, job=90 + k))
    return out


# ------------------------------------------------------------------------------------------------ iterations
ITERATIONS = (1, 2, 255, 256, 257, 513, 4096)


def iteration_cases():
    P, Q, _ = scene(seed=1)
    return [_case("iterations_%d" % it, P, Q, iters=it, job=100 + k) for k, it in enumerate(ITERATIONS)]


# ------------------------------------------------------------------------------------------------ steered stops
STEER_M, STEER_BP = 200, 0.05


def steered_scene(j0):
    """200 correspondences whose inliers occupy only the tail j0..M of the list: PROSAC's growing prefix reaches them late."""
    rng = np.random.default_rng(7000 + j0)
    P = rng.uniform(-2, 2, (3, STEER_M))
    Q = rot(ROTVEC) @ P + TRANS[:, None] + rng.normal(0, NOISE, (3, STEER_M))
    Q[:, :j0] += rng.uniform(3, 6, (3, j0)) * rng.choice([-1., 1.], (3, j0))
    return P, Q


# (iterations, the oracle's iterations_run, j0, job_id): found by search_steered() below, a CPU search over the oracle
STEERED = (
    (600, 255, 56, 104),
    (600, 256, 56, 15),
    (600, 257, 57, 53),
    (600, 258, 57, 86),
    (600, 512, 142, 117),
    (257, 256, 171, 109),
    (257, 93, 50, 0),          # the same run length, stopped inside the first round
    (513, 512, 171, 1169),
    (513, 46, 10, 0),          # the same run length, stopped inside the first round
)


def search_steered(oracle, max_jobs=4000):
    """Finds STEERED: for each (iterations, wanted iterations_run) the first (j0, job_id) at which the oracle stops there."""
    wanted = [(600, 255), (600, 256), (600, 257), (600, 258), (600, 512), (257, 256), (257, 100), (513, 512), (513, 100)]
    found = []
    for iters, want in wanted:
        hit = None
        # the inliers must be inside the prefix ceil((i + 3) / iterations * M) shortly before the wanted stop
        n_at = int(np.ceil((want + 2.) / iters * STEER_M))
        for j0 in (max(n_at - 30, 3), max(n_at - 40, 3), max(n_at - 20, 3)):
            P, Q = steered_scene(j0)
            for job in range(max_jobs):
                r = oracle.prosac(P, Q, BASE_THR, iters, STEER_BP, True, seed=SEED, job_id=job)
                ok = r["iterations_run"] == want if want not in (100,) else 3 < r["iterations_run"] < 256
                if ok and r["iterations_run"] < iters:
                    hit = (iters, r["iterations_run"], j0, job)
                    break
            if hit:
                break
        found.append(hit)
    return found


def steered_cases():
    out = []
    for iters, want, j0, job in STEERED:
        P, Q = steered_scene(j0)
        out.append(_case("steered_%d_of_%d" % (want, iters), P, Q, iters=iters, bp=STEER_BP, job=job))
    return out


# ------------------------------------------------------------------------------------------------ LDS tile / HBM scratch edge
PATH_EDGE_M = (2716, 2717, 2718)
PATH_ITERS = 200


def path_scene():
    return scene(m=max(PATH_EDGE_M), seed=110)[:2]


def path_cases():
    P, Q = path_scene()
    return [_case("path_%d" % m, P[:, :m], Q[:, :m], iters=PATH_ITERS, prosac=False, job=110 + k) for k, m in enumerate(PATH_EDGE_M)]


def odd_stride_case():
    """The base scene as the second problem of a call whose first has 2717 points: HBM scratch with an odd row stride, so the second
    problem's distance row starts at an address that is a multiple of 8 and not of 16."""
    P, Q, _ = scene(seed=1)
    return _case("odd_stride_second", P, Q, iters=PATH_ITERS, prosac=False, job=120)


def filler(iterations, hbm):
    """The problem that decides where a ransac_points call keeps its points: the largest that fits the LDS tile at this iteration
    count, or (hbm) the next even size up, which moves every problem of the call to HBM scratch."""
    n = lds_max_points(iterations) + (2 if hbm else 0)
    rng = np.random.default_rng(4242)
    P = rng.uniform(-2, 2, (3, n))
    return P, rot(ROTVEC) @ P + TRANS[:, None]


# ------------------------------------------------------------------------------------------------ the whole estimator at 1e6
ESTIMATE_CFG = dict(ransac_threshold=BASE_THR, ransac_iteration=BASE_ITERS, ransac_break_percentage=BASE_BP, do_prosac=1, seed=SEED)
ESTIMATE_JOBS = (7, 8)


def estimate_offset_pairs():
    """Two node pairs of 200 keypoints whose positions carry an offset of 1e6: in the first the float refit loses the whole
    consensus (recount 0, mse = 0 / 0), in the second a part of it."""
    from uzliti_slam_amd import synth
    out = []
    for seed in (300, 302):
        (f, t, _), = synth.make_pairs(1, n_kp=200, seed=seed, sigma=NOISE)
        out.append((dict(f, pos=f["pos"] + 1e6), dict(t, pos=t["pos"] + 1e6)))
    return out


def estimate_on_oracle(oracle, f, t, job_id):
    return oracle.estimate_edge([f], [t], ransac_threshold=BASE_THR, ransac_iteration=BASE_ITERS, break_percentage=BASE_BP,
                                do_prosac=True, seed=SEED, job_id=job_id)


CLASSES = dict(geometry=geometry_cases, m_edge=m_edge_cases, offset=offset_cases, scale=scale_cases, nonfinite=nonfinite_cases,
               threshold=threshold_cases, break_pct=break_cases, iterations=iteration_cases, steered=steered_cases, path_edge=path_cases)
CLASSES["odd_stride"] = lambda: [odd_stride_case()]
SMALL_CLASSES = tuple(k for k in CLASSES if k not in ("path_edge", "odd_stride"))


def all_cases():
    return [c for f in CLASSES.values() for c in f()]


# ------------------------------------------------------------------------------------------------ comparison
FIELDS = ("T", "consensus", "iterations_run", "mask", "mse")


def canonical(r):
    """The compared fields as bytes.  A NaN equals a NaN whatever its sign and payload; nothing else is relaxed (-0.0 != +0.0)."""
    T = np.array(r["T"], np.float64).reshape(12).copy()
    T[np.isnan(T)] = np.nan
    mse = np.array([r["mse"]], np.float64)
    mse[np.isnan(mse)] = np.nan
    return b"".join([T.tobytes(), np.array([r["consensus"], r["iterations_run"]], np.int64).tobytes(),
                     np.ascontiguousarray(r["mask"], np.uint8).tobytes(), mse.tobytes()])


def digest(r):
    return hashlib.sha256(canonical(r)).hexdigest()


def differing_fields(got, want):
    bad = []
    for f in FIELDS:
        a = np.asarray(got[f], np.float64 if f in ("T", "mse") else np.int64).reshape(-1)
        b = np.asarray(want[f], a.dtype).reshape(-1)
        if a.shape != b.shape:
            bad.append(f)
        elif a.dtype == np.float64:
            a = a.copy(); b = b.copy()
            a[np.isnan(a)] = np.nan; b[np.isnan(b)] = np.nan
            if a.tobytes() != b.tobytes():
                bad.append(f)
        elif not np.array_equal(a, b):
            bad.append(f)
    return bad


def run_on_device(matcher, case, hbm):
    """One ransac_points call: the case next to the filler that fixes the placement.  Returns the case's result."""
    return matcher.ransac_points([(case.P, case.Q), filler(case.iterations, hbm)], case.max_error, case.iterations,
                                 case.break_percentage, do_prosac=case.do_prosac, job_ids=[case.job_id, 900])[0]


def run_path_case(matcher, case):
    """A path-edge case alone: its own size decides the placement."""
    return matcher.ransac_points([(case.P, case.Q)], case.max_error, case.iterations, case.break_percentage,
                                 do_prosac=case.do_prosac, job_ids=[case.job_id])[0]


def device_results(matcher):
    """{(case name, 'lds' | 'hbm'): result} for every case; the path-edge cases run alone under the placement their size gives."""
    out = {}
    for cls in SMALL_CLASSES:
        for c in CLASSES[cls]():
            out[c.name, "lds"] = run_on_device(matcher, c, False)
            out[c.name, "hbm"] = run_on_device(matcher, c, True)
    for c in path_cases():
        out[c.name, "lds" if c.P.shape[1] <= lds_max_points(c.iterations) else "hbm"] = run_path_case(matcher, c)
    c, big = odd_stride_case(), path_cases()[1]
    out[c.name, "hbm"] = matcher.ransac_points([(big.P, big.Q), (c.P, c.Q)], c.max_error, c.iterations, c.break_percentage,
                                               do_prosac=c.do_prosac, job_ids=[big.job_id, c.job_id])[1]
    return out


def device_digests(matcher):
    return {"%s/%s" % k: digest(r) for k, r in device_results(matcher).items()}


def run_on_oracle(oracle, case):
    return oracle.prosac(case.P, case.Q, case.max_error, case.iterations, case.break_percentage, case.do_prosac, seed=SEED,
                         job_id=case.job_id)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle as O
    O.build()
    for row in search_steered(O):
        print("    %r," % (row,))
