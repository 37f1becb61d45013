"""CPU tests of what tests/test_cloud_step_gpu.py holds the device to: the restatement's device-order sums, trial log and
numpy.longdouble variants (tests/cloud_reference.py) on the scenes of tests/cloud_step_scenes.py.  The device order against
numpy.sum and both against longdouble, M against longdouble, the sums as derivatives of f at degenerate geometry (the Jacobian by
finite differences of the residuals), the trial log's own consistency, the scenes' stated properties, the damping branches the
scenes reach, and the admitted gicp_epsilon below which an exact plane cannot be registered.  Nothing here involves the code
under test."""
import numpy as np
import pytest

import cloud_reference as LR
import cloud_scenes as CS
import cloud_step_scenes as SS

SCENES = SS.scenes()
CASES = SS.cases()
IDS = ["%s-g%d-t%d-%s" % c for c in CASES]
# Largest |sum in f64 - sum in numpy.longdouble| / (sum of |term| in longdouble) over the 28 sums, both orders, every case of
# cloud_step_scenes, measured here on the CPU: DESIGN.md, "Cloud registration".  The terms are computed in the type of the sum, so the
# figure holds the rounding of a term (a few units of 2^-53) and of the additions.  The f64 restatement is held to ten times it: the
# margin covers rounding, not mistakes (a wrong term is off by the size of a term).  The worst case is `plane` at the estimates that
# already lie on the answer in some direction: there the residual d = (R p + t) - q is the f32 rounding of q, 1e-9 m, left over from
# the difference of two numbers of size 1, so g's terms carry 1e-16 / 1e-9 of their own size.  Every other scene stays below
# SUMS_MEASURED_ELSEWHERE and is held to ten times that.
SUMS_MEASURED = 9.702e-10
SUMS_MEASURED_ELSEWHERE = 9.961e-15
# Likewise for M of step 6: largest |M in f64 - M in longdouble| over a row, divided by the row's largest |entry| in longdouble.
M_MEASURED = 5.670e-14
_clouds, _problems = {}, {}


def clouds(name):
    if name not in _clouds:
        s = SCENES[name]
        _clouds[name] = (LR.make_cloud(*s["cloud_from"]), LR.make_cloud(*s["cloud_to"]))
    return _clouds[name]


def problem(case):
    """(G, T, cfg, rows, p, q, M) of a case, made once"""
    if case not in _problems:
        name, g, t, c = case
        s = SCENES[name]
        a, b = clouds(name)
        G, T = s["guesses"][g], s["poses"][t]
        j, _, kept = LR.correspondences(a, b, G, T)
        rows = np.flatnonzero(kept)
        p, q = a["xyz"][rows].astype(np.float64), LR.move32(b["xyz"], G)[j[rows]].astype(np.float64)
        M = LR.mahalanobis(T, G, a["cov"][rows], b["cov"][j[rows]]) if len(rows) else np.zeros((0, 6))
        _problems[case] = (G, T, LR.config(**SS.CONFIGS[c]), rows, p, q, M, (a["cov"][rows], b["cov"][j[rows]]))
    return _problems[case]


def test_the_scenes_are_what_they_say():
    for name, s in SCENES.items():
        assert max(len(s["cloud_from"][0]), len(s["cloud_to"][0])) <= SS.MAX_POINTS
    for case in CASES:
        s = SCENES[case[0]]
        rows = problem(case)[3]
        if s["kept"] is not None:
            assert rows.tolist() == s["kept"].tolist(), case
        else:
            assert len(rows) >= 50, case
    for n in SS.SIZES:
        assert len(SCENES["all%d" % n]["kept"]) == n == len(SCENES["all%d" % n]["cloud_from"][0])
    lanes = SCENES["lanes192"]["kept"]
    assert (lanes % 256 >= 192).all() and (lanes // 256).max() == 3 and len(lanes) == 256
    assert SCENES["second_stride"]["kept"].min() == 256 and (SCENES["one_wave_few"]["kept"] // 64 == 1).all()
    assert np.array_equal(SCENES["alternate"]["kept"], np.arange(0, 513, 2))
    # plane: an exact plane, the same points on both sides; line: collinear
    P = SCENES["plane"]["cloud_from"][0]
    assert (P[:, 2] == 1.5).all() and np.array_equal(P, SCENES["plane"]["cloud_to"][0])
    L = SCENES["line"]["cloud_from"][0][SCENES["line"]["kept"]].astype(np.float64)
    assert np.linalg.svd(L - L.mean(0), compute_uv=False)[1] < 1e-15
    # far: about (3, -2, 4.5); turned: the first guesses turn by 90 and 180 degrees, the estimate by 30
    assert np.abs(SCENES["far"]["cloud_from"][0].mean(0) - [3, -2, 4.5]).max() < 0.4
    for name, deg in (("turned_quarter", 90.0), ("turned_half", 180.0)):
        G = SCENES[name]["guesses"][0]
        assert abs(np.degrees(np.arccos(np.clip((np.trace(G[:, :3] @ SCENES["turned_quarter"]["true"][:, :3].T) - 1) / 2, -1, 1))) - deg) < 1e-6
        T = SCENES[name]["poses"][1]
        assert abs(np.degrees(np.arccos((np.trace(T[:, :3]) - 1) / 2)) - 30.0) < 1e-9


@pytest.mark.parametrize("k", [1, 2, 3, 6])
def test_few_kept_correspondences_in_the_whole_solve(k):
    """2 outer iterations, LOW_SCORE; rejected trials at 2, 3 and 6 kept, none at 1"""
    s = SCENES["few%d" % k]
    a, b = clouds("few%d" % k)
    e = LR.estimate(a, b, s["guesses"][0])
    assert (e["status"], e["iterations"], e["num_corr_iter"]) == (LR.LOW_SCORE, 2, [k, k])
    for T in s["poses"]:
        r = LR.step(a, b, s["guesses"][0], T)
        rejected = sum(x["outcome"] == LR.REJECTED for x in r["log"])
        assert (rejected == 0) if k == 1 else (rejected > 0), (k, [x["outcome"] for x in r["log"]])


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "default"], ids=[i for i, c in zip(IDS, CASES) if c[3] == "default"])
def test_sums_in_device_order_and_against_longdouble(case):
    G, T, cfg, rows, p, q, M, _ = problem(case)
    if len(rows) == 0:
        assert not LR.evaluate(T, p, q, M, "device", rows).any() and not LR.evaluate(T, p, q, M).any()
        return
    ld = np.longdouble
    exact = LR.evaluate(T, p, q, M, dtype=ld)
    scale = np.abs(LR.terms(T, p, q, M, ld)).sum(1)
    dev, plain = LR.evaluate(T, p, q, M, "device", rows), LR.evaluate(T, p, q, M)
    assert dev.dtype == plain.dtype == np.float64 and exact.dtype == ld
    # the longdouble sums in the two orders differ by the rounding of longdouble only
    assert (np.abs(LR.evaluate(T, p, q, M, "device", rows, ld) - exact) <= 2.0 ** -60 * scale).all()
    ok = scale > 0
    worst = max(float((np.abs(x - exact)[ok] / scale[ok]).max()) for x in (dev, plain))
    print("%s: sums differ from longdouble by at most %.3e of the sum of |term|" % (case, worst))
    assert worst <= 10 * (SUMS_MEASURED if case[0] == "plane" else SUMS_MEASURED_ELSEWHERE)
    assert (np.abs(dev - plain) <= 2 * 10 * SUMS_MEASURED * scale).all()       # each is within 10 SUMS_MEASURED of longdouble
    # a sum whose terms are all zero is an exact zero in every order (H[2][2] of `axis`)
    assert not dev[~ok].any() and not plain[~ok].any()


def test_device_order_on_known_patterns():
    """the device order by a scalar loop, lane by lane, on rows that exercise each level: strips, the butterfly, the four waves"""
    rng = np.random.default_rng(5)
    for rows in (np.arange(5), np.arange(64, 70), np.array([0, 255, 256, 511, 512]), np.arange(0, 700, 3), np.arange(300, 1025)):
        t = rng.normal(size=(3, len(rows))) * 10.0 ** rng.integers(-8, 8, (3, len(rows)))
        got = LR.device_sum(t, rows)
        for k in range(3):
            lane = [0.0] * 256
            for v, i in zip(t[k], rows):
                lane[i % 256] = lane[i % 256] + float(v)
            waves = []
            for w in range(4):
                v = lane[64 * w:64 * w + 64]
                off = 32
                while off >= 1:
                    v = [v[i] + v[i ^ off] for i in range(64)]
                    off //= 2
                assert len(set(v)) == 1                        # every lane of a wave ends with the same bits
                waves.append(v[0])
            assert got[k] == (waves[0] + waves[1]) + (waves[2] + waves[3])
    assert LR.device_sum(np.zeros((2, 0)), np.zeros(0, np.int64)).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "default"], ids=[i for i, c in zip(IDS, CASES) if c[3] == "default"])
def test_mahalanobis_against_longdouble(case):
    G, T, cfg, rows, p, q, M, (c1, c2) = problem(case)
    if len(rows) == 0:
        return
    exact = LR.mahalanobis(T, G, c1, c2, np.longdouble)
    assert exact.dtype == np.longdouble and M.dtype == np.float64
    worst = float((np.abs(M - exact).max(1) / np.abs(exact).max(1)).max())
    print("%s: M differs from longdouble by at most %.3e of a row's largest entry" % (case, worst))
    assert worst <= 10 * M_MEASURED
    # and it is the inverse it is said to be
    S = T[:, :3] @ LR.full(c1) @ T[:, :3].T + G[:, :3] @ LR.full(c2) @ G[:, :3].T
    assert np.abs(LR.full(M) @ S - np.eye(3)).max() < 1e-9


def hessian(S):
    H = np.zeros((6, 6))
    H[np.triu_indices(3)] = S[:6]
    H[:3, 3:] = S[6:15].reshape(3, 3)
    H[3:, 3:][np.triu_indices(3)] = S[15:21]
    return np.triu(H) + np.triu(H, 1).T


DERIVATIVE_CASES = [c for c in CASES if c[3] == "default" and (c[0] == "plane" or c[0].startswith("few") or c[0].startswith("turned"))]


@pytest.mark.parametrize("case", DERIVATIVE_CASES, ids=["%s-g%d-t%d-%s" % c for c in DERIVATIVE_CASES])
def test_the_sums_are_the_derivatives_of_f_at_degenerate_geometry(case):
    """tests/test_cloud_reference.py::test_the_sums_are_the_derivatives_of_f on `plane`, `few` and `turned`: g against central
    differences of f, H against sum J^T M J with J the central differences of the residuals under T <- [dR(w) | v] T"""
    G, T, cfg, rows, p, q, M, _ = problem(case)
    for order in ("numpy", "device"):
        S = LR.evaluate(T, p, q, M, order, rows)
        h = 1e-5
        E = np.eye(6)
        f = lambda d: LR.evaluate(LR.apply(T, d), p, q, M)[27]
        g = np.array([(f(h * E[k]) - f(-h * E[k])) / (2 * h) for k in range(6)])
        assert np.allclose(g, 2 * S[21:27], rtol=1e-5, atol=1e-6 * max(np.abs(S[21:27]).max(), np.abs(S[15:21]).max() * 1e-3)), case

        def residuals(d):
            Tn = LR.apply(T, d)
            return p @ Tn[:, :3].T + Tn[:, 3] - q
        J = np.stack([(residuals(h * E[k]) - residuals(-h * E[k])) / (2 * h) for k in range(6)], 2)      # (n, 3, 6)
        H = np.einsum("nak,nab,nbm->km", J, LR.full(M), J)
        assert np.allclose(H, hessian(S), rtol=0, atol=1e-7 * np.abs(H).max()), case
        d0 = residuals(np.zeros(6))
        assert np.allclose(np.einsum("nak,nab,nb->k", J, LR.full(M), d0), S[21:27], rtol=0, atol=1e-7 * np.abs(H).max() * np.abs(d0).max())
        assert np.isclose(np.einsum("na,nab,nb->", d0, LR.full(M), d0), S[27], rtol=1e-12)
        # the damped system is the one solved
        d = LR.solve(S, LR.MU0)
        A = hessian(S) + LR.MU0 * np.diag(np.diag(hessian(S)))
        assert np.abs(A @ d + S[21:27]).max() <= 1e-9 * np.abs(A).max() * np.abs(d).max()


def test_the_undamped_hessian_is_singular_where_the_geometry_says_so():
    for name, rank in (("few1", 3), ("few2", 5), ("line", 5)):
        case = next(c for c in CASES if c[0] == name)
        G, T, cfg, rows, p, q, M, _ = problem(case)
        H = hessian(LR.evaluate(T, p, q, M, "device", rows))
        w = np.linalg.eigvalsh(H)
        assert (w > 1e-9 * w[-1]).sum() == rank, (name, w)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_trial_log_is_consistent(case):
    G, T, cfg, rows, p, q, M, _ = problem(case)
    if len(rows) == 0:
        return
    for order in ("numpy", "device"):
        log = []
        with np.errstate(all="ignore"):
            Tn = LR.inner(T, p, q, M, cfg, log, order, rows)
            f = LR.evaluate(T, p, q, M, order, rows)[27]
        assert 1 <= len(log) <= cfg["inner_iterations"]
        mu, Tc = LR.MU0, np.asarray(T, np.float64)
        for e in log:
            assert e["mu"] == mu
            if e["outcome"] == LR.ACCEPTED:
                assert e["f"] <= f
                f, Tc, mu = e["f"], LR.apply(Tc, e["delta"]), max(mu / 10.0, LR.MU_MIN)
            else:
                assert (e["f"] > f) if e["outcome"] == LR.REJECTED else (e["f"] == 0.0 and not e["delta"].any())
                mu = mu * 10.0
        assert np.array_equal(Tc, Tn)                          # only accepted trials change T
        assert LR.branches(log, cfg)
        # without a log and in the default call the result is the same
        if order == "numpy":
            with np.errstate(all="ignore"):
                assert np.array_equal(LR.inner(T, p, q, M, cfg), Tn)


def test_step_is_estimate_one_iteration_at_a_time():
    """cloud_reference.step chained, with the default order of the sums, walks through estimate's outer iterations"""
    for name in ("far", "few3", "plane"):
        s = SCENES[name]
        a, b = clouds(name)
        G = s["guesses"][0]
        want = LR.estimate(a, b, G)
        T, hist = np.eye(3, 4), []
        for it in range(20):
            r = LR.step(a, b, G, T, order="numpy")
            hist.append(r["num_corr"])
            stop = LR.converged(T, r["T"])
            assert r["done"] == int(stop)
            T = r["T"]
            if stop:
                break
        got = LR.finish(T, G, LR.OK, hist, a["n"], b["n"])
        assert got["num_corr_iter"] == want["num_corr_iter"] and got["status"] == want["status"] and got["iterations"] == want["iterations"]
        assert np.array_equal(got["transform"], want["transform"])


def test_the_damping_branches_the_scenes_reach():
    """DESIGN.md, "Cloud registration": every way through step 7's loop is reached by a scene, and by which"""
    seen = {}
    for case in CASES:
        G, T, cfg, rows, p, q, M, _ = problem(case)
        if len(rows) == 0:
            seen.setdefault("no_corr", []).append(case[0])
            continue
        log = []
        with np.errstate(all="ignore"):
            LR.inner(T, p, q, M, cfg, log, "device", rows)
        for b in LR.branches(log, cfg):
            seen.setdefault(b, []).append(case[0])
    print({k: sorted(set(v)) for k, v in seen.items()})
    assert set(seen) == {"accepted", "rejected", "refused", "mu_floor", "inner_eps", "ran_out", "no_corr"}
    assert set(seen["refused"]) == {"axis"}                   # the optical axis: H[2][2] is an exact 0 (cloud_step_scenes.axis)
    assert "second_stride" in seen["mu_floor"] and "plane" in seen["inner_eps"] and "few3" in seen["ran_out"]


def test_an_exact_plane_needs_one_minus_epsilon_below_one():
    """the restatement at gicp_epsilon = 2^-54 (1.0 - eps == 1.0, which uzl_cloud_create now refuses): C = I - n n^T has an exact
    zero, M is not finite, every trial is refused and the pair ends OK at the unmoved pose; at 2^-53 it converges"""
    s = SCENES["plane"]
    G = s["guesses"][0]
    out = {}
    for e in (2.0 ** -54, 2.0 ** -53, 2.0 ** -52):
        cfg = LR.config(gicp_epsilon=e)
        with np.errstate(all="ignore"):
            a, b = LR.make_cloud(*s["cloud_from"], cfg), LR.make_cloud(*s["cloud_to"], cfg)
            out[e] = (LR.estimate(a, b, G, cfg), LR.step(a, b, G, np.eye(3, 4), cfg))
    bad, first = out[2.0 ** -54]
    assert not (1.0 - 2.0 ** -54 < 1.0) and 1.0 - 2.0 ** -53 < 1.0
    assert (bad["status"], bad["iterations"], bad["matching_score"]) == (LR.OK, 1, 1.0) and np.array_equal(bad["T"], np.eye(3, 4))
    assert [x["outcome"] for x in first["log"]] == [LR.REFUSED] * 10 and not np.isfinite(first["M"]).all()
    for e in (2.0 ** -53, 2.0 ** -52):
        good = out[e][0]
        print("gicp_epsilon %.3e: z of T %.3e from 0.03" % (e, abs(good["T"][2, 3] - 0.03)))
        assert good["status"] == LR.OK and abs(good["T"][2, 3] - 0.03) < 1e-6
