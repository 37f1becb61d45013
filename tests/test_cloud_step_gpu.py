"""GPU tests of one outer iteration of uzl_cloud_* stage by stage (steps 6-8: M_i, the 28 sums, the damped Gauss-Newton trials),
through the diagnostic library's hook uzl_debug_cloud_step, which runs the kernels uzl_cloud_estimate runs.  The restatement
(tests/cloud_reference.py, sums in the device's order) is given what the device holds - the covariances read back, j and kept of
uzl_cloud_correspondences, which tests/test_cloud_gpu.py already holds to the restatement - and every stage must equal it bit for
bit on the scenes of tests/cloud_step_scenes.py: an exact plane, collinear kept points, 1 - 6 kept correspondences, the optical
axis, a room corner far from the origin, first guesses that turn the target by 90 and 180 degrees, and the source sizes and kept
patterns at the edges of the reduction.  The hook chained m times is tied to the product library's uzl_cloud_estimate with
max_iterations = m, and gicp_epsilon's floor is checked on both sides of it."""
import numpy as np
import pytest

import cloud_reference as LR
import cloud_scenes as CS
import cloud_step_scenes as SS

pytestmark = pytest.mark.gpu

SCENES = SS.scenes()
NAMES = list(SCENES)
CASES = SS.cases()
_want = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def six(cov):
    """uzl_cloud_read's (n, 3, 3) -> the (n, 6) upper triangles the device stores"""
    return np.ascontiguousarray(cov[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]])


@pytest.fixture(scope="module")
def rig(capi):
    """a handle of the diagnostic library and one of the product library with every scene's clouds (2 k = from, 2 k + 1 = to of
    scene k), and the clouds as the device holds them: the points as given, the covariances read back"""
    d, h = capi.DiagCloud(), capi.Cloud()
    held = {}
    for k, name in enumerate(NAMES):
        s = SCENES[name]
        for side, idx in (("from", 2 * k), ("to", 2 * k + 1)):
            xyz, bgr = s["cloud_" + side]
            assert d.add_points(xyz, bgr) == idx and h.add_points(xyz, bgr) == idx
        a, b = d.read(2 * k), d.read(2 * k + 1)
        for i, c in ((2 * k, a), (2 * k + 1, b)):
            assert np.array_equal(bits(h.read(i)["cov"]), bits(c["cov"]))          # both libraries run the same kernel
            assert np.array_equal(bits(c["xyz"]), bits(s["cloud_" + ("from" if i % 2 == 0 else "to")][0]))
        held[name] = tuple(dict(xyz=c["xyz"], cov=six(c["cov"]), lab=c["lab"], n=len(c["xyz"])) for c in (a, b))
    yield d, h, held
    d.close()
    h.close()


def want(rig, case):
    """the restatement's outer iteration of a case on the device's inputs, computed once"""
    d, _, held = rig
    if case not in _want:
        name, g, t, c = case
        s, k = SCENES[name], NAMES.index(name)
        G, T = s["guesses"][g], s["poses"][t]
        j, _, kept = d.correspondences(2 * k, 2 * k + 1, G, T)
        a, b = held[name]
        _want[case] = LR.step(a, b, G, T, LR.config(**SS.CONFIGS[c]), "device", j, kept)
    return _want[case]


def test_the_restatement_reaches_every_damping_branch_on_the_devices_inputs(rig):
    """before the device is compared: over the scenes the restatement's logs hold accepted and rejected trials, a stop by
    UZL_CLOUD_INNER_EPS, a loop that runs out of inner_iterations, and the branches the CPU search found scenes for - the
    UZL_CLOUD_MU_MIN floor (second_stride) and a refused Cholesky (axis); NO_CORR is reached at the first outer iteration only"""
    seen = {}
    for case in CASES:
        w = want(rig, case)
        cfg = LR.config(**SS.CONFIGS[case[3]])
        for b in (LR.branches(w["log"], cfg) if w["status"] == LR.OK else {"no_corr"}):
            seen.setdefault(b, set()).add(case[0])
    print({k: sorted(v) for k, v in seen.items()})
    assert set(seen) == {"accepted", "rejected", "refused", "mu_floor", "inner_eps", "ran_out", "no_corr"}
    assert seen["refused"] == {"axis"} and seen["no_corr"] == {"none"} and "second_stride" in seen["mu_floor"]


@pytest.mark.parametrize("case", CASES, ids=["%s-g%d-t%d-%s" % c for c in CASES])
def test_one_outer_iteration_equals_the_restatement_bit_for_bit(capi, rig, case):
    """M, the 28 sums, the trial log entry by entry (mu, outcome, delta, f), the next T and the pair's state"""
    d, _, _ = rig
    name, g, t, c = case
    s, k = SCENES[name], NAMES.index(name)
    w = want(rig, case)
    if s["kept"] is not None:
        assert w["num_corr"] == len(s["kept"]) and np.array_equal(np.flatnonzero(w["M"].any(1)), s["kept"])
    d.set_config(**SS.CONFIGS[c])
    got = d.debug_step(2 * k, 2 * k + 1, s["guesses"][g], s["poses"][t])
    assert (got["status"], got["num_corr"]) == (w["status"], w["num_corr"])
    assert got["M"].shape == w["M"].shape and np.array_equal(bits(got["M"]), bits(w["M"])), np.flatnonzero((bits(got["M"]) != bits(w["M"])).any(1))[:8]
    assert np.array_equal(bits(got["sums"]), bits(w["sums"])), np.flatnonzero(bits(got["sums"]) != bits(w["sums"]))
    assert [e["outcome"] for e in got["log"]] == [e["outcome"] for e in w["log"]]
    for i, (x, y) in enumerate(zip(got["log"], w["log"])):
        assert bits(np.float64(x["mu"])) == bits(np.float64(y["mu"])) and bits(np.float64(x["f"])) == bits(np.float64(y["f"])), i
        assert np.array_equal(bits(x["delta"]), bits(y["delta"])), i
    assert np.array_equal(bits(got["T"]), bits(w["T"]))
    assert got["done"] == w["done"]


TIES = ["far", "plane", "line", "axis", "none", "few3", "turned_quarter", "turned_half", "all257", "second_stride"]


@pytest.mark.parametrize("name", TIES)
def test_the_hook_chained_is_the_product_estimate(capi, rig, name):
    """uzl_cloud_estimate of the product library with max_iterations = m returns the transform (byte for byte), iterations,
    num_corr_iter and status that the restatement's steps 8-10 make of the hook's T chained m times"""
    d, h, held = rig
    s, k = SCENES[name], NAMES.index(name)
    G = s["guesses"][0]
    a, b = held[name]
    for m in (1, 2, 3):
        cfg = LR.config(max_iterations=m)
        d.set_config(inner_iterations=10, max_iterations=m)
        h.set_config(max_iterations=m)
        T, hist, status = np.eye(3, 4), [], LR.OK
        for it in range(m):
            r = d.debug_step(2 * k, 2 * k + 1, G, T)
            hist.append(r["num_corr"])
            if r["status"] == LR.NO_CORR:
                status = LR.NO_CORR
                break
            stop = LR.converged(T, r["T"], cfg)
            T = r["T"]
            if stop:
                break
        w = LR.finish(T, G, status, hist, a["n"], b["n"], cfg)
        e = h.estimate([(2 * k, 2 * k + 1, G)])[0]
        assert (e["status"], e["iterations"], e["num_corr"]) == (w["status"], w["iterations"], w["num_corr"]), m
        assert e["num_corr_iter"][:len(hist)].tolist() == hist and not e["num_corr_iter"][len(hist):].any(), m
        assert e["transform"].tobytes() == np.ascontiguousarray(w["transform"]).tobytes(), m
        assert e["match_score"] == w["match_score"] and e["matching_score"] == w["matching_score"]
    h.set_config(max_iterations=20)


def test_the_hook_refuses_what_correspondences_refuses(capi, rig):
    d, h, _ = rig
    bad = np.eye(3, 4)
    bad[1, 2] = np.nan
    for args in ((0, 1, np.eye(3, 4), bad), (0, 1, bad, np.eye(3, 4)), (0, 2 * len(NAMES), np.eye(3, 4), np.eye(3, 4))):
        with pytest.raises(capi.UzlError) as e:
            d.debug_step(*args)
        assert e.value.status == capi.UZL_ERR_BAD_ARG
    with pytest.raises(capi.UzlError) as e:                   # a handle of the product library never reaches the hook
        h.debug_step(0, 1, np.eye(3, 4), np.eye(3, 4))
    assert e.value.status == capi.UZL_ERR_STATE


def test_gicp_epsilon_has_a_floor(capi):
    """1.0 - gicp_epsilon < 1.0 must hold: 2^-54 is refused at create and at set_config and leaves the handle as it was; 2^-53 is
    admitted, and the exact plane displaced by (0.02, 0.01, 0.03) then ends OK with z within 1e-6 of 0.03 (the restatement: 2.9e-8)"""
    s = SCENES["plane"]
    G = s["guesses"][0]
    assert G[:, 3].tolist() == [0.02, 0.01, 0.03]
    with pytest.raises(capi.UzlError) as e:
        capi.Cloud(gicp_epsilon=2.0 ** -54)
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    h = capi.Cloud()
    for side in ("from", "to"):
        h.add_points(*s["cloud_" + side])
    before = h.estimate([(0, 1, G)]).tobytes()
    with pytest.raises(capi.UzlError) as e:
        h.set_config(gicp_epsilon=2.0 ** -54)
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    assert h.estimate([(0, 1, G)]).tobytes() == before
    assert h.add_points(*s["cloud_from"]) == 2                 # a cloud added now still gets the covariances of the old configuration
    assert np.array_equal(bits(h.read(2)["cov"]), bits(h.read(0)["cov"]))
    h.close()
    for lib_handle in (capi.Cloud, capi.DiagCloud):
        t = lib_handle(gicp_epsilon=2.0 ** -53)
        for side in ("from", "to"):
            t.add_points(*s["cloud_" + side])
        e = t.estimate([(0, 1, G)])[0]
        T = CS.mul(G, CS.inv(e["transform"].reshape(3, 4)))   # T_final, from transform = T_final^-1 T_diff
        print("gicp_epsilon 2^-53: status %d after %d iterations, z of T %.3e from 0.03" % (e["status"], e["iterations"], abs(T[2, 3] - 0.03)))
        assert e["status"] == capi.CLOUD_OK and e["matching_score"] == 1.0 and e["iterations"] >= 2
        assert abs(T[2, 3] - 0.03) <= 1e-6
        if lib_handle is capi.DiagCloud:
            r = t.debug_step(0, 1, G, np.eye(3, 4))
            assert np.isfinite(r["M"]).all() and r["log"] and r["log"][0]["outcome"] == LR.ACCEPTED
        t.close()
