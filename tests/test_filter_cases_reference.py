"""CPU side of the edge-filter cases (filter_cases.py): every hand-made case on the oracle, on np_reference.FilterRef and on the two
in lockstep; the two formulas for the seconds between stamps; the pose chain against a long-double matrix product; and the
preconditions that the scenes of test_filter_edges_gpu.py rely on, asserted on the oracle."""
import math

import numpy as np
import pytest

import filter_cases as fc
from filter_common import assert_same_state
from np_reference import FilterRef
from ransac_cases import lds_max_points


def makers(oracle):
    ref = lambda **cfg: fc.RefFilter(oracle, **cfg)
    return {"oracle": oracle.Filter, "ref": ref, "lockstep": fc.lockstep(ref, oracle.Filter)}


@pytest.mark.parametrize("impl", ["oracle", "ref", "lockstep"])
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_case(oracle, name, impl):
    fc.CASES[name](makers(oracle)[impl], oracle)


# ---------------------------------------------------------------------------------------------------------------- time formula
def test_seconds_formulas_decide_alike_at_the_differences_the_cases_use():
    """The contract computes (double)(a - b) * 1e-9; ros::Duration::toSec() computes sec + 1e-9 * nsec.  At every difference the window
    and span cases use - exactly +-max_dt, 1 ns inside, and what the 1 s wide seed adds - both give the same verdict, and exactly
    +-max_dt and +-2 s come out as exactly that ("Edge filter")."""
    differ = []
    diffs = fc.window_differences()
    assert len(diffs) >= 24
    for d, max_dt in diffs:
        a, b = fc.contract_seconds(d), fc.ros_seconds(d)
        if (a > -max_dt, a < max_dt) != (b > -max_dt, b < max_dt):
            differ.append((d, max_dt, a, b))
        if abs(d) == int(max_dt * fc.S):
            assert abs(a) == max_dt and abs(b) == max_dt, (d, a, b)
    for d in fc.SPAN_DIFFERENCES:
        a, b = fc.contract_seconds(d), fc.ros_seconds(d)
        if (abs(a) < 2.0) != (abs(b) < 2.0):
            differ.append((d, 2.0, a, b))
    assert fc.contract_seconds(-2 * fc.S) == -2.0 and fc.ros_seconds(-2 * fc.S) == -2.0
    assert differ == []
    # the values may differ in the last place (they do, 1 ns inside a bound), only never across a limit
    assert any(fc.contract_seconds(d) != fc.ros_seconds(d) for d, _ in diffs)


# ---------------------------------------------------------------------------------------------------------------- pose chains
# Largest |FilterRef._points - long-double 4 x 4 product| over the chain scenes, relative to the sum of the magnitudes of the
# translation terms of the product, as measured on the CPU; the check holds ten times that.
CHAIN_MEASURED = 1.34e-16


def chain_errors():
    worst = 0.0
    for kind in fc.CHAIN_KINDS:
        if kind == "nan_pose":
            continue
        scn = fc.chain_scene(kind)
        r = FilterRef()
        r.set_sensors(scn["sensors"])
        for e in scn["edges"]:
            got = r._points(e)
            for g, (want, scale) in zip(got, fc.chain_longdouble(e, scn["sensors"])):
                assert scale > 0
                worst = max(worst, float(np.max(np.abs(np.array(g, np.longdouble) - want)) / scale))
    return worst


def test_pose_chain_equals_the_long_double_matrix_product():
    """The oracle, FilterRef and the kernel share one reading of :251-256; a shared mistake in the order of the five factors, or in
    the inverse, would pass every parity test.  The plain matrix product with a general inverse shares neither."""
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = chain_errors()
    print("largest relative difference: %.3e" % worst)
    assert worst <= 10 * CHAIN_MEASURED


def test_chain_scenes_reach_what_they_are_named_after(oracle):
    i32 = lambda kind: [(e["sensor_from"], e["sensor_to"]) for e in fc.chain_scene(kind)["edges"]]
    assert {2, 5} <= {i for p in i32("index_2_and_5") for i in p} and len(fc.chain_scene("index_2_and_5")["sensors"]) == 2
    assert -2 in {i for p in i32("index_minus_2") for i in p}
    assert {fc.INT32_MAX, fc.INT32_MIN} <= {i for p in i32("index_int32_extremes") for i in p}
    assert len(fc.chain_scene("no_sensors")["sensors"]) == 0 and {i for p in i32("no_sensors") for i in p} == {0, 1}
    scn = fc.chain_scene("near_half_turn")
    for m in list(scn["sensors"]) + [e[f] for e in scn["edges"] for f in ("pose_from", "displacement_from", "transform")]:
        R = np.asarray(m).reshape(3, 4)[:, :3]
        assert 0 < np.pi - np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)) < 1.5e-6
    assert {int(np.argmax(np.diag(e["pose_from"].reshape(3, 4)[:, :3]))) for e in scn["edges"]} == {0, 1, 2}       # about each axis
    assert min(np.abs(e["pose_from"].reshape(3, 4)[:, 3]).max() for e in fc.chain_scene("far")["edges"]) > 1e5
    one = fc.chain_scene("one_sided")["edges"]
    assert all(np.array_equal(e["displacement_from"], fc.I12) != np.array_equal(e["displacement_to"], fc.I12) for e in one)
    assert sum(bool(np.isnan(e["pose_from"]).any()) for e in fc.chain_scene("nan_pose")["edges"]) == 1
    # every scene is evaluated, the estimate succeeds and votes out exactly the two displaced edges; oracle and FilterRef agree in P, Q
    for kind in fc.CHAIN_KINDS:
        scn = fc.chain_scene(kind)
        o, r = oracle.Filter(**fc.CHAIN_CFG), fc.RefFilter(oracle, **fc.CHAIN_CFG)
        for f in (o, r):
            f.set_sensors(scn["sensors"])
            f.add(scn["edges"])
            assert f.calc_valid_edges() == 1
        c = o.clusters(with_eval=True)[0]
        assert_same_state([c], r.clusters(with_eval=True), tag=kind)
        out = {3, 8} | ({4} if kind == "nan_pose" else set())
        if kind != "far":           # at 1e6 m the estimator's single-precision SVD is not accurate to the threshold: its votes are the device's to match
            assert list(c["valid"]) == [0 if k in out else 1 for k in range(fc.CHAIN_N)], kind
        if kind == "nan_pose":
            assert np.isnan(c["P"][4]).any() and np.isfinite(np.delete(c["P"], 4, 0)).all() and np.isfinite(c["Q"]).all()


def test_sensor_table_replacement_changes_every_row(oracle):
    tabs, edges = fc.sensor_tables()
    o = oracle.Filter(**fc.CHAIN_CFG)
    rows = []
    for tab, lo, n in zip(tabs, (0, 12, 13), (12, 13, 14)):
        o.set_sensors(tab)
        o.add(edges[lo:n])
        assert o.calc_valid_edges() == 1
        rows.append(o.clusters(with_eval=True)[0]["P"])
        assert len(rows[-1]) == n
    assert (rows[0] != rows[1][:12]).any(1).all() and (rows[1] != rows[2][:13]).any(1).all()


# ---------------------------------------------------------------------------------------------------------------- threshold columns
THREE_FOUR_FIVE_IS_INSIDE = 0            # the side the oracle's rounding puts (0.15, 0.2, 0) on: sqrt(0.15^2 + 0.2^2) is not below 0.25


def test_threshold_columns_on_the_oracle(oracle):
    assert math.sqrt(fc.THRESHOLD * fc.THRESHOLD) == fc.THRESHOLD
    o = oracle.Filter(**fc.THRESHOLD_FAILED_CFG)
    o.add(fc.threshold_failed_edges())
    assert o.calc_valid_edges() == len(fc.THRESHOLD_OFFSETS)
    cl = dict(zip(fc.THRESHOLD_OFFSETS, o.clusters(with_eval=True)))
    for name, c in cl.items():
        assert c["ransac_consensus"] == 0 and np.array_equal(c["T"], fc.I12), name      # the estimate really fails
        assert np.array_equal(c["Q"][0] - c["P"][0], fc.THRESHOLD_OFFSETS[name]) and not c["P"][0].any(), name
        assert list(c["valid"][1:]) == [1, 0, 0]
    d = cl["at"]["Q"][0] - cl["at"]["P"][0]
    assert math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) == fc.THRESHOLD            # the error is exactly max_error
    assert [int(cl[n]["valid"][0]) for n in ("at", "below", "above")] == [0, 1, 0]     # strict <
    # 0.15^2 + 0.2^2 in the kernel's recipe: fma(dx, dx, fma(dy, dy, dz * dz)), then sqrt
    e = math.sqrt(math.fma(-0.15, -0.15, math.fma(-0.2, -0.2, 0.0))) if hasattr(math, "fma") else None
    assert int(cl["3-4-5"]["valid"][0]) == THREE_FOUR_FIVE_IS_INSIDE and (e is None or (e < fc.THRESHOLD) == bool(THREE_FOUR_FIVE_IS_INSIDE))


def test_threshold_columns_on_the_successful_path(oracle):
    o = oracle.Filter(**fc.THRESHOLD_FIT_CFG)
    o.add(fc.threshold_fit_edges())
    assert o.calc_valid_edges() == 1
    c = o.clusters(with_eval=True)[0]
    assert c["ransac_consensus"] >= 9 and list(c["valid"][:9]) == [1] * 9
    n, s = oracle.consensus3d(c["P"].T, c["Q"].T, c["T"], fc.THRESHOLD)
    assert np.array_equal(s, c["valid"]) and n == c["consensus"]


# ---------------------------------------------------------------------------------------------------------------- batch shapes
def test_batch_shapes_are_what_their_names_say(oracle):
    for total, sizes in fc.BATCH_SHAPES.items():
        assert sum(sizes) == total and set(sizes) <= {1, 2, 3, 61, 62}
        o = oracle.Filter(**fc.BATCH_CFG)
        o.add(fc.batch_edges(sizes))
        assert [c["size"] for c in o.clusters()] == list(sizes) and all(c["changed"] for c in o.clusters())
        assert o.calc_valid_edges() == len(sizes)
        cl = o.clusters(with_eval=True)
        for a, b in zip(cl, cl[1:]):                   # a first column voted under the transform next door would show
            if max(a["size"], b["size"]) < 3:          # (two clusters below three edges both get the identity)
                continue
            assert oracle.consensus3d(b["P"][:1].T, b["Q"][:1].T, a["T"], fc.BATCH_CFG["max_error"])[1][0] != b["valid"][0], (total, b["uid"])
        for c in cl:
            assert len(c["P"]) == c["size"]
            if c["size"] < 3:
                assert np.array_equal(c["T"], fc.I12) and c["ransac_consensus"] == 0 and list(c["valid"]) == [1] * c["size"]
    assert {s for sizes in fc.BATCH_SHAPES.values() for s in sizes} == {1, 2, 3, 61, 62}
    starts = lambda sizes: np.cumsum((0,) + sizes)
    assert any(a < 64 < b for sizes in fc.BATCH_SHAPES.values() for a, b in zip(starts(sizes), starts(sizes)[1:]))    # straddles column 64
    assert any(64 in starts(sizes) for sizes in fc.BATCH_SHAPES.values())                                             # and a boundary on it
    o = oracle.Filter(**fc.BATCH_CFG)
    o.add(fc.batch_edges(fc.MANY_SMALL))
    assert len(fc.MANY_SMALL) == 300 and o.calc_valid_edges() == 300


def test_large_cluster_leaves_the_lds_tile(oracle):
    assert fc.LARGE_M == lds_max_points(4096) + 1 and all(lds_max_points(i) >= lds_max_points(4096) for i in (1, 200, 1024, 4095))
    o = oracle.Filter(**fc.LARGE_CFG)
    o.add(fc.large_edges())
    assert [c["size"] for c in o.clusters()] == [fc.LARGE_M, 8, 12]
    assert o.calc_valid_edges() == 3
    c = o.clusters(with_eval=True)[0]
    assert c["consensus"] == fc.LARGE_M - len(range(0, fc.LARGE_M, 5)) and c["ransac_consensus"] == c["consensus"]
    o.add(fc.after_large_edges())
    assert o.calc_valid_edges() == 1 and [c["evaluations"] for c in o.clusters()] == [1, 1, 1, 1]
