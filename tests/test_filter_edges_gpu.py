"""The edge filter on the device (uzl_filter_*: uzl_filter.hip, filter_kernels.hip) at its gates, thresholds and batch edges, bit for
bit against the CPU oracle: the hand-made cases of filter_cases.py in lockstep, filter_points_kernel on pose chains with every kind
of sensor index, filter_consensus_kernel with columns at the threshold, the batch at wave and cluster boundaries and in the
estimator's HBM-scratch placement, and the C ABI's caps and refusals.  test_filter_cases_reference.py asserts on the CPU that every
scene reaches what it is named after."""
import ctypes as C

import numpy as np
import pytest

import filter_cases as fc
from filter_common import assert_same_state

pytestmark = pytest.mark.gpu


def both(capi, oracle, **cfg):
    return capi.Filter(**cfg), oracle.Filter(**cfg)


def same(g, o, tag=""):
    assert_same_state(g.clusters(with_eval=True), o.clusters(with_eval=True), with_eval=True, tag=tag)
    assert np.array_equal(g.all_edges(), o.all_edges()), tag
    assert np.array_equal(g.valid_edges(), o.valid_edges()), tag


# ---------------------------------------------------------------------------------------------------------------- host bookkeeping
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_case_in_lockstep_with_the_oracle(capi, oracle, name):
    fc.CASES[name](fc.lockstep(capi.Filter, oracle.Filter), oracle)


# ---------------------------------------------------------------------------------------------------------------- filter_points_kernel
@pytest.mark.parametrize("kind", fc.CHAIN_KINDS)
def test_pose_chains(capi, oracle, kind):
    scn = fc.chain_scene(kind)
    g, o = both(capi, oracle, **fc.CHAIN_CFG)
    for f in (g, o):
        f.set_sensors(scn["sensors"])
        f.add(scn["edges"])
        assert f.calc_valid_edges() == 1
    same(g, o, kind)
    c = g.clusters(with_eval=True)[0]
    assert len(c["P"]) == fc.CHAIN_N and c["evaluations"] == 1
    if kind == "nan_pose":
        assert np.isnan(c["P"][4]).any() and c["valid"][4] == 0 and c["valid"].sum() == fc.CHAIN_N - 3
    g.close(); o.close()


def test_sensor_table_replaced_between_evaluations(capi, oracle):
    tabs, edges = fc.sensor_tables()
    g, o = both(capi, oracle, **fc.CHAIN_CFG)
    rows = []
    for tab, lo, n in zip(tabs, (0, 12, 13), (12, 13, 14)):
        for f in (g, o):
            f.set_sensors(tab)
            f.add(edges[lo:n])
            assert f.calc_valid_edges() == 1
        same(g, o, n)
        rows.append(g.clusters(with_eval=True)[0]["P"])
    assert (rows[0] != rows[1][:12]).any(1).all() and (rows[1] != rows[2][:13]).any(1).all()      # every row follows the new table
    g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- filter_consensus_kernel
def test_threshold_columns_failed_estimate(capi, oracle):
    g, o = both(capi, oracle, **fc.THRESHOLD_FAILED_CFG)
    for f in (g, o):
        f.add(fc.threshold_failed_edges())
        assert f.calc_valid_edges() == len(fc.THRESHOLD_OFFSETS)
    same(g, o)
    cl = dict(zip(fc.THRESHOLD_OFFSETS, g.clusters(with_eval=True)))
    assert all(c["ransac_consensus"] == 0 and np.array_equal(c["T"], fc.I12) for c in cl.values())
    assert [int(cl[n]["valid"][0]) for n in ("at", "below", "above")] == [0, 1, 0]                  # strict <
    g.close(); o.close()


def test_threshold_columns_successful_estimate(capi, oracle):
    g, o = both(capi, oracle, **fc.THRESHOLD_FIT_CFG)
    for f in (g, o):
        f.add(fc.threshold_fit_edges())
        assert f.calc_valid_edges() == 1
    same(g, o)
    c = g.clusters(with_eval=True)[0]
    n, s = oracle.consensus3d(c["P"].T, c["Q"].T, c["T"], fc.THRESHOLD)
    assert c["ransac_consensus"] >= 9 and np.array_equal(s, c["valid"]) and n == c["consensus"]
    g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- batch shape
@pytest.mark.parametrize("total", sorted(fc.BATCH_SHAPES))
def test_batch_columns(capi, oracle, total):
    sizes = fc.BATCH_SHAPES[total]
    g, o = both(capi, oracle, **fc.BATCH_CFG)
    for f in (g, o):
        f.add(fc.batch_edges(sizes))
        assert f.calc_valid_edges() == len(sizes)
    same(g, o, total)
    cl = g.clusters(with_eval=True)
    assert sum(len(c["P"]) for c in cl) == total and [c["size"] for c in cl] == list(sizes)
    for c in cl:
        if c["size"] < 3:
            assert np.array_equal(c["T"], fc.I12) and c["ransac_consensus"] == 0
    g.close(); o.close()


def test_three_hundred_small_clusters_in_one_call(capi, oracle):
    g, o = both(capi, oracle, **fc.BATCH_CFG)
    es = fc.batch_edges(fc.MANY_SMALL)
    for f in (g, o):
        f.add(es)
        assert f.calc_valid_edges() == len(fc.MANY_SMALL)
    same(g, o)
    g.close(); o.close()


def test_large_cluster_in_hbm_scratch_then_a_small_batch(capi, oracle):
    g, o = both(capi, oracle, **fc.LARGE_CFG)
    for f in (g, o):
        f.add(fc.large_edges())
        assert f.calc_valid_edges() == 3
    same(g, o, "large")
    assert [c["size"] for c in g.clusters()] == [fc.LARGE_M, 8, 12]
    for f in (g, o):                                   # the buffers are larger than this batch needs and hold the last one's data
        f.add(fc.after_large_edges())
        assert f.calc_valid_edges() == 1
    same(g, o, "after")
    assert [c["evaluations"] for c in g.clusters()] == [1, 1, 1, 1]
    g.close(); o.close()


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_caps_and_refusals_of_the_c_abi(capi, oracle):
    L = capi.lib()
    u64p, u8p, f64p, i32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_int32
    g = capi.Filter(min_size=8.0, seed=3)
    g.add(fc.line_edges(12, bad=(3, 7)))
    assert g.calc_valid_edges() == 1
    g.add([fc.E(500, 5000 * fc.S, 200 * fc.S)])
    h = g._h

    def snapshot():
        return g.clusters(with_eval=True), g.all_edges().copy(), g.valid_edges().copy()

    kept = snapshot()

    def unchanged():
        now = snapshot()
        assert_same_state(now[0], kept[0], with_eval=True)
        assert np.array_equal(now[1], kept[1]) and np.array_equal(now[2], kept[2])

    def refused(rc):
        assert rc == capi.UZL_ERR_BAD_ARG, rc
        assert L.uzl_filter_last_error(h) != b""
        unchanged()

    # cap below the count: the first `cap` keys, the full count
    for fn, full in ((L.uzl_filter_all_edges, kept[1]), (L.uzl_filter_valid_edges, kept[2])):
        assert len(full) >= 10
        out = np.full(len(full), 0xDEAD, np.uint64); n = i32(-1)
        assert fn(h, i32(4), out.ctypes.data_as(u64p), C.byref(n)) == capi.UZL_OK
        assert n.value == len(full) and np.array_equal(out[:4], full[:4]) and (out[4:] == 0xDEAD).all()
        n = i32(-1)
        assert fn(h, i32(0), None, C.byref(n)) == capi.UZL_OK and n.value == len(full)              # cap = 0 with NULL keys
        refused(fn(h, i32(4), None, C.byref(n)))
        refused(fn(h, i32(-1), out.ctypes.data_as(u64p), C.byref(n)))
        refused(fn(h, i32(4), out.ctypes.data_as(u64p), None))
    # cluster_edges / cluster_last_eval
    keys = np.zeros(16, np.uint64); valid = np.zeros(16, np.uint8)
    kp, vp = keys.ctypes.data_as(u64p), valid.ctypes.data_as(u8p)
    assert L.uzl_filter_cluster_edges(h, i32(0), i32(12), kp, vp) == capi.UZL_OK and list(keys[:12]) == list(range(10, 22))
    refused(L.uzl_filter_cluster_edges(h, i32(0), i32(11), kp, vp))
    refused(L.uzl_filter_cluster_edges(h, i32(2), i32(16), kp, vp))
    refused(L.uzl_filter_cluster_edges(h, i32(-1), i32(16), kp, vp))
    refused(L.uzl_filter_cluster_edges(h, i32(0), i32(16), None, vp))
    refused(L.uzl_filter_cluster_edges(h, i32(0), i32(16), kp, None))
    P = np.zeros((16, 3)); Q = np.zeros((16, 3)); T = np.zeros(12); rc = i32(-1)
    pp, qp, tp = (a.ctypes.data_as(f64p) for a in (P, Q, T))
    assert L.uzl_filter_cluster_last_eval(h, i32(0), i32(12), pp, qp, tp, C.byref(rc)) == 12
    assert P[:12].tobytes() == kept[0][0]["P"].tobytes() and Q[:12].tobytes() == kept[0][0]["Q"].tobytes() and rc.value == 10
    assert not P[12:].any() and T.tobytes() == kept[0][0]["T"].tobytes()
    assert L.uzl_filter_cluster_last_eval(h, i32(0), i32(12), None, None, None, None) == 12          # NULL outputs are skipped
    assert L.uzl_filter_cluster_last_eval(h, i32(1), i32(0), None, None, None, None) == 0            # never evaluated
    refused(L.uzl_filter_cluster_last_eval(h, i32(0), i32(11), pp, qp, tp, C.byref(rc)))
    refused(L.uzl_filter_cluster_last_eval(h, i32(2), i32(16), pp, qp, tp, C.byref(rc)))
    refused(L.uzl_filter_cluster_last_eval(h, i32(-1), i32(16), pp, qp, tp, C.byref(rc)))
    info = capi.ClusterInfo()
    refused(L.uzl_filter_cluster_info(h, i32(2), C.byref(info)))
    refused(L.uzl_filter_cluster_info(h, i32(0), None))
    # add: a bad third edge refuses the whole call
    fresh = fc.line_edges(3, key0=900, from0_s=9000.0)
    for field, value in (("n_stamps_from", -1), ("n_stamps_to", -1), ("stamps_from_ns", None), ("stamps_to_ns", None)):
        arr, keep = capi.pack_filter_edges(fresh)
        setattr(arr[2], field, value)
        refused(L.uzl_filter_add(h, i32(3), arr))
    refused(L.uzl_filter_add(h, i32(3), None))
    refused(L.uzl_filter_add(h, i32(-1), arr))
    refused(L.uzl_filter_remove(h, i32(2), None))
    refused(L.uzl_filter_remove(h, i32(-1), kept[1].ctypes.data_as(u64p)))
    refused(L.uzl_filter_set_sensors(h, i32(2), None))
    refused(L.uzl_filter_set_sensors(h, i32(-1), P.ctypes.data_as(f64p)))
    # the handle still works, and as the oracle does
    o = oracle.Filter(min_size=8.0, seed=3)
    o.add(fc.line_edges(12, bad=(3, 7)))
    assert o.calc_valid_edges() == 1
    o.add([fc.E(500, 5000 * fc.S, 200 * fc.S)])
    for f in (g, o):
        f.add(fresh)
        f.remove([500])
    same(g, o)
    g.close(); o.close()
    # create
    for cfg in (dict(max_edges=0), dict(max_error=0.0), dict(max_error=float("nan")), dict(ransac_iterations=4097), dict(max_error=-0.3)):
        with pytest.raises(capi.UzlError):
            capi.Filter(**cfg)
    capi.Filter(ransac_iterations=4096).close()
