"""uzl_pgo_rewrite_graph: the resident graph shrunk in place - a merged pair (uzl_merge_plan) or nodes that left the scope - must be
the graph uzl_pgo_add_graph makes of the rewritten arrays (uzliti_slam_amd.merge.apply_merge_plan for a merge, the drop-list
restatement tests/rewrite_reference.py otherwise).

Before any solve the two handles hold the same bits: the surviving estimates are copied, the placed pose goes through the kernel
add_graph prepares a node pose with, and a displacement that takes a multiplier is composed with merge._compose's association and
no contraction - so poses, edge errors (NaN pattern included), edge_in_system and the gauge are compared with array_equal.  After a
solve the fresh handle starts from poses that went matrix -> quaternion -> matrix once more, the situation of tests/test_append_gpu.py,
and its tolerances apply: chi2_initial 1e-9, chi2_final 1e-6 relative, poses 1e-5 m / 1e-6 rad (the PCG's accuracy, pcg_tol = 1e-5 m)."""
import ctypes as C

import numpy as np
import pytest

import merge_scenes as S
import rewrite_reference as R
from uzliti_slam_amd import synth
from uzliti_slam_amd.merge import apply_merge_plan, pgo_rewrite_of_drops, pgo_rewrite_of_plan

pytestmark = pytest.mark.gpu

FAR = np.array([1.0e6, 0.0, 0.0])


def _sub(e, idx):
    return {k: np.asarray(v)[idx] for k, v in e.items()}


def _cat(a, b):
    return {k: np.concatenate([np.asarray(a[k]), np.asarray(b[k])]) for k in a}


def _transforms(rng, n, spread=1.0, deg=90.0):
    return np.array([S.pose(rng.uniform(-spread, spread, 3), S.rot_axis(rng.normal(size=3), rng.uniform(-deg, deg))) for _ in range(n)]).reshape(n, 12)


def solver_edges(rows, seed, odom_dt=0.0):
    """(from, to, type, valid) rows as the solver's uzl_edge arrays: non-identity transforms and displacements, every third edge
    through sensor 0 / 1"""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    ne = len(rows)
    rng = np.random.default_rng(seed)
    info = np.zeros((ne, 6, 6))
    for k in range(6):
        info[:, k, k] = rng.uniform(50, 400, ne) * (100.0 if k >= 3 else 1.0)
    k = np.arange(ne)
    return dict(**{"from": rows[:, 0].astype(np.int32)}, to=rows[:, 1].astype(np.int32), type=rows[:, 2].astype(np.int32),
                sensor_from=np.where(k % 3 == 0, k % 2, -1).astype(np.int32), sensor_to=np.where(k % 3 == 1, (k + 1) % 2, -1).astype(np.int32),
                valid=rows[:, 3].astype(np.int32), transform=_transforms(rng, ne), displacement_from=_transforms(rng, ne, 0.3, 40.0),
                displacement_to=_transforms(rng, ne, 0.3, 40.0), information=info.reshape(ne, 36), diff_time=np.full(ne, odom_dt))


def merged_arrays(capi, poses, fixed, ed, plan):
    """apply_merge_plan over the solver's arrays: the edges' other fields follow the survivors (tagged through matching_score)"""
    ne = len(ed["from"])
    E = capi.gate_edges(ed["from"], ed["to"], ed["type"], valid=ed["valid"], score=np.arange(ne, dtype=np.float64))
    P2, E2, (d_from, d_to), node_map = apply_merge_plan(poses, E, (np.asarray(ed["displacement_from"]).reshape(ne, 12), np.asarray(ed["displacement_to"]).reshape(ne, 12)), plan)
    alive = E2["matching_score"].astype(np.int64)
    out = _sub(ed, alive)
    out["from"] = E2["from"].copy(); out["to"] = E2["to"].copy(); out["displacement_from"] = d_from; out["displacement_to"] = d_to
    edge_map = np.full(ne, -1, np.int32); edge_map[alive] = np.arange(len(alive))
    return P2, np.delete(np.asarray(fixed), plan["drop"]), out, node_map, edge_map


def assert_same_bits(a, b):
    """two handles before any solve: store() and, after one LM iteration, the gauge"""
    Pa, ea, ua = a.store(); Pb, eb, ub = b.store()
    assert a.n == b.n and a.e_in == b.e_in
    assert np.array_equal(Pa, Pb)
    assert np.array_equal(np.isnan(ea), np.isnan(eb)) and np.array_equal(ea, eb, equal_nan=True)
    assert np.array_equal(ua, ub)
    sa, sb = a.optimize(1), b.optimize(1)
    assert np.array_equal(a.get_fixed(), b.get_fixed())
    for k in ("n_vertices", "n_edges", "n_gauge_fixed", "chi2_initial"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def rewrite_and_compare(capi, poses, fixed, ed, sensors, rw, want, **cfg):
    """handle A: add_graph + rewrite_graph(rw); fresh handle B: add_graph of `want` = (poses, fixed, edges, node_map, edge_map)"""
    a = capi.Pgo(**cfg); b = capi.Pgo(**cfg)
    try:
        a.add_graph(poses, fixed, ed, sensors)
        node_map, edge_map = a.rewrite_graph(**rw)
        assert np.array_equal(node_map, want[3]) and np.array_equal(edge_map, want[4])
        assert a.n == len(want[0]) and a.e_in == len(want[2]["from"])
        b.add_graph(want[0], want[1], want[2], sensors)
        assert_same_bits(a, b)
    finally:
        a.close(); b.close()


SENSORS = np.stack([S.pose((0.1, -0.2, 0.3), S.rot_axis((0.2, 1.0, 0.1), 25.0)), S.pose((-0.3, 0.05, 0.1), S.rot_axis((1.0, 0.3, -0.4), -50.0))])


# ------------------------------------------------------------------------------------------------ 1. bit-exact before any solve
@pytest.mark.parametrize("xy_only", [0, 1])
@pytest.mark.parametrize("name", list(S.PLAN_EDGES))
def test_merge_scenes_equal_a_fresh_handle(capi, name, xy_only):
    sc = S.plan_graph(S.PLAN_EDGES[name])
    P = sc["poses"]
    fixed = np.zeros(len(P), np.uint8); fixed[0] = 1
    ed = solver_edges([(e["from"], e["to"], e["type"], e["valid"]) for e in sc["edges"]], seed=5)
    plan = capi.merge_plan(len(P), P[S.K], P[S.D], sc["edges"], S.K, S.D, 1, 7)
    rw = pgo_rewrite_of_plan(plan)
    want = merged_arrays(capi, P, fixed, ed, plan)
    again = R.rewrite_arrays(P, fixed, ed, **{k: rw[k] for k in ("drop_nodes", "pose_nodes", "xf", "ops")}, new_poses=rw["poses"])
    assert np.array_equal(want[0], again[0]) and np.array_equal(want[3], again[3]) and np.array_equal(want[4], again[4])
    for k in want[2]:
        assert np.array_equal(np.asarray(want[2][k]).reshape(-1), np.asarray(again[2][k]).reshape(-1)), k
    rewrite_and_compare(capi, P, fixed, ed, SENSORS, rw, want, optimize_xy_only=xy_only)


def test_a_retargeted_odometry_edge(capi):
    """a chain of odometry edges under use_odometry_parameters: (1, 2) is retargeted to keep = 4, (2, 3) duplicates (3, 4) and goes"""
    ODOM = synth.EDGE_TYPE_ODOM
    rows = [(0, 1, ODOM, 1), (1, 2, ODOM, 1), (2, 3, ODOM, 1), (3, 4, ODOM, 1), (4, 5, ODOM, 1), (0, 5, S.FULL, 1)]
    sc = S.plan_graph(rows)
    P = sc["poses"]
    fixed = np.zeros(len(P), np.uint8); fixed[0] = 1
    ed = solver_edges(rows, seed=6, odom_dt=0.5)
    plan = capi.merge_plan(len(P), P[4], P[2], sc["edges"], 4, 2, 2, 1)
    assert list(plan["action"]) == [0, R.RETARGET_TO, R.DELETE, R.KEEP_TO, R.KEEP_FROM, 0]
    rewrite_and_compare(capi, P, fixed, ed, SENSORS, pgo_rewrite_of_plan(plan), merged_arrays(capi, P, fixed, ed, plan), use_odometry_parameters=1)


def test_edges_without_a_node_and_ops_on_both_sides(capi):
    rows = [(0, 1, S.FULL, 1), (1, 2, S.FULL, 1), (2, 3, S.FULL, 0), (-1, 3, S.FULL, 1), (4, -1, S.FULL, 1), (3, 4, S.FULL, 1), (4, 5, S.LASER, 1), (5, 9, S.FULL, 1), (5, 0, S.FULL, 1)]
    P = S.plan_graph(rows[:3])["poses"]
    fixed = np.zeros(len(P), np.uint8); fixed[[0, 3]] = 1
    ed = solver_edges(rows, seed=7)
    rng = np.random.default_rng(8)
    rw = dict(drop_nodes=[1], pose_nodes=[4, 0], poses=_transforms(rng, 2, 2.0, 170.0), xf=_transforms(rng, 3, 0.5, 120.0),
              ops=[(0, R.RETARGET_TO, 2, 2), (0, R.KEEP_FROM, 0, -1), (5, R.KEEP_TO, 1, 0), (5, R.RETARGET_FROM, 1, 5), (8, R.DELETE, 0, 0), (3, R.KEEP_TO, 2, 0)])
    want = R.rewrite_arrays(P, fixed, ed, rw["drop_nodes"], rw["pose_nodes"], rw["poses"], rw["xf"], rw["ops"])
    assert list(want[4]) == [0, -1, 1, 2, 3, 4, 5, 6, -1]
    for xy_only in (0, 1):
        rewrite_and_compare(capi, P, fixed, ed, SENSORS, rw, want, optimize_xy_only=xy_only)


# ------------------------------------------------------------------------------------------------ 2. kernel edges
@pytest.fixture(scope="module")
def graph300():
    return synth.make_pose_graph(300, 900, seed=301)


@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257, 900])
def test_edge_counts_around_a_wave_and_a_block(capi, graph300, m):
    """one wave per edge, four edges per 256-lane workgroup: edge counts at, below and above 64 and 256; nodes in several workgroups"""
    g = graph300
    ed = _sub(g["edges"], np.arange(m))
    rng = np.random.default_rng(m)
    rw = dict(drop_nodes=[0, 299, 30], pose_nodes=[40, 298], poses=_transforms(rng, 2, 3.0, 170.0), xf=_transforms(rng, 2, 0.5, 120.0),
              ops=[(5, R.KEEP_FROM, 0, 0), (10, R.RETARGET_TO, 1, 40), (20, R.DELETE, 0, 0), (50, R.KEEP_FROM, 1, 0), (50, R.KEEP_TO, 0, 0),
                   (m - 1, R.KEEP_TO, 1, 0), (m - 2, R.RETARGET_FROM, 0, 1)])
    want = R.rewrite_arrays(g["nodes_pose"], g["nodes_fixed"], ed, rw["drop_nodes"], rw["pose_nodes"], rw["poses"], rw["xf"], rw["ops"])
    assert len(want[0]) == 297 and 0 < len(want[2]["from"]) < m
    rewrite_and_compare(capi, g["nodes_pose"], g["nodes_fixed"], ed, None, rw, want)


def test_one_node_and_no_edge_left(capi, graph300):
    g = graph300
    rw = pgo_rewrite_of_drops([v for v in range(300) if v != 7])
    want = R.rewrite_arrays(g["nodes_pose"], g["nodes_fixed"], g["edges"], rw["drop_nodes"])
    assert len(want[0]) == 1 and len(want[2]["from"]) == 0 and want[3][7] == 0
    rewrite_and_compare(capi, g["nodes_pose"], g["nodes_fixed"], g["edges"], None, rw, want)


def test_a_scope_drop_after_an_append(capi, graph300):
    """the edge numbering a rewrite addresses is add_graph's followed by append_graph's"""
    g = graph300
    ed = g["edges"]
    first = np.nonzero((ed["from"] < 250) & (ed["to"] < 250))[0]; rest = np.nonzero(~((ed["from"] < 250) & (ed["to"] < 250)))[0]
    order = np.concatenate([first, rest])
    a = capi.Pgo(); b = capi.Pgo()
    a.add_graph(g["nodes_pose"][:250], g["nodes_fixed"][:250], _sub(ed, first))
    a.append_graph(g["nodes_pose"][250:], g["nodes_fixed"][250:], _sub(ed, rest))
    rw = pgo_rewrite_of_drops(np.arange(100, 130))
    want = R.rewrite_arrays(g["nodes_pose"], g["nodes_fixed"], _sub(ed, order), rw["drop_nodes"])
    node_map, edge_map = a.rewrite_graph(**rw)
    assert np.array_equal(node_map, want[3]) and np.array_equal(edge_map, want[4])
    b.add_graph(want[0], want[1], want[2])
    assert_same_bits(a, b)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------ 3. the real use, after a solve
def _close(sa, sb, Pa, Pb):
    for k in ("n_vertices", "n_edges", "n_gauge_fixed", "n_eliminated", "iterations_done", "lm_trials"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    print("chi2_initial", sa["chi2_initial"], sb["chi2_initial"], "chi2_final", sa["chi2_final"], sb["chi2_final"])
    assert abs(sa["chi2_initial"] - sb["chi2_initial"]) <= 1e-9 * sb["chi2_initial"]
    assert abs(sa["chi2_final"] - sb["chi2_final"]) <= 1e-6 * sb["chi2_final"]
    dt, dr = synth.pose_errors(Pa.reshape(-1, 3, 4), Pb.reshape(-1, 3, 4))
    print("pose difference", dt, dr)
    assert dt < 1e-5 and dr < 1e-6, (dt, dr)


@pytest.mark.parametrize("numbering", [1, 2])
@pytest.mark.parametrize("n,e", [(600, 2400), (3000, 3300)])
def test_merge_after_a_solve_then_grow(capi, n, e, numbering):
    g = synth.make_pose_graph(n, e, seed=n + 1)
    ed = g["edges"]
    n1 = n - 20
    old = (ed["from"] < n1) & (ed["to"] < n1)
    first, rest = np.nonzero(old)[0], np.nonzero(~old)[0]
    ed1 = _sub(ed, first)
    p = capi.Pgo(reduced_numbering=numbering)
    p.add_graph(g["nodes_pose"][:n1], g["nodes_fixed"][:n1], ed1)
    st0 = p.optimize(4)
    P1 = p.store()[0]
    # ---- one merge, found on the device at the solved poses
    E = capi.gate_edges(ed1["from"], ed1["to"], ed1["type"], valid=ed1["valid"])
    table, plan = np.zeros(0, np.int32), None
    for gates in (dict(max_distance=0.25, max_rotation_deg=15.0), dict(max_distance=1.0, max_rotation_deg=45.0)):      # (the reference's, then widened)
        with capi.Merge(**gates) as m:
            m.set_graph(g["nodes_pose"][:n1], E)
            m.poses_from_pgo(p)
            table = m.partners(FAR, 0.0)
            if (table >= 0).any():
                i = int(np.flatnonzero(table >= 0)[0])
                plan = m.plan(max(i, int(table[i])), min(i, int(table[i])), 1, 1)
                break
    assert plan is not None, "no node has a merge partner, even with the widened gates"
    assert plan["touched"] > 0
    node_map, edge_map = p.rewrite_graph(**pgo_rewrite_of_plan(plan))
    sa = p.optimize(6)
    Pa = p.store()[0]
    # ---- a fresh handle given apply_merge_plan of the stored poses and the edges
    P2, fixed2, ed2, want_nodes, want_edges = merged_arrays(capi, P1, g["nodes_fixed"][:n1], ed1, plan)
    assert np.array_equal(node_map, want_nodes) and np.array_equal(edge_map, want_edges)
    q = capi.Pgo(reduced_numbering=numbering)
    q.add_graph(P2, fixed2, ed2)
    sb = q.optimize(6)
    _close(sa, sb, Pa, q.store()[0])
    q.close()
    # ---- reset() goes back to the state the rewrite left
    p.reset(); sc = p.optimize(6)
    assert np.array_equal(p.store()[0], Pa) and sc["chi2_final"] == sa["chi2_final"]
    # ---- shrink, then grow: 20 new nodes with their edges, and a few old feature edges flipped through the rewrite's edge map
    new_of = np.concatenate([node_map, np.arange(n1, n, dtype=np.int32) - 1])
    ed3 = _sub(ed, rest)
    named = (new_of[ed3["from"]] >= 0) & (new_of[ed3["to"]] >= 0)                 # (an edge to the merged-away node is not offered)
    ed3 = _sub(ed3, np.nonzero(named)[0])
    ed3["from"] = new_of[ed3["from"]]; ed3["to"] = new_of[ed3["to"]]
    feat = np.nonzero((np.asarray(ed1["type"]) != synth.EDGE_TYPE_ODOM) & (edge_map >= 0))[0]
    flip = feat[:: max(1, len(feat) // 7)][:7]
    valid2 = np.asarray(ed2["valid"]).copy()
    valid2[edge_map[flip]] = 1 - valid2[edge_map[flip]]
    p.append_graph(g["nodes_pose"][n1:], g["nodes_fixed"][n1:], ed3, edge_map[flip].astype(np.int32), valid2[edge_map[flip]].astype(np.uint8))
    sg = p.optimize(6)
    Pg = p.store()[0]
    full = _cat(dict(ed2, valid=valid2), ed3)
    r = capi.Pgo(reduced_numbering=numbering)
    r.add_graph(np.concatenate([Pa.reshape(-1, 12), np.asarray(g["nodes_pose"], np.float64).reshape(-1, 12)[n1:]]), np.concatenate([fixed2, g["nodes_fixed"][n1:]]), full)
    sr = r.optimize(6)
    _close(sg, sr, Pg, r.store()[0])
    r.close(); p.close()
    assert st0["status"] == 0 and sa["status"] == 0 and sg["status"] == 0


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_a_refused_rewrite_changes_nothing(capi):
    g = synth.make_pose_graph(50, 120, seed=3)
    n, e = 50, 120
    p = capi.Pgo()
    with pytest.raises(capi.UzlError) as err:                                    # no graph yet
        p.rewrite_graph(drop_nodes=[0])
    assert err.value.status == capi.UZL_ERR_BAD_ARG
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    p.optimize(2)
    before = p.store()
    X = np.tile(np.eye(3, 4).reshape(12), (2, 1))
    bad = [dict(drop_nodes=[n]), dict(drop_nodes=[-1]), dict(drop_nodes=[3, 3]), dict(pose_nodes=[n], poses=X[:1]), dict(drop_nodes=[2], pose_nodes=[2], poses=X[:1]),
           dict(pose_nodes=[1, 1], poses=X), dict(xf=X, ops=[(e, R.KEEP_FROM, 0, 0)]), dict(ops=[(-1, R.DELETE, 0, 0)]),
           dict(xf=X, ops=[(0, R.KEEP_FROM, 0, 0), (0, R.RETARGET_FROM, 1, 3)]), dict(xf=X, ops=[(0, R.KEEP_TO, 0, 0), (0, R.KEEP_TO, 0, 0)]),
           dict(xf=X, ops=[(0, R.DELETE, 0, 0), (0, R.KEEP_TO, 0, 0)]), dict(xf=X, ops=[(0, R.KEEP_TO, 0, 0), (0, R.DELETE, 0, 0)]),
           dict(xf=X, ops=[(0, R.KEEP_FROM, 2, 0)]), dict(ops=[(0, R.KEEP_FROM, 0, 0)]), dict(drop_nodes=[3], xf=X, ops=[(0, R.RETARGET_TO, 0, 3)]),
           dict(xf=X, ops=[(0, R.RETARGET_FROM, 0, n)]), dict(xf=X, ops=[(0, 6, 0, 0)]), dict(xf=X, ops=[(0, 0, 0, 0)])]
    for kw in bad:
        with pytest.raises(capi.UzlError) as err:
            p.rewrite_graph(**kw)
        assert err.value.status == capi.UZL_ERR_BAD_ARG, kw
        after = p.store()
        assert (p.n, p.e_in) == (n, e)
        assert all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(before, after)), kw
    # a map's capacity below the old count
    rw = capi.PgoRewrite()
    maps = np.zeros(e, np.int32)
    for cap_n, cap_e in ((n - 1, e), (n, e - 1)):
        assert capi.lib().uzl_pgo_rewrite_graph(p._h, C.byref(rw), C.c_int32(cap_n), maps.ctypes.data_as(capi.c_i32p), C.c_int32(cap_e), maps.ctypes.data_as(capi.c_i32p)) == capi.UZL_ERR_BAD_ARG
    assert all(np.array_equal(x, y, equal_nan=x.dtype.kind == "f") for x, y in zip(before, p.store()))
    # the handle still solves, and still takes a rewrite
    p.rewrite_graph(drop_nodes=[49])
    assert p.optimize(2)["n_vertices"] == 49
    p.close()


def test_a_set_graph_handle_is_refused_and_an_empty_rewrite_keeps_the_structure(capi, oracle):
    g = synth.make_pose_graph(50, 120, seed=3)
    fl = oracle.flatten_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    p = capi.Pgo()
    p.set_graph(fl["poses"], fl["fixed"], fl["ij"], fl["meas"], fl["info"], fl["robust"])
    with pytest.raises(capi.UzlError) as err:
        p.rewrite_graph(drop_nodes=[3])
    assert err.value.status == capi.UZL_ERR_BAD_ARG
    assert p.optimize(2)["n_vertices"] == 50                                     # (and is left as it was)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    p.optimize(3)
    node_map, edge_map = p.rewrite_graph()
    assert np.array_equal(node_map, np.arange(50)) and np.array_equal(edge_map, np.arange(120))
    assert p.optimize(3)["structure_reused"] == 1
    p.close()
