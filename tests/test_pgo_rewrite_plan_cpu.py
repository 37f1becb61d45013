"""CPU tests (no GPU needed): rewrite_plan (csrc/pgo_structure.hip), the host half of uzl_pgo_rewrite_graph, through the diagnostic
library's uzl_debug_pgo_rewrite_plan.  Index maps, the surviving edges' records and the new input edges are integers and are compared
exactly with the NumPy restatement tests/rewrite_reference.py; for merge plans the restatement itself is held to
uzliti_slam_amd.merge.apply_merge_plan, whose index part it generalises."""
import numpy as np
import pytest

import merge_scenes as S
import rewrite_reference as R
from uzliti_slam_amd import capi
from uzliti_slam_amd.merge import apply_merge_plan, pgo_rewrite_of_drops, pgo_rewrite_of_plan

ODOM = 104          # UZL_EDGE_TYPE_2D_WHEEL_ODOMETRY
N = 8
# a ring with chords over 8 nodes; two edges with a missing endpoint (-1), one naming a node outside the graph, one self-loop
RING = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 0), (0, 4), (2, 6), (-1, 3), (5, -1), (1, 11), (6, 6), (7, 1), (3, 2)]


def ring_graph():
    frm = np.array([a for a, _ in RING], np.int32); to = np.array([b for _, b in RING], np.int32)
    odom = (np.arange(len(RING)) < 8).astype(np.int32)
    valid = (np.arange(len(RING)) % 5 != 3).astype(np.int32)
    fixed = np.zeros(N, np.uint8); fixed[[0, 5]] = 1
    return frm, to, odom, valid, fixed


def check(n, fixed, frm, to, odom, valid, drop=(), pose_nodes=(), n_xf=0, ops=()):
    """the plan of the library against the restatement, everything it returns"""
    in_edges = np.stack([frm, to, odom, valid], axis=1).astype(np.int32).reshape(-1, 4)
    got = capi.pgo_rewrite_plan(n, fixed, in_edges, drop, pose_nodes, n_xf, R.op_rows(ops).astype(np.int32))
    want = R.restate_index(n, frm, to, drop, ops)
    for k in ("old_to_new_node", "new_to_old_node", "old_to_new_edge", "new_to_old_edge", "rec"):
        assert np.array_equal(got[k], want[k]), k
    alive = want["new_to_old_edge"]
    assert got["n_new"] == len(want["new_to_old_node"]) and got["e_new"] == len(alive)
    assert np.array_equal(got["in_edges"][:, :2], want["rec"][:, :2])                          # the endpoints, renumbered
    assert np.array_equal(got["in_edges"][:, 2], np.asarray(odom)[alive]) and np.array_equal(got["in_edges"][:, 3], np.asarray(valid)[alive])
    assert np.array_equal(got["fixed"], np.asarray(fixed, np.uint8)[want["new_to_old_node"]])
    return got, want


@pytest.mark.parametrize("name", list(S.PLAN_EDGES))
def test_merge_plans(name):
    sc = S.plan_graph(S.PLAN_EDGES[name])
    P, E = sc["poses"], sc["edges"]
    plan = capi.merge_plan(len(P), P[S.K], P[S.D], E, S.K, S.D, 1, 7)
    rw = pgo_rewrite_of_plan(plan)
    assert list(rw["drop_nodes"]) == [S.D] and list(rw["pose_nodes"]) == [S.K] and np.array_equal(rw["poses"][0], plan["new_pose"])
    assert np.array_equal(rw["xf"][0], plan["keep_displacement"]) and np.array_equal(rw["xf"][1], plan["drop_displacement"])
    fixed = np.zeros(len(P), np.uint8); fixed[0] = 1
    got, want = check(len(P), fixed, E["from"], E["to"], (E["type"] == ODOM).astype(np.int32), E["valid"], rw["drop_nodes"], rw["pose_nodes"], 2, rw["ops"])
    # the restatement's index part is apply_merge_plan's
    _, E2, _, old_to_new = apply_merge_plan(P, E, None, plan)
    assert np.array_equal(old_to_new, got["old_to_new_node"])
    assert np.array_equal(E2["from"], got["rec"][:, 0]) and np.array_equal(E2["to"], got["rec"][:, 1]) and len(E2) == got["e_new"]
    # which multiplier a touched side takes: keep_displacement (0) for KEEP_x, drop_displacement (1) for RETARGET_x
    act = np.asarray(plan["action"])[got["new_to_old_edge"]]
    assert np.array_equal(got["rec"][:, 2], np.where(act == R.KEEP_FROM, 0, np.where(act == R.RETARGET_FROM, 1, -1)))
    assert np.array_equal(got["rec"][:, 3], np.where(act == R.KEEP_TO, 0, np.where(act == R.RETARGET_TO, 1, -1)))
    if name == "self_loops":                  # the retargeted self-loop of drop still names drop at its `to` end: it goes with the node
        assert list(plan["action"]) == [R.KEEP_FROM, R.DELETE, R.DELETE, R.RETARGET_FROM] and list(got["old_to_new_edge"]) == [0, -1, -1, -1]
    if name == "no_edges":
        assert got["e_new"] == 0 and got["n_new"] == len(P) - 1


@pytest.mark.parametrize("drop", [[0], [N - 1], [3, 4], [4, 3], [1, 2, 3, 4, 5, 6, 7], [0, 1, 2, 3, 4, 5, 6], list(range(N)), []],
                         ids=["first", "last", "adjacent", "adjacent_unsorted", "all_but_first", "all_but_last", "all", "none"])
def test_drop_lists(drop):
    frm, to, odom, valid, fixed = ring_graph()
    rw = pgo_rewrite_of_drops(drop)
    got, _ = check(N, fixed, frm, to, odom, valid, rw["drop_nodes"])
    assert got["n_new"] == N - len(drop)
    gone = set(drop)
    for k, (a, b) in enumerate(RING):                                      # removeNode: exactly the edges that name a dropped node go
        assert (got["old_to_new_edge"][k] < 0) == (a in gone or b in gone)
    if not drop:                                                           # an empty rewrite is the identity
        assert np.array_equal(got["in_edges"][:, 0], frm) and np.array_equal(got["in_edges"][:, 1], to)


def test_endpoints_outside_the_graph_stay_as_they_are():
    frm, to, odom, valid, fixed = ring_graph()
    got, _ = check(N, fixed, frm, to, odom, valid, [0, 2])
    new_of = got["old_to_new_edge"]
    assert got["in_edges"][new_of[10]][0] == -1 and got["in_edges"][new_of[10]][1] == got["old_to_new_node"][3]
    assert got["in_edges"][new_of[11]][1] == -1
    assert got["in_edges"][new_of[12]].tolist()[:2] == [0, 11]             # (1, 11): node 1 is node 0 now; 11 still names no node of the graph
    got, _ = check(N, fixed, frm, to, odom, valid, [1])
    assert got["old_to_new_edge"][12] == -1                                # ... and goes with node 1


def test_one_op_on_each_side_of_an_edge():
    frm, to, odom, valid, fixed = ring_graph()
    # edge 8 = (0, 4): retarget from -> 1 with xf 2, keep to with xf 0; edge 9 = (2, 6): to -> 7; edge 2 = (2, 3): from -> 3 makes a self-loop of a surviving node
    ops = [(8, R.RETARGET_FROM, 2, 1), (8, R.KEEP_TO, 0, -5), (9, R.RETARGET_TO, 1, 7), (2, R.RETARGET_FROM, 0, 3), (15, R.DELETE, 99, 99)]
    got, _ = check(N, fixed, frm, to, odom, valid, [0, 2], [4], 3, ops)
    o2n = got["old_to_new_node"]
    assert got["rec"][got["old_to_new_edge"][8]].tolist() == [o2n[1], o2n[4], 2, 0]
    assert got["old_to_new_edge"][9] == -1                                 # its `from` end still names the dropped node 2
    assert got["rec"][got["old_to_new_edge"][2]].tolist() == [o2n[3], o2n[3], 0, -1]
    assert got["old_to_new_edge"][15] == -1
    # an edge of a dropped node is saved by retargeting it away
    got, _ = check(N, fixed, frm, to, odom, valid, [0], [], 1, [(0, R.RETARGET_FROM, 0, 7), (7, R.RETARGET_TO, 0, 7)])
    assert got["old_to_new_edge"][0] >= 0 and got["old_to_new_edge"][7] >= 0 and got["old_to_new_edge"][8] == -1


BAD = {
    "drop_out_of_range": dict(drop=[N]),
    "drop_negative": dict(drop=[-1]),
    "drop_duplicate": dict(drop=[3, 5, 3]),
    "pose_node_out_of_range": dict(pose_nodes=[N]),
    "pose_node_dropped": dict(drop=[2], pose_nodes=[2]),
    "pose_node_duplicate": dict(pose_nodes=[1, 1]),
    "edge_out_of_range": dict(n_xf=1, ops=[(len(RING), R.KEEP_FROM, 0, 0)]),
    "edge_negative": dict(ops=[(-1, R.DELETE, 0, 0)]),
    "two_ops_on_from": dict(n_xf=1, ops=[(0, R.KEEP_FROM, 0, 0), (0, R.RETARGET_FROM, 0, 3)]),
    "two_ops_on_to": dict(n_xf=1, ops=[(0, R.RETARGET_TO, 0, 3), (0, R.KEEP_TO, 0, 0)]),
    "delete_then_op": dict(n_xf=1, ops=[(0, R.DELETE, 0, 0), (0, R.KEEP_TO, 0, 0)]),
    "op_then_delete": dict(n_xf=1, ops=[(0, R.KEEP_TO, 0, 0), (0, R.DELETE, 0, 0)]),
    "delete_twice": dict(ops=[(0, R.DELETE, 0, 0), (0, R.DELETE, 0, 0)]),
    "xf_out_of_range": dict(n_xf=2, ops=[(0, R.KEEP_FROM, 2, 0)]),
    "xf_negative": dict(n_xf=2, ops=[(0, R.KEEP_FROM, -1, 0)]),
    "xf_without_any": dict(n_xf=0, ops=[(0, R.KEEP_FROM, 0, 0)]),
    "retarget_to_dropped": dict(drop=[3], n_xf=1, ops=[(0, R.RETARGET_TO, 0, 3)]),
    "retarget_out_of_range": dict(n_xf=1, ops=[(0, R.RETARGET_FROM, 0, N)]),
    "retarget_negative": dict(n_xf=1, ops=[(0, R.RETARGET_FROM, 0, -1)]),
    "unknown_action": dict(n_xf=1, ops=[(0, 6, 0, 0)]),
    "action_untouched": dict(n_xf=1, ops=[(0, capi.MERGE_EDGE_UNTOUCHED, 0, 0)]),
}


@pytest.mark.parametrize("name", list(BAD))
def test_bad_arguments(name):
    frm, to, odom, valid, fixed = ring_graph()
    kw = dict(drop=[], pose_nodes=[], n_xf=0, ops=[]); kw.update(BAD[name])
    in_edges = np.stack([frm, to, odom, valid], axis=1)
    with pytest.raises(capi.UzlError) as e:
        capi.pgo_rewrite_plan(N, fixed, in_edges, kw["drop"], kw["pose_nodes"], kw["n_xf"], kw["ops"])
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_what_the_refusals_are_not():
    """the neighbours of the refused cases pass: DELETE ignores xf and node, KEEP ignores node, the last node and edge are in range"""
    frm, to, odom, valid, fixed = ring_graph()
    ops = [(len(RING) - 1, R.DELETE, -7, -7), (0, R.KEEP_FROM, 1, N + 3), (0, R.KEEP_TO, 1, -9), (1, R.RETARGET_TO, 0, N - 1)]
    check(N, fixed, frm, to, odom, valid, [0], [N - 1], 2, ops)
