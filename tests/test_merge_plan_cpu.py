"""CPU tests (no GPU needed): the rewrite plan of uzl_merge_plan - mergeNodes, graph_slam_node.cpp:919-986 - against the restatement
tests/merge_reference.py, and uzliti_slam_amd.merge.apply_merge_plan against the restatement's rewritten graph.

uzl_merge_plan reads the two poses from the device (the header says why), so the handle call is covered in tests/test_merge_gpu.py;
the arithmetic itself is one pure host function, reached here without a handle through the diagnostic library's uzl_debug_merge_plan.

edge_action, ratio, the counts and the translation of new_pose are compared exactly.  The rotation block and the two displacements
go through acos / sin / cos / atan2, so equal bits are hoped for, not promised.  Measured over every case below on the build host
(x86-64, glibc): the largest absolute entry difference between the C plan and the restatement is 0.0 - both call the same libm with
the same arguments.  The bound is four times that, 0.0: the two agree bit for bit here.  Should another libm or compiler ever
disagree, the agreed ceiling is 1e-12; at or above it the restatement is not followed."""
import numpy as np
import pytest

import merge_reference as M
import merge_scenes as S
from uzliti_slam_amd import capi
from uzliti_slam_amd.merge import apply_merge_plan

MEASURED = 0.0
BOUND = 4.0 * MEASURED
assert BOUND < 1e-12

CASES = [(name, kind, st) for name in S.PLAN_EDGES for kind in S.PLAN_POSES for st in S.PLAN_STAMPS]


def rows_of(edges):
    return [[int(e["from"]), int(e["to"]), int(e["type"]), int(e["valid"])] for e in edges]


def both(name, kind, stamps):
    sc = S.plan_graph(S.PLAN_EDGES[name])
    P = S.plan_poses(kind, sc)
    c = capi.merge_plan(len(P), P[S.K], P[S.D], sc["edges"], S.K, S.D, *stamps)
    r = M.merge_plan(P[S.K], P[S.D], rows_of(sc["edges"]), S.K, S.D, *stamps)
    return sc, P, c, r


@pytest.mark.parametrize("name,kind,stamps", CASES, ids=["%s-%s-%d:%d" % (n, k, s[0], s[1]) for n, k, s in CASES])
def test_plan_equals_the_restatement(name, kind, stamps):
    sc, P, c, r = both(name, kind, stamps)
    assert np.array_equal(c["action"], r["action"])
    assert (c["touched"], c["retargeted"], c["deleted"]) == (r["touched"], r["retargeted"], r["deleted"])
    assert c["ratio"] == r["ratio"] == stamps[1] / (stamps[0] + stamps[1])
    assert [c["new_pose"][k] for k in (3, 7, 11)] == [r["new_pose"][k] for k in (3, 7, 11)]
    worst = max(float(np.abs(np.asarray(c[k]) - np.asarray(r[k])).max()) for k in ("new_pose", "keep_displacement", "drop_displacement"))
    print("largest entry difference", worst)
    assert worst <= BOUND


def test_expected_actions():
    """what each case is about, spelled out"""
    U, KF, KT, RF, RT, DEL = range(6)
    want = {"joins_the_two": [DEL, DEL, RT, KF], "second_deleted_by_first_retarget": [RF, DEL, U], "other_type_both_kept": [RF, RT],
            "duplicate_on_keep_same_direction": [KF, DEL, RF], "duplicate_on_keep_other_direction": [KT, DEL, RT],
            "drop_on_from_and_to": [RF, RT, RF, RT, KF, KT], "invalid_edges_are_edges": [KF, DEL, RF, DEL, DEL],
            "self_loops": [KF, DEL, DEL, RF], "no_edges": []}
    for name, w in want.items():
        _, _, c, _ = both(name, "drawn", (1, 1))
        assert list(c["action"]) == w, name


def angle_between(A, B):
    Ra, Rb = np.asarray(A).reshape(3, 4)[:, :3], np.asarray(B).reshape(3, 4)[:, :3]
    return np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0)))


@pytest.mark.parametrize("kind", S.PLAN_POSES)
@pytest.mark.parametrize("stamps", S.PLAN_STAMPS)
def test_the_new_pose_lies_between_the_two(kind, stamps):
    """independent of the restatement: a rotation, `ratio` of the way from keep to drop, and the displacements lead back"""
    _, P, c, _ = both("no_edges", kind, stamps)
    T = np.asarray(c["new_pose"]).reshape(3, 4)
    assert np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-12 and np.linalg.det(T[:, :3]) > 0.999
    total = angle_between(P[S.K], P[S.D])
    if kind != "half_turn":                                                # (half a turn apart, the slerp may go either way round)
        # arccos near 1 turns a rounding of 2^-52 in the trace into sqrt(2^-52) rad = 1.2e-6 degrees: 1e-5 degrees is the yardstick's own error
        assert abs(angle_between(P[S.K], c["new_pose"]) - c["ratio"] * total) < 1e-5
    else:
        assert abs(total - 180.0) < 1e-5
    assert np.allclose(T[:, 3], (1 - c["ratio"]) * P[S.K].reshape(3, 4)[:, 3] + c["ratio"] * P[S.D].reshape(3, 4)[:, 3], atol=1e-15)
    for disp, node in (("keep_displacement", S.K), ("drop_displacement", S.D)):
        assert np.abs(np.asarray(M.compose(c["new_pose"], c[disp])) - P[node]).max() < 1e-12
    if kind == "identical":
        assert np.abs(np.asarray(c["keep_displacement"]) - np.eye(3, 4).reshape(12)).max() < 1e-12


@pytest.mark.parametrize("name", list(S.PLAN_EDGES))
@pytest.mark.parametrize("kind", ["drawn", "near"])
def test_apply_merge_plan_equals_the_rewritten_graph(name, kind):
    sc, P, c, _ = both(name, kind, (1, 7))
    ne = len(sc["edges"])
    rng = np.random.default_rng(3)
    D_from = np.array([S.pose(rng.uniform(-1, 1, 3), S.rot_axis(rng.normal(size=3), rng.uniform(-90, 90))) for _ in range(ne)]).reshape(ne, 12)
    D_to = np.array([S.pose(rng.uniform(-1, 1, 3), S.rot_axis(rng.normal(size=3), rng.uniform(-90, 90))) for _ in range(ne)]).reshape(ne, 12)
    before = (P.copy(), sc["edges"].copy(), D_from.copy(), D_to.copy())
    gotP, gotE, (got_from, got_to), old_to_new = apply_merge_plan(P, sc["edges"], (D_from, D_to), c)
    wantP, rows, want_from, want_to, want_map = M.rewritten_graph(P, rows_of(sc["edges"]), D_from, D_to, S.K, S.D, c)
    assert np.array_equal(gotP, np.array(wantP)) and list(old_to_new) == want_map and len(gotP) == len(P) - 1
    assert [[int(e["from"]), int(e["to"]), int(e["type"]), int(e["valid"])] for e in gotE] == rows
    assert np.array_equal(got_from, np.array(want_from).reshape(-1, 12)) and np.array_equal(got_to, np.array(want_to).reshape(-1, 12))
    assert len(gotE) == 0 or (gotE["from"].max() < len(gotP) and gotE["to"].max() < len(gotP) and gotE["from"].min() >= 0)
    assert old_to_new[S.D] == -1 and old_to_new[S.K] == S.K - 1
    for a, b in zip(before, (P, sc["edges"], D_from, D_to)):
        assert np.array_equal(a, b)                                        # the caller's arrays are left alone
    ident = apply_merge_plan(P, sc["edges"], None, c)
    assert len(ident[1]) == len(gotE)


def test_apply_refuses_a_plan_of_another_graph():
    sc, P, c, _ = both("joins_the_two", "drawn", (1, 1))
    with pytest.raises(ValueError):
        apply_merge_plan(P, sc["edges"][:-1], None, c)
    with pytest.raises(ValueError):
        apply_merge_plan(P[:3], sc["edges"], None, c)


def test_argument_errors_of_the_pure_plan():
    sc = S.plan_graph(S.PLAN_EDGES["joins_the_two"])
    P = sc["poses"]
    for keep, drop, a, b in ((S.K, S.K, 1, 1), (-1, S.D, 1, 1), (S.K, 6, 1, 1), (S.K, S.D, 0, 0), (S.K, S.D, -1, 2)):
        with pytest.raises(capi.UzlError) as e:
            capi.merge_plan(len(P), P[0], P[1], sc["edges"], keep, drop, a, b)
        assert e.value.status == capi.UZL_ERR_BAD_ARG
    with pytest.raises(capi.UzlError):
        capi.merge_plan(3, P[0], P[1], sc["edges"], 1, 2, 1, 1)           # an edge names a node outside a graph of 3
    assert capi.merge_plan(len(P), P[S.K], P[S.D], sc["edges"], S.K, S.D, 0, 3)["ratio"] == 1.0
