"""What the device holds of a pose graph's structure equals the CPU plan for the same input (csrc/pgo_structure.hpp through
capi.pgo_structure_plan; test_pgo_structure_plan.py holds that plan against its references).  The device side is read through the stage
hooks that exist: uzl_debug_pgo_linearize (sizes, v2b, row_ptr, col) and uzl_debug_pgo_reduced (the reduced system's sizes and block-CSR),
and the solve's stats (n_gauge_fixed, n_eliminated, reduced_strong).  No kernel of its own: index arrays only."""
import numpy as np
import pytest

import structure_reference as SR
from uzliti_slam_amd import synth

pytestmark = pytest.mark.gpu


def cpu_plan(capi, n, fixed, ij, robust, edge_w):
    plan = capi.pgo_structure_plan
    G = plan("gauge", n=n, fixed=fixed, ij=ij)
    b2v = plan("order", n=n, fixed=G["fixed_eff"], ij=ij, edge_w=edge_w)["b2v"]
    Y = plan("system", n=n, ij=ij, robust=robust, b2v=b2v)
    red = capi.schur_plan(Y["row_ptr"], Y["col"], 24) if Y["nb"] > 0 else None           # (reduced_numbering = 1 below: the row order's plan)
    if red is not None and not plan("admission", nb=Y["nb"], n_int=Y["nb"] - red["n_reduced"])["admitted"]:
        red = None
    return G, Y, red


def cpu_plan_of_graph(capi, g):
    ie, w = SR.in_edges_of(g)
    n = len(g["nodes_fixed"])
    F = capi.pgo_structure_plan("flatten", n=n, fixed=g["nodes_fixed"], in_edges=ie, in_w=w)
    return F, cpu_plan(capi, n, g["nodes_fixed"], F["ij"], F["robust"], F["edge_w"])


def check_device(p, e, G, Y, red):
    """p: a DiagPgo holding the graph; -> the stats of its first solve"""
    st = p.optimize(1)
    L = p.linearize()
    assert (len(L["v2b"]), len(L["row_ptr"]) - 1, len(L["col"])) == (len(Y["v2b"]), Y["nb"], Y["nslots"])
    assert np.array_equal(L["v2b"], Y["v2b"]) and np.array_equal(L["row_ptr"], Y["row_ptr"]) and np.array_equal(L["col"], Y["col"])
    R = p.reduced()
    assert (R is None) == (red is None)
    if R is not None:
        assert np.array_equal(R["row_ptr"], red["row_ptr"]) and np.array_equal(R["col"], red["col"])
        assert np.array_equal(R["sep_rows"], np.nonzero(red["red_row"] >= 0)[0])
    assert (st["n_vertices"], st["n_edges"], st["n_gauge_fixed"]) == (len(Y["v2b"]), e, G["n_gauge"])
    assert st["n_eliminated"] == (0 if red is None else Y["nb"] - red["n_reduced"]) and st["reduced_strong"] == 0
    assert np.array_equal(p.get_fixed(), G["fixed_eff"])
    return st


def chain_with_closures(n):
    g = synth.make_pose_graph(n, n + 2, seed=21)
    assert (np.asarray(g["edges"]["type"]) != synth.EDGE_TYPE_ODOM).sum() == 3
    return g


@pytest.mark.parametrize("case", ["10 / 20", "skip rules", "interleaved sessions", "chain, Schur-reduced"])
def test_device_structure_is_the_cpu_plan(capi, case):
    g = {"10 / 20": lambda: synth.make_pose_graph(10, 20), "skip rules": SR.skip_rule_graph,
         "interleaved sessions": lambda: synth.interleave_sessions(synth.make_pose_graph(20, 30, seed=1), synth.make_pose_graph(20, 30, seed=2), n_cross=6),
         "chain, Schur-reduced": lambda: chain_with_closures(200)}[case]()
    F, (G, Y, red) = cpu_plan_of_graph(capi, g)
    p = capi.DiagPgo(reduced_numbering=1)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    st = check_device(p, len(F["ij"]), G, Y, red)
    used = p.store()[2]
    assert np.array_equal(np.nonzero(used)[0], np.sort(F["src"]))
    if case == "chain, Schur-reduced":
        assert st["n_eliminated"] > 0                        # the case is what it says
    if case == "interleaved sessions":
        assert not np.all(np.diff(Y["v2b"][G["fixed_eff"] == 0]) > 0)          # not the index order
    p.close()


def test_hub_row_of_300_slots(capi):
    n, fixed, ij, robust = SR.hub_graph(300)
    I12 = np.tile(np.eye(3, 4).reshape(1, 12), (max(n, len(ij)), 1))
    info = np.tile(np.eye(6).reshape(1, 36), (len(ij), 1))
    G, Y, red = cpu_plan(capi, n, fixed, ij, robust, np.full(len(ij), 6.0))
    hub = Y["v2b"][1]
    assert Y["row_ptr"][hub + 1] - Y["row_ptr"][hub] == 300 and {hub, hub + 1} <= set(Y["rb_ptr"].tolist())          # a row block of its own
    p = capi.DiagPgo(reduced_numbering=1)
    p.set_graph(I12[:n], fixed, ij, I12[:len(ij)], info, robust)
    check_device(p, len(ij), G, Y, red)
    p.close()


def test_appended_graph_is_rebuilt_to_the_cpu_plan(capi):
    n1 = 200
    g = chain_with_closures(n1 + 5)
    ed = g["edges"]
    old = (np.asarray(ed["from"]) < n1) & (np.asarray(ed["to"]) < n1)
    first, rest = np.nonzero(old)[0], np.nonzero(~old)[0]
    sub = lambda idx: {k: np.asarray(v)[idx] for k, v in ed.items()}
    g1 = dict(g, nodes_pose=g["nodes_pose"][:n1], nodes_fixed=g["nodes_fixed"][:n1], edges=sub(first))
    F1, (G1, Y1, red1) = cpu_plan_of_graph(capi, g1)
    p = capi.DiagPgo(reduced_numbering=1)
    p.add_graph(g1["nodes_pose"], g1["nodes_fixed"], g1["edges"])
    assert check_device(p, len(F1["ij"]), G1, Y1, red1)["n_eliminated"] > 0
    p.append_graph(g["nodes_pose"][n1:], g["nodes_fixed"][n1:], sub(rest))
    g2 = dict(g, edges=sub(np.concatenate([first, rest])))
    F2, (G2, Y2, red2) = cpu_plan_of_graph(capi, g2)
    st = check_device(p, len(F2["ij"]), G2, Y2, red2)
    assert st["structure_reused"] == 0 and st["n_eliminated"] > 0 and Y2["nb"] > Y1["nb"]
    # ... and is the old graph grown: the numbering history of the handle stays
    assert capi.pgo_structure_plan("grown", old=(n1, g1["nodes_fixed"], F1["ij"]), new=(n1 + 5, g["nodes_fixed"], F2["ij"]))["grown"]
    p.close()
