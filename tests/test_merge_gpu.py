"""GPU tests of uzl_merge_* (node merging): partner(i) of every node and the tick equal the CPU restatement tests/merge_reference.py
exactly, on the smallest scenes at which each piece can go wrong (tests/merge_scenes.py): degenerate sizes, the order dependence of
the reference's recursive walk, the hop limit, invalid / laser / self-loop / parallel edges, rows around the 64 entries a wave loads
per step, node counts around the words of the visited bitmap, every threshold at its edge, the choice among several qualifying
nodes, two ticks with the plan applied in between, many starts in one launch, and poses read from a solver handle."""
import math

import numpy as np
import pytest

import merge_scenes as S
from uzliti_slam_amd import synth
from uzliti_slam_amd.merge import apply_merge_plan

pytestmark = pytest.mark.gpu


def pair(capi, sc):
    h = capi.Merge(**sc["cfg"])
    h.set_graph(sc["poses"], sc["edges"])
    return h, S.reference_of(sc)


def same(h, r, center, radius, firsts=None):
    """the whole table and the ticks from the given first indices -> the table"""
    got, want = h.partners(center, radius), r.partners(center, radius)
    assert np.array_equal(got, want)
    n = r.n
    for first in sorted(set(v for v in ((0, 1, n - 1, n, n + 5) if firsts is None else firsts) if v >= 0)):
        assert h.search(first, center, radius) == r.search(first, center, radius), first
    return got


def check(capi, sc, firsts=None):
    h, r = pair(capi, sc)
    table = same(h, r, sc["center"], sc["radius"], firsts)
    h.close()
    return table


# ------------------------------------------------------------------------------------------------ sizes
def test_sizes(capi):
    for name, sc in S.sizes().items():
        h, r = pair(capi, sc)
        table = same(h, r, sc["center"], sc["radius"])
        if name == "n2":
            assert list(table) == [1, -1]                                  # node 0 is never a partner, but an ordinary start
            assert h.search(0, S.FAR, 0.0) == (1, 0, 0) and h.search(1, S.FAR, 0.0) == (-1, -1, 2) == h.search(2, S.FAR, 0.0)
        else:
            assert (table == -1).all()
        if name in ("n0", "n1"):
            assert h.search(7, S.FAR, 0.0) == (-1, -1, 7)                 # fewer than two nodes: the index stays
        with pytest.raises(capi.UzlError) as e:
            h.search(-1, S.FAR, 0.0)
        assert e.value.status == capi.UZL_ERR_BAD_ARG
        h.close()


# ------------------------------------------------------------------------------------------------ walk order
def test_the_gadget_in_both_edge_orders(capi):
    assert check(capi, S.gadget(False))[1] == -1                           # node 4 is two hops from node 1 and missed
    assert check(capi, S.gadget(True))[1] == 4
    assert check(capi, S.gadget(False, shift=0))[0] == -1 and check(capi, S.gadget(True, shift=0))[0] == 3       # the root as a start


def test_a_chain_of_ten_beside_a_shortcut(capi):
    assert check(capi, S.long_gadget(False))[1] == -1
    assert check(capi, S.long_gadget(True))[1] == 12


def test_no_hops_means_no_partner(capi):
    sc = S.chain_of_12(1)
    sc["cfg"]["max_hops"] = 0
    h, r = pair(capi, sc)
    assert (same(h, r, sc["center"], sc["radius"]) == -1).all()
    assert h.stats() == dict(starts_walked=2, nodes_visited=2)            # the two nodes side by side, each marking itself only
    h.close()


def test_the_hop_limit_on_a_chain(capi):
    t10, t11 = check(capi, S.chain_of_12(10)), check(capi, S.chain_of_12(11))
    assert t10[1] == 11 and t10[11] == 1 and (t11 == -1).all()


# ------------------------------------------------------------------------------------------------ edges
def test_the_only_way_there(capi):
    assert check(capi, S.only_way())[1] == 3
    assert (check(capi, S.only_way(valid=0)) == -1).all()                  # an invalid edge is not followed
    assert check(capi, S.only_way(typ=S.LASER))[1] == 3                    # a laser edge is, unlike in uzl_scope_*


def test_self_loops_and_parallel_edges(capi):
    assert check(capi, S.loops_and_parallels())[1] == 4


def test_set_valid_flips_the_outcome_on_a_live_handle(capi):
    sc = S.only_way()
    h, r = pair(capi, sc)
    assert same(h, r, sc["center"], sc["radius"])[1] == 3
    for flags in ([0], [1], [0]):
        h.set_valid([1], flags); r.set_valid([1], flags)
        assert same(h, r, sc["center"], sc["radius"])[1] == (3 if flags[0] else -1)
    h.close()


# ------------------------------------------------------------------------------------------------ rows
@pytest.mark.parametrize("deg", [63, 64, 65, 130])
def test_a_hub_whose_last_entry_is_the_only_useful_one(capi, deg):
    h, r = pair(capi, S.hub(deg))
    table = same(h, r, S.FAR, 0.0, firsts=(1,))
    assert table[1] == deg + 1 and table[deg + 1] == 1
    assert h.stats() == dict(starts_walked=2, nodes_visited=(deg + 1) + 2)
    h.close()


def test_a_hub_whose_early_entries_are_already_visited(capi):
    assert check(capi, S.hub_with_visited_head(), firsts=(1,))[1] == 74


# ------------------------------------------------------------------------------------------------ bitmap words
@pytest.mark.parametrize("n", [31, 32, 33, 64, 65, 2049])
def test_node_counts_around_the_words_of_the_bitmap(capi, n):
    table = check(capi, S.chain_with_far_pair(n), firsts=(1, n - 1, n))
    assert table[n - 1] == n - 2 and table[n - 2] == n - 1 and (table[:n - 2] == -1).all()


def test_one_node_above_the_bound_is_refused(capi):
    n = capi.MERGE_MAX_NODES + 1
    small = S.chain_with_far_pair(5)
    with capi.Merge() as h:
        h.set_graph(small["poses"], small["edges"])
        with pytest.raises(capi.UzlError) as e:
            h.set_graph(np.zeros((n, 12)), None)
        assert e.value.status == capi.UZL_ERR_BAD_ARG and "uzl_merge_max_nodes" in str(e.value)
        assert h.search(1, S.FAR, 0.0) == (4, 3, 3)                        # nothing changed


# ------------------------------------------------------------------------------------------------ thresholds
def test_the_distance_at_its_edge(capi):
    assert (check(capi, S.distance_edge(True)) == -1).all()                # exactly 0.25: >= rejects
    assert list(check(capi, S.distance_edge(False))) == [-1, 2, 1]


def test_the_start_test_at_its_edge(capi):
    t = check(capi, S.start_edge(False))
    assert t[1] == -1 and t[2] == 1                                        # exactly radius + 6 is not a start; node 2, further out, is
    assert list(check(capi, S.start_edge(True))) == [-1, 2, 1]


@pytest.mark.parametrize("axis", list(S.AXES))
@pytest.mark.parametrize("deg", S.ANGLES)
def test_rotations_on_both_sides_of_the_bound(capi, axis, deg):
    table = check(capi, S.rotated_pair(axis, deg))
    assert list(table) == ([-1, 2, 1] if abs(deg) < 15.0 else [-1, -1, -1])


def test_close_but_turned_then_a_later_node_that_passes_both(capi):
    assert list(check(capi, S.turned_then_straight())) == [-1, 3, -1, 1]


# ------------------------------------------------------------------------------------------------ choice
def test_the_smallest_qualifying_node_wins_and_the_root_never_does(capi):
    table = check(capi, S.several())
    assert table[6] == 2                                                   # of {2, 4, 5}; node 0 qualifies geometrically only


def test_keep_is_the_larger_index_whichever_was_the_start(capi):
    sc = S.two_ticks()
    h, r = pair(capi, sc)
    same(h, r, sc["center"], sc["radius"], firsts=range(0, 17))
    assert h.search(1, S.FAR, 0.0) == (7, 2, 2)                            # start 2, partner 7
    assert h.search(5, S.FAR, 0.0) == (7, 2, 7)                            # start 7, partner 2
    assert h.search(10, S.FAR, 0.0) == (-1, -1, 11)                        # a miss leaves the node count
    assert h.search(11, S.FAR, 0.0) == (7, 2, 2)                           # wrapped to 1
    h.close()


def test_two_ticks_with_the_plan_applied_in_between(capi):
    sc = S.two_ticks()
    h, r = pair(capi, sc)
    P, E, D = sc["poses"], sc["edges"], None
    index, merges = 1, []
    for _ in range(3):
        got = h.search(index, sc["center"], sc["radius"])
        assert got == r.search(index, sc["center"], sc["radius"])
        keep, drop, index = got
        if keep < 0:
            break
        plan, want = h.plan(keep, drop, 2, 1), r.plan(keep, drop, 2, 1)
        assert np.array_equal(plan["action"], want["action"]) and plan["ratio"] == want["ratio"] == 1.0 / 3.0
        assert (plan["touched"], plan["retargeted"], plan["deleted"]) == (want["touched"], want["retargeted"], want["deleted"])
        for k in ("new_pose", "keep_displacement", "drop_displacement"):
            assert np.array_equal(plan[k], np.array(want[k]))              # the bound of tests/test_merge_plan_cpu.py: 0.0
        P, E, D, old_to_new = apply_merge_plan(P, E, D, plan)
        merges.append((keep, drop))
        h.set_graph(P, E); r.set_graph(P, E)
        assert np.array_equal(h.partners(sc["center"], sc["radius"]), r.partners(sc["center"], sc["radius"]))
    assert merges == [(7, 2), (8, 3)] and len(P) == 9                      # (9, 4) of the first graph, one index lower each
    h.close()


# ------------------------------------------------------------------------------------------------ many starts in one launch
@pytest.fixture(scope="module")
def laps():
    sc = S.random_laps()
    return sc, S.reference_of(sc)


@pytest.mark.parametrize("circle", ["all", "none", "half"])
def test_the_whole_table_of_the_random_scene(capi, laps, circle):
    sc, r = laps
    center, radius = (sc["center"], sc["radius"]) if circle == "all" else (sc[circle]["center"], sc[circle]["radius"])
    with capi.Merge() as h:
        h.set_graph(sc["poses"], sc["edges"])
        table = same(h, r, center, radius, firsts=(0, 1, 160, 319, 320))
        st = h.stats()
    hits = int((table >= 0).sum())
    assert {"all": hits >= 100, "none": hits == 0, "half": 0 < hits < 200}[circle]
    assert st["starts_walked"] >= hits and (st["starts_walked"] == 0) == (circle == "none")


def test_poses_from_a_solver_handle(capi, laps):
    """poses_from_pgo leaves the bits the solver's own read-back would hand to set_poses: same table, same plan"""
    sc, r = laps
    g = synth.make_pose_graph(320, 900, seed=11)
    p = capi.Pgo(device=0)
    p.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    p.optimize(3)
    solved, _, _ = p.store()
    ed = g["edges"]
    E = capi.gate_edges(ed["from"], ed["to"], ed["type"], valid=ed["valid"])
    cfg = dict(max_distance=2.5, max_rotation_deg=60.0)                    # a graph drawn for the solver: wider gates find partners
    a, b = capi.Merge(**cfg), capi.Merge(**cfg)
    a.set_graph(g["nodes_pose"], E); a.poses_from_pgo(p)
    b.set_graph(g["nodes_pose"], E); b.set_poses(solved)
    ref = S.MergeReference(**cfg); ref.set_graph(solved, E)
    ta, tb = a.partners(S.FAR, 0.0), b.partners(S.FAR, 0.0)
    assert np.array_equal(ta, tb) and np.array_equal(ta, ref.partners(S.FAR, 0.0)) and (ta >= 0).sum() > 0
    i = int(np.flatnonzero(ta >= 0)[0])
    pa, pb = a.plan(max(i, ta[i]), min(i, ta[i])), b.plan(max(i, ta[i]), min(i, ta[i]))
    assert np.array_equal(pa["new_pose"], pb["new_pose"]) and np.array_equal(pa["action"], pb["action"])
    other = capi.Merge(); other.set_graph(g["nodes_pose"][:5], None)
    with pytest.raises(capi.UzlError) as e:
        other.poses_from_pgo(p)                                            # another node count
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    for h in (a, b, other):
        h.close()
    p.close()
