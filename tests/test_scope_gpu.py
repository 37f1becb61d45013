"""GPU tests of uzl_scope_* (node uncertainty and local scope): distance_ and uncertainty_ equal the CPU restatement
tests/scope_reference.py bit for bit (compared as uint64), id lists exactly, on the smallest scenes at which each piece can go wrong
(tests/scope_scenes.py): degenerate sizes, sums that differ by association, ties, parallel edges, self-loops, every branch of
reevaluate(id), chains / rings / combs with the bound on the barrier rounds, a hub, both sides of the LDS bound, random graphs driven
through set_poses / set_valid / add, the float radius of request, select's bitmap, and poses read from a solver handle."""
import math

import numpy as np
import pytest

import scope_scenes as S
from scope_reference import DBL_MAX, ScopeReference
from uzliti_slam_amd import synth

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def pair(capi, sc, **cfg):
    h = capi.Scope(**cfg)
    h.set_graph(sc["poses"], sc["unc"], sc["edges"])
    return h, S.reference_of(sc, **cfg)


def same(h, r):
    assert np.array_equal(bits(h.distance()), bits(r.distance()))
    assert np.array_equal(bits(h.uncertainty()), bits(r.uncertainty()))


def step(h, r, node=-1):
    got, want = h.reevaluate(node), r.reevaluate(node)
    assert got == want
    same(h, r)
    return got


# ------------------------------------------------------------------------------------------------ degenerate sizes
def test_degenerate_sizes(capi):
    for name, sc in S.degenerate().items():
        h, r = pair(capi, sc)
        start, reached = step(h, r)
        assert start == 0 and reached == (2 if name == "n2_valid" else 1), name
        if name in ("n2_invalid", "n2_laser_only"):
            assert h.distance()[1] == DBL_MAX and h.uncertainty()[1] == 7.0
        if name == "n2_valid":
            assert h.uncertainty()[1] == 3.0                               # |(1, 2, 2)|
        assert h.uncertainty()[0] == 0.0
        h.close()


# ------------------------------------------------------------------------------------------------ the fixed-point claim
@pytest.mark.parametrize("name", list(S.fixed_point_scenes()))
def test_fixed_point_gadgets(capi, name):
    sc = S.fixed_point_scenes()[name]
    h, r = pair(capi, sc)
    step(h, r)
    if name.startswith("assoc"):
        a, b, c = S.association_triple()
        assert h.distance()[3] == min((a + b) + c, (a + c) + b) != max((a + b) + c, (a + c) + b)
    for node in range(len(sc["poses"])):
        step(h, r, node)
    h.close()


# ------------------------------------------------------------------------------------------------ reevaluate(id)
def test_second_component_and_initial_uncertainty(capi):
    sc = S.two_components()
    h, r = pair(capi, sc)
    assert step(h, r, 5) == (3, 3)
    u = h.uncertainty()
    assert list(u[:3]) == [7.0, 0.25, 0.5]                                 # the other component is untouched
    assert u[3] == 2.5 and u[4] == 2.5 + 1.5 and u[5] == 2.5 + (1.5 + 2.25)
    assert step(h, r, 4) == (3, 3)
    h.close()


def test_joined_to_its_minimum_by_an_invalid_edge_only(capi):
    h, r = pair(capi, S.behind_an_invalid_edge())
    assert step(h, r, 5) == (3, 1)
    assert h.uncertainty()[5] == 200.0 and h.distance()[5] == DBL_MAX
    assert step(h, r, 100) == (-1, 0)                                      # no such node: nothing changes
    h.close()


def test_two_calls_in_sequence(capi):
    h, r = pair(capi, S.two_components())
    assert step(h, r, -1) == (0, 3) and h.uncertainty()[0] == 0.0          # the 7.0 of node 0 is overwritten ...
    assert step(h, r, 2) == (0, 3) and h.uncertainty()[1] == 1.0           # ... and read by the next call
    h.set_uncertainty(0, 4.0); r.set_uncertainty(0, 4.0)
    assert step(h, r, 1) == (0, 3) and h.uncertainty()[1] == 5.0
    h.close()


# ------------------------------------------------------------------------------------------------ chains, rings, combs
CHAINS = {"chain": lambda: S.chain(), "chain_shuffled": lambda: S.chain(shuffled=True), "comb": lambda: S.comb(),
          "comb_long": lambda: S.comb(4096, 64, 7)}


@pytest.mark.parametrize("name", list(CHAINS))
def test_the_walk_bounds_the_rounds(capi, name):
    """rounds <= (nodes of degree != 2) + 2 - a condition on the design: lanes walk through nodes of degree 2, so only the source and
    nodes of another degree are ever on a frontier, and every round settles at least one of them for good (the one of the smallest
    label).  The hop depth of the chains and of the long comb is over ten times the bound (checked in round_bound); the 512-node
    comb of 130 such nodes has a hop depth of some 520, four times its bound of 132: a pass of one round per hop fails there too."""
    sc = CHAINS[name]()
    n = len(sc["poses"])
    h, r = pair(capi, sc)
    source = 0
    bound = S.round_bound(sc, source, 3 if name == "comb" else 10)
    if name.startswith("chain"):
        assert bound == 4
    assert step(h, r) == (0, n)
    st = h.stats()
    print(name, "rounds", st["rounds"], "bound", bound, "relaxations", st["relaxations"])
    assert 1 <= st["rounds"] <= bound and st["in_lds"] == 1
    if name.startswith("chain"):
        mid = int(np.argsort(r.distance())[n // 2])                       # the middle of the chain: start is node 0 anyway
        assert step(h, r, mid) == (0, n)
        assert h.stats()["rounds"] <= bound
    h.close()


@pytest.mark.parametrize("zero", [True, False], ids=["coincident", "positive"])
def test_rings_terminate(capi, zero):
    sc = S.ring(zero=zero)
    h, r = pair(capi, sc)
    assert step(h, r) == (0, 64)
    if zero:
        assert not h.distance().any()
    assert step(h, r, 40) == (0, 64)
    h.close()


# ------------------------------------------------------------------------------------------------ hub, storage boundary
def test_hub_with_more_neighbours_than_lanes(capi):
    sc = S.hub()
    h, r = pair(capi, sc)
    assert step(h, r) == (0, len(sc["poses"]))
    assert step(h, r, 700) == (0, len(sc["poses"]))
    h.close()


@pytest.mark.parametrize("over", [0, 1], ids=["at_the_bound", "one_above"])
def test_both_sides_of_the_lds_bound(capi, over):
    bound = capi.lib().uzl_scope_lds_nodes()
    assert bound == capi.SCOPE_LDS_NODES
    sc = S.loopy(bound + over, 77)
    h, r = pair(capi, sc)
    start, reached = step(h, r)
    assert start == 0 and reached > bound // 2
    assert h.stats()["in_lds"] == 1 - over
    step(h, r, bound - 1 + over)
    h.close()


# ------------------------------------------------------------------------------------------------ random graphs
@pytest.mark.parametrize("n,e,seed", [(200, 700, 5), (2000, 7000, 6)], ids=["200_700", "2000_7000"])
def test_random_graphs_through_every_update(capi, n, e, seed):
    sc = S.synth_graph(n, e, seed)
    h, r = pair(capi, sc)
    step(h, r)
    h.set_poses(sc["poses2"]); r.set_poses(sc["poses2"])
    step(h, r)
    flags = 1 - sc["edges"]["valid"][sc["flips"]]
    h.set_valid(sc["flips"], flags); r.set_valid(sc["flips"], flags)
    step(h, r)
    step(h, r, n - 1)
    h.add(sc["add_poses"], sc["add_unc"], sc["add_edges"]); r.add(sc["add_poses"], sc["add_unc"], sc["add_edges"])
    assert np.array_equal(bits(h.uncertainty()), bits(r.uncertainty()))
    step(h, r)
    step(h, r, n + 49)
    for cur in (0, n // 2, n + 49):
        radius, ids = h.request(cur)
        want_radius, want = r.request(cur)
        assert radius == want_radius and np.array_equal(ids, want)
    h.close()


# ------------------------------------------------------------------------------------------------ request
def _request_pair(capi, planted, unc0, **cfg):
    P, at = S.request_scene(planted)
    unc = np.zeros(len(P)); unc[0] = unc0
    h = capi.Scope(**cfg); r = ScopeReference(**cfg)
    h.set_graph(P, unc, None); r.set_graph(P, unc, None)
    return h, r, at


def test_request_at_the_radius_and_the_next_double(capi):
    h, r, at = _request_pair(capi, [12.0, math.nextafter(12.0, 13.0), math.nextafter(12.0, 0.0)], 1.0)     # scope_size_min wins: 8 + 4
    radius, ids = h.request(0)
    want_radius, want = r.request(0)
    assert radius == want_radius == 8.0 and np.array_equal(ids, want)
    assert at[0] not in ids and at[1] in ids and at[2] not in ids          # strict >: the node at the radius stays in
    assert len(ids) > 2048                                                 # hits from every slab of the scan
    small = h.request(0, cap=7)[1]
    assert h.last_total == len(want) and np.array_equal(small, want[:7])   # cap below the count: the total, and cap entries
    none = h.request(0, cap=0)[1]
    assert h.last_total == len(want) and len(none) == 0
    h.close()


@pytest.mark.parametrize("down", [True, False], ids=["float_rounds_down", "float_rounds_up"])
def test_request_uses_the_float_radius(capi, down):
    u, s, f, d = S.rounding_radius(down)
    h, r, at = _request_pair(capi, [d, f, s], u)
    radius, ids = h.request(0)
    want_radius, want = r.request(0)
    assert radius == want_radius == 0.1 * u > 8.0 and np.array_equal(ids, want)
    assert (at[0] in ids) == (d > f) != (d > s)                            # the float decides, the double would say otherwise
    assert at[1] not in ids
    h.close()


# ------------------------------------------------------------------------------------------------ select
def test_select(capi):
    P, at = S.request_scene([20.0, math.nextafter(20.0, 0.0)])
    h = capi.Scope(); r = ScopeReference()
    h.set_graph(P, None, None); r.set_graph(P, None, None)
    n = len(P)
    origin = (0.0, 0.0, 0.0)
    inside = r.select(origin, 20.0, [])
    assert 100 < len(inside) < n
    assert np.array_equal(h.select(origin, 20.0, []), inside)                                  # have empty
    assert at[0] not in inside and at[1] in inside                                             # strict <: the node at the radius is out
    assert len(h.select(origin, 20.0, np.arange(n))) == 0                                      # have = all
    have = np.concatenate([inside[::3], inside[::3], [-1, n, n + 5, 2**31 - 1, -2**31]])       # duplicates, ids the graph lacks
    assert np.array_equal(h.select(origin, 20.0, have), r.select(origin, 20.0, have))
    centre = (3.25, -7.5, 11.0)                                                                # no node's position
    assert np.array_equal(h.select(centre, 25.0, inside[:50]), r.select(centre, 25.0, inside[:50]))
    got = h.select(centre, 25.0, [], cap=5)
    assert h.last_total == len(r.select(centre, 25.0, [])) and np.array_equal(got, r.select(centre, 25.0, [])[:5])
    assert len(h.select(centre, 0.0, [])) == 0
    h.close()


# ------------------------------------------------------------------------------------------------ poses from the solver
def test_poses_from_pgo_equal_its_host_read_back(capi):
    g = synth.make_pose_graph(100, 300)
    pgo = capi.Pgo()
    pgo.add_graph(g["nodes_pose"], g["nodes_fixed"], g["edges"])
    pgo.optimize(10)
    solved = pgo.store()[0]
    assert np.abs(solved - np.asarray(g["nodes_pose"]).reshape(100, 12)).max() > 1e-6          # the solve moved the poses
    ed = g["edges"]
    E = capi.gate_edges(ed["from"], ed["to"], ed["type"], valid=ed["valid"])
    a = capi.Scope(); b = capi.Scope()
    a.set_graph(g["nodes_pose"], None, E); b.set_graph(g["nodes_pose"], None, E)
    a.poses_from_pgo(pgo)
    b.set_poses(solved)
    assert a.reevaluate() == b.reevaluate() == (0, 100)
    assert np.array_equal(bits(a.uncertainty()), bits(b.uncertainty())) and np.array_equal(bits(a.distance()), bits(b.distance()))
    r = ScopeReference(); r.set_graph(solved, None, E); r.reevaluate()
    assert np.array_equal(bits(a.uncertainty()), bits(r.uncertainty()))
    after = pgo.store()[0]
    assert np.array_equal(bits(after), bits(solved))                                           # the solver was only read
    short = capi.Scope(); short.set_graph(g["nodes_pose"][:50], None, None)
    with pytest.raises(capi.UzlError) as e:
        short.poses_from_pgo(pgo)
    assert e.value.status == capi.UZL_ERR_BAD_ARG
    empty = capi.Pgo()
    with pytest.raises(capi.UzlError) as e:
        a.poses_from_pgo(empty)
    assert e.value.status == capi.UZL_ERR_STATE
    for x in (a, b, short, empty, pgo):
        x.close()
