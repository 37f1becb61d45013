"""CPU tests (no GPU): the restatement tests/merge_reference.py itself, the parity target of uzl_merge_*.  The recursive walk of
getNodesWithinHops is not a breadth-first ball; these tests pin where the two differ, and that the random scene the device is held to
(tests/test_merge_gpu.py) is one on which they differ often."""
import numpy as np
import pytest

import merge_scenes as S
from merge_reference import MergeReference


@pytest.fixture(scope="module")
def laps():
    sc = S.random_laps()
    r = S.reference_of(sc)
    return sc, r, r.partners(sc["center"], sc["radius"]), r.partners(sc["center"], sc["radius"], use_ball=True)


def test_the_four_edge_gadget_depends_on_the_edge_order():
    a, b = S.reference_of(S.gadget(False, shift=0)), S.reference_of(S.gadget(True, shift=0))
    assert a.walk(0) == {0, 1, 2} and a.ball(0) == {0, 1, 2, 3}              # node 3 is two hops away and missed
    assert b.walk(0) == {0, 1, 2, 3}
    assert list(a.partners(S.FAR, 0.0)) == [-1, -1, -1, -1] and list(b.partners(S.FAR, 0.0))[0] == 3


def test_the_same_at_ten_hops():
    a, b = S.reference_of(S.long_gadget(False)), S.reference_of(S.long_gadget(True))
    assert 12 not in a.walk(1) and 12 in a.ball(1) and 12 in b.walk(1)
    assert a.partners(S.FAR, 0.0)[1] == -1 and b.partners(S.FAR, 0.0)[1] == 12


def test_hop_limit_on_a_chain():
    assert S.reference_of(S.chain_of_12(10)).partners(S.FAR, 0.0)[1] == 11
    assert S.reference_of(S.chain_of_12(11)).partners(S.FAR, 0.0)[1] == -1
    r = MergeReference(max_hops=0)
    sc = S.chain_of_12(1)
    r.set_graph(sc["poses"], sc["edges"])
    assert r.walk(1) == {1} and (r.partners(S.FAR, 0.0) == -1).all()


def test_the_walk_is_a_subset_of_the_ball(laps):
    sc, r, _, _ = laps
    adj = r.rows()
    strict = 0
    for v in range(r.n):
        w, b = r.walk(v, adj=adj), r.ball(v, adj=adj)
        assert w <= b and v in w
        strict += w != b
    assert strict > 0
    for hops in (0, 1, 2, 5):
        for v in (0, 17, 319):
            assert r.walk(v, hops, adj) <= r.ball(v, hops, adj)


def test_the_random_scene_meets_its_conditions(laps):
    sc, r, walk, ball = laps
    assert r.n == 320 and 480 <= len(sc["edges"]) <= 520
    invalid = float(np.mean(sc["edges"]["valid"] == 0))
    assert 0.10 < invalid < 0.20
    assert int((walk >= 0).sum()) >= 100
    assert int(((walk != ball) & (walk >= 0)).sum()) >= 20                   # min Q under the walk is not min Q under the ball
    none = r.partners(sc["none"]["center"], sc["none"]["radius"])
    half = r.partners(sc["half"]["center"], sc["half"]["radius"])
    eligible = sum(r.is_start(v, sc["half"]["center"], sc["half"]["radius"]) for v in range(r.n))
    assert (none == -1).all() and 100 <= eligible <= 220 and 0 < (half >= 0).sum() < (walk >= 0).sum()


def test_search_is_the_first_start_with_a_partner(laps):
    sc, r, walk, _ = laps
    hits = np.flatnonzero(walk >= 0)
    for first in (0, 1, int(hits[3]), int(hits[3]) + 1, r.n - 1, r.n, r.n + 5):
        keep, drop, nxt = r.search(first, sc["center"], sc["radius"])
        f = 1 if first >= r.n else first
        later = hits[hits >= f]
        if len(later):
            i = int(later[0])
            assert (keep, drop, nxt) == (max(i, walk[i]), min(i, walk[i]), i)
        else:
            assert (keep, drop, nxt) == (-1, -1, r.n)
    with pytest.raises(ValueError):
        r.search(-1, sc["center"], sc["radius"])


def test_scene_claims():
    """the assertions inside the scene builders run here, on the CPU"""
    for exactly in (True, False):
        S.distance_edge(exactly); S.start_edge(exactly)
    for axis in S.AXES:
        for deg in S.ANGLES:
            S.rotated_pair(axis, deg)
    r = S.reference_of(S.hub_with_visited_head())
    assert r.partners(S.FAR, 0.0)[1] == 74
    r = S.reference_of(S.several())
    assert r.qualifying(6) == [2, 4, 5] and r.close(6, 0)
