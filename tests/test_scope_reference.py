"""CPU tests of tests/scope_reference.py, the checker of uzl_scope_*: its dijkstra against scipy's on the random scenes, and the claim the
device pass rests on - the reference's distance_ is the least fixed point of d[u] = min fl(d[v] + w), so any label-correcting order ends
in the same bits - checked with a second loop of another order (Bellman-Ford sweeps over all edges at once) on every scene."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

import scope_scenes as S
from scope_reference import DBL_MAX, TYPE_2D_LASER, ScopeReference


def _all_scenes():
    out = {}
    out.update(S.degenerate())
    out.update(S.fixed_point_scenes())
    out["two_components"] = S.two_components()
    out["behind_invalid"] = S.behind_an_invalid_edge()
    out["chain"] = S.chain()
    out["chain_shuffled"] = S.chain(shuffled=True)
    out["ring_zero"] = S.ring(zero=True)
    out["ring"] = S.ring()
    out["comb"] = S.comb()
    out["hub"] = S.hub()
    out.update(RANDOM)
    return out


RANDOM = {"loopy_2000": S.loopy(2000, 41), "synth_200": S.synth_graph(200, 700, 5), "synth_2000": S.synth_graph(2000, 7000, 6)}
SCENES = _all_scenes()


def _walked(sc):
    E = sc["edges"]
    k = (E["valid"] != 0) & (E["type"] != TYPE_2D_LASER)
    return E["from"][k].astype(np.int64), E["to"][k].astype(np.int64)


def _lengths(sc, a, b):
    t = sc["poses"][:, [3, 7, 11]]
    d = t[a] - t[b]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def bellman_ford(sc, source):
    """sweeps over the edges in both directions at once, from the labels of the sweep before, until a sweep changes nothing (an edge whose
    tail kept its label since the sweep before offers what it offered then, and is left out)"""
    a, b = _walked(sc)
    w = _lengths(sc, a, b)
    frm = np.concatenate([a, b]); to = np.concatenate([b, a]); w2 = np.concatenate([w, w])
    d = np.full(len(sc["poses"]), DBL_MAX)
    d[source] = 0.0
    changed = np.zeros(len(d), bool); changed[source] = True
    sweeps = 0
    while changed.any():
        k = changed[frm]
        new = d.copy()
        np.minimum.at(new, to[k], d[frm[k]] + w2[k])
        sweeps += 1
        changed = new != d
        d = new
    return d, sweeps


@pytest.mark.parametrize("name", list(SCENES))
def test_any_label_correcting_order_ends_in_the_same_bits(name):
    sc = SCENES[name]
    r = S.reference_of(sc)
    for source in sorted({0, len(sc["poses"]) // 2, len(sc["poses"]) - 1}):
        r.dijkstra(source)
        d, _ = bellman_ford(sc, source)
        assert np.array_equal(r.distance().view(np.uint64), d.view(np.uint64)), (name, source)


@pytest.mark.parametrize("name", list(RANDOM))
def test_dijkstra_against_scipy(name):
    sc = RANDOM[name]
    n = len(sc["poses"])
    a, b = _walked(sc)
    keep = a != b
    a, b = a[keep], b[keep]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    pairs = np.unique(np.stack([lo, hi], 1), axis=0)                    # parallel edges have one length: keep one of each
    w = _lengths(sc, pairs[:, 0], pairs[:, 1])
    assert (w > 0).all()
    G = sp.csr_matrix((w, (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    r = S.reference_of(sc)
    for source in (0, n // 3):
        r.dijkstra(source)
        mine = r.distance()
        ref = dijkstra(G, directed=False, indices=source)
        reached = mine != DBL_MAX
        assert np.array_equal(reached, np.isfinite(ref))
        assert 0 < reached.sum()
        assert np.all(np.abs(mine[reached] - ref[reached]) <= 1e-12 * np.maximum(ref[reached], 1e-300))


def test_the_scenes_say_what_they_claim():
    a, b, c = S.association_triple()
    assert (a + b) + c != (a + c) + b
    sc = S.association_gadget(False)
    r = S.reference_of(sc)
    r.dijkstra(0)
    assert r.dist[3] == min((a + b) + c, (a + c) + b) and r.dist[6] == r.dist[3] + 1.0
    # hop depth against the round bound: a pass that needs one barrier round per hop cannot meet it
    assert S.round_bound(S.chain(), 0, 10) == 4
    assert S.round_bound(S.chain(shuffled=True), 0, 1) == 4
    assert S.round_bound(S.comb(4096, 64, 7), 0, 10) == 132
    # the 512-node comb has 130 nodes of degree != 2 and a hop depth of some 520: beyond the bound, not ten times beyond
    assert S.round_bound(S.comb(), 0, 3) == 132
    for down in (True, False):
        u, s, f, d = S.rounding_radius(down)
        assert (f < s) == down and 0.1 * u > 8.0


def test_reevaluate_branches_of_the_restatement():
    sc = S.two_components()
    r = S.reference_of(sc)
    assert r.reevaluate(5) == (3, 3)
    assert r.unc[:3] == [7.0, 0.25, 0.5] and r.unc[3] == 2.5 and r.unc[4] == 2.5 + 1.5 and r.unc[5] == 2.5 + (1.5 + 2.25)
    r = S.reference_of(S.behind_an_invalid_edge())
    assert r.reevaluate(5) == (3, 1) and r.unc[5] == 200.0 and r.unc[4] == 100.0
    assert r.reevaluate(6) == (-1, 0)
    r = S.reference_of(sc)
    assert r.reevaluate(-1) == (0, 3) and r.unc[0] == 0.0               # overwrites the 7.0 ...
    assert r.reevaluate(2) == (0, 3) and r.unc[1] == 1.0                # ... and the second call reads that
    rq = ScopeReference()
    rq.set_graph(S.poses_at([(0, 0, 0), (12, 0, 0), (np.nextafter(12.0, 13.0), 0, 0)]), [0.0, 0.0, 0.0], None)
    assert rq.request(0)[0] == 8.0 and list(rq.request(0)[1]) == [2]
    assert list(rq.select((0, 0, 0), 12.0, [0])) == [] and list(rq.select((0, 0, 0), 12.5, [0, 0, 99])) == [1, 2]
