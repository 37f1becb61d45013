"""Scenes for the uzl_scope_* tests: the smallest graphs at which each piece of the uncertainty pass and of the scope scans can go
wrong.  Every scene is a dict(poses (n,12), unc (n), edges GATE_EDGE_DTYPE); what a scene claims about itself (a sum that differs in
its last bit, a hop depth far beyond the round bound, a float and a double verdict that differ) is asserted here, on the CPU."""
import math
from collections import deque

import numpy as np

from uzliti_slam_amd import capi, synth
from scope_reference import TYPE_2D_LASER, ScopeReference

FULL = 1            # UZL_EDGE_TYPE_3D_FULL
FULL_2D = 101


def poses_at(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    P = np.tile(np.eye(3, 4).reshape(1, 12), (len(xyz), 1))
    P[:, 3] = xyz[:, 0]; P[:, 7] = xyz[:, 1]; P[:, 11] = xyz[:, 2]
    return P


def edges_of(pairs, typ=FULL, valid=1):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    return capi.gate_edges(pairs[:, 0], pairs[:, 1], np.broadcast_to(typ, n), valid=np.broadcast_to(valid, n))


def scene(xyz, pairs, typ=FULL, valid=1, unc=None):
    P = poses_at(xyz)
    return dict(poses=P, unc=np.zeros(len(P)) if unc is None else np.asarray(unc, np.float64), edges=edges_of(pairs, typ, valid))


def reference_of(sc, **cfg):
    r = ScopeReference(**cfg)
    r.set_graph(sc["poses"], sc["unc"], sc["edges"])
    return r


# ------------------------------------------------------------------------------------------------ degenerate sizes
def degenerate():
    two = [(0, 0, 0), (1, 2, 2)]
    return {
        "n1": scene([(0, 0, 0)], [], unc=[3.0]),
        "n2_valid": scene(two, [(0, 1)], unc=[5.0, 7.0]),
        "n2_invalid": scene(two, [(0, 1)], valid=0, unc=[5.0, 7.0]),
        "n2_laser_only": scene(two, [(0, 1)], typ=TYPE_2D_LASER, unc=[5.0, 7.0]),
    }


# ------------------------------------------------------------------------------------------------ the fixed-point claim
def association_triple(seed=1):
    """(a, b, c) with (a + b) + c != (a + c) + b, the two one ulp apart"""
    rng = np.random.default_rng(seed)
    while True:
        a, b, c = (float(v) for v in rng.uniform(0.1, 3.0, 3))
        s1, s2 = (a + b) + c, (a + c) + b
        if s1 != s2 and (math.nextafter(s1, s2) == s2):
            return a, b, c


def association_gadget(swap):
    """Two routes from node 0 to node 3 whose lengths are (a+b)+c and (a+c)+b: axis-aligned legs, so every edge length is exactly a, b or
    c (sqrt(v*v) == |v| in binary floating point).  Node 6 hangs off node 3 and inherits the smaller sum.  swap: the routes trade indices."""
    a, b, c = association_triple()
    if swap:
        b, c = c, b
    assert (a + b) + c != (a + c) + b
    for v in (a, b, c):
        assert math.sqrt(v * v) == v
    xyz = [(0, 0, 0), (a, 0, 0), (a, b, 0), (a, b, c), (a, 0, 0), (a, 0, c), (a, b, c + 1.0)]
    return scene(xyz, [(0, 1), (1, 2), (2, 3), (0, 4), (4, 5), (5, 3), (3, 6)])


def fixed_point_scenes():
    square = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 1, 2)]
    out = {
        "assoc": association_gadget(False),
        "assoc_swapped": association_gadget(True),
        "exact_tie": scene(square, [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4)]),
        # the same pair joined four times: a 3-D edge, a 2-D edge, a laser edge (ignored) and an invalid one (ignored)
        "parallel": dict(poses=poses_at(square[:3]), unc=np.zeros(3),
                         edges=capi.gate_edges([0, 1, 0, 0, 1], [1, 0, 1, 1, 2], [FULL, FULL_2D, TYPE_2D_LASER, FULL, FULL], valid=[1, 1, 1, 0, 1])),
        "self_loop": scene(square[:3], [(0, 1), (1, 1), (1, 2), (2, 2)]),
    }
    return out


# ------------------------------------------------------------------------------------------------ reevaluate(id)
def two_components():
    """A = {0, 1, 2} and B = {3, 4, 5}, both chains; B's oldest node carries a non-zero uncertainty"""
    xyz = [(0, 0, 0), (1, 0, 0), (2, 0.5, 0), (10, 0, 0), (10, 1.5, 0), (10, 1.5, 2.25)]
    return scene(xyz, [(0, 1), (1, 2), (3, 4), (4, 5)], unc=[7.0, 0.25, 0.5, 2.5, 100.0, 200.0])


def behind_an_invalid_edge():
    """3 - 4 is invalid, 4 - 5 valid: oldestReachableNode(5) is 3 (it walks invalid edges), dijkstra from 3 reaches 3 alone"""
    sc = two_components()
    sc["edges"]["valid"][2] = 0
    return sc


# ------------------------------------------------------------------------------------------------ chains, rings, combs
def _trajectory(n, seed):
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.uniform(-0.3, 0.3, (n, 3)) + np.array([0.2, 0.0, 0.0]), axis=0)


def chain(n=4096, seed=3, shuffled=False):
    xyz = _trajectory(n, seed)
    order = np.arange(n)
    if shuffled:
        order = np.random.default_rng(seed + 1).permutation(n)          # order[k] = index of the k-th node along the chain
    P = np.zeros((n, 3)); P[order] = xyz
    return scene(P, np.stack([order[:-1], order[1:]], 1))


def ring(n=64, zero=False):
    ang = 2 * np.pi * np.arange(n) / n
    xyz = np.zeros((n, 3)) if zero else np.stack([3 * np.cos(ang), 3 * np.sin(ang), 0.1 * np.sin(3 * ang)], 1)
    return scene(xyz, [(i, (i + 1) % n) for i in range(n)])


def comb(spine=512, every=8, tooth=7, seed=5):
    """a spine with a `tooth`-node tooth on every `every`-th node (from node every // 2 on)"""
    sp = _trajectory(spine, seed)
    xyz = [tuple(p) for p in sp]
    pairs = [(i, i + 1) for i in range(spine - 1)]
    rng = np.random.default_rng(seed + 1)
    for j in range(every // 2, spine, every):
        prev, at = j, sp[j].copy()
        for _ in range(tooth):
            at = at + np.array([0.0, 0.2, 0.0]) + rng.uniform(-0.05, 0.05, 3)
            xyz.append(tuple(at)); pairs.append((prev, len(xyz) - 1)); prev = len(xyz) - 1
    return scene(xyz, pairs)


def degrees(sc):
    d = np.zeros(len(sc["poses"]), np.int64)
    for e in sc["edges"]:
        if e["valid"] and e["type"] != TYPE_2D_LASER:
            d[e["from"]] += 1
            if e["to"] != e["from"]:
                d[e["to"]] += 1
    return d


def hop_depth(sc, source):
    r = reference_of(sc)
    hops = {source: 0}
    q = deque([source])
    while q:
        v = q.popleft()
        for u in r.neighbors(v, True):
            if u not in hops:
                hops[u] = hops[v] + 1; q.append(u)
    return max(hops.values())


def round_bound(sc, source, factor):
    """(nodes of degree != 2) + 2, the bound on the barrier rounds of a pass; asserts that the scene's hop depth is at least `factor`
    times that, so that a pass needing one round per hop cannot meet it"""
    bound = int((degrees(sc) != 2).sum()) + 2
    depth = hop_depth(sc, source)
    assert depth >= factor * bound, (depth, bound)
    return bound


# ------------------------------------------------------------------------------------------------ hub, storage boundary
def hub(leaves=1500, seed=9):
    """node 0 joined to `leaves` leaves at distinct distances; every tenth leaf has a child of its own"""
    rng = np.random.default_rng(seed)
    d = np.linspace(0.5, 40.0, leaves) + rng.uniform(0, 0.01, leaves)
    assert len(np.unique(d)) == leaves
    dirs = rng.normal(size=(leaves, 3)); dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    xyz = [(0.0, 0.0, 0.0)] + [tuple(p) for p in d[:, None] * dirs]
    pairs = [(0, 1 + i) for i in range(leaves)]
    for i in range(0, leaves, 10):
        xyz.append(tuple(np.array(xyz[1 + i]) + rng.uniform(-1, 1, 3))); pairs.append((1 + i, len(xyz) - 1))
    return scene(xyz, pairs)


def loopy(n, seed, n_loops=None, invalid_frac=0.1, laser_frac=0.1):
    """a trajectory of n nodes with loop closures between nodes that lie close, about 10 % invalid and 10 % laser edges"""
    rng = np.random.default_rng(seed)
    xyz = _trajectory(n, seed)
    n_loops = n // 2 if n_loops is None else n_loops
    a = rng.integers(0, n, n_loops); b = np.clip(a + rng.integers(-400, 400, n_loops), 0, n - 1)
    pairs = np.concatenate([np.stack([np.arange(n - 1), np.arange(1, n)], 1), np.stack([a, b], 1)])
    m = len(pairs)
    typ = np.where(rng.random(m) < laser_frac, TYPE_2D_LASER, np.where(rng.random(m) < 0.5, FULL, FULL_2D))
    valid = (rng.random(m) >= invalid_frac).astype(np.int32)
    sc = scene(xyz, pairs, typ=typ, valid=valid, unc=rng.uniform(0, 5, n))
    return sc


def synth_graph(n, e, seed, extra_nodes=50):
    """the gate tests' trajectory + loop-closure generator with n + extra nodes, cut into the first n nodes with the edges among them and
    the rest (to be added); about 10 % invalid and 10 % laser edges; a second set of poses (perturbed); 20 flags to flip"""
    nt = n + extra_nodes
    g = synth.make_pose_graph(nt, e + (extra_nodes * e) // n, seed=seed)
    ed = g["edges"]
    rng = np.random.default_rng(seed + 17)
    m = len(ed["from"])
    typ = np.where(rng.random(m) < 0.1, TYPE_2D_LASER, ed["type"])
    valid = (rng.random(m) >= 0.1).astype(np.int32)
    E = capi.gate_edges(ed["from"], ed["to"], typ, valid=valid)
    old = (E["from"] < n) & (E["to"] < n)
    P = np.asarray(g["nodes_pose"], np.float64).reshape(nt, 12)
    unc = rng.uniform(0, 3, nt)
    P2 = P[:n].copy()
    P2[:, [3, 7, 11]] += rng.normal(0, 0.05, (n, 3))
    flips = rng.choice(int(old.sum()), 20, replace=False)
    return dict(poses=P[:n], unc=unc[:n], edges=E[old], poses2=P2, flips=flips,
                add_poses=P[n:], add_unc=unc[n:], add_edges=E[~old])


# ------------------------------------------------------------------------------------------------ request / select
def cloud(n=5000, seed=21, spread=30.0):
    """n scattered nodes, more than two slabs of the scan kernel; node 0 is the current node at the origin"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-spread, spread, (n, 3))
    xyz[0] = 0.0
    return xyz


def rounding_radius(down, factor=0.1, margin=4.0, seed=31):
    """an uncertainty u > 80 (so that factor * u beats scope_size_min = 8) whose current_scope_ + margin is no float and rounds down (or
    up), and a distance strictly between the float and the double value: there the two verdicts of `norm > radius` differ"""
    rng = np.random.default_rng(seed)
    while True:
        u = float(rng.uniform(90.0, 400.0))
        s = factor * u + margin
        f = float(np.float32(s))
        if (f < s) if down else (f > s):
            d = math.nextafter(f, s)
            if d == s:
                continue
            assert min(f, s) < d < max(f, s)
            assert (d > f) != (d > s)                                  # the float verdict and the double verdict differ
            assert math.sqrt(d * d) == d
            return u, s, f, d


def request_scene(planted):
    """the cloud with nodes planted on the x axis at the given distances from node 0, at indices on both sides of the slab boundaries"""
    xyz = cloud()
    at = [2047, 2048, 4095, 4096, 4999, 1, 2500, 3000][:len(planted)]
    for i, d in zip(at, planted):
        xyz[i] = (d, 0.0, 0.0)
    return poses_at(xyz), at
