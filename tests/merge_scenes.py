"""Scenes for the uzl_merge_* tests: the smallest graphs at which each piece of the merge search and of the rewrite plan can go wrong.
A search scene is a dict(poses (n,12), edges GATE_EDGE_DTYPE, center (3), radius, cfg); what a scene claims about itself (a norm that
is exact, a trace away from its bound) is asserted here, on the CPU.

Layout used by most scenes: node v sits at (3 v, 0, 0), three metres from its neighbours in index, so nothing is close to anything
- except that every pair (a, b) of `near` puts b 0.1 m beside a.  partner(a) = b then says "the walk from a marked b"."""
import math

import numpy as np

from merge_reference import MergeReference, rotation_bound, trace_of
from uzliti_slam_amd import capi

FULL = 1            # UZL_EDGE_TYPE_3D_FULL
LASER = 105         # UZL_EDGE_TYPE_2D_LASER
FAR = (1.0e6, 0.0, 0.0)     # a scope centre from which every node is a start


def rot_axis(axis, deg):
    """Rodrigues: the rotation by deg degrees about axis"""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def pose(xyz, R=None):
    T = np.zeros((3, 4))
    T[:, :3] = np.eye(3) if R is None else R
    T[:, 3] = xyz
    return T.reshape(12)


def poses_at(xyz, rots=None):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    return np.array([pose(p, None if rots is None else rots[i]) for i, p in enumerate(xyz)]).reshape(-1, 12)


def edges_of(pairs, typ=FULL, valid=1):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    return capi.gate_edges(pairs[:, 0], pairs[:, 1], np.broadcast_to(typ, n), valid=np.broadcast_to(valid, n))


def scene(xyz, pairs, typ=FULL, valid=1, rots=None, center=FAR, radius=0.0, **cfg):
    return dict(poses=poses_at(xyz, rots), edges=edges_of(pairs, typ, valid), center=np.array(center, np.float64), radius=float(radius), cfg=cfg)


def spread(n, near=()):
    xyz = np.zeros((n, 3))
    xyz[:, 0] = 3.0 * np.arange(n)
    for a, b in near:
        xyz[b] = xyz[a] + (0.0, 0.1, 0.0)
    return xyz


def reference_of(sc):
    r = MergeReference(**sc["cfg"])
    r.set_graph(sc["poses"], sc["edges"])
    return r


def chain(lo, hi):
    return [(v, v + 1) for v in range(lo, hi)]


# ------------------------------------------------------------------------------------------------ sizes
def sizes():
    two = [(0, 0, 0), (0.1, 0, 0)]
    return {"n0": scene(np.zeros((0, 3)), []), "n1": scene([(0, 0, 0)], []), "n2": scene(two, [(0, 1)]),
            "n2_no_edge": scene(two, [])}


# ------------------------------------------------------------------------------------------------ walk order
def gadget(shortcut_first, shift=1):
    """the header's example on the nodes shift .. shift + 3 (node 0 stays a root nobody is near): max_hops = 2, edges 0-1, 1-2, 0-2, 2-3.
    Node 3 is beside node 0.  In that order the walk from 0 marks {0, 1, 2}; with 0-2 first it reaches 3."""
    e = [(0, 2), (0, 1), (1, 2), (2, 3)] if shortcut_first else [(0, 1), (1, 2), (0, 2), (2, 3)]
    e = [(a + shift, b + shift) for a, b in e]
    return scene(spread(4 + shift, near=[(shift, shift + 3)]), e, max_hops=2)


def long_gadget(shortcut_first):
    """the same idea at max_hops = 10: a chain 1-2-...-11 reaches node 11 with no hop left, the shortcut 1-11 comes later in node
    1's row and finds it visited, so node 12 behind it is missed although it is two hops away"""
    ch, short = chain(1, 11), [(1, 11)]
    e = (short + ch if shortcut_first else ch + short) + [(11, 12)]
    return scene(spread(13, near=[(1, 12)]), e, max_hops=10)


def chain_of_12(hops_away):
    """nodes 1 .. 12 in a chain (node 0 apart); the node `hops_away` hops from node 1 lies beside it"""
    return scene(spread(13, near=[(1, 1 + hops_away)]), chain(1, 12), max_hops=10)


# ------------------------------------------------------------------------------------------------ edges
def only_way(typ=FULL, valid=1):
    """1 - 2 - 3 with 3 beside 1; the edge 2-3 is the only way there"""
    sc = scene(spread(4, near=[(1, 3)]), [(1, 2), (2, 3)])
    sc["edges"]["type"][1] = typ; sc["edges"]["valid"][1] = valid
    return sc


def loops_and_parallels():
    return scene(spread(5, near=[(1, 4)]), [(1, 1), (1, 2), (1, 2), (2, 1), (2, 2), (2, 3), (3, 3), (3, 4), (3, 4)], max_hops=3)


# ------------------------------------------------------------------------------------------------ rows
def hub(deg):
    """node 1 has `deg` neighbours; the only useful one, node deg + 1 beside it, is the last entry of its row"""
    n = deg + 2
    return scene(spread(n, near=[(1, deg + 1)]), [(1, v) for v in range(2, deg + 2)], max_hops=1)


def hub_with_visited_head(leaves=70):
    """max_hops = 2.  Start 1 -> 2, whose row marks the leaves 4 .. with no hop left; back at 1 -> the hub 3, whose row begins with
    those leaves - all visited by now - and ends with the target beside the start"""
    L = list(range(4, 4 + leaves)); target = 4 + leaves
    e = [(1, 2)] + [(2, v) for v in L] + [(1, 3)] + [(3, v) for v in L] + [(3, target)]
    return scene(spread(target + 1, near=[(1, target)]), e, max_hops=2)


# ------------------------------------------------------------------------------------------------ bitmap words
def chain_with_far_pair(n):
    """0 - 1 - ... - n-1 with the last two nodes beside each other"""
    return scene(spread(n, near=[(n - 2, n - 1)]), chain(0, n - 1))


# ------------------------------------------------------------------------------------------------ thresholds
def distance_edge(exactly):
    """node 1 at the origin, node 2 on the x axis at exactly max_distance or one ulp inside: the norm is exact"""
    d = 0.25 if exactly else math.nextafter(0.25, 0.0)
    assert math.sqrt((d * d + 0.0) + 0.0) == d
    return scene([(50, 0, 0), (0, 0, 0), (d, 0, 0)], [(1, 2)])


def start_edge(beyond):
    """radius 2 + margin 6 about the origin: node 1 at exactly 8 m is not a start, one ulp further it is"""
    d = math.nextafter(8.0, math.inf) if beyond else 8.0
    assert math.sqrt((d * d + 0.0) + 0.0) == d and 2.0 + 6.0 == 8.0
    return scene([(50, 0, 0), (d, 0, 0), (d, 0.1, 0)], [(1, 2)], center=(0, 0, 0), radius=2.0)


ANGLES = [14.9, -14.9, 15.1, -15.1, 180.0]
AXES = {"z": (0, 0, 1), "tilted": (0.3, -0.5, 0.8)}


def rotated_pair(axis, deg):
    """nodes 1 and 2 side by side, 2 turned by deg about axis relative to 1 (which is itself turned, so no entry is trivial)"""
    base = rot_axis((0.2, 0.9, -0.4), 33.0)
    R = base @ rot_axis(AXES[axis], deg)
    sc = scene([(50, 0, 0), (0, 0, 0), (0.1, 0, 0)], [(1, 2)], rots=[np.eye(3), base, R])
    tr = trace_of(sc["poses"][1], sc["poses"][2])
    assert abs(tr - rotation_bound(15.0)) > 1e-9                           # away from the bound by more than rounding
    assert (tr >= rotation_bound(15.0)) == (abs(deg) < 15.0)
    return sc


def turned_then_straight():
    """node 2 is beside node 1 but turned by 40 degrees; node 3, also beside it, is not"""
    xyz = [(50, 0, 0), (0, 0, 0), (0.1, 0, 0), (0, 0.1, 0)]
    return scene(xyz, [(1, 2), (1, 3)], rots=[np.eye(3), np.eye(3), rot_axis((0, 0, 1), 40.0), rot_axis((0, 0, 1), 5.0)])


# ------------------------------------------------------------------------------------------------ choice
def several():
    """nodes 2, 4, 5 are all beside node 6 and within its walk; so is node 0"""
    xyz = spread(7)
    for k, v in enumerate((0, 2, 4, 5)):
        xyz[v] = xyz[6] + (0.0, 0.02 * (k + 1), 0.0)
    return scene(xyz, [(6, 5), (6, 4), (6, 0), (0, 2), (1, 3)])


def two_ticks():
    """two revisited places on a chain: (2, 7) and (4, 9)"""
    return scene(spread(11, near=[(2, 7), (4, 9)]), chain(0, 10) + [(2, 7), (9, 4), (7, 3)])


# ------------------------------------------------------------------------------------------------ many starts in one launch
RANDOM_SEED = 1


def random_laps(seed=RANDOM_SEED, laps=4, per_lap=80, extra=190, invalid=0.15):
    """320 nodes on four noisy laps of an 80-pose loop (half a metre apart along the loop), the chain edges, about 190 extra edges
    between poses of different laps at about the same place (a few of them laser edges), 15 % of all edges invalid"""
    rng = np.random.default_rng(seed)
    n = laps * per_lap
    R = 0.5 * per_lap / (2.0 * math.pi)
    xyz = np.zeros((n, 3)); rots = []
    for v in range(n):
        phi = 2.0 * math.pi * (v % per_lap) / per_lap
        xyz[v] = (R * math.cos(phi) + rng.normal(0, 0.06), R * math.sin(phi) + rng.normal(0, 0.06), rng.normal(0, 0.02))
        rots.append(rot_axis((0, 0, 1), math.degrees(phi) + 90.0 + rng.normal(0, 6.0)) @ rot_axis((1, 0, 0), rng.normal(0, 2.0)))
    pairs, typ = chain(0, n - 1), [FULL] * (n - 1)
    for _ in range(extra):
        a = int(rng.integers(0, n))
        b = (a + per_lap * int(rng.integers(1, laps)) + int(rng.integers(-3, 4))) % n
        if a != b:
            pairs.append((a, b)); typ.append(LASER if rng.random() < 0.2 else FULL)
    order = rng.permutation(len(pairs))                                   # the edge order decides the walk: mix chain and closures
    pairs = [pairs[k] for k in order]; typ = [typ[k] for k in order]
    valid = (rng.random(len(pairs)) >= invalid).astype(np.int32)
    sc = scene(xyz, pairs, typ=np.array(typ), valid=valid, rots=rots)
    sc["half"] = dict(center=np.array([R, 0.0, 0.0]), radius=R * math.sqrt(2.0) - 6.0)     # about half the loop lies beyond radius + 6
    sc["none"] = dict(center=np.zeros(3), radius=2.0 * R)
    return sc


# ------------------------------------------------------------------------------------------------ the plan
def plan_graph(edge_rows, n=6):
    """edges given as (from, to, type, valid) rows over n nodes with non-trivial poses"""
    rows = np.asarray(edge_rows, np.int64).reshape(-1, 4)
    rng = np.random.default_rng(17)
    rots = [rot_axis(rng.normal(size=3), rng.uniform(-170, 170)) for _ in range(n)]
    sc = scene(rng.uniform(-2, 2, (n, 3)), rows[:, :2], typ=rows[:, 2], valid=rows[:, 3], rots=rots)
    return sc


PLAN_KEEP, PLAN_DROP = 4, 2
K, D = PLAN_KEEP, PLAN_DROP
PLAN_EDGES = {
    "joins_the_two": [(D, K, FULL, 1), (K, D, LASER, 1), (1, D, FULL, 1), (K, 5, FULL, 1)],
    "second_deleted_by_first_retarget": [(D, 3, FULL, 1), (3, D, FULL, 1), (0, 1, FULL, 1)],
    "other_type_both_kept": [(D, 3, FULL, 1), (3, D, LASER, 1)],
    "duplicate_on_keep_same_direction": [(K, 3, FULL, 1), (D, 3, FULL, 1), (D, 1, FULL, 1)],
    "duplicate_on_keep_other_direction": [(3, K, FULL, 1), (D, 3, FULL, 1), (1, D, FULL, 1)],
    "drop_on_from_and_to": [(D, 0, FULL, 1), (1, D, FULL, 1), (D, 3, LASER, 1), (5, D, LASER, 1), (K, 0, LASER, 1), (1, K, LASER, 1)],
    "invalid_edges_are_edges": [(K, 3, FULL, 0), (D, 3, FULL, 1), (D, 1, FULL, 0), (1, D, FULL, 1), (D, K, FULL, 0)],
    "self_loops": [(K, K, FULL, 1), (D, D, FULL, 1), (D, K, FULL, 1), (D, D, LASER, 1)],
    "no_edges": [],
}
PLAN_STAMPS = [(1, 1), (1, 7), (7, 1)]


def plan_poses(kind, sc):
    """the poses of keep and drop: as drawn, identical, or half a turn apart"""
    P = sc["poses"].copy()
    if kind == "identical":
        P[D] = P[K]
    elif kind == "half_turn":
        Rk = P[K].reshape(3, 4)[:, :3]
        T = P[D].reshape(3, 4).copy(); T[:, :3] = Rk @ rot_axis((0.1, 0.7, -0.2), 180.0)
        P[D] = T.reshape(12)
    elif kind == "near":
        Rk = P[K].reshape(3, 4)[:, :3]
        T = P[K].reshape(3, 4).copy(); T[:, :3] = Rk @ rot_axis((0.4, 0.1, 0.9), 9.0); T[:, 3] += (0.1, -0.05, 0.02)
        P[D] = T.reshape(12)
    return P


PLAN_POSES = ["drawn", "identical", "half_turn", "near"]
