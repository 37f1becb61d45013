"""Named scenes of the edge acceptance gate, one per path of uzl_gate_check that a random pose graph does not reach.  Every scene is a
function -> dict(poses [n,12], edges, merged, cand, cfg) plus what its conditions need (test_gate_reference.py asserts every condition
with gate_reference alone, so a scene that stops exercising its case fails there and not silently on the GPU)."""
import functools

import numpy as np

from uzliti_slam_amd import capi, synth

ODOM, FULL, LASER = synth.EDGE_TYPE_ODOM, synth.EDGE_TYPE_3D_FULL, synth.EDGE_TYPE_2D_LASER
WIDE = dict(max_edge_distance_T=100.0, max_edge_distance_R=360.0)


def poses_at(xyz, yaw_deg=None):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    P = np.tile(np.eye(3, 4).reshape(12), (len(xyz), 1))
    if yaw_deg is not None:
        a = np.deg2rad(np.asarray(yaw_deg, np.float64))
        P[:, 0] = np.cos(a); P[:, 1] = -np.sin(a); P[:, 4] = np.sin(a); P[:, 5] = np.cos(a)
    P[:, [3, 7, 11]] = xyz
    return P


def _edges(fr, to, ty=None, valid=None):
    fr = np.asarray(fr, np.int64); to = np.asarray(to, np.int64)
    return capi.gate_edges(fr, to, np.full(len(fr), ODOM) if ty is None else ty, valid=np.ones(len(fr), int) if valid is None else valid)


def _cands(fr, to, ty=None, score=None):
    fr = np.asarray(fr, np.int64); to = np.asarray(to, np.int64)
    T = np.tile(np.eye(3, 4).reshape(12), (len(fr), 1)); T[:, 3] = 0.1
    return capi.gate_edges(fr, to, np.full(len(fr), FULL) if ty is None else ty, score=np.full(len(fr), 50.0) if score is None else score, transform=T)


def _scene(poses, edges, cand, cfg=None, merged=None, **more):
    return dict(poses=np.ascontiguousarray(poses), edges=edges, merged=merged, cand=cand, cfg=dict(cfg or {}), **more)


# ------------------------------------------------------------------------------------------------------------------ ties
@functools.lru_cache(None)
def ties():
    """A robot on a survey grid that also stands still: a 12 x 12 lattice at 0.25 m (every coordinate, difference and partial sum is
    exact, so equal distances are EQUAL), node ids shuffled, ~80 % of the 4-neighbour edges, and 24 nodes at the exact position of a
    lattice node, chained to it.  Equal priorities of different nodes are the rule here: the pop order is decided by the node id."""
    rng = np.random.default_rng(41)
    side = 12
    ids = rng.permutation(side * side + 24)
    lat = ids[:side * side].reshape(side, side); still = ids[side * side:]
    xyz = np.zeros((len(ids), 3))
    ii, jj = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    xyz[lat.reshape(-1)] = np.stack([0.25 * ii.reshape(-1), 0.25 * jj.reshape(-1), np.zeros(side * side)], 1)
    fr = np.concatenate([lat[:-1, :].reshape(-1), lat[:, :-1].reshape(-1)]); to = np.concatenate([lat[1:, :].reshape(-1), lat[:, 1:].reshape(-1)])
    keep = rng.random(len(fr)) < 0.8
    fr, to = fr[keep], to[keep]
    host = rng.choice(lat.reshape(-1), len(still), replace=False)
    xyz[still] = xyz[host]
    fr = np.concatenate([fr, still]); to = np.concatenate([to, host])
    order = rng.permutation(len(fr))
    E = _edges(fr[order], to[order])
    s = rng.integers(0, len(ids), 300); t = rng.integers(0, len(ids), 300)
    s[:6] = still[:6]; t[:6] = host[:6]                    # source and target at one position
    t[6:9] = still[6:9]                                    # targets with a twin at their position: h = 0 twice
    return _scene(poses_at(xyz), E, _cands(s, t), pairs=np.stack([s, t], 1))


# ------------------------------------------------------------------------------------------------------------------ hubs
HUB_DEGREES = (8, 9, 63, 64, 65, 128, 129, 200)            # 8 = kGateRecNbr; 64 = one chunk of neighbours; 128 = gate_reg_kernel<2>'s list


@functools.lru_cache(None)
def hubs():
    """280 chain nodes on a random walk and 8 hubs whose neighbour lists are exactly as long as HUB_DEGREES and in a known order (a
    hub's edges are listed together and nothing else touches it).  Twins (one neighbour listed twice, by edges of two types): positions
    3 and 7 of the degree-9 hub and 70 and 100 of the degree-129 hub (inside one chunk of 64, the first and the second), 63 and 64 of
    the degree-65 hub (astride two chunks), 10 and 140 of the degree-200 hub; the degree-128 hub carries a self-loop (one list entry).
    The degree-129 hub has 128 distinct neighbours: a search from it to its twin ends with exactly the 128 entries gate_reg_kernel<2>
    can hold, and with one more if both occurrences of the twin were pushed (only a chunk's own de-duplication prevents that: twins in
    two chunks see each other's state)."""
    rng = np.random.default_rng(43)
    nch = 280
    step = rng.normal(0, 1, (nch, 3)) * [0.3, 0.3, 0.02]
    xyz = np.cumsum(step, 0)
    fr = list(range(nch - 1)); to = list(range(1, nch)); ty = [ODOM] * (nch - 1)
    hub_ids = []; twins = {}; hub_xyz = []
    for d in HUB_DEGREES:
        h = nch + len(hub_ids); hub_ids.append(h)
        slots = d - (1 if d == 128 else 0)                 # list entries that name a neighbour (the self-loop takes one)
        twin = {9: (3, 7), 65: (63, 64), 129: (70, 100), 200: (10, 140)}.get(d)
        nb = list(rng.choice(nch, slots - (1 if twin else 0), replace=False))
        if twin:
            nb.insert(twin[1], nb[twin[0]]); twins[h] = (twin, int(nb[twin[0]]))
        types = [FULL] * len(nb)
        if twin:
            types[twin[1]] = 3
        if d == 128:
            nb.append(h); types.append(FULL)               # the self-loop, last in the list
        fr += [h] * len(nb); to += [int(u) for u in nb]; ty += types
        hub_xyz.append(xyz[rng.integers(0, nch)] + rng.normal(0, 0.2, 3))
    xyz = np.concatenate([xyz, np.array(hub_xyz)])
    E = _edges(fr, to, np.array(ty))
    # candidates: from every hub to four chain nodes (the hub is expanded first), to the hub's twin and to its last neighbour (the
    # search ends with the hub's own pushes in the list: list length = distinct neighbours), and between random chain nodes
    cs, ct = [], []
    for h in hub_ids:
        cs += [h] * 4; ct += [int(u) for u in rng.choice(nch, 4, replace=False)]
        if h in twins:
            cs.append(h); ct.append(twins[h][1])
    a = rng.integers(0, nch, 60); b = rng.integers(0, nch, 60)
    cs += list(a[a != b]); ct += list(b[a != b])
    return _scene(poses_at(xyz), E, _cands(cs, ct, ty=np.full(len(cs), 7)), WIDE, hub_ids=hub_ids, twins=twins)      # (a type no edge has)


# ------------------------------------------------------------------------------------------------------------------ components
@functools.lru_cache(None)
def components():
    """Three components that a search must not leave: A = nodes 0..159 (chain + loop closures), cut from B = 160..199 by an INVALID
    odometry edge; B and C = 200..229 bridged only by a valid TYPE_2D_LASER edge; A and C bridged only by an invalid loop closure.  A
    search from A to B or C expands all of A and ends on n_open == 0."""
    rng = np.random.default_rng(47)
    n = 230
    th = 0.22 * np.arange(n)
    xyz = np.stack([(1.5 + 0.05 * th) * np.cos(th), (1.5 + 0.05 * th) * np.sin(th), 0.01 * np.arange(n)], 1) + rng.normal(0, 0.02, (n, 3))
    fr = list(range(n - 1)); to = list(range(1, n)); ty = [ODOM] * (n - 1); va = [1] * (n - 1)
    va[159] = 0                                            # 159 - 160: odometry edge, not valid
    va[199] = 0                                            # (199 - 200 likewise: B and C are joined by the laser edge alone)
    fr += [180, 100]; to += [210, 215]; ty += [LASER, FULL]; va += [1, 0]
    for lo, hi, k in ((0, 160, 60), (160, 200, 10), (200, 230, 8)):     # loop closures inside each component, some not valid
        a = rng.integers(lo, hi, k); b = rng.integers(lo, hi, k); ok = a != b
        fr += list(a[ok]); to += list(b[ok]); ty += [FULL] * int(ok.sum()); va += list((rng.random(int(ok.sum())) < 0.7).astype(int))
    E = _edges(fr, to, np.array(ty), np.array(va))
    cs = list(rng.integers(0, 160, 14)) + list(rng.integers(160, 200, 4)) + list(rng.integers(200, 230, 4))
    ct = list(rng.integers(160, 230, 14)) + list(rng.integers(200, 230, 4)) + list(rng.integers(0, 160, 4))
    a = rng.integers(0, 160, 30); b = rng.integers(0, 160, 30)
    cs += list(a[a != b]); ct += list(b[a != b])
    return _scene(poses_at(xyz), E, _cands(cs, ct, ty=np.full(len(cs), 7)), WIDE)


# ------------------------------------------------------------------------------------------------------------------ stages
STAGE_ROWS = ("i", "ii", "iii", "iv", "v", "vi", "vii", "viii", "xi")


@functools.lru_cache(None)
def stages(ssf=None):
    """Hand-made gadgets, one candidate each (STAGE_ROWS), identity rotations unless noted; default cfg, or scope_size_factor = ssf
    (the same candidates at 0, where the tests ignore the path length, and at a negative factor, where they are not monotone
    in it and every candidate must be searched).  With the default factor 0.1:
      i    two hops of 0.3 m: the straight line decides (1.12 > 0.6)
      ii   2.0 m apart, joined by a 9.2 m detour: the line fails (1.4 < 2), Dijkstra's key 5.6 passes (2.12 > 2) before the target
      iii  2.0 m apart, the source in a component of three nodes: the list runs empty
      iv   the graph of test_astar_is_greedy_best_first: shortest path 4.159 (1.83 < 2), greedy path 6.367 (2.27 > 2): accepted
      v    ten hops of 0.3 m along a line: 1.6 < 3.0, rejected by the search
      vi   0.3 m apart, the target turned by 29 deg: the rotation test decides on the line (30.3 > 29)
      vii  0.3 m apart, joined only by a 7.2 m loop, the target turned by 35 deg: the rotation test alone fails on the line
           (30.3 < 35) and alone passes in the ball (key 5.4: 35.4 > 35)
      viii source == target
      xi   neighbours 0.3 m apart, the target turned by 120 deg: the rotation test alone rejects, after the search (30.3 < 120)"""
    xyz = []; yaw = []; fr = []; to = []; cs = []; ct = []

    def add(points, yaws=None, chain=True, at=(0.0, 0.0)):
        base = len(xyz)
        for q, p in enumerate(points):
            xyz.append((p[0] + at[0], p[1] + at[1], 0.0)); yaw.append(0.0 if yaws is None else yaws[q])
        if chain:
            fr.extend(range(base, base + len(points) - 1)); to.extend(range(base + 1, base + len(points)))
        return base

    b = add([(0, 0), (0.3, 0), (0.6, 0)]); cs.append(b); ct.append(b + 2)                                    # i
    b_i = b
    detour = [(0, 0), (0, 0.9), (0, 1.8), (0, 2.7), (0, 3.6), (1, 3.6), (2, 3.6), (2, 2.7), (2, 1.8), (2, 0.9), (2, 0)]
    b = add(detour, at=(10, 0)); cs.append(b); ct.append(b + 10)                                            # ii
    b = add([(0, 0), (0.3, 0), (0.3, 0.3)], at=(20, 0)); t = add([(2, 0)], at=(20, 0)); cs.append(b); ct.append(t)     # iii
    b = add([(0, 0), (-1, 0.5), (1, 2), (2, 0), (2.5, 2.5)], chain=False, at=(30, 0))                           # iv
    fr.extend([b + 0, b + 1, b + 0, b + 2, b + 4]); to.extend([b + 1, b + 3, b + 2, b + 4, b + 3]); cs.append(b); ct.append(b + 3)
    b = add([(0.3 * q, 0) for q in range(11)], at=(40, 0)); cs.append(b); ct.append(b + 10)                   # v
    b = add([(0, 0), (0.3, 0)], yaws=[0, 29.0], at=(50, 0)); cs.append(b); ct.append(b + 1)                    # vi
    loop = [(0, 0), (0, 0.9), (0, 1.8), (0, 2.7), (0, 3.6), (0.3, 3.6), (0.3, 2.7), (0.3, 1.8), (0.3, 0.9), (0.3, 0)]
    b = add(loop, yaws=[0] * 9 + [35.0], at=(60, 0)); cs.append(b); ct.append(b + 9)                          # vii
    cs.append(b_i + 1); ct.append(b_i + 1)                                                                  # viii
    b = add([(0, 0), (0.3, 0)], yaws=[0, 120.0], at=(70, 0)); cs.append(b); ct.append(b + 1)                   # xi
    cfg = {} if ssf is None else dict(scope_size_factor=float(ssf))
    return _scene(poses_at(np.array(xyz), np.array(yaw)), _edges(fr, to), _cands(cs, ct), cfg, rows=STAGE_ROWS)


# ------------------------------------------------------------------------------------------------------------------ escalation
@functools.lru_cache(None)
def escalation():
    """A small dense graph on which the largest open list of a search falls in each of gate_reg_kernel's classes: at most 128 entries
    (two per lane), 129 to 256 (four per lane), more (the lane kernel).  Found with gate_reference.astar's largest-heap figure."""
    rng = np.random.default_rng(53)
    n = 500
    xyz = rng.uniform(-12, 12, (n, 3)) * [1, 1, 0.1]
    fr = rng.integers(0, n, 3000); to = rng.integers(0, n, 3000); ok = fr != to
    E = _edges(fr[ok], to[ok], np.full(int(ok.sum()), FULL))
    far = np.argsort(xyz[:, 0])
    cs = list(far[:40]) + list(rng.integers(0, n, 60)); ct = list(far[::-1][:40]) + list(rng.integers(0, n, 60))
    cs, ct = np.array(cs), np.array(ct)
    return _scene(poses_at(xyz), E, _cands(cs[cs != ct], ct[cs != ct]), WIDE)


# ------------------------------------------------------------------------------------------------------------------ chunks
@functools.lru_cache(None)
def chunks(seed=59):
    """640 candidates on 80 nodes with min_accept_valid = 60 within reach: the host's replay over chunks of 256 candidates, the
    re-search after a valid accept, and existsEdge across a chunk edge (candidate 255 is accepted as valid; 256 is its reverse)."""
    rng = np.random.default_rng(seed)
    n = 80
    th = 0.35 * np.arange(n)
    xyz = np.stack([(1.0 + 0.04 * th) * np.cos(th), (1.0 + 0.04 * th) * np.sin(th), np.zeros(n)], 1) + rng.normal(0, 0.02, (n, 3))
    E = _edges(np.arange(n - 1), np.arange(1, n))
    nc = 640
    a = rng.integers(0, n, nc); b = (a + rng.integers(1, n, nc)) % n
    ty = rng.choice([1, 3, 5, 7, 9, 11], nc)
    sc = rng.uniform(5, 120, nc)
    valid_rare = rng.random(nc) < 0.85
    sc = np.where(valid_rare, np.minimum(sc, 59.0 - 30.0 * rng.random(nc)), sc)       # about 1 in 12 reaches min_accept_valid
    a[255], b[255], ty[255], sc[255] = 3, 21, 13, 90.0                                # neighbours on adjacent turns: plausible, valid
    a[256], b[256], ty[256], sc[256] = 21, 3, 13, 95.0
    return _scene(poses_at(xyz), E, _cands(a, b, ty=ty, score=sc), dict(WIDE, min_accept_valid=60.0))


# ------------------------------------------------------------------------------------------------------------------ bitmap_edges
BITMAP_SIZES = (1, 2, 31, 32, 33, 1025, 2081)


@functools.lru_cache(None)
def bitmap_edges(n):
    """A chain of n nodes, n at the ends of the closed / open bitmaps' words and of the record cache's blocks; candidates end at node
    n - 1.  From 1025 nodes on, node 0 lists neighbours whose ids differ by 1024 and (from 2081 nodes on) 2048 from each other and from 0: their records
    share a slot of gate_reg_kernel's direct-mapped cache (kGateCacheBlocks * kGateBlockNodes = 1024 in gate_types.hpp)."""
    rng = np.random.default_rng(61 + n)
    xyz = np.cumsum(rng.normal(0, 1, (n, 3)) * [0.3, 0.3, 0.02], 0)
    fr = list(range(n - 1)); to = list(range(1, n)); ty = [ODOM] * (n - 1)
    extra = [u for u in (1024, 7, 7 + 1024, 2048, 7 + 2048) if u < n]
    if n > 1024:
        fr += [0] * len(extra); to += extra; ty += [FULL] * len(extra)
        xyz[extra] = xyz[0] + rng.normal(0, 0.3, (len(extra), 3))                      # loop closures join nodes that are close
    E = _edges(fr, to, np.array(ty)) if n > 1 else _edges([], [])
    src = sorted(set(int(v) for v in (0, 5, n // 2, n - 2, n - 1, max(n - 33, 0), max(n - 40, 0)) if v < n))
    cs = src + [n - 1] * len(src); ct = [n - 1] * len(src) + src
    if n > 1024:
        cs += [0, 1024]; ct += [extra[-1], 0]
    return _scene(poses_at(xyz), E, _cands(cs, ct, ty=np.arange(len(cs)) + 1), WIDE)


# ------------------------------------------------------------------------------------------------------------------ large
# gate_types.hpp: gate_lds_bytes(n) = kGateLdsFixed + 8 * ceil(n / 32) with kGateLdsFixed = 32 * 32 * 64 + 32 * 4 = 65 664, and
# kGateLdsMax = 160 * 1024 - 2048 = 161 792: n = 384 512 is the last size whose bitmaps fit (exactly kGateLdsMax: the largest dynamic-LDS
# launch gate_reg_kernel / gate_bound_kernel ever make), n = 384 513 the first one that gate_wave_kernel searches.
LARGE_LAST_LDS = 384512
LARGE_FIRST_WAVE = 384513
LARGE_HUB, LARGE_CLUSTER, LARGE_CUT = 200000, 6000, 3000
LARGE_ROWS = ("last node", "last word", "long walk", "cluster", "hub", "unreachable")


@functools.lru_cache(2)
def large(n):
    """An odometry chain of n nodes on a slow spiral (0.3 m steps, turns 1 m apart), built with numpy; a hub of degree 130 at node
    LARGE_HUB whose list holds one neighbour at positions 63 and 64; a dense random cluster (120 000 edges) over the first LARGE_CLUSTER nodes; the chain
    cut once (an invalid odometry edge) LARGE_CUT nodes before its end.  Six candidates (LARGE_ROWS); the unreachable one expands the whole tail behind the cut."""
    assert (65664 + 8 * ((LARGE_LAST_LDS + 31) // 32) == 161792) and (65664 + 8 * ((LARGE_FIRST_WAVE + 31) // 32) > 161792)
    rng = np.random.default_rng(67)
    # the first LARGE_CLUSTER nodes wind up a disc of 24 m radius (turns 1 m apart), a straight run leads 2 km out, the rest circles
    # there: nine turns, 20 000 hops of which are less than half a turn (a walk along them only ever comes closer to its target)
    r = np.sqrt(25.0 + 0.3 * np.arange(LARGE_CLUSTER) / np.pi); th = 2 * np.pi * (r - 5.0)
    n_run = int((2000.0 - r[-1]) / 0.3)
    r = np.concatenate([r, r[-1] + 0.3 * np.arange(1, n_run + 1)]); th = np.concatenate([th, np.full(n_run, th[-1])])
    r_out = np.sqrt(r[-1] ** 2 + 0.3 * np.arange(1, n - len(r) + 1) / np.pi)
    th = np.concatenate([th, th[-1] + 2 * np.pi * (r_out - r[-1])]); r = np.concatenate([r, r_out])
    xyz = np.stack([r * np.cos(th), r * np.sin(th), np.zeros(n)], 1)
    H = LARGE_HUB
    hub_nb = list(range(H + 2, H + 2 + 127)); hub_nb.insert(64, hub_nb[63])          # 128 entries, then the hub's two chain edges: 130
    hub_ty = [FULL] * 128; hub_ty[64] = 3
    cl_f = rng.integers(0, LARGE_CLUSTER, 120000); cl_t = rng.integers(0, LARGE_CLUSTER, 120000); ok = cl_f != cl_t
    cl_f, cl_t = cl_f[ok], cl_t[ok]
    fr = np.concatenate([np.full(128, H), np.arange(n - 1), cl_f]); to = np.concatenate([hub_nb, np.arange(1, n), cl_t])
    ty = np.concatenate([hub_ty, np.full(n - 1, ODOM), np.full(len(cl_f), FULL)])
    va = np.ones(len(fr), int); cut = n - LARGE_CUT
    va[128 + cut - 1] = 0                                                              # the odometry edge (cut - 1) - cut
    # "cluster": the pair with the largest open list (2 358 entries > kGateOpenCap = 2 048) among 3 000 random pairs of the cluster
    cs = [n - 4, n - 1, 100000, 4799, H - 40, n - 100]
    ct = [n - 1, n - 25, 118000, 5219, H + 400, cut - 50]
    return _scene(poses_at(xyz), _edges(fr, to, ty, va), _cands(cs, ct), WIDE, rows=LARGE_ROWS, hub=H)


SMALL = dict(ties=ties, hubs=hubs, components=components, stages=stages, stages_ssf0=lambda: stages(0.0), stages_ssfneg=lambda: stages(-0.1),
             escalation=escalation, chunks=chunks, **{"bitmap_edges_%d" % n: functools.partial(bitmap_edges, n) for n in BITMAP_SIZES})
