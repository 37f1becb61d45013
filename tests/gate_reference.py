"""Plain-Python float64 restatement of the edge acceptance gate (GraphSlamNode::newEdgeCallback / checkEdgeHeuristic,
graph_slam_node.cpp:779-829,1064-1085; SlamGraph::astar, slam_graph.cpp:843-890): the search with what it expanded and how large its
open list grew, the whole callback in candidate order, and which stage of uzl_gate_check settles a candidate when nobody asks for the
path length.  Python floats are IEEE doubles and every expression below keeps the operand order of oracle/uzl_oracle_gate.c, so the
results are comparable bit by bit.  Nothing here calls the code under test."""
import heapq
import math

import numpy as np

DMAX = float(np.finfo(np.float64).max)
TYPE_2D_LASER = 105
DEFAULT_CFG = dict(min_matching_score=20.0, max_edge_distance_T=1.0, max_edge_distance_R=20.0, scope_size_factor=0.1, min_accept_valid=DMAX)


def positions(poses):
    """[n,12] poses -> list of (x, y, z) Python floats"""
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    return [tuple(r) for r in P[:, [3, 7, 11]].tolist()]


def node_dist(pos, a, b):
    A = pos[a]; B = pos[b]
    dx = A[0] - B[0]; dy = A[1] - B[1]; dz = A[2] - B[2]
    return 1. * math.sqrt((dx * dx + dy * dy) + dz * dz)


def adjacency(n, edges):
    """getNeighbors(v, only_valid=true) for every v: valid non-laser edges in edge order, both directions (a self-loop once)"""
    adj = [[] for _ in range(n)]
    for f, t, ty, v in zip(edges["from"].tolist(), edges["to"].tolist(), edges["type"].tolist(), edges["valid"].tolist()):
        if f < 0 or t < 0 or f >= n or t >= n or not v or ty == TYPE_2D_LASER:
            continue
        adj[f].append(t)
        if t != f:
            adj[t].append(f)
    return adj


class CsrAdjacency:
    """The same lists for a graph too large for a list of lists: adj[v] slices numpy arrays"""

    def __init__(self, n, edges):
        f = np.asarray(edges["from"], np.int64); t = np.asarray(edges["to"], np.int64)
        ok = (f >= 0) & (t >= 0) & (f < n) & (t < n) & (np.asarray(edges["valid"]) != 0) & (np.asarray(edges["type"]) != TYPE_2D_LASER)
        f, t = f[ok], t[ok]
        src = np.stack([f, t], 1).reshape(-1); dst = np.stack([t, f], 1).reshape(-1)
        keep = np.ones(len(src), bool); keep[1::2] = f != t
        src, dst = src[keep], dst[keep]
        order = np.argsort(src, kind="stable")
        self.nbr = dst[order]
        self.ptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(src, minlength=n), out=self.ptr[1:])

    def __getitem__(self, v):
        return self.nbr[self.ptr[v]:self.ptr[v + 1]].tolist()

    def degree(self):
        return np.diff(self.ptr)


def astar(pos, adj, s, t, reverse_ids=False):
    """The reference's loop, literally: priority = straight-line distance to the target only, stale entries are expanded again, equal
    priorities in node order (reverse_ids: in reversed node order - a scene's own check that ties matter in it).
    -> (dist, expanded nodes in order, largest heap size with stale entries, heap non-empty at the stop).  The largest heap size is the
    largest open list of every device kernel: the same multiset of entries and the same pops."""
    sign = -1 if reverse_ids else 1
    g = {s: 0.0}; open_ = {s}; closed = set(); heap = [(node_dist(pos, s, t), sign * s)]
    expanded = []; peak = 1
    while open_ and heap:
        v = sign * heap[0][1]
        if v == t:
            return g[t], expanded, peak, True
        heapq.heappop(heap); open_.discard(v); closed.add(v)
        expanded.append(v)
        gv = g[v]
        for u in adj[v]:
            if u in closed:
                continue
            tent = gv + node_dist(pos, v, u)
            if u not in open_ or tent < g[u]:
                g[u] = tent; heapq.heappush(heap, (node_dist(pos, u, t), sign * u)); open_.add(u)
        peak = max(peak, len(heap))
    return DMAX, expanded, peak, bool(heap)


def angle_of(m):
    """Eigen::Quaterniond(R) then AngleAxisd::angle() = 2 acos(clamp(w)); m = 9 row-major entries"""
    t = m[0] + m[4] + m[8]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0.:
        t = math.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[7] - m[5]) * t; q[2] = (m[2] - m[6]) * t; q[3] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[i * 4]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = math.sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k * 3 + j] - m[j * 3 + k]) * t
        q[1 + j] = (m[j * 3 + i] + m[i * 3 + j]) * t
        q[1 + k] = (m[k * 3 + i] + m[i * 3 + k]) * t
    n2 = (q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]
    if n2 < 1e-12 * 1e-12:
        return 0.
    w = min(max(q[0], -1.), 1.)
    return 2. * math.acos(w)


def pose_gap(A, B):
    """diff_pose = A^-1 B (12 row-major entries each): translation norm [m], rotation angle [deg]"""
    Rd = [0.0] * 9; ti = [0.0] * 3; td = [0.0] * 3
    for r in range(3):
        for c in range(3):
            Rd[r * 3 + c] = (A[0 * 4 + r] * B[0 * 4 + c] + A[1 * 4 + r] * B[1 * 4 + c]) + A[2 * 4 + r] * B[2 * 4 + c]
        ti[r] = -((A[0 * 4 + r] * A[3] + A[1 * 4 + r] * A[7]) + A[2 * 4 + r] * A[11])
    for r in range(3):
        td[r] = ((A[0 * 4 + r] * B[3] + A[1 * 4 + r] * B[7]) + A[2 * 4 + r] * B[11]) + ti[r]
    dn = math.sqrt((td[0] * td[0] + td[1] * td[1]) + td[2] * td[2])
    return dn, 180. * angle_of(Rd) / math.pi


def thresholds_ok(cfg, score, T):
    """score and transform thresholds (:798-803); T = the candidate's 12 transform entries"""
    if not (score >= cfg["min_matching_score"]):
        return False
    R = [T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]
    diff_rot = abs(angle_of(R)) * 180 / math.pi
    tn = math.sqrt((T[3] * T[3] + T[7] * T[7]) + T[11] * T[11])
    return tn <= cfg["max_edge_distance_T"] and diff_rot <= cfg["max_edge_distance_R"]


def full_cfg(cfg):
    c = dict(DEFAULT_CFG); c.update(cfg)
    return c


def check(cfg, poses, edges, merged, cand, trace=None):
    """The whole callback, candidate by candidate -> (accept u8, valid u8, dist f64) as the oracle's check returns them.
    trace (a list): gets astar's tuple for every candidate that reached the search, None for the others."""
    cfg = full_cfg(cfg)
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    n = len(P)
    rows = P.tolist(); pos = positions(P)
    mg = [0] * n if merged is None else list(np.asarray(merged).tolist())
    adj = adjacency(n, edges)
    exists = set()
    for f, t, ty in zip(edges["from"].tolist(), edges["to"].tolist(), edges["type"].tolist()):
        if 0 <= f < n and 0 <= t < n:
            exists.add((min(f, t), max(f, t), ty))
    nc = len(cand)
    accept = np.zeros(nc, np.uint8); valid = np.zeros(nc, np.uint8); dist = np.full(nc, -1.0)
    ssf = cfg["scope_size_factor"]
    for k in range(nc):
        if trace is not None:
            trace.append(None)
        f, t, ty = int(cand["from"][k]), int(cand["to"][k]), int(cand["type"][k])
        if f < 0 or t < 0 or f >= n or t >= n:
            continue
        if mg[f] or mg[t]:
            continue
        if (min(f, t), max(f, t), ty) in exists:
            continue
        score = float(cand["matching_score"][k])
        if not thresholds_ok(cfg, score, cand["transform"][k].tolist()):
            continue
        res = astar(pos, adj, f, t)
        if trace is not None:
            trace[-1] = res
        d = res[0]
        dist[k] = d
        ok = True
        if d != DMAX:
            dn, drot = pose_gap(rows[f], rows[t])
            ok = (2 * ssf * d + 1.0 > dn) and (10 * ssf * d + 30.0 > drot)
        if not ok:
            continue
        v = 1 if score >= cfg["min_accept_valid"] else 0
        exists.add((min(f, t), max(f, t), ty))
        if v and ty != TYPE_2D_LASER:
            adj[f].append(t)
            if t != f:
                adj[t].append(f)
        accept[k] = 1; valid[k] = v
    return accept, valid, dist


def _rel(lhs, rhs):
    """relative margin of `lhs > rhs` (positive: holds)"""
    return (lhs - rhs) / max(abs(lhs), abs(rhs), 1e-300)


def _tests(ssf, d, dn, drot):
    """(holds, margin): both plausibility tests at path length d.  A conjunction holds by its weakest test and fails by its clearest
    failure."""
    a = _rel(2 * ssf * d + 1.0, dn); b = _rel(10 * ssf * d + 30.0, drot)
    ok = (2 * ssf * d + 1.0 > dn) and (10 * ssf * d + 30.0 > drot)
    return ok, (min(a, b) if ok else max(-a, -b))


def line_decides(cfg, A, B):
    """gate_decided for the poses A (source) and B (target), 12 entries each -> (holds, margin): both tests hold for the straight line
    between the nodes shortened by 1e-9 of itself, so they hold for every path length the search can return"""
    ssf = full_cfg(cfg)["scope_size_factor"]
    if not (ssf >= 0.):
        return False, math.inf
    dn, drot = pose_gap(A, B)
    dx = B[3] - A[3]; dy = B[7] - A[7]; dz = B[11] - A[11]
    lower = math.sqrt((dx * dx + dy * dy) + dz * dz) * (1. - 1e-9)
    return _tests(ssf, lower, dn, drot)


def stage(cfg, poses, adj, cand_k):
    """Which stage settles a candidate that passed the index checks when no distance is asked for ->
    dict(stage, how, margin, peak): stage 'pre' (a threshold refuses it), 'line' (gate_decided holds), 'ball' (Dijkstra from the source
    pops a key that passes both tests before it pops the target, how='key'; or its list runs empty, how='exhausted') or 'search' (the
    target is popped first, or the tests are not monotone: scope_size_factor < 0).  margin = the smallest relative margin of every
    comparison of a test with its bound the decision went through (the final verdict's included, for 'search'); peak = the largest
    list of the Dijkstra search."""
    cfg = full_cfg(cfg)
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    rows = P.tolist(); pos = positions(P)
    s, t = int(cand_k["from"]), int(cand_k["to"])
    if not thresholds_ok(cfg, float(cand_k["matching_score"]), cand_k["transform"].tolist()):
        return dict(stage="pre", how="thresholds", margin=math.inf, peak=0)
    ssf = cfg["scope_size_factor"]
    dn, drot = pose_gap(rows[s], rows[t])

    def verdict(margin, how):
        d = astar(pos, adj, s, t)[0]
        if d != DMAX:
            margin = min(margin, _tests(ssf, d, dn, drot)[1])
        return dict(stage="search", how=how, margin=margin, peak=0)

    if not (ssf >= 0.):
        return verdict(math.inf, "not monotone")
    ok, margin = line_decides(cfg, rows[s], rows[t])
    if ok:
        return dict(stage="line", how="line", margin=margin, peak=0)
    heap = [(0.0, s)]; closed = set(); peak = 1
    while heap:
        m, v = heap[0]
        ok, mg = _tests(ssf, m, dn, drot)
        margin = min(margin, mg)
        if ok:
            return dict(stage="ball", how="key", margin=margin, peak=peak)
        if v == t:
            r = verdict(margin, "target first"); r["peak"] = peak
            return r
        heapq.heappop(heap)
        if v in closed:
            continue
        closed.add(v)
        for u in adj[v]:
            if u != v and u not in closed:
                heapq.heappush(heap, (m + node_dist(pos, v, u), u))
        peak = max(peak, len(heap))
    return dict(stage="ball", how="exhausted", margin=margin, peak=peak)
