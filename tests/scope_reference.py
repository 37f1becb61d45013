"""NumPy / heapq restatement of the reference's node uncertainty and local scope, the checker of uzl_scope_* (include/uzl_mi355x.h).

SlamGraph (graph_slam_common/src/slam_graph.cpp): getNeighbors :558-578, dijkstra :765-797 written as the reference writes it (push on
improvement, read distance_ at pop, stop at a DBL_MAX key, lazy duplicates processed), oldestReachableNode :892-910 (iterative),
reevaluateUncertainty() :506-517 and (id) :519-556, getOutOfScopeNodes :216-229 with its float radius; GraphSlamNode
(graph_slam/src/graph_slam_node.cpp): scopeRequestTimerCallback's radius :586 and :623, scopeRequestCallback's node test :549-559.
Node ids are indices in the reference's std::map order.  Every double operation is a single IEEE operation in the reference's order."""
import heapq
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
TYPE_2D_LASER = 105


def edge_length(a, b):
    """(a - b).norm() as Eigen evaluates it for three components: sqrt((dx*dx + dy*dy) + dz*dz)"""
    dx = a[0] - b[0]; dy = a[1] - b[1]; dz = a[2] - b[2]
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


class ScopeReference:
    def __init__(self, scope_size_min=8.0, scope_size_factor=0.1, out_margin=4.0):
        self.scope_size_min, self.scope_size_factor, self.out_margin = scope_size_min, scope_size_factor, out_margin
        self.t = []             # translations, python floats
        self.unc = []           # uncertainty_
        self.dist = []          # distance_
        self.edges = []         # [from, to, type, valid]
        self.inc = []           # node.edges_: indices of the node's edges, in insertion order

    # ---- graph
    def set_graph(self, poses, uncertainty, edges):
        self.t, self.unc, self.dist, self.edges, self.inc = [], [], [], [], []
        self.add(poses, uncertainty, edges)

    def add(self, poses, uncertainty, edges):
        P = np.asarray(poses, np.float64).reshape(-1, 12)
        u = np.zeros(len(P)) if uncertainty is None else np.asarray(uncertainty, np.float64)
        for i in range(len(P)):
            self.t.append((float(P[i, 3]), float(P[i, 7]), float(P[i, 11])))
            self.unc.append(float(u[i])); self.dist.append(DBL_MAX); self.inc.append([])
        for e in ([] if edges is None else edges):
            k = len(self.edges)
            f, t = int(e["from"]), int(e["to"])
            self.edges.append([f, t, int(e["type"]), int(e["valid"])])
            self.inc[f].append(k)
            if t != f:
                self.inc[t].append(k)

    def set_poses(self, poses):
        P = np.asarray(poses, np.float64).reshape(-1, 12)
        assert len(P) == len(self.t)
        self.t = [(float(p[3]), float(p[7]), float(p[11])) for p in P]

    def set_valid(self, edge_index, valid):
        for k, v in zip(edge_index, valid):
            self.edges[int(k)][3] = 1 if v else 0

    def set_uncertainty(self, node, value):
        self.unc[node] = float(value)

    @property
    def n(self):
        return len(self.t)

    # ---- slam_graph.cpp
    def neighbors(self, u, only_valid=False):
        """getNeighbors :558-578"""
        res = []
        for k in self.inc[u]:
            f, t, typ, valid = self.edges[k]
            if (not only_valid or valid) and typ != TYPE_2D_LASER:
                res.append(t if f == u else f)
        return res

    def dijkstra(self, start):
        """:765-797.  Returns the pops, a measure of the heap's work."""
        n = self.n
        self.dist = [DBL_MAX] * n
        self.dist[start] = 0.0
        heap = [(0.0, start)]
        pops = 0
        while heap:
            w, v = heapq.heappop(heap)
            pops += 1
            if w == DBL_MAX:
                break
            for u in self.neighbors(v, True):
                new_dist = self.dist[v] + edge_length(self.t[v], self.t[u])
                if new_dist < self.dist[u]:
                    self.dist[u] = new_dist
                    heapq.heappush(heap, (new_dist, u))
        return pops

    def oldest_reachable(self, v):
        """:892-910, the recursion unrolled: the smallest index of v's component over all non-laser edges"""
        oldest = v
        seen = [False] * self.n
        seen[v] = True
        stack = [v]
        while stack:
            x = stack.pop()
            oldest = min(oldest, x)
            for u in self.neighbors(x):
                if not seen[u]:
                    seen[u] = True
                    stack.append(u)
        return oldest

    def reevaluate(self, node=-1):
        """-> (start, n_reached) as uzl_scope_reevaluate returns them"""
        if self.n == 0 or node >= self.n:
            return -1, 0
        if node < 0:                                    # :506-517
            start = 0
            self.dijkstra(start)
            for i in range(self.n):
                if self.dist[i] != DBL_MAX:
                    self.unc[i] = self.dist[i]
        else:                                           # :519-556
            start = self.oldest_reachable(node)
            initial = self.unc[start]
            self.dijkstra(start)
            for i in range(self.n):
                if self.dist[i] != DBL_MAX:
                    self.unc[i] = initial + self.dist[i]
        return start, sum(1 for d in self.dist if d != DBL_MAX)

    def uncertainty(self):
        return np.array(self.unc, np.float64)

    def distance(self):
        return np.array(self.dist, np.float64)

    # ---- scope
    def current_scope(self, current):
        """graph_slam_node.cpp:586"""
        return max(self.scope_size_min, self.scope_size_factor * self.unc[current])

    def out_of_scope(self, center, radius):
        """getOutOfScopeNodes :216-229: the radius arrives as a float"""
        r = float(np.float32(radius))
        return [i for i in range(self.n) if edge_length(self.t[i], self.t[center]) > r]

    def request(self, current):
        """-> (current_scope_, out-of-scope ids ascending): :586, :623"""
        scope = self.current_scope(current)
        return scope, np.array(self.out_of_scope(current, scope + self.out_margin), np.int32)

    def select(self, center, radius, have):
        """scopeRequestCallback :549-559"""
        have = set(int(h) for h in have)
        c = (float(center[0]), float(center[1]), float(center[2]))
        return np.array([i for i in range(self.n) if edge_length(self.t[i], c) < radius and i not in have], np.int32)
