"""Plain-Python restatement of node merging, the parity target of uzl_merge_* (include/uzl_mi355x.h, "Node merging").

Search: GraphSlamNode::mergeTimerCallback (graph_slam/src/graph_slam_node.cpp:665-777) over SlamGraph::getNodesWithinHops
(graph_slam_common/src/slam_graph.cpp:231-264).  Rewrite: GraphSlamNode::mergeNodes (:919-986).  Node and edge ids are indices in the
reference's std::map order.  Every floating-point expression is written with the association the header states; the steps the
reference hands to Eigen are marked [EXT] and spelled out with math.* one operation at a time.  ball() is a breadth-first ball, kept
for contrast only: the reference's walk is NOT one."""
import math
from collections import deque

import numpy as np

UNTOUCHED, KEEP_FROM, KEEP_TO, RETARGET_FROM, RETARGET_TO, DELETE = range(6)


def norm3(dx, dy, dz):
    return math.sqrt((dx * dx + dy * dy) + dz * dz)


def rotation_bound(max_rotation_deg):
    """the right-hand side of the trace test: angle <= a  <=>  tr >= 1 + 2 cos a"""
    return 1.0 + 2.0 * math.cos(max_rotation_deg * math.pi / 180.0)


def trace_of(Ta, Tb):
    """tr(R_a^T R_b): the nine entry-wise products of the rotation blocks in row-major order, summed left to right"""
    s = None
    for k in (0, 1, 2, 4, 5, 6, 8, 9, 10):
        p = float(Ta[k]) * float(Tb[k])
        s = p if s is None else s + p
    return s


class MergeReference:
    def __init__(self, max_distance=0.25, max_rotation_deg=15.0, scope_margin=6.0, max_hops=10):
        self.max_distance, self.scope_margin, self.max_hops = max_distance, scope_margin, max_hops
        self.bound = rotation_bound(max_rotation_deg)
        self.set_graph(np.zeros((0, 12)), None)

    # ------------------------------------------------------------------------------------------------ graph
    def set_graph(self, poses, edges):
        self.P = np.array(poses, np.float64).reshape(-1, 12)
        self.n = len(self.P)
        self.E = [] if edges is None else [[int(e["from"]), int(e["to"]), int(e["type"]), int(e["valid"])] for e in edges]

    def set_poses(self, poses):
        P = np.array(poses, np.float64).reshape(-1, 12)
        assert len(P) == self.n
        self.P = P

    def set_valid(self, edge_index, valid):
        for k, v in zip(edge_index, valid):
            self.E[int(k)][3] = int(v != 0)

    def rows(self):
        """node.edges_ is a std::set of edge ids: a node's row is its edges in ascending edge index; only valid_ edges are followed
        (only_valid = true, slam_graph.h:92), whatever their type"""
        adj = [[] for _ in range(self.n)]
        for f, t, _, valid in self.E:
            if not valid:
                continue
            adj[f].append(t)
            if t != f:
                adj[t].append(f)
        return adj

    # ------------------------------------------------------------------------------------------------ the walk
    def walk(self, start, hops=None, adj=None):
        """slam_graph.cpp:231-253 as written: depth first, one visited_ flag per node, tested when the loop reaches the edge"""
        adj = self.rows() if adj is None else adj
        visited = set()

        def helper(v, h):
            visited.add(v)
            if h > 0:
                for nxt in adj[v]:
                    if nxt not in visited:
                        helper(nxt, h - 1)

        helper(start, self.max_hops if hops is None else hops)
        return visited

    def ball(self, start, hops=None, adj=None):
        """breadth-first ball of the same radius - what the walk is NOT (it is a subset of this)"""
        adj = self.rows() if adj is None else adj
        hops = self.max_hops if hops is None else hops
        depth = {start: 0}
        q = deque([start])
        while q:
            v = q.popleft()
            if depth[v] == hops:
                continue
            for nxt in adj[v]:
                if nxt not in depth:
                    depth[nxt] = depth[v] + 1
                    q.append(nxt)
        return set(depth)

    # ------------------------------------------------------------------------------------------------ geometry
    def is_start(self, i, center, radius):
        T = self.P[i]
        return norm3(T[3] - center[0], T[7] - center[1], T[11] - center[2]) > radius + self.scope_margin         # :696, strict

    def close(self, a, b):
        A, B = self.P[a], self.P[b]
        if not norm3(A[3] - B[3], A[7] - B[7], A[11] - B[11]) < self.max_distance:                               # :740
            return False
        return trace_of(A, B) >= self.bound                                                                      # :743-747 [EXT]

    def qualifying(self, start, reach=None, adj=None):
        reach = self.walk(start, adj=adj) if reach is None else reach
        return sorted(v for v in reach if v != start and v != 0 and self.close(start, v))

    def partners(self, center, radius, first_index=0, use_ball=False):
        adj = self.rows()
        out = np.full(self.n, -1, np.int32)
        for i in range(first_index, self.n):
            if not self.is_start(i, center, radius):
                continue
            q = self.qualifying(i, self.ball(i, adj=adj) if use_ball else None, adj)
            if q:
                out[i] = q[0]
        return out

    def search(self, first_index, center, radius):
        """-> (keep, drop, next_index)"""
        if first_index < 0:
            raise ValueError("first_index")
        n = self.n
        if n < 2:                                                          # :671: nothing runs, current_merge_index_ stays
            return -1, -1, first_index
        if first_index >= n:                                               # :677-679
            first_index = 1
        adj = self.rows()
        for i in range(first_index, n):
            if not self.is_start(i, center, radius):
                continue
            q = self.qualifying(i, adj=adj)
            if q:
                return max(i, q[0]), min(i, q[0]), i                       # :751-753 keeps the larger id
        return -1, -1, n

    # ------------------------------------------------------------------------------------------------ mergeNodes :919-986
    def plan(self, keep, drop, n_stamps_keep, n_stamps_drop):
        return merge_plan(self.P[keep], self.P[drop], self.E, keep, drop, n_stamps_keep, n_stamps_drop)


def quat_of(T):
    """Eigen::Quaterniond(Matrix3d) [EXT] -> (w, x, y, z); not normalised"""
    m = [T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]]
    t = m[0] + m[4] + m[8]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return w, (m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t
    if m[0] >= m[4] and m[0] >= m[8]:
        t = math.sqrt(m[0] - m[4] - m[8] + 1.0)
        x = 0.5 * t
        t = 0.5 / t
        return (m[7] - m[5]) * t, x, (m[3] + m[1]) * t, (m[6] + m[2]) * t
    if m[4] > m[0] and m[4] >= m[8]:
        t = math.sqrt(m[4] - m[8] - m[0] + 1.0)
        y = 0.5 * t
        t = 0.5 / t
        return (m[2] - m[6]) * t, (m[1] + m[3]) * t, y, (m[7] + m[5]) * t
    t = math.sqrt(m[8] - m[0] - m[4] + 1.0)
    z = 0.5 * t
    t = 0.5 / t
    return (m[3] - m[1]) * t, (m[2] + m[6]) * t, (m[5] + m[7]) * t, z


def slerp(t, a, b):
    """Eigen::Quaterniond::slerp [EXT]; quaternions as (w, x, y, z)"""
    d = ((a[1] * b[1] + a[2] * b[2]) + a[3] * b[3]) + a[0] * b[0]
    ad = abs(d)
    if ad >= 1.0 - 2.220446049250313e-16:
        s0, s1 = 1.0 - t, t
    else:
        theta = math.acos(ad)
        st = math.sin(theta)
        s0 = math.sin((1.0 - t) * theta) / st
        s1 = math.sin(t * theta) / st
    if d < 0.0:
        s1 = -s1
    return tuple(s0 * a[k] + s1 * b[k] for k in range(4))


def rotation_of(q):
    """Eigen::AngleAxisd(Quaterniond) and its toRotationMatrix [EXT] -> 9 entries, row-major"""
    w, x, y, z = q
    n = math.sqrt((x * x + y * y) + z * z)
    if n != 0.0:
        angle = 2.0 * math.atan2(n, abs(w))
        if w < 0.0:
            n = -n
        ax, ay, az = x / n, y / n, z / n
    else:
        angle, ax, ay, az = 0.0, 1.0, 0.0, 0.0
    s, c = math.sin(angle), math.cos(angle)
    sx, sy, sz = s * ax, s * ay, s * az
    cx, cy, cz = (1.0 - c) * ax, (1.0 - c) * ay, (1.0 - c) * az
    R = [0.0] * 9
    t = cx * ay; R[1] = t - sz; R[3] = t + sz
    t = cx * az; R[2] = t + sy; R[6] = t - sy
    t = cy * az; R[5] = t - sx; R[7] = t + sx
    R[0] = cx * ax + c; R[4] = cy * ay + c; R[8] = cz * az + c
    return R


def displacement_of(R, t, T):
    """new_pose.inverse() * T for new_pose = [R | t]: rotation R^T R_T, translation R^T t_T + (-(R^T t))"""
    out = [0.0] * 12
    Rt = [R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]]
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (Rt[3 * i] * T[j] + Rt[3 * i + 1] * T[4 + j]) + Rt[3 * i + 2] * T[8 + j]
        inv_t = -((Rt[3 * i] * t[0] + Rt[3 * i + 1] * t[1]) + Rt[3 * i + 2] * t[2])
        out[4 * i + 3] = ((Rt[3 * i] * T[3] + Rt[3 * i + 1] * T[7]) + Rt[3 * i + 2] * T[11]) + inv_t
    return out


def merge_plan(Tk, Td, edges, keep, drop, n_stamps_keep, n_stamps_drop):
    """first = keep, second = drop.  -> dict(ratio, new_pose, keep_displacement, drop_displacement, action [n_edges], touched,
    retargeted, deleted)"""
    Tk = [float(v) for v in Tk]; Td = [float(v) for v in Td]
    ratio = float(n_stamps_drop) / (float(n_stamps_keep) + float(n_stamps_drop))                                 # :920-922
    R = rotation_of(slerp(ratio, quat_of(Tk), quat_of(Td)))                                                      # :923, :926
    t = [(1.0 - ratio) * Tk[k] + ratio * Td[k] for k in (3, 7, 11)]                                              # :924
    new_pose = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
    ends = [[e[0], e[1]] for e in edges]
    action = [UNTOUCHED] * len(edges)
    of_keep = set()                                                        # first.edges_
    for k, (f, t_) in enumerate(ends):                                      # :943-953
        if f == keep or t_ == keep:
            of_keep.add(k)
            action[k] = KEEP_FROM if f == keep else KEEP_TO
    for k in range(len(edges)):                                            # :960-986, second.edges_ in ascending edge id
        f, t_ = ends[k]
        if f != drop and t_ != drop:
            continue
        if f == keep or t_ == keep:                                        # :963
            action[k] = DELETE
            continue
        other = t_ if f == drop else f
        typ = edges[k][2]
        if any(edges[j][2] == typ and ((ends[j][0] == keep and ends[j][1] == other) or (ends[j][0] == other and ends[j][1] == keep))
               for j in of_keep):                                          # existsEdge(first, other, type), slam_graph.cpp:407-422
            action[k] = DELETE
            continue
        if f == drop:
            action[k] = RETARGET_FROM; ends[k][0] = keep
        else:
            action[k] = RETARGET_TO; ends[k][1] = keep
        of_keep.add(k)                                                     # :979
    return dict(ratio=ratio, new_pose=new_pose, keep_displacement=displacement_of(R, t, Tk), drop_displacement=displacement_of(R, t, Td),
                action=np.array(action, np.int8), touched=sum(a != UNTOUCHED for a in action),
                retargeted=sum(a in (RETARGET_FROM, RETARGET_TO) for a in action), deleted=sum(a == DELETE for a in action))


def compose(A, B):
    """A * B of two 3 x 4 transforms (Eigen's Isometry3d product): rows of A times columns of B, summed left to right"""
    out = [0.0] * 12
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]
        out[4 * i + 3] = ((A[4 * i] * B[3] + A[4 * i + 1] * B[7]) + A[4 * i + 2] * B[11]) + A[4 * i + 3]
    return out


def rewritten_graph(poses, edges, disp_from, disp_to, keep, drop, plan):
    """The graph after mergeNodes, restated edge by edge in plain Python: -> (poses, [from, to, type, valid] rows, displacement_from,
    displacement_to, old_to_new) with `drop` gone and the nodes behind it one index lower.  An edge that still names `drop` after the
    loop (a self-loop of `drop` that was retargeted on its from side) goes with the node."""
    n = len(poses)
    old_to_new = [(-1 if v == drop else v - (v > drop)) for v in range(n)]
    P = [list(map(float, poses[v])) for v in range(n) if v != drop]
    P[old_to_new[keep]] = list(plan["new_pose"])
    rows, df, dt = [], [], []
    for k, e in enumerate(edges):
        a = int(plan["action"][k])
        f, t, typ, valid = (int(v) for v in e[:4])
        F, T = [float(v) for v in disp_from[k]], [float(v) for v in disp_to[k]]
        if a == DELETE:
            continue
        if a == KEEP_FROM:
            F = compose(plan["keep_displacement"], F)
        elif a == KEEP_TO:
            T = compose(plan["keep_displacement"], T)
        elif a == RETARGET_FROM:
            F = compose(plan["drop_displacement"], F); f = keep
        elif a == RETARGET_TO:
            T = compose(plan["drop_displacement"], T); t = keep
        if f == drop or t == drop:
            continue
        rows.append([old_to_new[f], old_to_new[t], typ, valid]); df.append(F); dt.append(T)
    return P, rows, df, dt, old_to_new
