"""Vectorised float64 NumPy restatement of the uzl_radius_* contract (include/uzl_mi355x.h): SlamGraph::getNodesWithinRadius
(graph_slam_common/src/slam_graph.cpp:266-278) and the filters of its caller (graph_slam/src/graph_slam_node.cpp:272-289).

For a query node q, every other node c in index order is a job (from = c, to = q) when
  1. ||t_c - t_q|| < radius                                  (strict),
  2. |stamp_q - stamp_c| * 1e-9 > new_edge_time              (strict; the difference is taken on the integers),
  3. angle(R_c^T R_q) in degrees < max_rotation_deg          (strict),
where angle is Eigen 3.2's AngleAxisd(Quaterniond(R)).angle() = 2 acos(clamp(w)): the quaternion conversion keeps w >= 0 while the
trace is positive, but its other branch (trace <= 0, rotations of 120 degrees and more) may return w < 0, and the angle is then
360 degrees - theta, not theta = arccos((trace - 1) / 2).  Unknown query ids (negative or >= n) yield nothing.  Jobs are ordered
by query, then by node index."""
import numpy as np


def quat_w_eigen32(R):
    """(m,3,3) -> (w, |vec|^2) of Eigen 3.2's Quaterniond(R) (Quaternion.h, quaternionbase_assign_impl for a 3x3 matrix)"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    m = len(R)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    pos = tr > 0.
    with np.errstate(invalid="ignore", divide="ignore"):
        # trace > 0
        t1 = np.sqrt(np.where(pos, tr, 0.) + 1.0)
        w1 = 0.5 * t1
        s1 = 0.5 / t1
        v1 = np.stack([(R[:, 2, 1] - R[:, 1, 2]) * s1, (R[:, 0, 2] - R[:, 2, 0]) * s1, (R[:, 1, 0] - R[:, 0, 1]) * s1], axis=1)
        # trace <= 0: i = index of the largest diagonal element (first one wins ties), j, k the next two cyclically
        i = np.zeros(m, np.int64)
        i[R[:, 1, 1] > R[:, 0, 0]] = 1
        ar = np.arange(m)
        i[R[:, 2, 2] > R[ar, i, i]] = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t2 = np.sqrt(R[ar, i, i] - R[ar, j, j] - R[ar, k, k] + 1.0)
        s2 = 0.5 / t2
        w2 = (R[ar, k, j] - R[ar, j, k]) * s2
        v2 = np.zeros((m, 3))
        v2[ar, i] = 0.5 * t2
        v2[ar, j] = (R[ar, j, i] + R[ar, i, j]) * s2
        v2[ar, k] = (R[ar, k, i] + R[ar, i, k]) * s2
    w = np.where(pos, w1, w2)
    v = np.where(pos[:, None], v1, v2)
    return w, (v * v).sum(axis=1)


def angle_eigen32(R):
    """Eigen 3.2 AngleAxisd(Quaterniond(R)).angle() in radians, in [0, 2 pi]"""
    w, n2 = quat_w_eigen32(R)
    a = 2. * np.arccos(np.clip(w, -1., 1.))
    return np.where(n2 < 1e-24, 0., a)                           # NumTraits<double>::dummy_precision()^2: the identity


def angle_plain(R):
    """theta = arccos((trace - 1) / 2) in radians, in [0, pi]: the rule the contract does NOT follow for w < 0"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    return np.arccos(np.clip((R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.) * 0.5, -1., 1.))


def check_angle_property(R, tol=1e-6):
    """longdouble check of angle_eigen32: it is theta or 2 pi - theta, and theta wherever the trace is positive.
    tol: acos loses half the digits at its ends (an input error d moves the angle by up to sqrt(2 d)); the rotation matrices are
    orthonormal to a few 1e-16, so both angles carry at most ~1e-7 rad there.  -> share of angles equal to 2 pi - theta"""
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    L = R.astype(np.longdouble)
    tr = L[:, 0, 0] + L[:, 1, 1] + L[:, 2, 2]
    theta = np.arccos(np.clip((tr - 1) / 2, -1, 1))
    a = angle_eigen32(R).astype(np.longdouble)
    is_theta = np.abs(a - theta) < tol
    is_flip = np.abs(a - (2 * np.pi - theta)) < tol
    assert np.all(is_theta | is_flip)
    assert np.all(is_theta[tr > 0])
    return float(np.mean(is_flip & ~is_theta))


def candidates(poses, stamps_ns, queries, radius=0.5, new_edge_time=5.0, max_rotation_deg=30.0, band=0.0, plain_angle=False):
    """-> (jobs, near, inside): jobs = list of (from, to) in contract order; near = set of (from, to) pairs one of whose tested
    quantities lies within the relative `band` of its threshold (a pair is tested for the time gap only inside the radius and for
    the angle only past the time gap, as in the contract); inside = number of pairs within the radius."""
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 3, 4)
    st = np.ascontiguousarray(stamps_ns, np.int64)
    n = len(P)
    jobs, near, inside = [], set(), 0
    angle = angle_plain if plain_angle else angle_eigen32
    for q in np.asarray(queries, np.int64).reshape(-1):
        q = int(q)
        if not 0 <= q < n:
            continue
        d = P[:, :, 3] - P[q, :, 3]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        others = np.arange(n) != q
        in_r = (dist < radius) & others
        inside += int(in_r.sum())
        dts = np.abs((st[q] - st).astype(np.float64) * 1e-9)      # int64 difference first
        in_t = in_r & (dts > new_edge_time)
        c_idx = np.nonzero(in_t)[0]
        deg = np.zeros(n)
        if len(c_idx):
            Rd = np.einsum("cji,jk->cik", P[c_idx, :, :3], P[q, :, :3])      # R_c^T R_q
            deg[c_idx] = np.abs(180. * angle(Rd) / np.pi)
        hit = in_t.copy()
        hit[c_idx] = deg[c_idx] < max_rotation_deg
        jobs += [(int(c), q) for c in np.nonzero(hit)[0]]
        if band > 0:
            nr = others & (np.abs(dist - radius) <= band * abs(radius))
            nr |= in_r & (np.abs(dts - new_edge_time) <= band * abs(new_edge_time))
            nr |= in_t & (np.abs(deg - max_rotation_deg) <= band * abs(max_rotation_deg))
            near |= {(int(c), q) for c in np.nonzero(nr)[0]}
    return jobs, near, inside
