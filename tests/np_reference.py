"""Independent NumPy/SciPy second implementation of the hot path's arithmetic (test infrastructure).

It exists to pin the C oracle (oracle/uzl_oracle_*.c), which has no reference golden vectors to be
checked against.  It shares no code with the oracle and deliberately takes different
routes to the same numbers:
  * Hamming distances through np.unpackbits, 2-NN through a stable argsort;
  * the rigid fit through np.linalg.svd in float64 (Kabsch), compared within tolerance;
  * EdgeSE3 error through scipy.spatial.transform.Rotation, Jacobians through central differences
    (g2o's own fallback is numeric differentiation [EXT]), the LM linear solve through
    scipy.sparse.linalg.spsolve (sparse direct, like the reference's CSparse).
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl
from scipy.spatial.transform import Rotation


# ----------------------------------------------------------------------------- matching
def hamming_matrix(query, train):
    q = np.unpackbits(np.ascontiguousarray(query, np.uint8), axis=1).astype(np.int32)
    t = np.unpackbits(np.ascontiguousarray(train, np.uint8), axis=1).astype(np.int32)
    # |a xor b| = |a| + |b| - 2 a.b
    return q.sum(1)[:, None] + t.sum(1)[None, :] - 2 * (q @ t.T)


def knn2(query, train):
    D = hamming_matrix(query, train)
    nq, nt = D.shape
    order = np.argsort(D, axis=1, kind="stable")          # ties -> lower train index first
    idx0 = order[:, 0] if nt >= 1 else np.full(nq, -1)
    idx1 = order[:, 1] if nt >= 2 else np.full(nq, -1)
    d0 = D[np.arange(nq), idx0] if nt >= 1 else np.full(nq, -1)
    d1 = D[np.arange(nq), idx1] if nt >= 2 else np.full(nq, -1)
    return idx0.astype(np.int32), d0.astype(np.int32), idx1.astype(np.int32), d1.astype(np.int32)


def filter_sort(idx0, d0, idx1, d1, valid_train, valid_query):
    ok = (idx0 >= 0) & (idx1 >= 0)
    ratio = ok & (d0.astype(np.float32).astype(np.float64) < 0.99 * d1.astype(np.float32).astype(np.float64))
    n_ratio = int(ratio.sum())
    q = np.nonzero(ratio)[0]
    keep = (np.asarray(valid_train)[idx0[q]] != 0) & (np.asarray(valid_query)[q] != 0)
    q = q[keep]
    order = np.lexsort((q, d0[q]))                         # (distance, queryIdx)
    q = q[order]
    return q.astype(np.int32), idx0[q].astype(np.int32), d0[q].astype(np.int32), n_ratio


def kabsch(P, Q):
    """Least-squares rigid T (3,4) with Q ~= T P, float64 (Arun/Kabsch)."""
    mp = P.mean(1, keepdims=True); mq = Q.mean(1, keepdims=True)
    C = (Q - mq) @ (P - mp).T
    U, S, Vt = np.linalg.svd(C)
    s = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        s[2, 2] = -1
    R = U @ s @ Vt
    return np.concatenate([R, mq - R @ mp], axis=1)


def point_distances(P, Q, T):
    return np.linalg.norm(T[:, :3] @ P + T[:, 3:4] - Q, axis=0)


# ----------------------------------------------------------------------------- SE(3)
def se3_mul(A, B):
    R = A[..., :3, :3] @ B[..., :3, :3]
    t = (A[..., :3, :3] @ B[..., :3, 3:4])[..., 0] + A[..., :3, 3]
    return np.concatenate([R, t[..., None]], axis=-1)


def se3_inv(A):
    Rt = np.swapaxes(A[..., :3, :3], -1, -2)
    t = -(Rt @ A[..., :3, 3:4])[..., 0]
    return np.concatenate([Rt, t[..., None]], axis=-1)


def to_vector_mqt(T):
    """(...,3,4) -> (...,6): translation + (qx,qy,qz) of the unit quaternion with w >= 0."""
    T = np.asarray(T)
    q = Rotation.from_matrix(T[..., :3, :3].reshape(-1, 3, 3)).as_quat()     # (x,y,z,w)
    q = q * np.where(q[:, 3:4] < 0, -1.0, 1.0)
    v = np.concatenate([T[..., :3, 3].reshape(-1, 3), q[:, :3]], axis=1)
    return v.reshape(T.shape[:-2] + (6,))


def from_vector_mqt(v):
    v = np.asarray(v, np.float64)
    vv = v.reshape(-1, 6)
    w2 = 1.0 - (vv[:, 3:] ** 2).sum(1)
    q = np.concatenate([vv[:, 3:], np.sqrt(np.maximum(w2, 0.0))[:, None]], axis=1)
    R = Rotation.from_quat(q).as_matrix()
    R[w2 < 0] = np.eye(3)
    T = np.concatenate([R, vv[:, :3, None]], axis=2)
    return T.reshape(v.shape[:-1] + (3, 4))


def edge_errors(poses, ij, meas):
    X = np.asarray(poses).reshape(-1, 3, 4); Z = np.asarray(meas).reshape(-1, 3, 4)
    E = se3_mul(se3_inv(Z), se3_mul(se3_inv(X[ij[:, 0]]), X[ij[:, 1]]))
    return to_vector_mqt(E)


def huber(e2, delta=1.0):
    e2 = np.asarray(e2, np.float64)
    big = e2 > delta * delta
    sq = np.sqrt(np.where(big, e2, 1.0))
    rho0 = np.where(big, 2 * sq * delta - delta * delta, e2)
    rho1 = np.where(big, delta / sq, 1.0)
    return rho0, rho1


def chi2(poses, ij, meas, info, robust, delta=1.0):
    e = edge_errors(poses, ij, meas)
    Om = np.asarray(info).reshape(-1, 6, 6)
    c = np.einsum("ki,kij,kj->k", e, Om, e)
    r0, _ = huber(c, delta)
    return float(np.where(np.asarray(robust) != 0, r0, c).sum())


def numeric_jacobians(poses, ij, meas, h=1e-6):
    X = np.asarray(poses).reshape(-1, 3, 4); Z = np.asarray(meas).reshape(-1, 3, 4)
    Xi = X[ij[:, 0]]; Xj = X[ij[:, 1]]
    Zi = se3_inv(Z)

    def err(Xi_, Xj_):
        return to_vector_mqt(se3_mul(Zi, se3_mul(se3_inv(Xi_), Xj_)))

    E = ij.shape[0]
    Ji = np.empty((E, 6, 6)); Jj = np.empty((E, 6, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        Dp = from_vector_mqt(d); Dm = from_vector_mqt(-d)
        Ji[:, :, k] = (err(se3_mul(Xi, Dp), Xj) - err(se3_mul(Xi, Dm), Xj)) / (2 * h)
        Jj[:, :, k] = (err(Xi, se3_mul(Xj, Dp)) - err(Xi, se3_mul(Xj, Dm))) / (2 * h)
    return Ji, Jj


def build_system(poses, fixed, ij, meas, info, robust, delta=1.0, jac=None):
    """Sparse H (BSR over all vertices; fixed rows/cols empty), b, chi2."""
    n = np.asarray(poses).reshape(-1, 12).shape[0]
    ij = np.asarray(ij).reshape(-1, 2)
    e = edge_errors(poses, ij, meas)
    Om = np.asarray(info).reshape(-1, 6, 6)
    c = np.einsum("ki,kij,kj->k", e, Om, e)
    r0, r1 = huber(c, delta)
    rb = np.asarray(robust) != 0
    w = np.where(rb, r1, 1.0)
    chi = float(np.where(rb, r0, c).sum())
    Ji, Jj = jac if jac is not None else numeric_jacobians(poses, ij, meas)
    Ow = Om * w[:, None, None]
    OJi = Ow @ Ji; OJj = Ow @ Jj
    Hii = np.swapaxes(Ji, 1, 2) @ OJi; Hjj = np.swapaxes(Jj, 1, 2) @ OJj; Hij = np.swapaxes(Ji, 1, 2) @ OJj
    Oe = np.einsum("kij,kj->ki", Ow, e)
    bi = -np.einsum("kji,kj->ki", Ji, Oe); bj = -np.einsum("kji,kj->ki", Jj, Oe)
    fi = np.asarray(fixed)[ij[:, 0]] == 0; fj = np.asarray(fixed)[ij[:, 1]] == 0
    rows = []; cols = []; blocks = []
    rows.append(ij[fi, 0]); cols.append(ij[fi, 0]); blocks.append(Hii[fi])
    rows.append(ij[fj, 1]); cols.append(ij[fj, 1]); blocks.append(Hjj[fj])
    both = fi & fj
    rows.append(ij[both, 0]); cols.append(ij[both, 1]); blocks.append(Hij[both])
    rows.append(ij[both, 1]); cols.append(ij[both, 0]); blocks.append(np.swapaxes(Hij[both], 1, 2))
    rows = np.concatenate(rows); cols = np.concatenate(cols); blocks = np.concatenate(blocks)
    # scalar COO
    rr = (6 * rows[:, None, None] + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), np.int64)
    cc = (6 * cols[:, None, None] + np.arange(6)[None, None, :]) + np.zeros((1, 6, 1), np.int64)
    H = sp.coo_matrix((blocks.ravel(), (rr.ravel(), cc.ravel())), shape=(6 * n, 6 * n)).tocsr()
    b = np.zeros((n, 6))
    np.add.at(b, ij[fi, 0], bi[fi]); np.add.at(b, ij[fj, 1], bj[fj])
    return H, b.reshape(-1), chi


def pgo_lm(poses, fixed, ij, meas, info, robust, iterations=20, delta=1.0):
    """LM as g2o's OptimizationAlgorithmLevenberg [EXT] with a sparse direct solve."""
    X = np.asarray(poses, np.float64).reshape(-1, 3, 4).copy()
    fixed = np.asarray(fixed); ij = np.asarray(ij).reshape(-1, 2)
    free = np.repeat(fixed == 0, 6)
    fidx = np.nonzero(free)[0]
    lam = 0.0; ni = 2.0
    stats = dict(iterations_done=0, lm_trials=0, terminated_early=0)
    for it in range(iterations):
        H, b, cur = build_system(X, fixed, ij, meas, info, robust, delta)
        Hf = H[fidx][:, fidx].tocsc(); bf = b[fidx]
        if it == 0:
            stats["chi2_initial"] = cur
            lam = 1e-5 * np.abs(Hf.diagonal()).max()
            ni = 2.0
        rho = 0.0; qmax = 0
        while True:
            A = Hf + lam * sp.identity(Hf.shape[0], format="csc")
            dx = spl.spsolve(A, bf)
            stats["lm_trials"] += 1
            full = np.zeros(free.shape[0]); full[fidx] = dx
            Xn = se3_mul(X, from_vector_mqt(full.reshape(-1, 6)))
            tmp = chi2(Xn, ij, meas, info, robust, delta)
            rho = (cur - tmp) / (float(dx @ (lam * dx + bf)) + 1e-3)
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); ni = 2.0
                cur = tmp; X = Xn
            else:
                lam *= ni; ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        stats["iterations_done"] = it + 1
        stats["chi2_final"] = cur
        if qmax == 10 or rho == 0:
            stats["terminated_early"] = 1
            break
    stats["lambda_final"] = lam
    return X.reshape(-1, 12), stats


# ----------------------------------------------------------------------------- the linear system stage by stage (test_pgo_system_gpu.py)
def bcsr_to_sparse(row_ptr, col, blk, diag=None, nrows=None):
    """Block-CSR (6 x 6 blocks, one slot per incident edge) -> scipy CSR of size 6 nrows.  Slots that name the same column are SUMMED
    (multi-edges); col = -1 (the neighbour is fixed) contributes nothing; diag [nrows,6,6], when given, is added on the block diagonal."""
    row_ptr = np.asarray(row_ptr, np.int64); col = np.asarray(col, np.int64); blk = np.asarray(blk, np.float64).reshape(-1, 6, 6)
    nr = len(row_ptr) - 1 if nrows is None else int(nrows)
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    keep = col >= 0
    r, c, B = rows[keep], col[keep], blk[:len(col)][keep]
    if diag is not None:
        d = np.asarray(diag, np.float64).reshape(-1, 6, 6)
        r = np.concatenate([r, np.arange(len(d))]); c = np.concatenate([c, np.arange(len(d))]); B = np.concatenate([B, d])
    rr = 6 * r[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64)
    cc = 6 * c[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
    return sp.coo_matrix((B.ravel(), (rr.ravel(), cc.ravel())), shape=(6 * nr, 6 * nr)).tocsr()      # (tocsr sums duplicates)


def block_index(blocks):
    """Scalar indices of the 6-blocks `blocks`, in order."""
    blocks = np.asarray(blocks, np.int64)
    return (6 * blocks[:, None] + np.arange(6)[None, :]).reshape(-1)


def schur_dense(A, b, keep):
    """Dense Schur complement of the blocks not in `keep`: S = A_ss - A_si A_ii^-1 A_is, g = b_s - A_si A_ii^-1 b_i (s = keep, in the order
    given; i = the other blocks, ascending)."""
    A = np.asarray(A.toarray() if sp.issparse(A) else A, np.float64); b = np.asarray(b, np.float64)
    nbk = A.shape[0] // 6
    keep = np.asarray(keep, np.int64)
    elim = np.setdiff1d(np.arange(nbk), keep)
    s, i = block_index(keep), block_index(elim)
    if len(i) == 0:
        return A[np.ix_(s, s)].copy(), b[s].copy()
    X = np.linalg.solve(A[np.ix_(i, i)], np.concatenate([A[np.ix_(i, s)], b[i][:, None]], axis=1))
    return A[np.ix_(s, s)] - A[np.ix_(s, i)] @ X[:, :-1], b[s] - A[np.ix_(s, i)] @ X[:, -1]


def step_error(dx, dx_ref):
    """Largest error of a step per kind of component: (translation [m], quaternion vector) over all vertices, dx [n,6] = (t, q_xyz)."""
    d = np.abs(np.asarray(dx, np.float64).reshape(-1, 6) - np.asarray(dx_ref, np.float64).reshape(-1, 6))
    if d.size == 0:
        return 0.0, 0.0
    return float(d[:, :3].max()), float(d[:, 3:].max())


def system_magnitudes(poses, fixed, ij, meas, info, robust, jac, delta=1.0, extra=None):
    """Per entry, the sum of the magnitudes of the terms behind H and b (as build_system adds them, with |J| + s, |Omega'|): the scale of
    the round-off an evaluation of H and b in another order or at poses rounded once differently can show.  b's terms carry |e| + s,
    s = 1 + |t_i| + |t_j| + |t_z|: the error of an edge is a difference of translations of that size, so it is only known to eps s
    absolutely however small it is (at the LM fixed point, b itself is rounding noise).  extra [E], when given, is added to s: the
    translation norms of further factors a measurement was composed from (sensor transforms, displacements), whose rounding the
    measurement carries even where its own translation cancels.  Returns (|H| terms as CSR, |b| terms [6 n])."""
    P = np.asarray(poses, np.float64).reshape(-1, 3, 4); Z = np.asarray(meas, np.float64).reshape(-1, 3, 4)
    ij = np.asarray(ij).reshape(-1, 2)
    e = edge_errors(poses, ij, meas)
    Om = np.asarray(info).reshape(-1, 6, 6)
    c = np.einsum("ki,kij,kj->k", e, Om, e)
    _, r1 = huber(c, delta)
    w = np.where(np.asarray(robust) != 0, r1, 1.0)
    s = 1.0 + np.abs(P[ij[:, 0], :, 3]).max(1) + np.abs(P[ij[:, 1], :, 3]).max(1) + np.abs(Z[:, :, 3]).max(1)
    if extra is not None:
        s = s + np.asarray(extra, np.float64)
    # a Jacobian entry is built from rotations (|.| <= 1) and relative translations (|.| <= s): rounded once differently it moves by a few
    # eps s whatever its own size (a coupling term 2 R [t_b]x of two nearby vertices far from the origin cancels): |J| + s bounds its terms
    Ji, Jj = (np.abs(np.asarray(j)) + s[:, None, None] for j in jac)
    Aw = np.abs(Om) * w[:, None, None]
    Hii = np.swapaxes(Ji, 1, 2) @ Aw @ Ji; Hjj = np.swapaxes(Jj, 1, 2) @ Aw @ Jj; Hij = np.swapaxes(Ji, 1, 2) @ Aw @ Jj
    ae = np.abs(e) + s[:, None]
    bi = np.einsum("kji,kjl,kl->ki", Ji, Aw, ae); bj = np.einsum("kji,kjl,kl->ki", Jj, Aw, ae)
    n = P.shape[0]
    fi = np.asarray(fixed)[ij[:, 0]] == 0; fj = np.asarray(fixed)[ij[:, 1]] == 0
    both = fi & fj
    rows = np.concatenate([ij[fi, 0], ij[fj, 1], ij[both, 0], ij[both, 1]])
    cols = np.concatenate([ij[fi, 0], ij[fj, 1], ij[both, 1], ij[both, 0]])
    blocks = np.concatenate([Hii[fi], Hjj[fj], Hij[both], np.swapaxes(Hij[both], 1, 2)])
    rr = 6 * rows[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 6), np.int64)
    cc = 6 * cols[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
    H = sp.coo_matrix((blocks.ravel(), (rr.ravel(), cc.ravel())), shape=(6 * n, 6 * n)).tocsr()
    b = np.zeros((n, 6))
    np.add.at(b, ij[fi, 0], bi[fi]); np.add.at(b, ij[fj, 1], bj[fj])
    return H, b.reshape(-1)


# ------------------------------------------------------------------------------------------------------------
# Edge filter: a third, pure-Python statement of TransformationFilter / EdgeCluster
# (transformation_estimation/src/transformation_filter.cpp:43-350) with the reference's object semantics
# (shared cluster objects, only the first listing repointed on merge).  Small cases only.  Point pairs are
# computed with Python floats in the oracle's operation order, so they are bit-identical; the RANSAC itself is
# passed in (it has its own independent checks above).
# ------------------------------------------------------------------------------------------------------------
def _iso_mul(A, B):
    o = [0.0] * 12
    for r in range(3):
        for c in range(3):
            o[r * 4 + c] = (A[r * 4 + 0] * B[0 * 4 + c] + A[r * 4 + 1] * B[1 * 4 + c]) + A[r * 4 + 2] * B[2 * 4 + c]
        o[r * 4 + 3] = ((A[r * 4 + 0] * B[3] + A[r * 4 + 1] * B[7]) + A[r * 4 + 2] * B[11]) + A[r * 4 + 3]
    return o


def _iso_inv(A):
    o = [0.0] * 12
    for r in range(3):
        for c in range(3):
            o[r * 4 + c] = A[c * 4 + r]
        o[r * 4 + 3] = -((A[0 * 4 + r] * A[3] + A[1 * 4 + r] * A[7]) + A[2 * 4 + r] * A[11])
    return o


_I12 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


class _Cluster:
    def __init__(self, uid, e, tf, tt):
        self.uid = uid
        self.fs = self.fe = tf
        self.ts = self.te = tt
        self.changed = False
        self.consensus = 0
        self.evals = 0
        self.edges = {}                       # key -> dict (python dicts keep insertion order)
        self.put(e, tf, tt)

    def put(self, e, tf, tt):
        d = dict(e); d["t_from"] = tf; d["t_to"] = tt; d["valid_"] = bool(e["valid"])
        self.edges[e["key"]] = d              # a present key keeps its slot
        if e["valid"]:
            self.consensus += 1

    def add(self, e, tf, tt):
        self.fs = min(tf, self.fs); self.fe = max(tf, self.fe); self.ts = min(tt, self.ts); self.te = max(tt, self.te)
        self.changed = True
        self.put(e, tf, tt)

    def is_part(self, tf, tt, max_dt):
        s = lambda a, b: (a - b) * 1e-9
        return s(tf, self.fs) > -max_dt and s(tf, self.fe) < max_dt and s(tt, self.ts) > -max_dt and s(tt, self.te) < max_dt

    def merge(self, o):
        self.fs = min(o.fs, self.fs); self.fe = max(o.fe, self.fe); self.ts = min(o.ts, self.ts); self.te = max(o.te, self.te)
        self.changed = True
        self.consensus += o.consensus
        for k, d in o.edges.items():
            self.edges.setdefault(k, d)


class FilterRef:
    def __init__(self, max_dt=5.0, min_size=8.0, max_cluster_size=100, ransac_iterations=200, max_error=0.3,
                 min_time_span=2.0, max_edges=5, seed=0):
        self.__dict__.update(locals())
        self.clusters = []
        self.edges = {}
        self.sensors = []
        self.next_uid = 0

    def set_sensors(self, sensors):
        self.sensors = [list(map(float, s)) for s in np.asarray(sensors).reshape(-1, 12)]

    def add(self, edges):
        for e in edges:
            if e["key"] in self.edges:
                for c in self.edges[e["key"]]:
                    if e["key"] in c.edges:
                        d = c.edges[e["key"]]
                        for f in ("pose_from", "pose_to", "transform", "displacement_from", "displacement_to", "sensor_from",
                                  "sensor_to", "matching_score", "valid"):
                            d[f] = e[f]
                continue
            for tf in map(int, e["stamps_from"]):
                for tt in map(int, e["stamps_to"]):
                    matched = [i for i, c in enumerate(self.clusters)
                               if len(c.edges) < self.max_cluster_size and c.is_part(tf, tt, self.max_dt)]
                    if not matched:
                        c = _Cluster(self.next_uid, e, tf, tt); self.next_uid += 1
                        self.clusters.append(c)
                        self.edges.setdefault(e["key"], []).append(c)
                    else:
                        c0 = self.clusters[matched[0]]
                        c0.add(e, tf, tt)
                        self.edges.setdefault(e["key"], []).append(c0)
                        for i in reversed(matched[1:]):
                            ci = self.clusters[i]
                            if len(c0.edges) + len(ci.edges) < self.max_cluster_size:
                                for k in ci.edges:
                                    lst = self.edges.get(k, [])
                                    for u in range(len(lst)):
                                        if lst[u] is ci:
                                            lst[u] = c0
                                            break
                                c0.merge(ci)
                                del self.clusters[i]

    def remove(self, keys):
        for key in map(int, keys):
            if key not in self.edges:
                continue
            for c in self.edges[key]:
                if key in c.edges:
                    if c.edges[key]["valid_"]:
                        c.consensus -= 1
                    del c.edges[key]
                if len(c.edges) == 0:
                    self.clusters = [x for x in self.clusters if x is not c]
            del self.edges[key]

    def all_edges(self):
        return np.array(sorted(self.edges), np.uint64)

    def _points(self, d):
        Sf = self.sensors[d["sensor_from"]] if 0 <= d["sensor_from"] < len(self.sensors) else _I12
        St = self.sensors[d["sensor_to"]] if 0 <= d["sensor_to"] < len(self.sensors) else _I12
        f = lambda v: list(map(float, v))
        a = _iso_mul(f(d["pose_from"]), f(d["displacement_from"]))
        a = _iso_mul(a, Sf)
        a = _iso_mul(a, f(d["transform"]))
        a = _iso_mul(a, _iso_inv(St))
        b = _iso_mul(f(d["pose_to"]), f(d["displacement_to"]))
        return [a[3], a[7], a[11]], [b[3], b[7], b[11]]

    def calc_valid_edges(self, ransac):
        """ransac(P (m,3), Q (m,3), job_id) -> (T(12), set(m) of consensus3D with that T)"""
        n = 0
        for c in self.clusters:
            if len(c.edges) < self.min_size or not c.changed:
                continue
            if abs((c.fs - c.fe) * 1e-9) < self.min_time_span or abs((c.ts - c.te) * 1e-9) < self.min_time_span:
                continue
            c.changed = False
            pq = [self._points(d) for d in c.edges.values()]
            P = np.array([p for p, _ in pq]); Q = np.array([q for _, q in pq])
            T, s = ransac(P, Q, (c.uid << 20) + c.evals)
            c.evals += 1; n += 1
            c.lastP, c.lastQ = P, Q
            cons = int(np.sum(s))
            if cons >= self.min_size and cons >= c.consensus:
                c.consensus = cons
                for d, v in zip(c.edges.values(), s):
                    d["valid_"] = bool(v)
        return n

    def valid_edges(self):
        ids = set()
        for c in self.clusters:
            v = [d for d in c.edges.values() if d["valid_"]]
            if len(v) > 2 * self.max_edges:
                v = sorted(v, key=lambda d: -d["matching_score"])          # python's sort is stable
                ids.update(d["key"] for d in v[:self.max_edges])
                inc = len(v) / self.max_edges
                ids.update(v[int(np.floor(inc * i))]["key"] for i in range(self.max_edges - 1))
                ids.add(v[-1]["key"])
            else:
                ids.update(d["key"] for d in v)
        return np.array(sorted(ids), np.uint64)

    def state(self):
        return [dict(uid=c.uid, from_start_ns=c.fs, from_end_ns=c.fe, to_start_ns=c.ts, to_end_ns=c.te, size=len(c.edges),
                     consensus=c.consensus, changed=int(c.changed), evaluations=c.evals,
                     keys=np.array(list(c.edges), np.uint64), valid=np.array([d["valid_"] for d in c.edges.values()], np.uint8))
                for c in self.clusters]


# ------------------------------------------------------------------------------------------------------------
# The multilevel preconditioner stage by stage (test_pgo_hierarchy_gpu.py, test_np_reference_system.py): a float64 restatement of the
# aggregation hierarchy of csrc/pgo_types.hpp.  Level 0 = the rows of a block system (row_ptr, col, blk, hdiag); level l+1 aggregates
# fan_{l+1} consecutive level-l entities.  Nothing is ever formed densely at level 0; levels >= 1 are, for the dense operators.
# Every stage has an absolute-value twin (absolute=True, or a *_mag function): the same sums over the magnitudes of their terms, the
# scale its round-off bound is built from.  `fault` plants one defect ON THE REFERENCE SIDE, so a test can show that the bound would
# see it; no kernel ever carries one.
# ------------------------------------------------------------------------------------------------------------
def skew(d):
    """[d]x for d [..., 3]"""
    d = np.asarray(d, np.float64)
    z = np.zeros(d.shape[:-1])
    return np.stack([np.stack([z, -d[..., 2], d[..., 1]], -1), np.stack([d[..., 2], z, -d[..., 0]], -1),
                     np.stack([-d[..., 1], d[..., 0], z], -1)], -2)


def ml_level_sizes(nb, fans):
    """n_l of every level for the fan-outs fans[1..L] (fans[0] is not read)."""
    n = [int(nb)]
    for f in fans[1:]:
        n.append(-(-n[-1] // int(f)))
    return n


def ml_geometry(t, R, fans, fault=None):
    """Centroids and offsets of a hierarchy over level-0 rows with translations t [n0,3] and rotations R [n0,3,3]; a row whose t is NaN is
    EMPTY (no pose: weight 0, zero prolongation block).  Returns (cen, geo): cen[l] [n_l,4] = weighted mean of the children's centroids
    and the vertices underneath (cen[0] is None); geo[0] [n0,12] = R^T | t - c_parent, geo[l] [n_l,3] = c_self - c_parent (l < L),
    geo[L] = zeros.  fault = ("fan", l): the centroids of level l divide by fan_l children instead of the weight that is there."""
    t = np.asarray(t, np.float64); R = np.asarray(R, np.float64)
    live = ~np.isnan(t).any(1)
    c = np.where(live[:, None], t, 0.0); w = live.astype(np.float64)
    n = ml_level_sizes(len(t), fans)
    L = len(fans) - 1
    cen = [None]; geo = []
    child_c = c
    for l in range(1, L + 1):
        par = np.arange(n[l - 1]) // fans[l]
        ws = np.bincount(par, w, minlength=n[l])
        den = np.full(n[l], float(fans[l])) if fault == ("fan", l) else ws
        cl_ = np.stack([np.bincount(par, w * child_c[:, k], minlength=n[l]) for k in range(3)], 1)
        cl_ = np.where(ws[:, None] > 0, cl_ / np.where(den > 0, den, 1.0)[:, None], 0.0)
        d = child_c - cl_[par]
        if l == 1:
            g0 = np.zeros((n[0], 12))
            g0[:, :9] = np.swapaxes(R, 1, 2).reshape(-1, 9); g0[:, 9:] = d
            g0[~live] = 0.0
            geo.append(g0)
        else:
            geo.append(d)
        cen.append(np.concatenate([cl_, ws[:, None]], 1))
        child_c, w = cl_, ws
    geo.append(np.zeros((n[L], 3)))
    return cen, geo


def ml_prolong_blocks(level, geo, absolute=False):
    """The 6 x 6 prolongation block of every entity of `level` towards its parent, from the level's geo array:
    level 0: [[R^T, -R^T [d]x], [0, 1/2 R^T]] (all zero for an EMPTY row); above: [[I, -[d]x], [0, I]]."""
    geo = np.asarray(geo, np.float64)
    n = len(geo)
    P = np.zeros((n, 6, 6))
    if level == 0:
        Rt = geo[:, :9].reshape(n, 3, 3)
        S = -skew(geo[:, 9:])
        P[:, :3, :3] = Rt; P[:, 3:, 3:] = 0.5 * Rt
        P[:, :3, 3:] = (np.abs(Rt) @ np.abs(S)) if absolute else (Rt @ S)
    else:
        P[:, :3, :3] = np.eye(3); P[:, 3:, 3:] = np.eye(3); P[:, :3, 3:] = -skew(geo[:, :3])
    return np.abs(P) if absolute else P


def ml_coarse_structure(row_ptr, col, fan, n_c):
    """Slots of level l+1 from those of level l: exactly the pairs (A, C), A != C, of aggregates joined by a level-l slot, rows ascending,
    columns ascending within a row.  Returns (row_ptr_c, col_c, fine -> coarse slot index or -1)."""
    row_ptr = np.asarray(row_ptr, np.int64); col = np.asarray(col, np.int64)
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    A = rows // fan; Cc = np.where(col >= 0, col // fan, -1)
    off = (col >= 0) & (A != Cc)
    key = A[off] * n_c + Cc[off]
    uk, inv = np.unique(key, return_inverse=True)
    m = np.full(len(col), -1, np.int64); m[off] = inv
    rp = np.zeros(n_c + 1, np.int64)
    np.add.at(rp, uk // n_c + 1, 1)
    return np.cumsum(rp), uk % n_c, m


def ml_galerkin(row_ptr, col, blk, G, M, P, fan, absolute=False, fault=None):
    """A_{l+1}(0) = P^T A_l(0) P in the device's slot structure and the lambda multiplier M_{l+1} = P^T M_l P (M = None: M_0 = I; an EMPTY
    row has P = 0 and adds nothing).  Returns (row_ptr_c, col_c, blk_c [slots,6,6], G_c [n_c,6,6], M_c [n_c,6,6]).  absolute: |P|^T |A_l| |P|
    with P = |P| given.  fault = ("drop", q): contribution q (a level-l slot with col >= 0) is left out."""
    row_ptr = np.asarray(row_ptr, np.int64); col = np.asarray(col, np.int64)
    blk = np.asarray(blk, np.float64).reshape(-1, 6, 6); G = np.asarray(G, np.float64).reshape(-1, 6, 6)
    n = len(row_ptr) - 1
    n_c = -(-n // fan)
    if absolute:
        blk, G, P = np.abs(blk), np.abs(G), np.abs(P)
    Mf = np.tile(np.eye(6), (n, 1, 1)) if M is None else (np.abs(M) if absolute else np.asarray(M, np.float64)).reshape(-1, 6, 6)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    rp, cc, m = ml_coarse_structure(row_ptr, col, fan, n_c)
    ok = col >= 0
    T = np.zeros((len(col), 6, 6))
    T[ok] = np.swapaxes(P[rows[ok]], 1, 2) @ blk[:len(col)][ok] @ P[col[ok]]
    if fault is not None and fault[0] == "drop":
        T[np.nonzero(ok)[0][fault[1]]] = 0.0
    blk_c = np.zeros((len(cc), 6, 6))
    np.add.at(blk_c, m[m >= 0], T[m >= 0])
    par = np.arange(n) // fan
    G_c = np.zeros((n_c, 6, 6)); M_c = np.zeros((n_c, 6, 6))
    same = ok & (m < 0)
    np.add.at(G_c, rows[same] // fan, T[same])
    Pt = np.swapaxes(P, 1, 2)
    np.add.at(G_c, par, Pt @ G[:n] @ P)
    np.add.at(M_c, par, Pt @ Mf @ P)
    return rp, cc, blk_c, G_c, M_c


def ml_sibling_blocks(level, row_ptr, col, blk, G, M, lam, fan, couple=True, fault=None):
    """A_l(lambda) restricted to the children of every level-(l+1) aggregate: [n_{l+1}, 6 fan, 6 fan].  Diagonal blocks G + lambda M
    (level 0: G + lambda I); off-diagonal blocks between siblings, multi-edges summed (couple = False: none - the block-diagonal level-0
    smoother, PgoDev::sibling0 = 0); a missing child (the last aggregate) or a child whose diagonal block is all zero (an aggregate of
    EMPTY rows of a coarse level) gets identity rows.  Returns (W, padded [n_{l+1}, fan] bool).  fault = ("drop", q): the q-th slot that
    couples two siblings is left out."""
    row_ptr = np.asarray(row_ptr, np.int64); col = np.asarray(col, np.int64)
    blk = np.asarray(blk, np.float64).reshape(-1, 6, 6)
    n = len(row_ptr) - 1
    n_c = -(-n // fan)
    D = np.asarray(G, np.float64).reshape(-1, 6, 6)[:n] + lam * (np.tile(np.eye(6), (n, 1, 1)) if level == 0 else np.asarray(M, np.float64).reshape(-1, 6, 6)[:n])
    W = np.zeros((n_c, fan, 6, fan, 6))
    ent = np.arange(n)
    zero = np.abs(D).reshape(n, -1).max(1) == 0
    D[zero] = np.eye(6)
    W[ent // fan, ent % fan, :, ent % fan, :] = D
    padded = np.ones((n_c, fan), bool)
    padded[ent // fan, ent % fan] = False
    for A, j in zip(*np.nonzero(padded)):
        W[A, j, :, j, :] = np.eye(6)
    if couple:
        rows = np.repeat(ent, np.diff(row_ptr))
        s = (col >= 0) & (rows // fan == col // fan) & (rows != col)
        if fault is not None and fault[0] == "drop":
            s[np.nonzero(s)[0][fault[1]]] = False
        np.add.at(W, (rows[s] // fan, rows[s] % fan, slice(None), col[s] % fan, slice(None)), blk[:len(col)][s])
    return W.reshape(n_c, 6 * fan, 6 * fan), padded


def ml_level_matrix(row_ptr, col, blk, G, M, lam):
    """A_l(lambda) of a coarse level (l >= 1) as a dense matrix."""
    D = np.asarray(G, np.float64).reshape(-1, 6, 6) + lam * np.asarray(M, np.float64).reshape(-1, 6, 6)
    return bcsr_to_sparse(row_ptr, col, blk, diag=D, nrows=len(D)).toarray()


def ml_dense_P(geo, fan, absolute=False):
    """Prolongation from level l+1 to level l (l >= 1) as a dense [6 n_l, 6 n_{l+1}] matrix."""
    B = ml_prolong_blocks(1, geo, absolute)
    n = len(B); n_c = -(-n // fan)
    P = np.zeros((n, 6, n_c, 6))
    P[np.arange(n), :, np.arange(n) // fan, :] = B
    return P.reshape(6 * n, 6 * n_c)


def ml_dense_S(Winv, n, fault=None):
    """blockdiag of the sibling inverses Winv [n_{l+1}, m, m], cut to the 6 n rows that exist.  fault = ("transpose", A, i, j): the 6 x 6
    tile (i, j) of aggregate A is transposed."""
    Winv = np.array(Winv, np.float64)
    if fault is not None and fault[0] == "transpose":
        _, A, i, j = fault
        Winv[A, 6 * i:6 * i + 6, 6 * j:6 * j + 6] = Winv[A, 6 * i:6 * i + 6, 6 * j:6 * j + 6].T.copy()
    n_c, m, _ = Winv.shape
    S = np.zeros((n_c * m, n_c * m))
    for A in range(n_c):
        S[A * m:(A + 1) * m, A * m:(A + 1) * m] = Winv[A]
    return S[:6 * n, :6 * n]


def ml_additive(S, P, Yup, absolute=False):
    """Y_l = blockdiag(W_l^-1) + P Y_{l+1} P^T; absolute: |S| + |P| |Y_{l+1}| |P|^T."""
    if absolute:
        S, P, Yup = np.abs(S), np.abs(P), np.abs(Yup)
    return S + P @ Yup @ P.T


def tile_mirror(Z, tile):
    """Z with every tile x tile tile BELOW the diagonal replaced by the transpose of its partner above (diagonal tiles as they are): what
    a kernel leaves that computes the tiles on and above the diagonal of a symmetric result and mirrors them."""
    if not tile:
        return Z
    b = np.arange(Z.shape[0]) // tile
    return np.where(b[:, None] > b[None, :], Z.T, Z)


def ml_mult_cycle(S, A, P, Yup, absolute=False, fault=None, tile=None):
    """X_0 = 2 S - S A S + Q Y_{l+1} Q^T, Q = P - S A P; absolute: 2 |S| + |S| |A| |S| + |Q| |Y| |Q|^T with |Q| = |P| + |S| |A| |P|.
    tile: the result is tile_mirror'ed (S is symmetric only to the round-off of its inversion, so X_0 is, too: the kernel that adds
    Q Y Q^T settles which half counts).  fault = ("tile", i, j): the 16 x 16 tile (i, j) of Q Y Q^T is left out."""
    if absolute:
        S, A, P, Yup = np.abs(S), np.abs(A), np.abs(P), np.abs(Yup)
        Q = P + S @ A @ P
        return 2 * S + S @ A @ S + Q @ Yup @ Q.T
    Q = P - S @ (A @ P)
    C = Q @ Yup @ Q.T
    if fault is not None and fault[0] == "tile":
        _, i, j = fault
        C[16 * i:16 * i + 16, 16 * j:16 * j + 16] = 0.0
    return tile_mirror(2 * S - S @ A @ S + C, tile)


def ml_newton_schulz(X, A, steps, skip=None, tile=None):
    """k steps X <- 2 X - X A X.  tile: as the kernels take a step (ml_ns_ax + ml_ns_gemm / ml_ns_gemm32) - the left factor is read
    through X's symmetry, X <- 2 X - X^T (A X), on the tiles on and above the diagonal, mirrored (tile_mirror); the same step for a
    symmetric X, and X is symmetric only to the round-off of the sibling inverses.  Returns (X_k, sum over the steps of
    2 |X| + |X|^T |A| |X|: the magnitude of the steps' round-off).  skip: a step that is not taken (planted fault)."""
    X = np.array(X, np.float64)
    mag = np.zeros_like(X)
    Aa = np.abs(A)
    for k in range(steps):
        if k == skip:
            continue
        Xa = np.abs(X)
        Xl = X.T if tile else X
        mag += 2 * Xa + np.abs(Xl) @ Aa @ Xa
        X = tile_mirror(2 * X - Xl @ (A @ X), tile)
    return X, mag


def ml_restrict(P, r, fan):
    """r_{l+1}[A] = sum over the children c of A of P_c^T r_l[c]"""
    n = len(P); n_c = -(-n // fan)
    out = np.zeros((n_c, 6))
    np.add.at(out, np.arange(n) // fan, np.einsum("nij,ni->nj", P, np.asarray(r, np.float64).reshape(n, 6)))
    return out


def ml_apply(r, Pblk, Winv, fans, top_inv, cl=0, Ycl=None, absolute=False, coarse_from=None):
    """z = W_0^-1 r + P_1 ( W_1^-1 r_1 + P_2 ( ... ) ), r_{l+1} = P_{l+1}^T r_l, walked to A_L^-1 = top_inv, or with the levels from cl up
    replaced by the dense operator Ycl (the f32 values, accumulated in float64) when cl > 0.  Pblk[l]: prolongation blocks of level l
    (ml_prolong_blocks), Winv[l]: [n_{l+1}, 6 fan, 6 fan].  absolute: every operand by magnitude (give |r|) - the application's bound.
    coarse_from = g: without the smoothers below level g - the part of z that goes through the residual gathered at level g."""
    a = np.abs if absolute else (lambda x: x)
    L = len(fans) - 1
    stop = cl if cl > 0 else L
    rs = [a(np.asarray(r, np.float64)).reshape(-1, 6)]
    for l in range(stop):
        rs.append(ml_restrict(a(Pblk[l]), rs[l], fans[l + 1]))
    top = a(np.asarray(Ycl, np.float64)) if cl > 0 else a(np.asarray(top_inv, np.float64))
    z = (top @ rs[stop].reshape(-1)).reshape(-1, 6)
    for l in range(stop - 1, -1, -1):
        n = len(rs[l]); fan = fans[l + 1]
        W = a(np.asarray(Winv[l], np.float64))
        n_c, m, _ = W.shape
        rp = np.zeros((n_c * fan, 6)); rp[:n] = rs[l]
        zl = np.einsum("aij,aj->ai", W, rp.reshape(n_c, m)).reshape(-1, 6)[:n] * (0.0 if (coarse_from is not None and l < coarse_from) else 1.0)
        z = zl + np.einsum("nij,nj->ni", a(Pblk[l]), z[np.arange(n) // fan])
    return z
