"""NumPy restatement of the colour point-cloud registration contract (include/uzl_mi355x.h, "Colour point-cloud registration"):
the pin of uzl_cloud_*.  Steps 1-2 (cloud from images, voxel grid) make the test clouds; steps 3-10 are what the device runs.
Every formula is written in the order the header gives; f32 values are numpy.float32 arrays (NumPy neither fuses nor widens),
the sums of steps 4 and 7 are the only place where the order differs from the device's (rank order is kept; the 28 sums of
step 7 go through numpy.sum unless order="device" asks for the kernel's strip -> butterfly -> four-wave order, which the stage
tests of tests/test_cloud_step_gpu.py compare bit for bit).  tests/test_cloud_reference.py and tests/test_cloud_step_reference.py
check this file by independent means."""
import math

import numpy as np

f32 = np.float32
JACOBI_SWEEPS = 8
MU0, MU_MIN, INNER_EPS = 1e-6, 1e-12, 1e-9
CBRT_STEPS = 6
MAX_POINTS = 32768
OK, NO_CORR, LOW_SCORE, TOO_FAR = range(4)
DEFAULTS = dict(leaf_size=f32(0.05), z_min=f32(0.0), z_max=f32(5.0), lab_weight=f32(0.024), k=20, gicp_epsilon=0.001,
                max_correspondence_dist=0.2, max_iterations=20, inner_iterations=10, rotation_epsilon=2e-3,
                transformation_epsilon=5e-4, min_score=0.3, max_translation=1.0, max_rotation_deg=30.0)


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


# ------------------------------------------------------------------------------------------------ steps 1-2
def cloud_from_images(depth, bgr, fx, fy, cx, cy):
    """step 1 -> (xyz f32 (n, 3), bgr u8 (n, 3)) in ascending pixel index"""
    depth = np.asarray(depth, f32)
    h, w = depth.shape
    v, u = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore"):
        ok = (depth > 0) & ~np.isnan(depth)
    d = depth[ok]
    x = ((u[ok] - cx) * d.astype(np.float64) / fx).astype(f32)
    y = ((v[ok] - cy) * d.astype(np.float64) / fy).astype(f32)
    return np.stack([x, y, d], 1), np.asarray(bgr, np.uint8)[ok]


def voxel_keys(xyz, cfg=DEFAULTS):
    """step 2's filter and keys -> (indices of the kept points, their int32 keys), or None when the grid overflows int32"""
    xyz = np.asarray(xyz, f32)
    keep = np.flatnonzero(np.isfinite(xyz).all(1) & (xyz[:, 2] >= cfg["z_min"]) & (xyz[:, 2] <= cfg["z_max"]))
    if len(keep) == 0:
        return keep, np.zeros(0, np.int32)
    p = xyz[keep]
    inv = f32(1.0) / f32(cfg["leaf_size"])
    lo = np.floor(p.min(0) * inv).astype(np.int64)
    hi = np.floor(p.max(0) * inv).astype(np.int64)
    dx, dy, dz = (hi - lo + 1).tolist()
    if dx * dy * dz > 2**31 - 1:
        return None
    ijk = np.floor(p * inv).astype(np.int64) - lo
    return keep, (ijk[:, 0] + ijk[:, 1] * dx + ijk[:, 2] * dx * dy).astype(np.int32)


def voxel_grid(xyz, bgr, cfg=DEFAULTS):
    """step 2 -> (xyz f32 (m, 3), bgr u8 (m, 3)), one point per occupied voxel in ascending key"""
    r = voxel_keys(xyz, cfg)
    if r is None:
        raise ValueError("the voxel grid overflows int32")
    keep, key = r
    order = np.argsort(key, kind="stable")
    keep, key = keep[order], key[order]
    vals = np.concatenate([np.asarray(xyz, f32)[keep], np.asarray(bgr, np.uint8)[keep][:, ::-1].astype(f32)], 1)   # x y z r g b
    head = np.flatnonzero(np.r_[True, key[1:] != key[:-1]]) if len(key) else np.zeros(0, np.int64)
    group = np.cumsum(np.r_[True, key[1:] != key[:-1]]) - 1 if len(key) else np.zeros(0, np.int64)
    rank = np.arange(len(key)) - head[group] if len(key) else np.zeros(0, np.int64)
    acc = np.zeros((len(head), 6), f32)
    for r_ in range(int(rank.max()) + 1 if len(key) else 0):          # the f32 sums in ascending pixel index
        m = rank == r_
        acc[group[m]] += vals[m]
    cnt = np.bincount(group, minlength=len(head)).astype(f32)[:, None] if len(key) else np.zeros((0, 1), f32)
    c = acc / cnt
    return c[:, :3].copy(), c[:, 5:2:-1].astype(np.uint8)


# ------------------------------------------------------------------------------------------------ step 3
def lin_table():
    return np.array([math.pow((v / 255.0 + 0.055) / 1.055, 2.4) if v / 255.0 > 0.04045 else v / 255.0 / 12.92 for v in range(256)])


def cbrt(x):
    x = np.asarray(x, np.float64)
    y = 0.35 + 0.7 * x
    for _ in range(CBRT_STEPS):
        y3 = (y * y) * y
        y = (y * (y3 + (x + x))) / ((y3 + y3) + x)
    return y


def _lab_f(x):
    return np.where(x > 0.008856, cbrt(np.maximum(x, 0.008856)), 7.787 * x + 16.0 / 116.0)


def lab(bgr):
    """-> f32 (n, 3): L, a, b"""
    t = lin_table()
    bgr = np.asarray(bgr, np.uint8).reshape(-1, 3)
    B, G, R = t[bgr[:, 0]], t[bgr[:, 1]], t[bgr[:, 2]]
    X = ((R * 0.4124 + G * 0.3576) + B * 0.1805) / 0.95047
    Y = (R * 0.2126 + G * 0.7152) + B * 0.0722
    Z = ((R * 0.0193 + G * 0.1192) + B * 0.9505) / 1.08883
    X, Y, Z = _lab_f(X), _lab_f(Y), _lab_f(Z)
    return np.stack([(116.0 * Y - 16.0).astype(f32), (500.0 * (X - Y)).astype(f32), (200.0 * (Y - Z)).astype(f32)], 1)


# ------------------------------------------------------------------------------------------------ step 4
def knn(xyz, k):
    """-> (n, k) indices in rank order, (n, k) f32 distances"""
    xyz = np.asarray(xyz, f32)
    n = len(xyz)
    idx = np.zeros((n, k), np.int64)
    dist = np.zeros((n, k), f32)
    for lo in range(0, n, 512):
        q = xyz[lo:lo + 512, None, :]
        dx, dy, dz = q[..., 0] - xyz[None, :, 0], q[..., 1] - xyz[None, :, 1], q[..., 2] - xyz[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        o = np.argsort(d, axis=1, kind="stable")[:, :k]
        idx[lo:lo + 512] = o
        dist[lo:lo + 512] = np.take_along_axis(d, o, 1)
    return idx, dist


def _jacobi(a, V, p, q, r):
    apq = a[(p, q)]
    live = apq != 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        theta = (a[(q, q)] - a[(p, p)]) / (2.0 * apq)
        t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        app, aqq = a[(p, p)] - t * apq, a[(q, q)] + t * apq
        rp_, rq_ = (min(r, p), max(r, p)), (min(r, q), max(r, q))
        arp, arq = c * a[rp_] - s * a[rq_], s * a[rp_] + c * a[rq_]
        new = {(p, p): app, (q, q): aqq, (p, q): np.zeros_like(apq), rp_: arp, rq_: arq}
        for k_, v in new.items():
            a[k_] = np.where(live, v, a[k_])
        for row in range(3):
            vp, vq = c * V[row][p] - s * V[row][q], s * V[row][p] + c * V[row][q]
            V[row][p], V[row][q] = np.where(live, vp, V[row][p]), np.where(live, vq, V[row][q])


def normals(cov6, dtype=np.float64):
    """cov6: (n, 6) upper triangles 00 01 02 11 12 22 -> (n, 3) unit eigenvectors of the smallest eigenvalue by cyclic Jacobi"""
    a = {(0, 0): cov6[:, 0].copy(), (0, 1): cov6[:, 1].copy(), (0, 2): cov6[:, 2].copy(), (1, 1): cov6[:, 3].copy(),
         (1, 2): cov6[:, 4].copy(), (2, 2): cov6[:, 5].copy()}
    one, zero = np.ones(len(cov6), dtype), np.zeros(len(cov6), dtype)
    V = [[one.copy(), zero.copy(), zero.copy()], [zero.copy(), one.copy(), zero.copy()], [zero.copy(), zero.copy(), one.copy()]]
    for _ in range(JACOBI_SWEEPS):
        _jacobi(a, V, 0, 1, 2)
        _jacobi(a, V, 0, 2, 1)
        _jacobi(a, V, 1, 2, 0)
    n = np.stack([V[0][0], V[1][0], V[2][0]], 1)
    e = a[(0, 0)].copy()
    for c in (1, 2):
        m = a[(c, c)] < e
        n[m] = np.stack([V[0][c], V[1][c], V[2][c]], 1)[m]
        e = np.where(m, a[(c, c)], e)
    ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n / ln[:, None]


def neighbour_cov(xyz, idx, dtype=np.float64):
    """the covariance of step 4 (before the normal) -> (n, 6)"""
    k = idx.shape[1]
    P = np.asarray(xyz, f32).astype(dtype)
    s = np.zeros((len(P), 3), dtype)
    S = np.zeros((len(P), 6), dtype)
    for r in range(k):
        p = P[idx[:, r]]
        s += p
        S += np.stack([p[:, 0] * p[:, 0], p[:, 0] * p[:, 1], p[:, 0] * p[:, 2], p[:, 1] * p[:, 1], p[:, 1] * p[:, 2], p[:, 2] * p[:, 2]], 1)
    kk = dtype(k)
    m = s / kk
    mm = np.stack([m[:, 0] * m[:, 0], m[:, 0] * m[:, 1], m[:, 0] * m[:, 2], m[:, 1] * m[:, 1], m[:, 1] * m[:, 2], m[:, 2] * m[:, 2]], 1)
    return S / kk - mm


def covariances(xyz, cfg=DEFAULTS, dtype=np.float64):
    """-> (n, 6) upper triangles of C = I - ((1 - eps) n) n^T"""
    idx, _ = knn(xyz, cfg["k"])
    n = normals(neighbour_cov(xyz, idx, dtype), dtype)
    w = dtype(1.0) - dtype(cfg["gicp_epsilon"])
    wn = w * n
    one, zero = dtype(1.0), dtype(0.0)
    return np.stack([one - wn[:, 0] * n[:, 0], zero - wn[:, 0] * n[:, 1], zero - wn[:, 0] * n[:, 2], one - wn[:, 1] * n[:, 1],
                     zero - wn[:, 1] * n[:, 2], one - wn[:, 2] * n[:, 2]], 1)


def full(c6):
    """(n, 6) -> (n, 3, 3)"""
    return c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def make_cloud(xyz, bgr, cfg=DEFAULTS):
    """what uzl_cloud_add_points stores"""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
    if len(xyz) < cfg["k"] or len(xyz) > MAX_POINTS or not np.isfinite(xyz).all():
        raise ValueError("refused")
    return dict(xyz=xyz, bgr=bgr, lab=lab(bgr), cov=covariances(xyz, cfg), n=len(xyz))


# ------------------------------------------------------------------------------------------------ steps 5-6
def move32(xyz, T):
    """((g0 x + g1 y) + g2 z) + g3 per row in f32"""
    g = np.asarray(T, np.float64).reshape(3, 4).astype(f32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.stack([((g[r, 0] * x + g[r, 1] * y) + g[r, 2] * z) + g[r, 3] for r in range(3)], 1)


def correspondences(src, tgt, G, T, cfg=DEFAULTS):
    """step 6's search at the estimate T with the target moved by G -> (j int32, dist2 f32, kept int32)"""
    w = f32(cfg["lab_weight"])
    q = np.concatenate([move32(src["xyz"], T), w * src["lab"]], 1)
    t = np.concatenate([move32(tgt["xyz"], G), w * tgt["lab"]], 1)
    j = np.zeros(len(q), np.int32)
    d2 = np.zeros(len(q), f32)
    for lo in range(0, len(q), 256):
        e = q[lo:lo + 256, None, :] - t[None, :, :]
        e = e * e
        d = ((((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]) + e[..., 4]) + e[..., 5]
        jj = np.argmin(d, 1)
        j[lo:lo + 256] = jj
        d2[lo:lo + 256] = d[np.arange(len(jj)), jj]
    thr = cfg["max_correspondence_dist"] * cfg["max_correspondence_dist"]
    return j, d2, (d2.astype(np.float64) < thr).astype(np.int32)


def _rcr(R, c6):
    """upper triangle of (R C) R^T, each product as ((a b) + (c d)) + (e f)"""
    C = full(np.asarray(c6, R.dtype))
    A = [[(R[r, 0] * C[:, 0, c] + R[r, 1] * C[:, 1, c]) + R[r, 2] * C[:, 2, c] for c in range(3)] for r in range(3)]
    return [(A[r][0] * R[c, 0] + A[r][1] * R[c, 1]) + A[r][2] * R[c, 2] for r in range(3) for c in range(r, 3)]


def mahalanobis(T, G, c1, c2, dtype=np.float64):
    """M_i of step 6 -> (n, 6)"""
    T, G = np.asarray(T, np.float64).reshape(3, 4).astype(dtype), np.asarray(G, np.float64).reshape(3, 4).astype(dtype)
    a, b = _rcr(T[:, :3], c1), _rcr(G[:, :3], c2)
    s00, s01, s02, s11, s12, s22 = [(dtype(0.0) + x) + y for x, y in zip(a, b)]
    c00, c01, c02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
    c11, c12, c22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
    det = (s00 * c00 + s01 * c01) + s02 * c02
    return np.stack([c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det], 1)


# ------------------------------------------------------------------------------------------------ step 7
BLOCK, WAVE = 256, 64                 # the step kernel's workgroup and its waves


def terms(T, p, q, M, dtype=np.float64):
    """the terms of step 7's 28 sums, one column per kept row -> (28, n)"""
    T = np.asarray(T, np.float64).reshape(3, 4).astype(dtype)
    p, q, M = np.asarray(p, dtype), np.asarray(q, dtype), np.asarray(M, dtype)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    ax, ay, az = [(T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z for r in range(3)]
    dx, dy, dz = (ax + T[0, 3]) - q[:, 0], (ay + T[1, 3]) - q[:, 1], (az + T[2, 3]) - q[:, 2]
    m00, m01, m02, m11, m12, m22 = M.T
    ex, ey, ez = (m00 * dx + m01 * dy) + m02 * dz, (m01 * dx + m11 * dy) + m12 * dz, (m02 * dx + m12 * dy) + m22 * dz
    A00, A01, A02 = ay * m02 - az * m01, ay * m12 - az * m11, ay * m22 - az * m12
    A10, A11, A12 = az * m00 - ax * m02, az * m01 - ax * m12, az * m02 - ax * m22
    A20, A21, A22 = ax * m01 - ay * m00, ax * m11 - ay * m01, ax * m12 - ay * m02
    return np.stack([ay * A02 - az * A01, az * A00 - ax * A02, ax * A01 - ay * A00, az * A10 - ax * A12, ax * A11 - ay * A10, ax * A21 - ay * A20,
                     A00, A01, A02, A10, A11, A12, A20, A21, A22, m00, m01, m02, m11, m12, m22,
                     ay * ez - az * ey, az * ex - ax * ez, ax * ey - ay * ex, ex, ey, ez, (dx * ex + dy * ey) + dz * ez]).reshape(28, len(p))


def device_sum(t, rows):
    """(k, n) terms of the kept rows `rows` (their indices in the source cloud, ascending) summed as cloud_eval sums them: lane l
    of 256 adds its rows l, l + 256, ... in increasing order from 0.0 (a row that is not kept adds nothing), an xor butterfly with
    offsets 32, 16, ..., 1 inside each wave of 64 lanes, then (w0 + w1) + (w2 + w3) -> (k,)"""
    rows = np.asarray(rows, np.int64)
    strips = int(rows.max()) // BLOCK + 1 if len(rows) else 0
    grid = np.zeros((t.shape[0], max(strips, 1), BLOCK), t.dtype)
    grid[:, rows // BLOCK, rows % BLOCK] = t
    acc = np.zeros((t.shape[0], BLOCK), t.dtype)
    for s in range(strips):                                   # one addition per strip; 0.0 for a row that is not kept changes nothing
        acc = acc + grid[:, s]
    acc = acc.reshape(t.shape[0], BLOCK // WAVE, WAVE)
    lane = np.arange(WAVE)
    off = WAVE // 2
    while off >= 1:
        acc = acc + acc[:, :, lane ^ off]
        off //= 2
    w = acc[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def evaluate(T, p, q, M, order="numpy", rows=None, dtype=np.float64):
    """the 28 sums at the pose T: H (ww 6, wv 9, vv 6), g (6), f.  p, q: (n, 3) f64; M: (n, 6), the kept rows only.  order "numpy":
    numpy.sum of every term; "device": the kernel's order, with rows = the kept rows' indices in the source cloud (all of
    0 .. n - 1 when None)"""
    t = terms(T, p, q, M, dtype)
    if order == "device":
        return device_sum(t, np.arange(t.shape[1]) if rows is None else rows)
    assert order == "numpy", order
    return np.array([np.sum(row) for row in t], dtype)


def solve(S, mu):
    """(H + mu diag H) delta = -g by Cholesky -> delta or None"""
    H = np.zeros((6, 6))
    for v, (r, c) in zip(S[:21], [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2), (0, 3), (0, 4), (0, 5), (1, 3), (1, 4), (1, 5), (2, 3),
                                  (2, 4), (2, 5), (3, 3), (3, 4), (3, 5), (4, 4), (4, 5), (5, 5)]):
        H[r, c] = v
    L = np.zeros((6, 6))
    ok = True
    with np.errstate(all="ignore"):
        for c in range(6):
            d = H[c, c] + mu * H[c, c]
            for k in range(c):
                d -= L[c, k] * L[c, k]
            if not d > 0.0:
                ok = False
            piv = np.sqrt(d)
            L[c, c] = piv
            for r in range(c + 1, 6):
                v = H[c, r]
                for k in range(c):
                    v -= L[r, k] * L[c, k]
                L[r, c] = v / piv
        yv = np.zeros(6)
        for r in range(6):
            v = 0.0 - S[21 + r]
            for k in range(r):
                v -= L[r, k] * yv[k]
            yv[r] = v / L[r, r]
        delta = np.zeros(6)
        for r in range(5, -1, -1):
            v = yv[r]
            for k in range(r + 1, 6):
                v -= L[k, r] * delta[k]
            delta[r] = v / L[r, r]
    return delta if ok and np.isfinite(delta).all() else None


def apply(T, delta):
    T = np.asarray(T, np.float64).reshape(3, 4)
    hx, hy, hz = delta[0] / 2.0, delta[1] / 2.0, delta[2] / 2.0
    nrm = math.sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz)
    qw, qx, qy, qz = 1.0 / nrm, hx / nrm, hy / nrm, hz / nrm
    D = np.array([[1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy)],
                  [2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx)],
                  [2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)]])
    Tn = np.zeros((3, 4))
    for r in range(3):
        for c in range(3):
            Tn[r, c] = (D[r, 0] * T[0, c] + D[r, 1] * T[1, c]) + D[r, 2] * T[2, c]
        Tn[r, 3] = T[r, 3] + delta[3 + r]
    return Tn


REFUSED, ACCEPTED, REJECTED = range(3)


def inner(T, p, q, M, cfg=DEFAULTS, log=None, order="numpy", rows=None):
    """step 7 from T -> the pose after the damped Gauss-Newton trials.  log: a list that receives one dict(mu, outcome, delta, f)
    per trial: mu as used, REFUSED (delta and f left zero) / ACCEPTED / REJECTED, the step and the trial pose's f"""
    S = evaluate(T, p, q, M, order, rows)
    mu = MU0
    for _ in range(cfg["inner_iterations"]):
        delta = solve(S, mu)
        if delta is None:
            if log is not None:
                log.append(dict(mu=mu, outcome=REFUSED, delta=np.zeros(6), f=0.0))
            mu = mu * 10.0
            continue
        Tn = apply(T, delta)
        Sn = evaluate(Tn, p, q, M, order, rows)
        if log is not None:
            log.append(dict(mu=mu, outcome=ACCEPTED if Sn[27] <= S[27] else REJECTED, delta=delta.copy(), f=float(Sn[27])))
        if Sn[27] <= S[27]:
            T, S = Tn, Sn
            mu = max(mu / 10.0, MU_MIN)
        else:
            mu = mu * 10.0
        if np.abs(delta).max() < INNER_EPS:
            break
    return T


def branches(log, cfg=DEFAULTS):
    """which ways through step 7's loop one trial log shows -> a set of "accepted", "rejected", "refused" (a Cholesky pivot that is
    not positive), "mu_floor" (an accepted trial whose mu / 10 lies below MU_MIN), "inner_eps" (stopped by a step below INNER_EPS),
    "ran_out" (stopped by inner_iterations)"""
    out = set()
    for e in log:
        out.add(("refused", "accepted", "rejected")[e["outcome"]])
        if e["outcome"] == ACCEPTED and e["mu"] / 10.0 < MU_MIN:
            out.add("mu_floor")
    if log:
        small = log[-1]["outcome"] != REFUSED and float(np.abs(log[-1]["delta"]).max()) < INNER_EPS
        assert small or len(log) == cfg["inner_iterations"], "a loop that stopped for no reason"
        out.add("inner_eps" if small else "ran_out")
    return out


def problem(src, tgt, G, T, cfg=DEFAULTS):
    """the inner problem of one outer iteration at T -> (p, q, M, num_corr)"""
    j, _, kept = correspondences(src, tgt, G, T, cfg)
    k = np.flatnonzero(kept)
    p = src["xyz"][k].astype(np.float64)
    q = move32(tgt["xyz"], G)[j[k]].astype(np.float64)
    M = mahalanobis(T, G, src["cov"][k], tgt["cov"][j[k]]) if len(k) else np.zeros((0, 6))
    return p, q, M, len(k)


# ------------------------------------------------------------------------------------------------ steps 8-10
def inv34(A):
    A = np.asarray(A, np.float64).reshape(3, 4)
    a, b, c, d, e, f, g, h, i = A[:, :3].reshape(9)
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = (a * c00 + b * c10) + c * c20
    R = np.array([[c00, c01, c02], [c10, c11, c12], [c20, c21, c22]]) / det
    B = np.zeros((3, 4))
    B[:, :3] = R
    for r in range(3):
        B[r, 3] = 0.0 - ((R[r, 0] * A[0, 3] + R[r, 1] * A[1, 3]) + R[r, 2] * A[2, 3])
    return B


def mul34(A, B):
    A, B = np.asarray(A, np.float64).reshape(3, 4), np.asarray(B, np.float64).reshape(3, 4)
    C = np.zeros((3, 4))
    for r in range(3):
        for c in range(4):
            C[r, c] = (A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]
        C[r, 3] += A[r, 3]
    return C


def converged(T, Tn, cfg=DEFAULTS):
    """step 8"""
    eps = np.array([[cfg["rotation_epsilon"]] * 3 + [cfg["transformation_epsilon"]]] * 3)
    return float((np.abs(np.asarray(T).reshape(3, 4) - np.asarray(Tn).reshape(3, 4)) / eps).max()) < 1.0


def step(src, tgt, G, T, cfg=DEFAULTS, order="device", j=None, kept=None):
    """one outer iteration (steps 6-8) at T with the state a fresh pair has, as the diagnostic hook uzl_debug_cloud_step returns it ->
    dict(M (n_from, 6) with zero rows where not kept, sums (28), T, status, done, num_corr, log).  src, tgt: dicts with xyz and cov
    (n, 6); j, kept: the correspondences to use instead of the restatement's own search"""
    G = np.asarray(G, np.float64).reshape(3, 4)
    T = np.asarray(T, np.float64).reshape(3, 4)
    if j is None:
        j, _, kept = correspondences(src, tgt, G, T, cfg)
    rows = np.flatnonzero(kept)
    M = np.zeros((len(src["xyz"]), 6))
    if len(rows) == 0:
        return dict(M=M, sums=np.zeros(28), T=T, status=NO_CORR, done=1, num_corr=0, log=[])
    p = src["xyz"][rows].astype(np.float64)
    q = move32(tgt["xyz"], G)[j[rows]].astype(np.float64)
    with np.errstate(all="ignore"):
        M[rows] = mahalanobis(T, G, src["cov"][rows], tgt["cov"][j[rows]])
        log = []
        Tn = inner(T, p, q, M[rows], cfg, log, order, rows)
        sums = evaluate(T, p, q, M[rows], order, rows)
    return dict(M=M, sums=sums, T=Tn, status=OK, done=int(converged(T, Tn, cfg) or cfg["max_iterations"] <= 1), num_corr=len(rows),
                log=log)


def finish(T, G, status, hist, n_from, n_to, cfg=DEFAULTS):
    """steps 9-10 from the final pose, the status and num_corr of every outer iteration taken"""
    G = np.asarray(G, np.float64).reshape(3, 4)
    T = np.asarray(T, np.float64).reshape(3, 4)
    its = len(hist) - (1 if status == NO_CORR else 0)
    out = dict(status=status, iterations=its, num_corr=hist[-1], num_corr_iter=hist, T=T, n_from=n_from, n_to=n_to,
               matching_score=0.0, information=np.zeros((6, 6)))
    Tf = T.astype(f32).astype(np.float64)
    X = mul34(inv34(Tf), G)
    out["transform"] = X
    out["match_score"] = hist[-1] / max(n_from, n_to)
    if status != OK:
        return out
    if not out["match_score"] > cfg["min_score"]:
        out["status"] = LOW_SCORE
        return out
    Tc = mul34(G, inv34(X))
    tn = math.sqrt((Tc[0, 3] * Tc[0, 3] + Tc[1, 3] * Tc[1, 3]) + Tc[2, 3] * Tc[2, 3])
    deg = abs(math.acos(min(1.0, max(-1.0, (((Tc[0, 0] + Tc[1, 1]) + Tc[2, 2]) - 1.0) / 2.0)))) * 180.0 / math.pi
    if not tn <= cfg["max_translation"] or not deg <= cfg["max_rotation_deg"]:
        out["status"] = TOO_FAR
        return out
    out["information"] = np.diag([1e4, 1e4, 1e4, 1e6, 1e6, 1e6])
    out["matching_score"] = 1.0
    return out


def estimate(src, tgt, G, cfg=DEFAULTS):
    """steps 5-10 -> dict(status, iterations, num_corr, num_corr_iter, T, transform, match_score, matching_score, information)"""
    G = np.asarray(G, np.float64).reshape(3, 4)
    T = np.eye(3, 4)
    status, hist = OK, []
    for it in range(cfg["max_iterations"]):
        p, q, M, cnt = problem(src, tgt, G, T, cfg)
        hist.append(cnt)
        if cnt == 0:
            status = NO_CORR
            break
        Tn = inner(T, p, q, M, cfg)
        stop = converged(T, Tn, cfg)
        T = Tn
        if stop:
            break
    return finish(T, G, status, hist, src["n"], tgt["n"], cfg)
