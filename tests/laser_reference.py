"""NumPy restatement of the laser scan matching contract (include/uzl_mi355x.h, "Laser scan matching", steps 1-10): f64, every
operation in the order the header writes it, no fused multiply-add (NumPy's ufuncs and Python floats round after every operation),
cos / sin / atan2 from the host's libm through `math`.  Steps 1-4 give the device's bits; from step 6 on the sums are NumPy's
(pairwise) instead of the kernel's strip / butterfly order, which is the only difference."""
import math

import numpy as np

F32 = np.float32
OK, FEW_CORR, VIEWPOINT, FEW_MATCHES, TOO_FAR, DEGENERATE = range(6)
DEFAULTS = dict(max_iterations=10, epsilon_xy=0.01, epsilon_theta=0.02, max_correspondence_dist=0.3, outliers_max_perc=0.80,
                outliers_adaptive_order=0.7, outliers_adaptive_mult=2.0, max_angular_correction_deg=45.0, max_linear_correction=1.5,
                min_valid_fraction=0.25, fail_fraction=0.05, goal_trace=10000.0, other_information=100.0)
BISECTIONS = 64


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def points(scan):
    """step 1 -> (points (n, 2) f64 with NaN rows for invalid beams, valid (n,) bool, readings (n,) f64)"""
    v = np.ascontiguousarray(scan["values"], F32).reshape(-1)
    amin, inc = float(F32(scan["angle_min"])), float(F32(scan["angle_increment"]))
    trig = np.array([(math.cos(amin + k * inc), math.sin(amin + k * inc)) for k in range(len(v))], np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        valid = (v >= F32(scan["range_min"])) & (v <= F32(scan["range_max"]))
    r = v.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([trig[:, 0] * r, trig[:, 1] * r], 1)
    p[~valid] = np.nan
    return p, valid, r


def guess_to_x(T):
    """x0 of a 3x4 first guess as the host takes it: (tx, ty, cos, sin) of theta0 = atan2(T[1][0], T[0][0])"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    th = math.atan2(T[1, 0], T[0, 0])
    return (float(T[0, 3]), float(T[1, 3]), math.cos(th), math.sin(th))


def moved(P, x):
    """step 2's w for points P (n, 2)"""
    tx, ty, c, s = x
    return np.stack([(c * P[:, 0] - s * P[:, 1]) + tx, (s * P[:, 0] + c * P[:, 1]) + ty], 1)


def normals(Q, j1, j2):
    """step 4's unit normal of the line (j1, j2)"""
    l = Q[j2] - Q[j1]
    length = np.sqrt(l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1])
    return np.stack([-l[:, 1] / length, l[:, 0] / length], 1)


def correspondences(F, T, x, cfg):
    """steps 2-4 at x = (tx, ty, c, s) -> j1, j2 (int32, -1: none), valid (int32), dist (f64; 0 where step 3 or 2 left nothing)"""
    Q, qv, _ = F if isinstance(F, tuple) else points(F)
    P, pv, _ = T if isinstance(T, tuple) else points(T)
    nt, nf = len(P), len(Q)
    j1 = np.full(nt, -1, np.int32); j2 = np.full(nt, -1, np.int32)
    valid = np.zeros(nt, np.int32); dist = np.zeros(nt, np.float64)
    d2min = np.full(nt, np.inf)
    idx = np.flatnonzero(pv)
    if len(idx) == 0 or not qv.any():
        return j1, j2, valid, dist
    W = np.full((nt, 2), np.nan)
    W[idx] = moved(P[idx], x)
    # step 2
    with np.errstate(invalid="ignore", over="ignore"):
        dx = W[idx, 0][:, None] - Q[None, :, 0]
        dy = W[idx, 1][:, None] - Q[None, :, 1]
        d2 = dx * dx + dy * dy
    d2[np.isnan(d2)] = np.inf
    bj = np.argmin(d2, 1)                                     # first occurrence: ties to the lowest index
    bd = d2[np.arange(len(idx)), bj]
    up_of = np.full(nf, -1); down_of = np.full(nf, -1)
    nxt = -1
    for j in range(nf - 1, -1, -1):
        up_of[j] = nxt
        if qv[j]:
            nxt = j
    prv = -1
    for j in range(nf):
        down_of[j] = prv
        if qv[j]:
            prv = j
    max_sq = cfg["max_correspondence_dist"] * cfg["max_correspondence_dist"]
    for a, i in enumerate(idx):
        if not bd[a] <= max_sq:
            continue
        b = int(bj[a]); up = int(up_of[b]); down = int(down_of[b])
        if up >= 0 and down >= 0:
            ux, uy = W[i, 0] - Q[up, 0], W[i, 1] - Q[up, 1]
            ex, ey = W[i, 0] - Q[down, 0], W[i, 1] - Q[down, 1]
            c2 = up if (ux * ux + uy * uy) <= (ex * ex + ey * ey) else down
        else:
            c2 = up if up >= 0 else down
        if c2 < 0:
            continue
        lx, ly = Q[c2, 0] - Q[b, 0], Q[c2, 1] - Q[b, 1]
        if not lx * lx + ly * ly > 0.0:
            continue
        j1[i] = b; j2[i] = c2; d2min[i] = bd[a]
    have = np.flatnonzero(j1 >= 0)
    if len(have) == 0:
        return j1, j2, valid, dist
    # step 3
    best = np.full(nf, np.inf)
    np.minimum.at(best, j1[have], d2min[have])
    left = have[~(best[j1[have]] < d2min[have])]
    # step 4
    n = normals(Q, j1[left], j2[left])
    d = np.abs(n[:, 0] * (W[left, 0] - Q[j1[left], 0]) + n[:, 1] * (W[left, 1] - Q[j1[left], 1]))
    dist[left] = d
    k = len(left)
    srt = np.sort(d)
    i1 = min(max(int(math.floor(k * cfg["outliers_max_perc"])), 0), k - 1)
    i2 = min(max(int(math.floor(k * cfg["outliers_adaptive_order"])), 0), k - 1)
    limit = min(srt[i1], cfg["outliers_adaptive_mult"] * srt[i2])
    valid[left[~(d > limit)]] = 1
    return j1, j2, valid, dist


def step_terms(F, T, j1, j2, valid):
    """step 6's a (k, 4), b (k,), w (k,) of the correspondences left, in beam order"""
    Q, _, _ = F
    P, _, r = T
    i = np.flatnonzero(valid)
    n = normals(Q, j1[i], j2[i])
    p, q = P[i], Q[j1[i]]
    a = np.stack([n[:, 0], n[:, 1], n[:, 0] * p[:, 0] + n[:, 1] * p[:, 1], n[:, 1] * p[:, 0] - n[:, 0] * p[:, 1]], 1)
    b = n[:, 0] * q[:, 0] + n[:, 1] * q[:, 1]
    w = 1.0 / (r[i] * r[i])
    return a, b, w


def sums(a, b, w):
    """step 6's M (4x4, symmetric), v (4), sum w b^2"""
    M = np.zeros((4, 4))
    for r in range(4):
        for c in range(r, 4):
            M[r, c] = M[c, r] = np.sum((w * a[:, r]) * a[:, c])
    v = np.array([np.sum((w * b) * a[:, c]) for c in range(4)])
    return M, v, float(np.sum((w * b) * b))


def solve(M, v):
    """step 6's closed form -> (tx, ty, c, s) or None when degenerate"""
    M = [[float(M[r][c]) for c in range(4)] for r in range(4)]
    v = [float(t) for t in v]
    det_a = M[0][0] * M[1][1] - M[0][1] * M[0][1]
    if not det_a > 0.0:
        return None
    E00 = (M[1][1] * M[0][2] - M[0][1] * M[1][2]) / det_a; E01 = (M[1][1] * M[0][3] - M[0][1] * M[1][3]) / det_a
    E10 = (M[0][0] * M[1][2] - M[0][1] * M[0][2]) / det_a; E11 = (M[0][0] * M[1][3] - M[0][1] * M[0][3]) / det_a
    f0 = (M[1][1] * v[0] - M[0][1] * v[1]) / det_a; f1 = (M[0][0] * v[1] - M[0][1] * v[0]) / det_a
    Q00 = M[2][2] - (M[0][2] * E00 + M[1][2] * E10); Q01 = M[2][3] - (M[0][2] * E01 + M[1][2] * E11)
    Q11 = M[3][3] - (M[0][3] * E01 + M[1][3] * E11)
    h0 = -2.0 * (v[2] - (M[0][2] * f0 + M[1][2] * f1)); h1 = -2.0 * (v[3] - (M[0][3] * f0 + M[1][3] * f1))
    dq = Q00 - Q11
    e_min = ((Q00 + Q11) - math.sqrt(dq * dq + 4.0 * (Q01 * Q01))) / 2.0
    hn = math.sqrt(h0 * h0 + h1 * h1)
    if not hn > 0.0 or not hn < 1.7e308 or e_min != e_min:
        return None
    lo = -e_min; hi = lo + hn
    for _ in range(BISECTIONS):
        mid = 0.5 * (lo + hi)
        p = Q00 + mid; q = Q11 + mid
        det = p * q - Q01 * Q01
        g0 = q * h0 - Q01 * h1; g1 = p * h1 - Q01 * h0
        if det * det - 0.25 * (g0 * g0 + g1 * g1) > 0.0:
            hi = mid
        else:
            lo = mid
    lam = 0.5 * (lo + hi)
    p = Q00 + lam; q = Q11 + lam
    det = p * q - Q01 * Q01
    g0 = q * h0 - Q01 * h1; g1 = p * h1 - Q01 * h0
    if det == 0.0:
        return None
    c = -g0 / (2.0 * det); s = -g1 / (2.0 * det)
    nrm = math.sqrt(c * c + s * s)
    if not nrm > 0.0 or not nrm < 1.7e308:
        return None
    c = c / nrm; s = s / nrm
    tx = f0 - (E00 * c + E01 * s); ty = f1 - (E10 * c + E11 * s)
    if tx != tx or ty != ty:
        return None
    return (tx, ty, c, s)


def cost(M, v, wbb, x):
    """sum w (a . x - b)^2 from the sums"""
    x = np.asarray(x, np.float64)
    return float(x @ M @ x - 2.0 * (v @ x) + wbb)


def deg_count(j1, valid):
    """step 8's walk"""
    last, deg = -1, 0
    for i in np.flatnonzero(valid):
        if j1[i] > last:
            deg += 1
        elif j1[i] < last:
            deg -= 1
        last = int(j1[i])
    return deg


def hessian(M, x):
    """step 9's inf3 before the rescale"""
    u0, u1 = -x[3], x[2]
    H = np.zeros((3, 3))
    H[0, 0] = M[0, 0]; H[0, 1] = H[1, 0] = M[0, 1]; H[1, 1] = M[1, 1]
    H[0, 2] = H[2, 0] = M[0, 2] * u0 + M[0, 3] * u1
    H[1, 2] = H[2, 1] = M[1, 2] * u0 + M[1, 3] * u1
    H[2, 2] = (M[2, 2] * (u0 * u0) + 2.0 * (M[2, 3] * (u0 * u1))) + M[3, 3] * (u1 * u1)
    return H


def information(H, cfg):
    """step 9 -> (inf3 scaled to goal_trace, the 6x6)"""
    inf3 = H * (cfg["goal_trace"] / ((H[0, 0] + H[1, 1]) + H[2, 2]))
    I = np.eye(6) * cfg["other_information"]
    I[0, 0] = inf3[0, 0]; I[0, 1] = inf3[0, 1]; I[1, 0] = inf3[1, 0]; I[1, 1] = inf3[1, 1]; I[5, 5] = inf3[2, 2]
    return inf3, I


def too_far(guess, x, cfg):
    """step 10"""
    g = guess_to_x(guess)
    dx, dy = x[0] - g[0], x[1] - g[1]
    angle_deg = abs(math.atan2(g[2] * x[3] - g[3] * x[2], g[2] * x[2] + g[3] * x[3])) * 180.0 / math.pi
    return 1.5 * math.sqrt(dx * dx + dy * dy) > cfg["max_linear_correction"] or 1.5 * angle_deg > cfg["max_angular_correction_deg"]


def estimate(scan_from, scan_to, guess, cfg=None):
    """steps 1-10 for one pair -> dict with the fields of uzl_laser_edge plus theta"""
    cfg = cfg or DEFAULTS
    F, T = points(scan_from), points(scan_to)
    nt = len(T[0])
    x = guess_to_x(guess)
    sin_eps = math.sin(min(cfg["epsilon_theta"], math.pi / 2))
    eps_sq = cfg["epsilon_xy"] * cfg["epsilon_xy"]
    status, iterations, left = OK, 0, 0
    while iterations < cfg["max_iterations"]:
        j1, j2, valid, dist = correspondences(F, T, x, cfg)
        left = int(valid.sum())
        if left == 0 or left < cfg["fail_fraction"] * nt:              # step 5
            status = FEW_CORR
            break
        M, v, wbb = sums(*step_terms(F, T, j1, j2, valid))
        y = solve(M, v)
        if y is None:
            status = DEGENERATE
            break
        iterations += 1
        dx, dy = y[0] - x[0], y[1] - x[1]                               # step 7
        cross, dot = x[2] * y[3] - x[3] * y[2], x[2] * y[2] + x[3] * y[3]
        converged = dx * dx + dy * dy < eps_sq and abs(cross) < sin_eps and dot > 0.0
        x = y
        if converged:
            break
    out = dict(status=status, nvalid=0, scan_valid=int(T[1].sum()), deg_count=0, iterations=iterations, matching_score=0.0, error=0.0,
               x=x, theta=math.atan2(x[3], x[2]), information=np.eye(6) * cfg["other_information"])
    out["transform"] = np.array([[x[2], -x[3], 0, x[0]], [x[3], x[2], 0, x[1]], [0, 0, 1, 0]], np.float64)
    if status != OK:
        return out
    out["nvalid"] = left
    out["deg_count"] = deg_count(j1, valid)
    i = np.flatnonzero(valid)                                           # step 8's error at the final estimate
    n, W = normals(F[0], j1[i], j2[i]), moved(T[0][i], x)
    e = n[:, 0] * (W[:, 0] - F[0][j1[i], 0]) + n[:, 1] * (W[:, 1] - F[0][j1[i], 1])
    out["error"] = float(np.sum(e * e))
    if out["deg_count"] <= 0:
        out["status"] = VIEWPOINT
        return out
    out["inf3"], out["information"] = information(hessian(M, x), cfg)
    if cfg["min_valid_fraction"] * out["scan_valid"] > left:
        out["status"] = FEW_MATCHES
    elif too_far(guess, x, cfg):
        out["status"] = TOO_FAR
    else:
        out["matching_score"] = float(left)
    return out
