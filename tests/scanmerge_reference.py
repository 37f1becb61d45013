"""NumPy restatement of the scan-merge contract in include/uzl_mi355x.h ("Node merging: the two nodes' laser scans"), written from
the contract alone: every f32 / f64 cast explicit, the bin of a point by the definition of the laser line's step 6
(laserline_reference.bins: all n + 1 boundaries tested), a's lists by "the last beam of a bin wins" and b's by grouping the points
of a bin and folding each group in beam order - no sort key, no LDS, nothing shared with the kernel.  `merge` mirrors one pair of
uzl_scanmerge_run.  `reference_loops` is a literal loop-by-loop transcription of graph_grid_mapper.cpp:45-133 over points and bin
indices handed to it, for the tests that hold the restatement's fold against the reference's."""
import math

import numpy as np

import laserline_reference as LR

F32, F64 = np.float32, np.float64
KEEP_RANGES, KEEP_INTENSITIES, DROP_RANGES, DROP_INTENSITIES = range(4)


def compose(A, B):
    """step 1: A * B of two 3 x 4 transforms, each 3-term sum as (a0 b0 + a1 b1) + a2 b2, A's translation added last"""
    A, B = np.asarray(A, F64).reshape(3, 4), np.asarray(B, F64).reshape(3, 4)
    out = np.empty((3, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
        out[i, 3] = ((A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3]) + A[i, 2] * B[2, 3]) + A[i, 3]
    return out


def scan(ranges, intensities, angle_min, angle_increment, range_min, range_max, displacement=None, stamp_ns=0):
    r, it = np.asarray(ranges, F32).reshape(-1), np.asarray(intensities, F32).reshape(-1)
    assert len(r) == len(it)
    return dict(ranges=r, intensities=it, angle_min=F32(angle_min), angle_increment=F32(angle_increment), range_min=F32(range_min),
                range_max=F32(range_max), displacement=np.eye(3, 4) if displacement is None else np.asarray(displacement, F64).reshape(3, 4),
                stamp_ns=int(stamp_ns))


def projected(S, values, D):
    """step 2 for one list -> (used, qx, qy): float32 per beam (qx, qy meaningless where not used)"""
    r = np.asarray(values, F32)
    n = len(r)
    with np.errstate(invalid="ignore"):
        used = ~np.isnan(r) & (r >= S["range_min"]) & (r <= S["range_max"])
    c, s = LR.trig_table(S["angle_min"], S["angle_increment"], n)
    D = np.asarray(D, F64).reshape(3, 4).astype(F32)
    with np.errstate(all="ignore"):
        x = (c[:n] * r.astype(F64)).astype(F32)
        y = (s[:n] * r.astype(F64)).astype(F32)
        qx = (D[0, 0] * x + D[0, 1] * y) + D[0, 3]
        qy = (D[1, 0] * x + D[1, 1] * y) + D[1, 3]
    assert qx.dtype == F32 and qy.dtype == F32
    return used, qx, qy


def points(S, values, D, a):
    """steps 2-3 for one list against a's grid -> (bin int64, -1 = unused or dropped; rho float32, 0 where bin = -1)"""
    used, qx, qy = projected(S, values, D)
    ca, sa = LR.trig_table(a["angle_min"], a["angle_increment"], len(a["ranges"]))
    b = np.full(len(qx), -1, np.int64)
    b[used] = LR.bins(qx[used], qy[used], ca, sa)
    with np.errstate(all="ignore"):
        rho = np.sqrt(qx * qx + qy * qy)
    assert rho.dtype == F32
    return b, np.where(b >= 0, rho, F32(0)).astype(F32)


def fold(cur, rho, lo, hi0, upper, b_newer, trace=None):
    """step 6 for one point"""
    cur, rho = F32(cur), F32(rho)
    if np.isnan(cur) or cur < lo or (upper and cur > hi0):
        branch, new = "take", rho
    elif np.abs(cur - rho) < F32(0.1):
        branch, new = "mean", F32(0.5) * (cur + rho)
    elif b_newer:
        branch, new = "newer", rho
    else:
        branch, new = "keep", cur
    if trace is not None:
        trace.append((cur, rho, branch))
    return F32(new)


def merge(a, b, keep_displacement, drop_displacement, trace=None):
    """one pair -> dict(ranges, intensities: float32 (n_a,); center: float64 (3,); bin, rho: per list of KEEP_RANGES .. DROP_INTENSITIES).
    trace (a list) receives (cur, rho, branch) of every fold step, ranges first."""
    Da, Db = compose(keep_displacement, a["displacement"]), compose(drop_displacement, b["displacement"])
    na = len(a["ranges"])
    lo, hi0 = a["range_min"], a["range_max"]
    b_newer = b["stamp_ns"] > a["stamp_ns"]
    lists = [points(a, a["ranges"], Da, a), points(a, a["intensities"], Da, a), points(b, b["ranges"], Db, a), points(b, b["intensities"], Db, a)]
    out = []
    for arr in range(2):
        o = np.full(na, hi0 + F32(1.0) if arr == 0 else F32(0), F32)               # step 4
        ba, ra = lists[arr]
        live = ba >= 0
        o[ba[live]] = ra[live]                                                     # step 5: a repeated index keeps the last value
        bb, rb = lists[2 + arr]
        beams = np.flatnonzero(bb >= 0)
        order = beams[np.argsort(bb[beams], kind="stable")]                        # by bin, beams ascending inside a bin
        for k in np.unique(bb[beams]):
            cur = o[k]
            for i in order[bb[order] == k]:
                cur = fold(cur, rb[i], lo, hi0, arr == 0, b_newer, trace)
            o[k] = cur
        out.append(o)
    ca, sa = LR.trig_table(a["angle_min"], a["angle_increment"], na)
    return dict(ranges=out[0], intensities=out[1], center=LR.scan_center(out[0], ca, sa, lo, hi0),
                bin=[l[0] for l in lists], rho=[l[1] for l in lists])


def on_laserline_grid(S):
    """the scope: angle_min = (float)(-pi) and n the n of the laser line's step 1"""
    amin, _, inc, n = LR.angular_grid(S["angle_increment"])
    return S["angle_min"] == amin and n == len(S["ranges"]) and 8 <= n <= 4096


# ------------------------------------------------------------------------------------- the reference's own loops
def reference_loops(a_ranges_n, range_min, range_max, poi_a, int_a, poi_b, int_b, idx, b_newer):
    """graph_grid_mapper.cpp:53-130, loop by loop.  poi_a .. int_b: (x, y) float32 arrays of the used points in beam order;
    idx: for each list the index :67 / :81 / :94 / :117 computes for its points (handed in, so that the fold is held apart from
    the reference's atan2f) with -1 for a point its angle test skips.  -> (ranges, intensities)"""
    range_min, range_max = F32(range_min), F32(range_max)
    ranges, intensities = np.zeros(a_ranges_n, F32), np.zeros(a_ranges_n, F32)
    for i in range(a_ranges_n):
        ranges[i] = range_max + F32(1.0)
        intensities[i] = F32(0.0)
    for i in range(len(poi_a)):
        x, y = F32(poi_a[i][0]), F32(poi_a[i][1])
        index = idx[0][i]
        if index < 0:
            continue
        rng = np.sqrt(x * x + y * y)
        ranges[index] = rng
    for i in range(len(int_a)):
        x, y = F32(int_a[i][0]), F32(int_a[i][1])
        index = idx[1][i]
        if index < 0:
            continue
        rng = np.sqrt(x * x + y * y)
        intensities[index] = rng
    for i in range(len(poi_b)):
        x, y = F32(poi_b[i][0]), F32(poi_b[i][1])
        index = idx[2][i]
        if index < 0:
            continue
        rng = np.sqrt(x * x + y * y)
        if np.isnan(ranges[index]) or ranges[index] < range_min or ranges[index] > range_max:
            ranges[index] = rng
        else:
            if np.abs(ranges[index] - rng) < F32(0.1):
                ranges[index] = F32(0.5) * (ranges[index] + rng)
            elif b_newer:
                ranges[index] = rng
    for i in range(len(int_b)):
        x, y = F32(int_b[i][0]), F32(int_b[i][1])
        index = idx[3][i]
        if index < 0:
            continue
        rng = np.sqrt(x * x + y * y)
        if np.isnan(intensities[index]) or intensities[index] < range_min:
            intensities[index] = rng
        else:
            if np.abs(intensities[index] - rng) < F32(0.1):
                intensities[index] = F32(0.5) * (intensities[index] + rng)
            elif b_newer:
                intensities[index] = rng
    return ranges, intensities


def reference_index(qx, qy, amin, amax, inc):
    """:62-67: angle = -atan2f(-y, x); skipped (-1) for angle < angle_min or angle > angle_max; else (int)((angle - angle_min) / inc)"""
    qx, qy = np.asarray(qx, F32), np.asarray(qy, F32)
    angle = -np.arctan2(-qy, qx)
    assert angle.dtype == F32
    idx = ((angle - F32(amin)) / F32(inc)).astype(np.int64)
    return np.where((angle < F32(amin)) | (angle > F32(amax)), -1, idx)
