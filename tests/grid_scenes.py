"""Synthetic laser scans for the occupancy-grid tests: a room (outer walls and boxes) around a make_pose_graph trajectory, each
node's scan ray-cast analytically in the plane from the sensor at pose * displacement.  Beams without a return within the scan's
range_max are range_max + 1, as extractImageLaserLine writes them (map_projection/src/graph_grid_mapper.cpp:420-468)."""
import math

import numpy as np

from uzliti_slam_amd import synth

DEPLOYED = dict(n_beams=720, angle_increment=math.pi / 360, range_max=6.0, resolution=0.05)   # iti_slam_launch slam.yaml


def room(poses, rng, n_boxes=12, margin=2.0):
    """wall segments (m, 2, 2): the bounding box of the trajectory grown by margin, and axis-aligned boxes inside it"""
    P = np.asarray(poses).reshape(-1, 12)
    x0, x1 = P[:, 3].min() - margin, P[:, 3].max() + margin
    y0, y1 = P[:, 7].min() - margin, P[:, 7].max() + margin
    segs = [((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1)), ((x0, y1), (x0, y0))]
    for _ in range(n_boxes):
        cx, cy = rng.uniform(x0, x1), rng.uniform(y0, y1)
        w, h = rng.uniform(0.2, 1.5, 2)
        a, b, c, d = (cx - w, cy - h), (cx + w, cy - h), (cx + w, cy + h), (cx - w, cy + h)
        segs += [(a, b), (b, c), (c, d), (d, a)]
    return np.array(segs, np.float64)


def cast(origins, yaw, angle_min, inc, n, segs, scan_range_max):
    """ranges (k, n) f32 from origins (k, 2) at headings yaw (k) against segs; no return -> scan_range_max + 1"""
    th = yaw[:, None] + (angle_min + inc * np.arange(n))[None, :]
    d = np.stack([np.cos(th), np.sin(th)], -1)                                   # (k, n, 2)
    a, b = segs[:, 0], segs[:, 1]
    e = b - a                                                                    # (m, 2)
    best = np.full(th.shape, np.inf)
    for j in range(len(segs)):
        w = a[j][None, :] - origins                                              # (k, 2)
        den = d[..., 0] * e[j, 1] - d[..., 1] * e[j, 0]                          # cross(d, e)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (w[:, None, 0] * e[j, 1] - w[:, None, 1] * e[j, 0]) / den       # along the beam
            u = (w[:, None, 0] * d[..., 1] - w[:, None, 1] * d[..., 0]) / den   # along the segment
        ok = (den != 0) & (t > 0) & (u >= 0) & (u <= 1)
        best = np.where(ok & (t < best), t, best)
    r = np.where(best <= scan_range_max, best, scan_range_max + 1.0)
    return r.astype(np.float32)


def scene(n_nodes, seed=0, n_beams=720, angle_increment=math.pi / 360, scan_range_max=6.0, displacement=None, chunk=256):
    """(poses (N, 12) = make_pose_graph's ground truth, scans: one per node) with the sensor at `displacement` (3x4, default 0.1 m
    ahead of the node)"""
    g = synth.make_pose_graph(n_nodes, n_nodes - 1, seed=seed)
    poses = np.ascontiguousarray(g["gt_pose"], np.float64).reshape(-1, 12)
    rng = np.random.default_rng(seed + 1000)
    segs = room(poses, rng)
    D = np.eye(3, 4) if displacement is None else np.asarray(displacement, np.float64).reshape(3, 4)
    if displacement is None:
        D[0, 3] = 0.1
    amin = -angle_increment * (n_beams // 2)
    scans = []
    for c0 in range(0, n_nodes, chunk):
        P = poses[c0:c0 + chunk].reshape(-1, 3, 4)
        S = P[:, :, :3] @ D[:, :3]
        o = (P[:, :, :3] @ D[:, 3] + P[:, :, 3])[:, :2]
        yaw = np.arctan2(S[:, 1, 0], S[:, 0, 0])
        R = cast(o, yaw, amin, angle_increment, n_beams, segs, scan_range_max)
        for i in range(len(P)):
            scans.append(dict(node=c0 + i, ranges=R[i], angle_min=np.float32(amin), angle_increment=np.float32(angle_increment),
                              range_min=np.float32(0.1), displacement=D.reshape(12).copy()))
    return poses, scans


def sprinkle(scans, rng, frac=0.02):
    """NaN, +inf and -inf into a fraction of every scan's beams, and exact range_min / range_max values"""
    for s in scans:
        r = s["ranges"].copy()
        k = max(1, int(frac * len(r)))
        idx = rng.choice(len(r), size=min(len(r), 3 * k), replace=False)
        r[idx[:k]] = np.nan
        r[idx[k:2 * k]] = np.inf
        r[idx[2 * k:3 * k]] = -np.inf
        s["ranges"] = r
    return scans
