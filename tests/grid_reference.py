"""NumPy restatement of the occupancy-grid contract in include/uzl_mi355x.h ("Occupancy-grid map from the stored laser scans"),
written from the contract alone.  GridReference mirrors a uzl_grid handle: add_scans, build (steps 1-6), extend (steps 2-6 for the
nodes >= first_node).  Rays are walked in lock-step over all of them (state arrays, finished rays dropped), or one at a time by
the plain walker `bresenham` (walker="plain") for small cases; the two must agree."""
import functools
import math

import numpy as np

DEFAULTS = dict(resolution=0.1, range_max=5.0, occupancy_threshold=0.1, max_distance=10.0, known_free_radius=0.5, min_pass_through=1)


def trig_table(angle_min, angle_increment, n):
    """step 3: theta_i = (double)angle_min + (double)i * (double)angle_increment; cos / sin from the host's libm (math, not np)"""
    return _trig(float(np.float32(angle_min)), float(np.float32(angle_increment)), int(n))


@functools.lru_cache(maxsize=64)
def _trig(a, d, n):
    th = [a + float(i) * d for i in range(n)]
    return np.array([math.cos(t) for t in th], np.float64), np.array([math.sin(t) for t in th], np.float64)


def compose(P, D):
    """S = P * D (3x4 row-major), each 3-term sum as (a0 b0 + a1 b1) + a2 b2, P.t added last"""
    P = [float(v) for v in np.asarray(P, np.float64).reshape(12)]
    D = [float(v) for v in np.asarray(D, np.float64).reshape(12)]
    S = [0.0] * 12
    for i in range(3):
        for j in range(3):
            S[4 * i + j] = (P[4 * i] * D[j] + P[4 * i + 1] * D[4 + j]) + P[4 * i + 2] * D[8 + j]
        S[4 * i + 3] = ((P[4 * i] * D[3] + P[4 * i + 1] * D[7]) + P[4 * i + 2] * D[11]) + P[4 * i + 3]
    return S


def geometry(cfg, poses, present=None):
    """step 1 -> (origin_x, origin_y, width, height); None without a present node"""
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    idx = [i for i in range(len(P)) if present is None or present[i]]
    if not idx:
        return None
    xs = [float(P[i, 3]) for i in idx]
    ys = [float(P[i, 7]) for i in idx]
    minx, maxx, miny, maxy = min(xs), max(xs), min(ys), max(ys)
    rm, res = cfg["range_max"], cfg["resolution"]
    return minx - 5 * rm, miny - 5 * rm, int((maxx - minx + 10 * rm) / res), int((maxy - miny + 10 * rm) / res)


def cell(v, origin, res):
    return np.floor((np.asarray(v, np.float64) - origin) / res).astype(np.int64)


def bresenham_iter(x0, y0, x1, y1):
    """step 5, literally: the visited cells of one ray in walk order, both ends included (lazily: a ray of 2^24 cells can be cut short)"""
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err, x, y = dx + dy, x0, y0
    while True:
        yield (x, y)
        if x == x1 and y == y1:
            return
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy


def bresenham(x0, y0, x1, y1):
    """the visited cells of one ray as a list"""
    return list(bresenham_iter(x0, y0, x1, y1))


def beams(cfg, scan, S):
    """steps 3-4 for one scan at S -> (valid count, end points ex, ey in metres, hit flags) of its valid beams"""
    r = np.asarray(scan["ranges"], np.float32).astype(np.float64)
    c, s = trig_table(scan["angle_min"], scan["angle_increment"], len(r))
    valid = (float(np.float32(scan["range_min"])) <= r) & (r < cfg["range_max"])
    r, c, s = r[valid], c[valid], s[valid]
    px = (r * c).astype(np.float32).astype(np.float64)
    py = (r * s).astype(np.float32).astype(np.float64)
    qx = (S[0] * px + S[1] * py) + S[3]
    qy = (S[4] * px + S[5] * py) + S[7]
    md = cfg["max_distance"]
    hit = r <= md
    f = md / np.where(hit, 1.0, r)
    ex = np.where(hit, qx, S[3] + f * (qx - S[3]))
    ey = np.where(hit, qy, S[7] + f * (qy - S[7]))
    return int(valid.sum()), ex, ey, hit


def steps(x0, y0, x1, y1):
    """step 5 for many rays at once: yields (ray indices, x, y) of the cells visited at step 0, 1, 2, ... (finished rays dropped)"""
    x, y = np.array(x0, np.int64), np.array(y0, np.int64)
    x1, y1 = np.array(x1, np.int64), np.array(y1, np.int64)
    idx = np.arange(len(x))
    dx, dy = np.abs(x1 - x), -np.abs(y1 - y)
    sx, sy = np.where(x < x1, 1, -1), np.where(y < y1, 1, -1)
    err = dx + dy
    while len(x):
        yield idx, x, y
        act = ~((x == x1) & (y == y1))
        idx, x, y, x1, y1, dx, dy, sx, sy, err = (a[act] for a in (idx, x, y, x1, y1, dx, dy, sx, sy, err))
        e2 = 2 * err
        mx, my = e2 >= dy, e2 <= dx
        err = err + np.where(mx, dy, 0) + np.where(my, dx, 0)
        x = x + np.where(mx, sx, 0)
        y = y + np.where(my, sy, 0)


def walk_lockstep(x0, y0, x1, y1, W, H, passes):
    """step 5 for many rays at once: passes (flat, W*H) += 1 on every visited in-bounds cell"""
    buf, nbuf = [], 0
    for _, x, y in steps(x0, y0, x1, y1):
        inb = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        buf.append(y[inb] * W + x[inb])
        nbuf += int(inb.sum())
        if nbuf > 20_000_000:
            passes += np.bincount(np.concatenate(buf), minlength=W * H).astype(passes.dtype)
            buf, nbuf = [], 0
    if buf:
        passes += np.bincount(np.concatenate(buf), minlength=W * H).astype(passes.dtype)


class GridReference:
    def __init__(self, **cfg):
        self.cfg = dict(DEFAULTS, **cfg)
        self.gcfg = None
        self.scans = []
        self.geom = None
        self.hits = self.passes = None

    def add_scans(self, scans):
        first = len(self.scans)
        for s in scans:
            d = dict(s)
            d["ranges"] = np.asarray(s["ranges"], np.float32).copy()
            d["displacement"] = np.asarray(s.get("displacement", np.eye(3, 4)), np.float64).reshape(12)
            self.scans.append(d)
        return first

    def build(self, poses, present=None, walker="lockstep"):
        g = geometry(self.cfg, poses, present)
        assert g is not None, "no present node"
        self.gcfg, self.geom = dict(self.cfg), g
        W, H = g[2], g[3]
        self.hits = np.zeros(W * H, np.int64)
        self.passes = np.zeros(W * H, np.int64)
        return self._add(poses, present, 0, walker)

    def use_geometry(self, cfg, geom):
        """start from empty counts on a given geometry (what an extend onto an earlier build's grid is compared against)"""
        self.gcfg, self.geom = dict(cfg), tuple(geom)
        self.hits = np.zeros(geom[2] * geom[3], np.int64)
        self.passes = np.zeros(geom[2] * geom[3], np.int64)

    def extend(self, poses, first_node, present=None, walker="lockstep"):
        info = self._add(poses, present, first_node, walker)
        info["off_grid"] = self.off_grid(poses, present, first_node)
        return info

    def _adds(self, present, i, first, n):
        return first <= i < n and (present is None or present[i])

    def off_grid(self, poses, present, first):
        """the force-clear test of graph_grid_mapper.cpp:336-342"""
        P = np.asarray(poses, np.float64).reshape(-1, 12)
        ox, oy, W, H = self.geom
        rm, res = self.gcfg["range_max"], self.gcfg["resolution"]
        for i in range(len(P)):
            if not self._adds(present, i, first, len(P)):
                continue
            x, y = float(P[i, 3]), float(P[i, 7])
            if x < ox + rm or y < oy + rm or x > (ox + float(W) * res) - rm or y > (oy + float(H) * res) - rm:
                return 1
        return 0

    def _add(self, poses, present, first, walker):
        cfg = self.gcfg
        P = np.asarray(poses, np.float64).reshape(-1, 12)
        n = len(P)
        ox, oy, W, H = self.geom
        res = cfg["resolution"]
        # step 2: known-free squares of the added nodes, before any ray
        k = int(cfg["known_free_radius"] / res)
        mpt = cfg["min_pass_through"]
        if k >= 0 and mpt > 0:
            pas = self.passes.reshape(H, W)
            for i in range(n):
                if not self._adds(present, i, first, n):
                    continue
                cx, cy = int(cell(P[i, 3], ox, res)), int(cell(P[i, 7], oy, res))
                x0, x1, y0, y1 = max(cx - k, 0), min(cx + k, W - 1), max(cy - k, 0), min(cy + k, H - 1)
                if x0 <= x1 and y0 <= y1:
                    np.maximum(pas[y0:y1 + 1, x0:x1 + 1], mpt, out=pas[y0:y1 + 1, x0:x1 + 1])
        # steps 3-5
        valid = hits_added = n_scans = 0
        X0, Y0, X1, Y1 = [], [], [], []
        for s in self.scans:
            if not self._adds(present, s["node"], first, n):
                continue
            n_scans += 1
            S = compose(P[s["node"]], s["displacement"])
            v, ex, ey, hit = beams(cfg, s, S)
            valid += v
            ocx, ocy = int(cell(S[3], ox, res)), int(cell(S[7], oy, res))
            cx, cy = cell(ex, ox, res), cell(ey, oy, res)
            X0.append(np.full(len(cx), ocx, np.int64)); Y0.append(np.full(len(cx), ocy, np.int64)); X1.append(cx); Y1.append(cy)
            h = hit & (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
            np.add.at(self.hits, cy[h] * W + cx[h], 1)
            hits_added += int(h.sum())
        if X0:
            x0, y0, x1, y1 = (np.concatenate(a) for a in (X0, Y0, X1, Y1))
            if walker == "lockstep":
                walk_lockstep(x0, y0, x1, y1, W, H, self.passes)
            else:
                for a, b, c, d in zip(x0.tolist(), y0.tolist(), x1.tolist(), y1.tolist()):
                    for x, y in bresenham(a, b, c, d):
                        if 0 <= x < W and 0 <= y < H:
                            self.passes[y * W + x] += 1
        return dict(origin_x=ox, origin_y=oy, resolution=res, width=W, height=H, valid_beams=valid, hits=hits_added, scans=n_scans,
                    off_grid=0)

    def counts(self):
        W, H = self.geom[2], self.geom[3]
        return self.hits.astype(np.uint32).reshape(H, W), self.passes.astype(np.uint32).reshape(H, W)

    def grid(self):
        """step 6"""
        h, p = self.hits, self.passes
        thr = self.gcfg["occupancy_threshold"]
        out = np.where(p < self.gcfg["min_pass_through"], -1,
                       np.where(h.astype(np.float64) > thr * p.astype(np.float64), 100, 0)).astype(np.int8)
        return out.reshape(self.geom[3], self.geom[2])
