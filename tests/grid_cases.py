"""Planted inputs for the occupancy-grid projection (uzl_grid_*) at what its ray-cast room scenes never reach: rays longer than a
128-cell tile (by non-unit rotation rows and by resolution < range_max / 128), single rays directed at a tile corner, grids of 1,
127, 128, 129 and 257 cells, long and ragged beam lists in one tile, known-free squares over several tiles, the range and
classification thresholds, and extends that add nothing, a square only, or rays through tiles the build never touched.
Plain NumPy, fixed seeds.  tests/test_grid_cases_reference.py shows on the restatement alone (grid_reference.py) that every case
reaches what it is named after; tests/test_grid_tiles_gpu.py runs them on the device; tests/test_grid_plan_cpu.py holds the host
binning over them.

A case is a dict: name, cfg (over grid_reference.DEFAULTS), poses [n, 12], present (or None), scans (dicts as Grid.add_scans takes
them), build = the number of leading poses of the full build, extends = [(number of leading poses, first_node), ...] applied after it,
and for the directed rays `cells` = the cells the one ray visits, stated by hand (None: from grid_reference.bresenham)."""
import math

import numpy as np

import grid_reference as GR

TILE = 128
F32 = np.float32


def pose(x, y, yaw=0.0):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([c, -s, 0, x, s, c, 0, y, 0, 0, 1, 0], np.float64)


def disp(A=((1, 0), (0, 1)), t=(0, 0)):
    """displacement with the planar linear part A (not necessarily a rotation) and translation t"""
    return np.array([A[0][0], A[0][1], 0, t[0], A[1][0], A[1][1], 0, t[1], 0, 0, 1, 0], np.float64)


def fan(node, ranges, D=None, range_min=0.1, angle_min=-math.pi, inc=None):
    r = np.asarray(ranges, np.float32)
    inc = 2 * math.pi / max(len(r), 1) if inc is None else inc
    return dict(node=node, ranges=r, angle_min=F32(angle_min), angle_increment=F32(inc), range_min=F32(range_min),
                displacement=disp() if D is None else np.asarray(D, np.float64).reshape(12))


def case(name, cfg, poses, scans, present=None, build=None, extends=(), cells=None):
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 12))
    scans = [dict(s, displacement=np.asarray(s.get("displacement", disp()), np.float64).reshape(12)) for s in scans]
    return dict(name=name, cfg=dict(cfg), poses=P, present=None if present is None else np.asarray(present, np.uint8), scans=list(scans),
                build=len(P) if build is None else build, extends=list(extends), cells=cells)


def full_cfg(c):
    return dict(GR.DEFAULTS, **c["cfg"])


def pres(c, n):
    return None if c["present"] is None else c["present"][:n]


# ------------------------------------------------------------------------------------------------ what a case's rays do
def rays(c, n_poses=None, first=0, geom=None):
    """(x0, y0, x1, y1, hit) int64 / bool arrays: cell(o) and cell(e) of every valid beam of the scans a build of the first n_poses
    poses (or an extend from `first` on the geometry geom) projects, by the reference's steps 3-4"""
    cfg = full_cfg(c)
    n = c["build"] if n_poses is None else n_poses
    P, pr = c["poses"][:n], pres(c, n)
    ox, oy, W, H = GR.geometry(cfg, P, pr) if geom is None else geom
    out = [[], [], [], [], []]
    for s in c["scans"]:
        i = s["node"]
        if not (first <= i < n and (pr is None or pr[i])):
            continue
        S = GR.compose(P[i], s["displacement"])
        _, ex, ey, hit = GR.beams(cfg, s, S)
        cx, cy = GR.cell(ex, ox, cfg["resolution"]), GR.cell(ey, oy, cfg["resolution"])
        out[0].append(np.full(len(cx), int(GR.cell(S[3], ox, cfg["resolution"])), np.int64))
        out[1].append(np.full(len(cx), int(GR.cell(S[7], oy, cfg["resolution"])), np.int64))
        out[2].append(cx); out[3].append(cy); out[4].append(hit)
    if not out[0]:
        return tuple(np.zeros(0, np.int64) for _ in range(4)) + (np.zeros(0, bool),)
    return tuple(np.concatenate(a) for a in out)


def tile_visits(x0, y0, x1, y1, W, H):
    """the tiles one ray visits with an in-bounds cell, in walk order, by the plain walker"""
    seen = []
    for x, y in GR.bresenham(x0, y0, x1, y1):
        if 0 <= x < W and 0 <= y < H:
            t = (x // TILE, y // TILE)
            if t not in seen:
                seen.append(t)
    return seen


# ------------------------------------------------------------------------------------------------ long rays
LONG_POSES = [pose(0, 0), pose(1.35, 1.15, 0.3)]          # default config: 513 x 511 cells at (-25, -25), 5 x 4 tiles, last column 1 wide
SHEAR = ((6, 2), (-1, 7.5))


def _ranges(rng, n, lo, hi):
    return rng.uniform(lo, hi, n).astype(np.float32)


def long_fans(node_a=0, node_b=1, seed=41):
    """three 720-beam fans whose displacements are no rotations: 9 I inside the grid, 9 I from 30 m left of it, a shear"""
    rng = np.random.default_rng(seed)
    return [fan(node_a, _ranges(rng, 720, 0.2, 4.99), disp(((9, 0), (0, 9)), (0.5, -0.3))),
            fan(node_a, _ranges(rng, 720, 0.2, 4.99), disp(((9, 0), (0, 9)), (-30.0, 0.2))),
            fan(node_b, _ranges(rng, 720, 0.2, 4.99), disp(SHEAR, (-0.4, 0.6)))]


def long_ray_cases():
    out = [case("long_scaled", {}, LONG_POSES, long_fans())]
    rng = np.random.default_rng(42)
    P = [pose(0, 0), pose(0.4, 0.25, 1.0)]
    out.append(case("long_fine", dict(resolution=0.01, range_max=3.0), P,
                    [fan(0, _ranges(rng, 720, 0.2, 2.99)), fan(1, _ranges(rng, 720, 0.2, 2.99), disp(t=(0.05, -0.02)))]))
    return out


# ------------------------------------------------------------------------------------------------ directed single rays
# resolution 1, range_max 30, one node at (0, 0): 300 x 300 cells at (-150, -150), 3 x 3 tiles (128, 128, 44); no known-free square,
# so the passes of a case are its one ray.  The beam is r = 1 at angle 0 (cos = 1, sin = 0 exactly), the displacement's first
# column carries the ray in cells and its translation puts the sensor on a cell centre: every operand is exact.
DIRECTED_CFG = dict(resolution=1.0, range_max=30.0, known_free_radius=-1.0, max_distance=10.0)


def directed(name, a, b, cells=None):
    (x0, y0), (x1, y1) = a, b
    D = disp(((x1 - x0, 0), (y1 - y0, 0)), (-150 + x0 + 0.5, -150 + y0 + 0.5))
    s = dict(node=0, ranges=np.array([1.0], np.float32), angle_min=F32(0), angle_increment=F32(0), range_min=F32(0.1), displacement=D)
    c = case(name, DIRECTED_CFG, [pose(0, 0)], [s], cells=cells)
    c["ray"] = (x0, y0, x1, y1)
    return c


def directed_cases():
    out = []
    corner = [(127, 127), (128, 127), (127, 128), (128, 128)]
    for cx, cy in corner:                                                       # from the diagonally opposite tile
        far = (cx + (13 if cx == 127 else -13), cy + (23 if cy == 127 else -23))
        out.append(directed(f"end_on_{cx}_{cy}", far, (cx, cy)))
        out.append(directed(f"start_on_{cx}_{cy}", (cx, cy), far))
    out.append(directed("along_last_row", (5, 127), (290, 127), [(x, 127) for x in range(5, 291)]))
    out.append(directed("along_first_row", (290, 128), (5, 128), [(x, 128) for x in range(290, 4, -1)]))
    out.append(directed("along_last_column", (127, 5), (127, 290), [(127, y) for y in range(5, 291)]))
    out.append(directed("along_first_column", (128, 290), (128, 5), [(128, y) for y in range(290, 4, -1)]))
    out.append(directed("diagonal_pp", (100, 100), (155, 155), [(100 + k, 100 + k) for k in range(56)]))
    out.append(directed("diagonal_mm", (155, 155), (100, 100), [(155 - k, 155 - k) for k in range(56)]))
    out.append(directed("diagonal_pm", (100, 155), (155, 100), [(100 + k, 155 - k) for k in range(56)]))
    out.append(directed("diagonal_mp", (155, 100), (100, 155), [(155 - k, 100 + k) for k in range(56)]))
    # slopes 1:2 and 2:1 (a tie of the error term every other step) through the corner, one per octant
    for sx in (1, -1):
        for sy in (1, -1):
            mx, my = (127 if sx > 0 else 128), (127 if sy > 0 else 128)       # the corner cell the ray leaves its first tile from
            out.append(directed(f"slope_1_2_{'p' if sx > 0 else 'm'}{'p' if sy > 0 else 'm'}", (mx - 20 * sx, my - 10 * sy), (mx + 22 * sx, my + 11 * sy)))
            out.append(directed(f"slope_2_1_{'p' if sx > 0 else 'm'}{'p' if sy > 0 else 'm'}", (mx - 10 * sx, my - 20 * sy), (mx + 11 * sx, my + 22 * sy)))
    out.append(directed("zero_length_on_corner", (128, 127), (128, 127), [(128, 127)]))
    out.append(directed("all_outside", (-20, -5), (-3, -40), []))
    out.append(directed("outside_to_outside", (-10, 270), (40, 320)))           # through the partial corner tile (0, 2)
    return out


# ------------------------------------------------------------------------------------------------ grid sizes
SIZES = [(1, 1), (1, 129), (127, 1), (127, 127), (128, 128), (129, 129), (257, 127), (128, 257), (257, 257)]


def size_case(W, H, resolution=1.0, seed=0):
    """two nodes and range_max 0.1 give exactly W x H cells; a 360-beam fan from the grid's centre, every other beam scaled to leave the grid"""
    rm = 0.1
    dx, dy = (W + 0.5) * resolution - 10 * rm, (H + 0.5) * resolution - 10 * rm
    rng = np.random.default_rng(100 + seed)
    k = 12.0 * max(W, H) * resolution
    D = disp(((k, 0), (0, k)), (dx / 2 + 0.013, dy / 2 - 0.021))
    r = _ranges(rng, 360, 0.01, 0.06)                                           # odd beams end within 0.72 of the longer side ...
    r[::2] = _ranges(rng, 180, 0.06, 0.0999)                                    # ... even ones (the four axis directions too) beyond it
    return case(f"size_{W}x{H}" + ("" if resolution == 1.0 else "_half"), dict(resolution=resolution, range_max=rm), [pose(0, 0), pose(dx, dy)],
                [fan(0, r, D, range_min=0.01)])


def size_cases():
    return [size_case(W, H, seed=i) for i, (W, H) in enumerate(SIZES)] + [size_case(129, 257, 0.5, seed=20)]


# ------------------------------------------------------------------------------------------------ beam lists in one tile
ONE_TILE = dict(range_max=1.0)                                                  # one node: 100 x 100 cells, one tile


def beam_list_cases():
    rng = np.random.default_rng(7)
    many = []
    for i in range(3000):                                                       # 64 distinct (cos, sin) tables
        many.append(dict(node=0, ranges=_ranges(rng, 1, 0.05, 1.1), angle_min=F32(0.1 * (i % 64)), angle_increment=F32(0.01), range_min=F32(0.1),
                         displacement=disp(t=(0.01 * (i % 7), -0.01 * (i % 5)))))
    out = [case("beams_3000_scans_of_one", ONE_TILE, [pose(0, 0)], many)]
    mixed = []
    for n in (1, 0, 2, 1023, 0, 0, 1024, 1025, 0, 4097, 1):
        mixed.append(fan(0, _ranges(rng, n, 0.05, 1.1)))
    bad = np.array([np.nan, np.inf, -np.inf, 1.0, 2.0, 0.0999, -1.0, 0.0] * 16, np.float32)    # not one valid beam (range_max is 1.0)
    mixed.insert(5, fan(0, bad))
    mixed.append(fan(0, bad[:1]))
    out.append(case("beams_ragged_scans", ONE_TILE, [pose(0, 0)], mixed))
    return out


# ------------------------------------------------------------------------------------------------ known free
def known_free_cases():
    rng = np.random.default_rng(8)
    three = [pose(0, 0), pose(41, 41), pose(20.5, 20.5, 0.7)]                   # range_max 1: 510 x 510 cells, nodes at cells 50, 460, 255
    fans3 = [fan(i, _ranges(rng, 90, 0.05, 1.1)) for i in range(3)]
    out = [case("known_free_20m", dict(range_max=1.0, known_free_radius=20.0), three, fans3)]
    near = [pose(0, 0), pose(0.3, 0.2, 0.5), pose(0.1, 0.4, -1.0)]
    fansn = [fan(i, _ranges(rng, 180, 0.05, 1.1)) for i in range(3)]
    for name, extra in (("known_free_zero", dict(known_free_radius=0.0)), ("known_free_negative", dict(known_free_radius=-0.25)),
                        ("known_free_small_negative", dict(known_free_radius=-0.05)),   # (int)(-0.5) = 0: truncation, so one cell
                        ("known_free_under_one_cell", dict(known_free_radius=0.0999)),
                        ("known_free_truncates", dict(known_free_radius=0.3)),     # 0.3 / 0.1 = 2.9999999999999996 -> k = 2
                        ("min_pass_through_0", dict(min_pass_through=0)), ("min_pass_through_3", dict(min_pass_through=3)),
                        ("min_pass_through_1000", dict(min_pass_through=1000)),
                        ("known_free_overlap", dict(known_free_radius=0.5, min_pass_through=4))):
        out.append(case(name, dict(ONE_TILE, **extra), near, fansn))
    return out


# ------------------------------------------------------------------------------------------------ thresholds
THRESHOLD_CFG = dict(range_max=5.0, max_distance=3.0)
RANGE_MIN = F32(0.5)
UP, DOWN = F32(np.inf), F32(0)
# name -> (range, valid, hit)
THRESHOLD_RANGES = {
    "below_range_min": (np.nextafter(RANGE_MIN, DOWN), 0, 0), "at_range_min": (RANGE_MIN, 1, 1), "above_range_min": (np.nextafter(RANGE_MIN, UP), 1, 1),
    "below_range_max": (np.nextafter(F32(5.0), DOWN), 1, 0), "at_range_max": (F32(5.0), 0, 0),
    "below_max_distance": (np.nextafter(F32(3.0), DOWN), 1, 1), "at_max_distance": (F32(3.0), 1, 1),
    "above_max_distance": (np.nextafter(F32(3.0), UP), 1, 0),
}
THRESHOLD_ANGLE = 0.3


def threshold_cases():
    out = []
    for name, (r, _, _) in THRESHOLD_RANGES.items():
        s = dict(node=0, ranges=np.array([r], np.float32), angle_min=F32(THRESHOLD_ANGLE), angle_increment=F32(0.01), range_min=RANGE_MIN)
        out.append(case("range_" + name, THRESHOLD_CFG, [pose(0, 0)], [s]))
    return out


# classification ties: `h` identical one-beam scans end on cell (260, 250) and p - h longer ones pass through it; no known-free square.
# name -> (hits, passes, occupancy_threshold, the int8 value of that cell stated by hand)
TIES = {"tie_1_of_10": (1, 10, 0.1, 0),       # 1 > 0.1 * 10 = 1.0 is false
        "tie_1_of_9": (1, 9, 0.1, 100),       # 1 > 0.9
        "tie_2_of_10": (2, 10, 0.1, 100),
        "tie_1_of_2_at_half": (1, 2, 0.5, 0),  # 1 > 1.0 is false
        "threshold_zero": (1, 4, 0.0, 100),   # and every passed cell without a hit: 0 > 0 is false -> 0
        "threshold_one": (3, 3, 1.0, 0),      # hits never exceed passes
        "threshold_above_one": (3, 3, 1.5, 0)}
TIE_CELL = (260, 250)


def tie_cases():
    out = []
    for name, (h, p, thr, _) in TIES.items():
        scans = [dict(node=0, ranges=np.array([1.05 if i < h else 2.05], np.float32), angle_min=F32(0), angle_increment=F32(0), range_min=F32(0.1))
                 for i in range(p)]
        out.append(case(name, dict(occupancy_threshold=thr, known_free_radius=-1.0), [pose(0, 0)], scans))
    return out


# ------------------------------------------------------------------------------------------------ extend
# the long-ray grid: the build holds nodes 0 and 1 (513 x 511 cells), node 0 with a plain fan only; node 2 carries the long fans,
# node 3 no scan at all and lies within range_max of the border (off_grid = 1)
EXTEND_POSES = LONG_POSES + [pose(0.7, 0.5, 0.3), pose(-21.0, 18.0)]


def extend_scans():
    rng = np.random.default_rng(9)
    return [fan(0, _ranges(rng, 360, 0.2, 4.99))] + long_fans(2, 2, seed=43)


def extend_cases():
    sc = extend_scans()
    return [case("extend_through_empty_tiles", {}, EXTEND_POSES[:3], sc, build=2, extends=[(3, 2)]),
            case("extend_nothing", {}, EXTEND_POSES[:3], sc, build=3, extends=[(3, 3)]),
            case("extend_known_free_only", {}, EXTEND_POSES, sc, build=3, extends=[(4, 3)]),
            # no known-free squares here: step 2's max rule makes a square laid over earlier rays differ from one laid before them,
            # so only without squares do two extends equal one projection of everything
            case("extend_twice", dict(known_free_radius=-1.0), EXTEND_POSES, sc + [fan(3, _ranges(np.random.default_rng(10), 360, 0.2, 4.99))],
                 build=2, extends=[(3, 2), (4, 3)])]


# ------------------------------------------------------------------------------------------------ the range square at its edge
# A ray that ends beyond o + |row| * R_eff, the bound plan() starts its box from: range_max lies just above the f32 value 2, so r = 2
# is valid, and the f32 roundings of p = ((float)(r c), (float)(r s)) push |p| above range_max.  The rotation's first row points
# along the beam and the sensor sits so that o.x + |row| * R_eff falls 1e-7 m short of the tile boundary at cell 128: the end cell is
# the first of the next tile column, which only the box's slack reaches.
TIGHT_RANGE_MAX = 2.0 + 1e-9
TIGHT_SCALE = 3.0


def tight(theta):
    """(excess of the ray's x extent over |row| * R_eff, the case) for a beam at angle theta (an f32 value)"""
    th = float(F32(theta))
    c, s = math.cos(th), math.sin(th)
    px, py = float(F32(2.0 * c)), float(F32(2.0 * s))
    r00, r01 = TIGHT_SCALE * c, TIGHT_SCALE * s
    reach = r00 * px + r01 * py
    bx = math.sqrt(r00 * r00 + r01 * r01) * TIGHT_RANGE_MAX
    ox = -5 * TIGHT_RANGE_MAX
    tx = (ox + 12.8) - bx - (reach - bx) / 2
    sc = dict(node=0, ranges=np.array([2.0], np.float32), angle_min=F32(theta), angle_increment=F32(0), range_min=F32(0.1),
              displacement=disp(((r00, r01), (-r01, r00)), (tx, 0.3)))
    return reach - bx, case("box_edge_%d" % round(100 * theta), dict(range_max=TIGHT_RANGE_MAX), [pose(0, 0)], [sc])


def box_cases():
    """the two beam angles of 0.05, 0.10, ... 1.50 whose roundings overshoot the bound the most"""
    best = sorted((tight(0.05 * k) for k in range(1, 31)), key=lambda t: -t[0])
    return [c for _, c in best[:2]]


CLASSES = dict(long=long_ray_cases, directed=directed_cases, size=size_cases, beams=beam_list_cases, known_free=known_free_cases,
               threshold=threshold_cases, tie=tie_cases, extend=extend_cases, box=box_cases)


def all_cases():
    return [c for f in CLASSES.values() for c in f()]


class Stage:
    """what the restatement holds after one stage of a case (read-only copies; counts() and grid() as a GridReference has them)"""

    def __init__(self, r, info):
        h, p = r.counts()
        self.hits, self.passes, self.cells = h.copy(), p.copy(), r.grid().copy()
        for a in (self.hits, self.passes, self.cells):
            a.setflags(write=False)
        self.info, self.geom = dict(info), r.geom

    def counts(self):
        return self.hits, self.passes

    def grid(self):
        return self.cells


_REFERENCE = {}


def reference(c, walker="lockstep"):
    """the case on the restatement, computed once per case and walker -> [Stage after the build, Stage after each extend, ...]"""
    key = (c["name"], walker)
    if key not in _REFERENCE:
        r = GR.GridReference(**c["cfg"])
        r.add_scans(c["scans"])
        out = [Stage(r, r.build(c["poses"][:c["build"]], pres(c, c["build"]), walker=walker))]
        for n, first in c["extends"]:
            out.append(Stage(r, r.extend(c["poses"][:n], first, pres(c, n), walker=walker)))
        _REFERENCE[key] = out
    return _REFERENCE[key]
