"""CPU tests of the occupancy-grid restatement tests/grid_reference.py against hand-computed answers, one contract step at a time
(include/uzl_mi355x.h, "Occupancy-grid map from the stored laser scans"), and of its two ray walkers against each other."""
import math

import numpy as np
import pytest

import grid_reference as GR


def pose(x, y, yaw=0.0):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([c, -s, 0, x, s, c, 0, y, 0, 0, 1, 0], np.float64)


def one_beam(r, angle=0.0, node=0, range_min=0.0):
    return dict(node=node, ranges=np.array([r], np.float32), angle_min=np.float32(angle), angle_increment=np.float32(0.0),
                range_min=np.float32(range_min))


def test_walkers_agree_on_random_rays():
    rng = np.random.default_rng(0)
    x0, y0, x1, y1 = (rng.integers(-15, 40, 3000) for _ in range(4))
    W, H = 25, 20
    a = np.zeros(W * H, np.int64)
    GR.walk_lockstep(x0, y0, x1, y1, W, H, a)
    b = np.zeros(W * H, np.int64)
    for p, q, r, s in zip(x0.tolist(), y0.tolist(), x1.tolist(), y1.tolist()):
        for x, y in GR.bresenham(p, q, r, s):
            if 0 <= x < W and 0 <= y < H:
                b[y * W + x] += 1
    assert np.array_equal(a, b)


def test_walkers_agree_on_a_scene():
    rng = np.random.default_rng(1)
    poses = np.stack([pose(rng.uniform(0, 3), rng.uniform(0, 3), rng.uniform(-3, 3)) for _ in range(6)])
    scans = [dict(node=i, ranges=rng.uniform(0.0, 6.0, 90).astype(np.float32), angle_min=np.float32(-1.5),
                  angle_increment=np.float32(0.035), range_min=np.float32(0.2)) for i in range(6)]
    a, b = GR.GridReference(range_max=5.0), GR.GridReference(range_max=5.0)
    a.add_scans(scans); b.add_scans(scans)
    ia, ib = a.build(poses), b.build(poses, walker="plain")
    assert ia == ib
    assert all(np.array_equal(u, v) for u, v in zip(a.counts(), b.counts()))


@pytest.mark.parametrize("end,cells", [
    ((4, 0), [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)]),
    ((0, -3), [(0, 0), (0, -1), (0, -2), (0, -3)]),
    ((3, 3), [(0, 0), (1, 1), (2, 2), (3, 3)]),
    ((-3, 2), [(0, 0), (-1, 1), (-2, 1), (-3, 2)]),
    ((2, 5), [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]),
    ((0, 0), [(0, 0)]),
])
def test_bresenham_by_hand(end, cells):
    assert GR.bresenham(0, 0, *end) == cells


def test_all_octants():
    for dx, dy in [(5, 2), (2, 5), (7, 7), (6, 1), (1, 6), (0, 4), (4, 0)]:
        for sx in (1, -1):
            for sy in (1, -1):
                got = GR.bresenham(0, 0, sx * dx, sy * dy)
                assert len(got) == max(dx, dy) + 1 and got[0] == (0, 0) and got[-1] == (sx * dx, sy * dy)
                steps = np.diff(np.array(got), axis=0)
                major = 0 if dx >= dy else 1
                assert (np.abs(steps[:, major]) == 1).all() and (np.abs(steps[:, 1 - major]) <= 1).all()
                assert (steps[:, 0] * sx >= 0).all() and (steps[:, 1] * sy >= 0).all()


def _single(r, cfg=None, angle=0.0, range_min=0.0, at=(0.0, 0.0)):
    g = GR.GridReference(**dict(dict(resolution=1.0, range_max=5.0, known_free_radius=-1.0), **(cfg or {})))
    g.add_scans([one_beam(r, angle, range_min=range_min)])
    info = g.build(pose(*at)[None])
    return g, info


def test_one_beam_along_x():
    g, info = _single(3.5)
    # origin (-25, -25), 50 x 50 cells; o = (0, 0) -> cell (25, 25); e = (3.5, 0) -> cell (28, 25)
    assert (info["origin_x"], info["origin_y"], info["width"], info["height"]) == (-25.0, -25.0, 50, 50)
    h, p = g.counts()
    assert p[25, 25:29].tolist() == [1, 1, 1, 1] and p.sum() == 4
    assert h[25, 28] == 1 and h.sum() == 1 and info["hits"] == 1 and info["valid_beams"] == 1


def test_zero_length_ray_is_the_sensor_cell():
    g, info = _single(0.2)
    h, p = g.counts()
    assert p[25, 25] == 1 and p.sum() == 1 and h[25, 25] == 1


@pytest.mark.parametrize("r,valid", [(5.0, 0), (4.999, 1), (0.5, 1), (0.4999, 0), (float("nan"), 0), (float("inf"), 0),
                                     (float("-inf"), 0)])
def test_valid_range(r, valid):
    g, info = _single(r, range_min=0.5)
    assert info["valid_beams"] == valid
    assert g.counts()[1].sum() == (0 if not valid else int(math.floor(r)) + 1)


def test_max_distance_truncates_without_a_hit():
    g, info = _single(7.5, cfg=dict(range_max=10.0, max_distance=4.0))
    # e = o + (4 / 7.5) (q - o) = (4, 0): cells 0..4 passed, no hit
    h, p = g.counts()
    c = 50                                                                       # origin -50: cell(0) = 50
    assert p[c, c:c + 5].tolist() == [1] * 5 and p.sum() == 5
    assert h.sum() == 0 and info["hits"] == 0 and info["valid_beams"] == 1
    g, info = _single(4.0, cfg=dict(range_max=10.0, max_distance=4.0))          # r == max_distance still hits
    assert info["hits"] == 1


def test_known_free_square_overlap_and_edge():
    g = GR.GridReference(resolution=1.0, range_max=1.0, known_free_radius=1.9, min_pass_through=3)
    # nodes at (0,0), (1,0) and (0,5): origin (-5, -5), width 11, height 15; k = 1
    poses = np.stack([pose(0, 0), pose(1, 0), pose(0, 5)])
    g.build(poses)
    p = g.counts()[1]
    assert p.shape == (15, 11)
    want = np.zeros((15, 11), np.int64)
    want[4:7, 4:7] = 3; want[4:7, 5:8] = 3; want[9:12, 4:7] = 3
    assert np.array_equal(p, want) and g.counts()[0].sum() == 0                # overlap: max, not sum


def test_known_free_at_the_border_is_clipped():
    g = GR.GridReference(resolution=1.0, range_max=0.2, known_free_radius=3.0)
    g.build(pose(0.5, 0.5)[None])
    # origin (-0.5, -0.5), width = int(2.0 / 1) = 2: the node's cell (1, 1); k = 3 reaches past every border, each cell set once
    assert np.array_equal(g.counts()[1], np.ones((2, 2), np.int64))


def test_classification_thresholds():
    g = GR.GridReference(min_pass_through=2, occupancy_threshold=0.1)
    g.geom, g.gcfg = (0.0, 0.0, 5, 1), dict(g.cfg)
    g.hits = np.array([0, 1, 1, 2, 0], np.int64)
    g.passes = np.array([1, 10, 9, 10, 2], np.int64)
    # passes 1 < 2 -> -1; 1 > 0.1*10 = 1.0 false -> 0; 1 > 0.9 -> 100; 2 > 1 -> 100; 0 > 0.2 false -> 0
    assert g.grid().tolist() == [[-1, 0, 100, 100, 0]]


def test_out_of_bounds_cells_are_skipped():
    # a sensor displaced 30 m outside the 50 x 50 grid, looking back through it
    g = GR.GridReference(resolution=1.0, range_max=60.0, max_distance=60.0, known_free_radius=-1.0)
    g.geom, g.gcfg = (-25.0, -25.0, 50, 50), dict(g.cfg)
    g.hits = np.zeros(2500, np.int64); g.passes = np.zeros(2500, np.int64)
    D = pose(-40.0, 0.0)
    g.add_scans([dict(one_beam(45.5), displacement=D)])
    info = g.extend(pose(0, 0)[None], 0)
    h, p = g.counts()
    # o = (-40, 0) -> cell (-15, 25); e = (5.5, 0) -> cell (30, 25): in-bounds cells 0..30 of row 25
    assert p[25].tolist() == [1] * 31 + [0] * 19 and p.sum() == 31
    assert h[25, 30] == 1 and info["hits"] == 1


def test_geometry_by_hand():
    cfg = dict(GR.DEFAULTS, range_max=5.0, resolution=0.3)
    poses = np.stack([pose(1.0, -2.0), pose(4.0, 7.5), pose(-0.5, 1.0)])
    ox, oy, w, h = GR.geometry(cfg, poses)
    assert (ox, oy) == (-0.5 - 25.0, -2.0 - 25.0)
    assert w == int((4.5 + 50.0) / 0.3) == 181                                 # 181.67 truncated
    assert h == int((9.5 + 50.0) / 0.3) == 198                                 # 198.33 truncated
    assert GR.geometry(cfg, poses, present=[0, 0, 1])[2:] == (166, 166)
    assert GR.geometry(cfg, poses, present=[0, 0, 0]) is None


def test_off_grid_condition():
    g = GR.GridReference(resolution=1.0, range_max=2.0)
    g.build(np.stack([pose(0, 0), pose(10, 10)]))                           # origin (-10, -10), 30 x 30: inner box [-8, 18]
    assert g.off_grid(np.stack([pose(0, 0), pose(10, 10), pose(17.9, 5)]), None, 2) == 0
    assert g.off_grid(np.stack([pose(0, 0), pose(10, 10), pose(18.1, 5)]), None, 2) == 1
    assert g.off_grid(np.stack([pose(0, 0), pose(10, 10), pose(3, -8.5)]), None, 2) == 1
    assert g.off_grid(np.stack([pose(0, 0), pose(10, 10), pose(3, -8.5)]), [1, 1, 0], 2) == 0   # absent: not added
    assert g.off_grid(np.stack([pose(-8.5, 0), pose(10, 10)]), None, 1) == 0                   # before first_node


def test_trig_comes_from_math_not_numpy():
    c, s = GR.trig_table(np.float32(-math.pi / 2), np.float32(math.pi / 360), 720)
    a, d = float(np.float32(-math.pi / 2)), float(np.float32(math.pi / 360))
    assert c[719] == math.cos(a + 719.0 * d) and s[1] == math.sin(a + 1.0 * d)
