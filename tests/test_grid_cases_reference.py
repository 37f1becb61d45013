"""The cases of tests/grid_cases.py are what they claim to be: shown on the restatement alone (grid_reference.py: its geometry, its
beams and the plain walker `bresenham`), so that the device test that replays them (tests/test_grid_tiles_gpu.py) compares against
inputs known to reach the tile clip, the tile corner, the grid size, the beam list, the square or the threshold each is named
after.  A property that is not reached fails here instead of silently testing something else."""
import numpy as np
import pytest

import grid_cases as GC
import grid_reference as GR

CASES = GC.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
T = GC.TILE


def test_case_list():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    assert {k: len(f()) for k, f in GC.CLASSES.items()} == dict(long=2, directed=27, size=10, beams=2, known_free=10, threshold=8, tie=7,
                                                                  extend=4, box=2)
    for c in CASES:                                                             # every input is one the contract admits
        assert np.isfinite(c["poses"]).all()
        for s in c["scans"]:
            assert s["node"] >= 0 and float(s["range_min"]) >= 0 and np.isfinite(s["displacement"]).all()
            assert np.isfinite(s["angle_min"]) and np.isfinite(s["angle_increment"]) and s["ranges"].dtype == np.float32


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["name"] not in ("long_fine",)])
def test_both_walkers_agree(name):
    """the lock-step walker the device is compared with equals the plain one on every case but the 9-million-cell one"""
    c = BY_NAME[name]
    for a, b in zip(GC.reference(c), GC.reference(c, walker="plain")):
        assert np.array_equal(a.hits, b.hits) and np.array_equal(a.passes, b.passes) and a.info == b.info


# ------------------------------------------------------------------------------------------------ long rays
def _visits(c):
    x0, y0, x1, y1, _ = GC.rays(c)
    _, _, W, H = GR.geometry(GC.full_cfg(c), c["poses"][:c["build"]])
    inb = lambda x, y: 0 <= x < W and 0 <= y < H
    out = []
    for a, b, e, f in zip(x0.tolist(), y0.tolist(), x1.tolist(), y1.tolist()):
        tv = GC.tile_visits(a, b, e, f, W, H)
        ends = {(a // T, b // T) if inb(a, b) else None, (e // T, f // T) if inb(e, f) else None}
        out.append((tv, sum(1 for t in tv if t not in ends), inb(a, b), inb(e, f)))
    return out, W, H


def test_long_scaled_crosses_whole_tiles():
    c = BY_NAME["long_scaled"]
    st = GC.reference(c)[0]
    assert (st.info["width"], st.info["height"], st.info["origin_x"], st.info["origin_y"]) == (513, 511, -25.0, -25.0)
    v, W, H = _visits(c)
    tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
    assert (tiles_x, tiles_y, W - (tiles_x - 1) * T, H - (tiles_y - 1) * T) == (5, 4, 1, 127)
    assert len(v) == st.info["valid_beams"] > 2000
    n_tiles = np.array([len(tv) for tv, _, _, _ in v])
    assert (n_tiles >= 3).sum() >= len(v) // 4                                  # measured 977 of 2160
    assert n_tiles.max() >= 5                                                   # measured: 114 rays visit five or more, one six
    assert sum(p for _, p, _, _ in v) >= 500                                    # visits of a tile holding neither end: measured 2169
    assert sum(1 for _, _, s, _ in v if not s) >= 100                           # measured 720 rays start outside the grid
    assert sum(1 for _, _, _, e in v if not e) >= 100                           # measured 920 end outside it
    assert sum(1 for _, _, s, e in v if s and e) >= 100
    visited = set(t for tv, _, _, _ in v for t in tv)
    assert visited == {(x, y) for x in range(5) for y in range(4)}              # every tile, the 1-cell-wide column included
    assert (st.passes[:, 512] > 0).sum() >= 50                                  # and that column's cells are really passed


def test_long_fine_rays_span_three_tiles():
    c = BY_NAME["long_fine"]
    st = GC.reference(c)[0]
    assert (st.info["width"], st.info["height"]) == (3040, 3025)
    x0, y0, x1, y1, _ = GC.rays(c)
    L = np.maximum(np.abs(x1 - x0), np.abs(y1 - y0))
    assert 256 < L.max() <= 299                                                 # longer than two tiles, within range_max / resolution
    n = [len(GC.tile_visits(int(x0[i]), int(y0[i]), int(x1[i]), int(y1[i]), 3040, 3025)) for i in np.argsort(-L)[:200]]
    assert max(n) >= 3 and sum(1 for k in n if k >= 3) >= 20


# ------------------------------------------------------------------------------------------------ directed rays
DIRECTED = [c["name"] for c in GC.directed_cases()]
CORNER = {(127, 127), (128, 127), (127, 128), (128, 128)}


@pytest.mark.parametrize("name", DIRECTED)
def test_directed_ray_is_the_ray_it_says(name):
    c = BY_NAME[name]
    st = GC.reference(c)[0]
    assert (st.info["width"], st.info["height"], st.info["origin_x"], st.info["origin_y"]) == (300, 300, -150.0, -150.0)
    x0, y0, x1, y1, hit = GC.rays(c)
    assert (int(x0[0]), int(y0[0]), int(x1[0]), int(y1[0])) == c["ray"] and len(x0) == 1 and hit[0]   # the cells chosen, exactly
    walk = GR.bresenham(*c["ray"])
    inb = [(x, y) for x, y in walk if 0 <= x < 300 and 0 <= y < 300]
    if c["cells"] is not None:
        assert inb == c["cells"]                                                # stated by hand in grid_cases.py
    want = np.zeros((300, 300), np.uint32)
    for x, y in inb:
        want[y, x] += 1
    assert np.array_equal(st.passes, want) and st.passes.max() <= 1
    end_in = 0 <= c["ray"][2] < 300 and 0 <= c["ray"][3] < 300
    assert st.info["hits"] == int(end_in) and int(st.hits.sum()) == int(end_in)
    if end_in:
        assert st.hits[c["ray"][3], c["ray"][2]] == 1


def test_directed_rays_reach_the_corner():
    walk = lambda n: GR.bresenham(*BY_NAME[n]["ray"])
    for cx, cy in CORNER:
        assert walk(f"end_on_{cx}_{cy}")[-1] == (cx, cy) and walk(f"start_on_{cx}_{cy}")[0] == (cx, cy)
        assert len(GC.tile_visits(*BY_NAME[f"end_on_{cx}_{cy}"]["ray"], 300, 300)) == 2
    for n in ("along_last_row", "along_first_row", "along_last_column", "along_first_column"):
        assert len(GC.tile_visits(*BY_NAME[n]["ray"], 300, 300)) == 3
    for n, two in (("diagonal_pp", {(127, 127), (128, 128)}), ("diagonal_mm", {(127, 127), (128, 128)}),
                   ("diagonal_pm", {(127, 128), (128, 127)}), ("diagonal_mp", {(127, 128), (128, 127)})):
        assert set(walk(n)) & CORNER == two
    # slopes 1:2 and 2:1: the error term ties at every other step, one of them on the step across the corner; the contract's rule moves
    # both coordinates there, so the ray goes from one corner cell to the diagonally opposite one and visits two tiles, not three
    for n in DIRECTED:
        if n.startswith("slope_"):
            w = walk(n)
            x0, y0, x1, y1 = BY_NAME[n]["ray"]
            assert max(abs(x1 - x0), abs(y1 - y0)) == 2 * min(abs(x1 - x0), abs(y1 - y0))
            hit = [p for p in w if p in CORNER]
            assert len(hit) == 2 and hit[0][0] != hit[1][0] and hit[0][1] != hit[1][1], (n, hit)
            assert w.index(hit[1]) == w.index(hit[0]) + 1 and len(GC.tile_visits(x0, y0, x1, y1, 300, 300)) == 2
    assert len({tuple(np.sign([c["ray"][2] - c["ray"][0], c["ray"][3] - c["ray"][1]])) + (abs(c["ray"][2] - c["ray"][0]) > abs(c["ray"][3] - c["ray"][1]),)
                for c in GC.directed_cases() if c["name"].startswith("slope_")}) == 8     # eight octants
    assert GC.tile_visits(*BY_NAME["outside_to_outside"]["ray"], 300, 300) == [(0, 2)]
    assert GC.reference(BY_NAME["all_outside"])[0].passes.sum() == 0
    assert GC.reference(BY_NAME["zero_length_on_corner"])[0].passes.sum() == 1


# ------------------------------------------------------------------------------------------------ grid sizes
def test_grid_sizes():
    got = []
    for c in GC.size_cases():
        st = GC.reference(c)[0]
        W, H = st.info["width"], st.info["height"]
        got.append((W, H))
        assert c["name"].startswith(f"size_{W}x{H}")
        p = st.passes
        for border in (p[0, :], p[-1, :], p[:, 0], p[:, -1]):                   # the fan reaches every border
            assert border.max() > 0
        assert st.info["valid_beams"] == 360 and st.info["hits"] <= 180         # the even beams leave the grid ...
        assert st.info["hits"] > 0 or (min(W, H) == 1 and max(W, H) > 1)        # ... odd ones end inside (a 1 x N strip catches none)
    assert got == GC.SIZES + [(129, 257)]
    for v in (1, 127, 128, 129, 257):
        assert v in [w for w, _ in got] and v in [h for _, h in got]


# ------------------------------------------------------------------------------------------------ beam lists
def test_beam_lists():
    c = BY_NAME["beams_3000_scans_of_one"]
    st = GC.reference(c)[0]
    assert (st.info["width"], st.info["height"]) == (100, 100) and len(c["scans"]) == 3000 == st.info["scans"]
    assert all(len(s["ranges"]) == 1 for s in c["scans"])
    assert 2000 < st.info["valid_beams"] < 3000 and st.info["hits"] == st.info["valid_beams"]       # some beams are invalid
    c = BY_NAME["beams_ragged_scans"]
    st = GC.reference(c)[0]
    n = [len(s["ranges"]) for s in c["scans"]]
    assert n == [1, 0, 2, 1023, 0, 128, 0, 1024, 1025, 0, 4097, 1, 1]
    assert (st.info["width"], st.info["height"]) == (100, 100) and st.info["scans"] == len(n)
    cfg = GC.full_cfg(c)
    valid = [GR.beams(cfg, s, GR.compose(c["poses"][0], s["displacement"]))[0] for s in c["scans"]]
    assert valid[5] == 0 and valid[-1] == 0 and all(v > 0 for v, k in zip(valid, n) if k > 1 and k != 128)   # the scans without a valid beam
    assert st.info["valid_beams"] == sum(valid) > 5000


# ------------------------------------------------------------------------------------------------ known free
def _only_square(c):
    """passes of the known-free squares alone: the case without its scans"""
    r = GR.GridReference(**c["cfg"])
    r.build(c["poses"])
    return r.counts()[1]


def test_known_free_squares():
    c = BY_NAME["known_free_20m"]
    st = GC.reference(c)[0]
    assert (st.info["width"], st.info["height"]) == (510, 510)
    sq = _only_square(c)
    assert sq.max() == 1                                                        # max, not sum, where the three squares overlap
    want = np.zeros((510, 510), np.uint32)
    for cx in (50, 460, 255):                                                   # the nodes' cells; k = 200
        want[max(cx - 200, 0):cx + 201, max(cx - 200, 0):cx + 201] = 1
    assert np.array_equal(sq, want)
    assert want[55:456, 55:456].all() and 401 == 456 - 55 and {55 // T, 455 // T} == {0, 3}      # 401 cells over 4 x 4 tiles
    assert want[0, 0] and want[509, 509] and not want[0, 509]                   # clipped at two borders each
    assert (st.passes >= want).all() and (st.passes > want).any()               # rays on top
    for name, k in (("known_free_zero", 0), ("known_free_under_one_cell", 0), ("known_free_truncates", 2), ("known_free_negative", -1),
                    ("known_free_small_negative", 0)):
        c = BY_NAME[name]
        assert (int(c["cfg"]["known_free_radius"] / 0.1) >= 0) == (k >= 0) and (k < 0 or int(c["cfg"]["known_free_radius"] / 0.1) == k)
        sq = _only_square(c)
        cells = {(int(GR.cell(p[3], -5.0, 0.1)), int(GR.cell(p[7], -5.0, 0.1))) for p in c["poses"]}
        want = np.zeros_like(sq)
        for x, y in cells:
            if k >= 0:
                want[y - k:y + k + 1, x - k:x + k + 1] = 1
        assert np.array_equal(sq, want) and len(cells) == 3
    assert 0.3 / 0.1 < 3.0                                                      # why known_free_truncates has k = 2


def test_min_pass_through():
    st0 = GC.reference(BY_NAME["min_pass_through_0"])[0]
    assert _only_square(BY_NAME["min_pass_through_0"]).sum() == 0 and not (st0.cells == -1).any()
    assert set(np.unique(st0.cells)) == {0, 100}
    st3 = GC.reference(BY_NAME["min_pass_through_3"])[0]
    assert set(np.unique(_only_square(BY_NAME["min_pass_through_3"]))) == {0, 3}
    assert ((st3.passes > 0) & (st3.passes < 3)).any() and (st3.cells[(st3.passes < 3)] == -1).all()
    assert (st3.cells[st3.passes >= 3] >= 0).all()
    stk = GC.reference(BY_NAME["min_pass_through_1000"])[0]
    assert set(np.unique(_only_square(BY_NAME["min_pass_through_1000"]))) == {0, 1000} and stk.passes.max() > 1000
    assert (stk.cells[stk.passes < 1000] == -1).all() and (stk.cells[stk.passes >= 1000] >= 0).all()
    assert (stk.hits[stk.passes < 1000] > 0).any()                             # hit cells that stay unknown
    c = BY_NAME["known_free_overlap"]
    sq = _only_square(c)
    assert set(np.unique(sq)) == {0, 4} and (sq == 4).sum() > 121               # three overlapping 11 x 11 squares: one value, not a sum
    st = GC.reference(c)[0]
    assert st.passes.max() > 4 and ((st.passes > 0) & (st.passes < 4)).any()


# ------------------------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("name", list(GC.THRESHOLD_RANGES))
def test_range_thresholds(name):
    r, valid, hit = GC.THRESHOLD_RANGES[name]
    c = BY_NAME["range_" + name]
    st = GC.reference(c)[0]
    assert st.info["valid_beams"] == valid and st.info["hits"] == hit and int(st.hits.sum()) == hit
    sq = _only_square(c)
    ray = st.passes.astype(np.int64) - sq
    assert (ray.sum() > 0) == bool(valid)
    if valid:
        # the ray's last cell: at distance min(r, max_distance) along the beam, stated from the config by hand
        d = min(float(r), 3.0)
        ex, ey = int(np.floor((d * np.cos(GC.THRESHOLD_ANGLE) + 25.0) / 0.1)), int(np.floor((d * np.sin(GC.THRESHOLD_ANGLE) + 25.0) / 0.1))
        ys, xs = np.nonzero(ray)
        far = np.argmax(np.hypot(xs - 250, ys - 250))
        assert (int(xs[far]), int(ys[far])) == (ex, ey)
        assert st.hits[ey, ex] == hit


def test_threshold_values_are_neighbours():
    f = np.float32
    R = {k: v[0] for k, v in GC.THRESHOLD_RANGES.items()}
    assert R["below_range_min"] < f(0.5) == R["at_range_min"] < R["above_range_min"] and R["above_range_min"] - R["below_range_min"] < 1e-7
    assert R["below_range_max"] < f(5.0) == R["at_range_max"] and f(5.0) - R["below_range_max"] < 1e-6
    assert R["below_max_distance"] < f(3.0) == R["at_max_distance"] < R["above_max_distance"] and R["above_max_distance"] - f(3.0) < 1e-6
    assert all(v.dtype == np.float32 for v in R.values())


@pytest.mark.parametrize("name", list(GC.TIES))
def test_classification_ties(name):
    h, p, thr, want = GC.TIES[name]
    c = BY_NAME[name]
    st = GC.reference(c)[0]
    x, y = GC.TIE_CELL
    assert (st.hits[y, x], st.passes[y, x]) == (h, p) and c["cfg"]["occupancy_threshold"] == thr
    assert st.cells[y, x] == want
    assert (st.cells[y, 250:260] == 0).all()                                    # passed, never hit
    assert st.cells[y, 249] == -1 and st.cells[y + 1, x] == -1                  # never passed, and no known-free square
    if p > h:
        assert (st.hits[y, 270], st.passes[y, 270]) == (p - h, p - h) and st.cells[y, 270] == (100 if thr < 1.0 else 0)


# ------------------------------------------------------------------------------------------------ extend
def _tile_sums(a):
    H, W = a.shape
    return {(x, y): int(a[y * T:(y + 1) * T, x * T:(x + 1) * T].sum()) for y in range((H + T - 1) // T) for x in range((W + T - 1) // T)}


def test_extend_reaches_tiles_the_build_left_empty():
    c = BY_NAME["extend_through_empty_tiles"]
    b, e = GC.reference(c)
    assert b.geom == e.geom == (-25.0, -25.0, 513, 511)
    empty = [t for t, s in _tile_sums(b.passes).items() if s == 0]
    assert len(empty) >= 12                                                     # the build's plain fan stays in the four central tiles
    after = _tile_sums(e.passes)
    assert all(after[t] > 0 for t in empty) and (4, 0) in empty and (4, 3) in empty
    x0, y0, x1, y1, _ = GC.rays(c, 3, 2, b.geom)
    through = 0
    for a, bb, cc, d in zip(x0.tolist()[::8], y0.tolist()[::8], x1.tolist()[::8], y1.tolist()[::8]):
        tv = GC.tile_visits(a, bb, cc, d, 513, 511)
        through += sum(1 for t in tv[1:-1] if t in empty)
    assert through >= 20                                                        # and passes through them, not only into them
    assert e.info["scans"] == 3 and e.info["valid_beams"] > 2000 and e.info["off_grid"] == 0


def test_extend_that_adds_nothing_or_a_square_only():
    b, e = GC.reference(BY_NAME["extend_nothing"])
    assert np.array_equal(b.hits, e.hits) and np.array_equal(b.passes, e.passes) and np.array_equal(b.cells, e.cells)
    assert (e.info["scans"], e.info["valid_beams"], e.info["hits"], e.info["off_grid"]) == (0, 0, 0, 0)
    b, e = GC.reference(BY_NAME["extend_known_free_only"])
    d = e.passes.astype(np.int64) - b.passes
    assert np.array_equal(b.hits, e.hits) and (e.info["scans"], e.info["valid_beams"], e.info["hits"]) == (0, 0, 0)
    ys, xs = np.nonzero(d)
    assert len(xs) > 0 and xs.min() >= 35 and xs.max() <= 45 and ys.min() >= 425 and ys.max() <= 435 and d.max() == 1   # node 3's cell is (40, 430)
    assert e.info["off_grid"] == 1                                              # it lies within range_max of the left border


def test_two_extends_equal_one_projection_of_everything():
    c = BY_NAME["extend_twice"]
    st = GC.reference(c)
    r = GR.GridReference(**c["cfg"])
    r.add_scans(c["scans"])
    r.use_geometry(GC.full_cfg(c), st[0].geom)
    r.extend(c["poses"], 0)
    h, p = r.counts()
    assert np.array_equal(h, st[2].hits) and np.array_equal(p, st[2].passes) and np.array_equal(r.grid(), st[2].cells)
    assert [s.info["off_grid"] for s in st] == [0, 0, 1]


# ------------------------------------------------------------------------------------------------ the range square at its edge
@pytest.mark.parametrize("name", [c["name"] for c in GC.box_cases()])
def test_box_edge_ray_ends_beyond_the_plain_bound(name):
    """the ray's end cell is the first of tile column 1 although sensor + |row| * R_eff still lies in cell 127: without slack, the
    range square of plan() would stop one tile short"""
    c = BY_NAME[name]
    cfg = GC.full_cfg(c)
    st = GC.reference(c)[0]
    ox = st.info["origin_x"]
    assert (st.info["width"], st.info["height"], st.info["valid_beams"], st.info["hits"]) == (200, 200, 1, 1)
    S = GR.compose(c["poses"][0], c["scans"][0]["displacement"])
    bound = S[3] + np.sqrt(S[0] * S[0] + S[1] * S[1]) * min(cfg["range_max"], cfg["max_distance"])
    assert int(np.floor((bound - ox) / 0.1)) == 127
    x0, y0, x1, y1, _ = GC.rays(c)
    assert int(x1[0]) == 128 and 0 <= int(y1[0]) < 128 and int(x0[0]) < 100
    _, ex, _, _ = GR.beams(cfg, c["scans"][0], S)
    assert 1e-8 < float(ex[0]) - bound < 1e-6                                   # f32 rounding of p, times the scale of 3
    assert st.hits[int(y1[0]), 128] == 1
