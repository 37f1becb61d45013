"""The host side of the occupancy-grid projection on the CPU, through two hooks of the diagnostic library (no device):

uzl_debug_grid_ray_clip runs grid_ray_clip (grid_types.hpp), the closed form that lets a workgroup enter a ray at its first cell inside
its tile, and is compared with the contract's loop (grid_reference.bresenham) filtered to the rectangle: the same cells in the same
order, nothing when the ray misses - on every small ray against every small rectangle, on random rays of up to 700 cells against
128-cell tiles and their partial neighbours, and on rays of almost 2^24 cells (the int64 arithmetic).

uzl_debug_grid_plan runs plan() (uzl_grid.hip), which sends each scan only to the tiles its conservative range square touches.  Held
here, for the cases of grid_cases.py and for random scans (yaw, scale 0.2 to 20, shear, sensors inside, outside and far outside):
every in-bounds cell of every ray lies in a tile that lists its scan (a box one tile too small fails this); the lists are exactly
what grid_tile_kernel walks (ascending tiles, prefix sums, ent_beam the exclusive prefix of the listed scans' n in scan order, no
empty or off-grid scan listed, ocx / ocy = cell(o)); the known-free rectangles are the reference's clipped squares in exactly the tiles
they intersect; rays beyond 2^24 cells are refused."""
import numpy as np
import pytest

import grid_cases as GC
import grid_reference as GR

T = GC.TILE
CASES = GC.all_cases()
BY_NAME = {c["name"]: c for c in CASES}


# ------------------------------------------------------------------------------------------------ grid_ray_clip
def expect_clip(cells, rects, cap):
    """cells [m, 2] of one ray in walk order, rects [R, 4] -> (count [R], the first cap inside cells per rectangle [R, cap, 2], zero-padded)"""
    x, y = cells[:, 0][None, :], cells[:, 1][None, :]
    inside = (x >= rects[:, 0:1]) & (x <= rects[:, 2:3]) & (y >= rects[:, 1:2]) & (y <= rects[:, 3:4])
    count = inside.sum(1)
    order = np.argsort(~inside, axis=1, kind="stable")[:, :cap]                 # the inside cells first, in walk order
    out = cells[order]
    if out.shape[1] < cap:
        out = np.concatenate([out, np.zeros((len(rects), cap - out.shape[1], 2), out.dtype)], 1)
    out[np.arange(cap)[None, :] >= count[:, None]] = 0
    return count, out


def check_clip(capi, ray, cells, rects, cap):
    q = np.concatenate([np.tile(np.array(ray, np.int64), (len(rects), 1)), rects], 1)
    count, got = capi.grid_ray_clip(q, cap)
    want_n, want = expect_clip(np.asarray(cells, np.int64).reshape(-1, 2), rects, cap)
    bad = np.nonzero((count != want_n) | (got != want).any((1, 2)))[0]
    assert not len(bad), (ray, rects[bad[0]].tolist(), int(count[bad[0]]), int(want_n[bad[0]]), got[bad[0], :4].tolist(), want[bad[0], :4].tolist())
    return want_n


def test_clip_every_small_ray_against_every_small_rectangle(capi):
    lo, hi = -4, 4
    v = np.arange(lo, hi + 1)
    a, b = np.meshgrid(v, v, indexing="ij")
    span = np.stack([a.ravel(), b.ravel()], 1)
    span = span[span[:, 0] <= span[:, 1]]                                       # 45 intervals per axis
    rects = np.array([(x[0], y[0], x[1], y[1]) for x in span for y in span], np.int64)          # 2025 rectangles
    n = hits = 0
    for ox, oy in ((0, 0), (3, -2), (-5, 6)):
        for ex in range(-9, 10):
            for ey in range(-9, 10):
                ray = (ox, oy, ox + ex, oy + ey)
                want_n = check_clip(capi, ray, GR.bresenham(*ray), rects, 20)
                n += len(rects); hits += int((want_n > 0).sum())
    assert n == 3 * 361 * 2025 and hits > n // 10 and hits < n                  # misses and visits both


def test_clip_long_rays_against_tiles(capi):
    rng = np.random.default_rng(5)
    W, H = 513, 511                                                             # 5 x 4 tiles, the last column 1 cell wide
    both = deep = 0
    for i in range(3000):
        L = int(rng.integers(1, 701))
        x0, y0 = int(rng.integers(-300, W + 300)), int(rng.integers(-300, H + 300))
        th = rng.uniform(0, 2 * np.pi)
        if i % 10 == 0:                                                         # exact slopes: 0, 1, 1:2, 2:1 and their mirror images
            dx, dy = [(L, 0), (0, L), (L, L), (L, L // 2), (L // 2, L), (-L, L), (-L, -(L // 2)), (L // 2, -L), (-L, 0), (0, -L)][(i // 10) % 10]
        else:
            dx, dy = int(round(L * np.cos(th))), int(round(L * np.sin(th)))
        ray = (x0, y0, x0 + dx, y0 + dy)
        cells = GR.bresenham(*ray)
        tiles = sorted({(x // T, y // T) for x, y in cells if 0 <= x < W and 0 <= y < H})
        cand = set(tiles)
        for tx, ty in tiles[:3]:                                                # and neighbours the ray may miss
            cand |= {(tx + 1, ty), (tx, ty + 1), (tx - 1, ty - 1)}
        cand = [t for t in cand if 0 <= t[0] < 5 and 0 <= t[1] < 4] or [(2, 2)]
        rects = np.array([(tx * T, ty * T, min(tx * T + T, W) - 1, min(ty * T + T, H) - 1) for tx, ty in cand], np.int64)
        check_clip(capi, ray, cells, rects, 130)
        ends = {(ray[0] // T, ray[1] // T), (ray[2] // T, ray[3] // T)}
        through = [t for t in tiles if t not in ends]
        both += len(through)
        deep += sum(1 for t in through if len(tiles) >= 4)
    assert both > 1500 and deep > 500                                           # tiles crossed with neither end inside: ka > 0 and kb < L at once


def test_clip_rays_of_almost_2_to_24_cells(capi):
    """L near 2^24: 2 L k and 2 L (dhi + 1) pass 2^31 within the first tile; the tile lies within 400 cells of the ray's start, so the
    contract's loop is walked only that far"""
    rng = np.random.default_rng(6)
    big = 1 << 24
    seen = 0
    for i in range(300):
        L = big - int(rng.integers(0, 1000))
        m = [0, L, L // 2, L - 1, 1, int(rng.integers(0, L)), int(rng.integers(0, L)), int(rng.integers(L // 2, L))][i % 8]
        sx, sy = (1, -1)[i % 2], (1, -1)[(i // 2) % 2]
        d = (L * sx, m * sy) if (i // 4) % 2 == 0 else (m * sx, L * sy)
        x0, y0 = int(rng.integers(-200, 200)), int(rng.integers(-200, 200))
        ray = (x0, y0, x0 + d[0], y0 + d[1])
        cells = []
        for k, c in enumerate(GR.bresenham_iter(*ray)):                         # the first 700 steps cover every tile below
            if k > 700:
                break
            cells.append(c)
        rects = np.array([(tx * T, ty * T, tx * T + T - 1, ty * T + T - 1) for tx in range(-2, 3) for ty in range(-2, 3)], np.int64)
        want_n = check_clip(capi, ray, cells, rects, 130)
        assert max(np.abs(rects[:, [0, 2]] - x0).max(), np.abs(rects[:, [1, 3]] - y0).max()) < 700   # step k lies k cells (Chebyshev) from the start
        seen += int((want_n > 0).sum())
    assert seen > 600


def test_clip_hook_refuses_bad_arguments(capi):
    import ctypes as C
    L = capi.diag_lib()
    capi.grid_ray_clip(np.zeros((0, 8), np.int32), 4)
    assert L.uzl_debug_grid_ray_clip(C.c_int32(-1), None, C.c_int32(4), None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_debug_grid_ray_clip(C.c_int32(1), None, C.c_int32(4), None, None) == capi.UZL_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ plan()
def projected(scans, n, present, first):
    """indices of the scans a call projects, in record order"""
    return [i for i, s in enumerate(scans) if first <= s["node"] < n and (present is None or present[s["node"]])]


def check_plan(capi, cfg, geom, poses, scans, present=None, first=0):
    """every invariant grid_tile_kernel relies on, for one call of plan(); returns the plan"""
    full = dict(GR.DEFAULTS, **cfg)
    ox, oy, W, H = geom
    res = full["resolution"]
    P = np.asarray(poses, np.float64).reshape(-1, 12)
    n = len(P)
    p = capi.grid_plan(cfg, geom, P, scans, present, first)
    tiles_x, tiles_y = (W + T - 1) // T, (H + T - 1) // T
    recs = projected(scans, n, present, first)
    assert len(p["ocx"]) == len(recs)
    nbeams = np.array([len(scans[i]["ranges"]) for i in recs], np.int64)
    # --- the lists
    t = p["tiles"]
    assert (np.diff(t) > 0).all() and (len(t) == 0 or (t[0] >= 0 and t[-1] < tiles_x * tiles_y))
    es, ks = p["ent_start"], p["kf_start"]
    assert es[0] == 0 and ks[0] == 0 and (np.diff(es) >= 0).all() and (np.diff(ks) >= 0).all()
    assert es[-1] == len(p["ent_scan"]) == len(p["ent_beam"]) and ks[-1] == len(p["kf_rect"])
    assert ((np.diff(es) > 0) | (np.diff(ks) > 0)).all()                        # no tile with neither entries nor rectangles
    listed = {}                                                                 # record -> set of tiles
    for j, tile in enumerate(t.tolist()):
        e = p["ent_scan"][es[j]:es[j + 1]]
        assert (np.diff(e) > 0).all() and (len(e) == 0 or (e[0] >= 0 and e[-1] < len(recs)))   # ascending scan order, each once
        assert np.array_equal(p["ent_beam"][es[j]:es[j + 1]], np.concatenate([[0], np.cumsum(nbeams[e])[:-1]]) if len(e) else [])
        assert (nbeams[e] > 0).all()                                            # no empty scan is listed
        for r in e.tolist():
            listed.setdefault(r, set()).add((tile % tiles_x, tile // tiles_x))
    for r, ts in listed.items():                                                # a box of tiles, and cell(o) of the listed scans
        xs, ys = [a for a, _ in ts], [b for _, b in ts]
        assert ts == {(a, b) for a in range(min(xs), max(xs) + 1) for b in range(min(ys), max(ys) + 1)}
        S = GR.compose(P[scans[recs[r]]["node"]], scans[recs[r]]["displacement"])
        assert (p["ocx"][r], p["ocy"][r]) == (int(GR.cell(S[3], ox, res)), int(GR.cell(S[7], oy, res)))
    # --- cover: every in-bounds cell of every ray, and every in-bounds end cell, lies in a tile that lists the ray's scan
    X0, Y0, X1, Y1, R = [], [], [], [], []
    for r, i in enumerate(recs):
        s = scans[i]
        S = GR.compose(P[s["node"]], s["displacement"])
        _, ex, ey, _ = GR.beams(full, s, S)
        cx, cy = GR.cell(ex, ox, res), GR.cell(ey, oy, res)
        X0.append(np.full(len(cx), int(GR.cell(S[3], ox, res)), np.int64)); Y0.append(np.full(len(cx), int(GR.cell(S[7], oy, res)), np.int64))
        X1.append(cx); Y1.append(cy); R.append(np.full(len(cx), r, np.int64))
    lists = np.zeros((len(recs) + 1, tiles_x * tiles_y + 1), bool)
    for r, ts in listed.items():
        for a, b in ts:
            lists[r, b * tiles_x + a] = True
    n_cells = 0
    if X0 and sum(len(a) for a in X0):
        x0, y0, x1, y1, rr = (np.concatenate(a) for a in (X0, Y0, X1, Y1, R))
        end_in = (x1 >= 0) & (x1 < W) & (y1 >= 0) & (y1 < H)
        assert lists[rr[end_in], (y1[end_in] // T) * tiles_x + x1[end_in] // T].all(), "an in-bounds end cell outside its scan's box"
        for idx, x, y in GR.steps(x0, y0, x1, y1):
            inb = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            ok = lists[rr[idx[inb]], (y[inb] // T) * tiles_x + x[inb] // T]
            n_cells += int(inb.sum())
            if not ok.all():
                k = np.nonzero(~ok)[0][0]
                raise AssertionError(f"cell ({x[inb][k]}, {y[inb][k]}) of a ray of scan {recs[rr[idx[inb]][k]]} lies in a tile that does not list it")
    # --- known-free rectangles: the reference's clipped squares, in exactly the tiles they intersect
    k = int(full["known_free_radius"] / res)
    want = []
    if k >= 0 and full["min_pass_through"] > 0:
        for i in range(n):
            if not (first <= i and (present is None or present[i])):
                continue
            cx, cy = int(GR.cell(P[i, 3], ox, res)), int(GR.cell(P[i, 7], oy, res))
            q = (max(cx - k, 0), max(cy - k, 0), min(cx + k, W - 1), min(cy + k, H - 1))
            if q[0] <= q[2] and q[1] <= q[3]:
                want.append(q)
    got = {}
    for j, tile in enumerate(t.tolist()):
        got[tile] = [tuple(q) for q in p["kf_rect"][ks[j]:ks[j + 1]].tolist()]
    for tile in range(tiles_x * tiles_y):
        a, b = (tile % tiles_x) * T, (tile // tiles_x) * T
        here = [q for q in want if q[0] <= a + T - 1 and q[2] >= a and q[1] <= b + T - 1 and q[3] >= b]
        assert got.get(tile, []) == here, (tile, got.get(tile), here)
    p["cells_checked"] = n_cells
    p["listed"] = listed
    return p


def stages(c):
    """(n poses, first_node, geometry) of the build and of every extend of a case"""
    g = GR.geometry(GC.full_cfg(c), c["poses"][:c["build"]], GC.pres(c, c["build"]))
    return [(c["build"], 0, g)] + [(n, first, g) for n, first in c["extends"]]


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_plan_of_every_case(capi, name):
    c = BY_NAME[name]
    for n, first, geom in stages(c):
        p = check_plan(capi, c["cfg"], geom, c["poses"][:n], c["scans"], GC.pres(c, n), first)
        if name == "long_scaled":
            assert p["cells_checked"] > 200000 and len(p["tiles"]) == 20
        if name == "extend_nothing" and first:
            assert len(p["tiles"]) == 0 and len(p["ocx"]) == 0
        if name == "extend_known_free_only" and first:
            assert len(p["ent_scan"]) == 0 and len(p["kf_rect"]) == 1 and len(p["tiles"]) == 1
        if name == "all_outside":
            assert p["cells_checked"] == 0


def random_scans(rng, n_nodes, n_scans, geom, res):
    ox, oy, W, H = geom
    out = []
    for i in range(n_scans):
        kind = i % 4
        yaw, scale = rng.uniform(-np.pi, np.pi), float(np.exp(rng.uniform(np.log(0.2), np.log(20.0))))
        A = scale * np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        if kind == 1:
            A = A @ np.array([[1.0, rng.uniform(-1.5, 1.5)], [0.0, rng.uniform(0.3, 1.2)]])      # shear and unequal rows
        if i % 3 == 0:
            t = rng.uniform(-3, 3, 2)                                           # near its node: inside the grid
        elif i % 3 == 1:
            t = np.array([ox - rng.uniform(0, 40), oy + rng.uniform(-20, H * res + 20)])      # left of the grid, rays may reach in
            if i % 2:
                t = t[::-1].copy()
        else:
            t = rng.uniform(-1, 1, 2) * 3000.0                                  # far outside
        nb = int(rng.choice([0, 1, 7, 64, 64, 64]))
        r = rng.uniform(0.05, 5.2, nb).astype(np.float32)
        if nb > 2:
            r[0] = np.nextafter(np.float32(5.0), np.float32(0)); r[1] = np.float32(np.nan)
        out.append(dict(node=int(rng.integers(0, n_nodes + 1)), ranges=r, angle_min=np.float32(rng.uniform(-3, 3)),
                        angle_increment=np.float32(2 * np.pi / max(nb, 1)), range_min=np.float32(0.1),
                        displacement=GC.disp(A, t)))
    return out


@pytest.mark.parametrize("seed,cfg", [(1, {}), (2, dict(max_distance=3.0)), (3, dict(resolution=0.05, range_max=3.0, known_free_radius=2.0))])
def test_plan_of_random_scans(capi, seed, cfg):
    rng = np.random.default_rng(seed)
    full = dict(GR.DEFAULTS, **cfg)
    poses = np.array([GC.pose(rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(-np.pi, np.pi)) for _ in range(6)])
    present = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    geom = GR.geometry(full, poses, present)
    scans = random_scans(rng, len(poses), 300, geom, full["resolution"])       # poses are about the origin: node-relative t is world-ish
    p = check_plan(capi, cfg, geom, poses, scans, present, 0)
    assert p["cells_checked"] > 50000 and len(p["listed"]) > 30
    assert len(p["listed"]) < len(p["ocx"])                                     # and some projected scans reach no tile at all
    p = check_plan(capi, cfg, geom, poses, scans, present, 3)                   # an extend's plan
    assert 0 < len(p["ocx"]) < 300


def test_plan_refuses_rays_beyond_2_to_24_cells(capi):
    cfg = dict(resolution=1.0, range_max=1.0)                                   # R_eff = 1: the bound is the rotation row's norm, in cells
    geom = (-5.0, -5.0, 10, 10)
    big = float(1 << 24)

    def scan(s, t=(0, 0), away=False):
        return dict(node=0, ranges=np.array([0.5], np.float32), angle_min=np.float32(np.pi if away else 0), angle_increment=np.float32(0),
                    range_min=np.float32(0.1), displacement=GC.disp(((s, 0), (0, 1)), t))

    # which side the bound falls on: a row norm of exactly 2^24 cells is accepted, the next double above it refused
    p = capi.grid_plan(cfg, geom, [GC.pose(0, 0)], [scan(big)])
    assert len(p["tiles"]) == 1 and len(p["ent_scan"]) == 1
    for s in (np.nextafter(big, np.inf), 2 * big, 1e300):
        with pytest.raises(capi.UzlError) as e:
            capi.grid_plan(cfg, geom, [GC.pose(0, 0)], [scan(s)])
        assert e.value.status == capi.UZL_ERR_BAD_ARG and "2^24" in str(e.value)
    with pytest.raises(capi.UzlError):                                          # the y row likewise
        capi.grid_plan(cfg, geom, [GC.pose(0, 0)], [dict(scan(1.0), displacement=GC.disp(((1, 0), (big, big)), (0, 0)))])
    # a sensor 2^24 cells from the grid: accepted, listed nowhere (whatever its rays do, none comes within 2^24 - 1 cells of it)
    p = capi.grid_plan(dict(cfg, known_free_radius=-1.0), geom, [GC.pose(0, 0)], [scan(1.0, (-5.0 - big, 0.0), away=True), scan(1.0, (0.0, 5.0 + big))])
    assert len(p["tiles"]) == 0 and len(p["ent_scan"]) == 0 and len(p["ocx"]) == 2
    # the absent and the out-of-range node project nothing
    p = capi.grid_plan(cfg, geom, [GC.pose(0, 0), GC.pose(1, 1)], [dict(scan(1.0), node=1), dict(scan(1.0), node=2)], present=[1, 0])
    assert len(p["ocx"]) == 0 and len(p["ent_scan"]) == 0 and len(p["kf_rect"]) == 1
