"""GPU tests of uzl_grid_* on the planted cases of tests/grid_cases.py: rays that cross whole 128-cell tiles (the closed-form tile clip
with both its minor-axis bounds at once), single rays directed at a tile corner, grids of 1, 127, 128, 129 and 257 cells, long and
ragged beam lists of one tile, known-free squares over several tiles, the range and classification thresholds, and extends onto
tiles the build never touched.  hits, passes, the int8 grid and the info equal the NumPy restatement (tests/grid_reference.py)
exactly after the build and after every extend; tests/test_grid_cases_reference.py shows that each case reaches what it is named
after.  A mismatch names the first differing cells and their tiles."""
import numpy as np
import pytest

import grid_cases as GC
import grid_reference as GR
from test_grid_gpu import same

pytestmark = pytest.mark.gpu

CASES = GC.all_cases()
BY_NAME = {c["name"]: c for c in CASES}
T = GC.TILE


def differences(what, got, want, limit=8):
    """'' when equal, else the first differing cells with their tiles: (x, y) tile (tx, ty): got != want"""
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} != {want.shape}"
    ys, xs = np.nonzero(got != want)
    if not len(xs):
        return ""
    tiles = sorted(set(zip((xs // T).tolist(), (ys // T).tolist())))
    first = "; ".join(f"({x}, {y}) tile ({x // T}, {y // T}): {got[y, x]} != {want[y, x]}" for x, y in zip(xs[:limit].tolist(), ys[:limit].tolist()))
    return f"{what}: {len(xs)} cells differ in {len(tiles)} tiles {tiles[:limit]}: {first}"


def same_cells(g, stage, info=None, where=""):
    """the device's counts, grid and info against one stage of the restatement, with the differing cells named"""
    h, p = g.counts()
    msg = [m for m in (differences("hits", h, stage.hits), differences("passes", p, stage.passes),
                       differences("grid", g.read(), stage.cells)) if m]
    assert not msg, where + " " + " | ".join(msg)
    same(g, stage, info, stage.info if info is not None else None)


def run(capi, c, one_by_one=False):
    """the case on a fresh handle, compared after every stage; returns the handle"""
    g = capi.Grid(**c["cfg"])
    if one_by_one:
        for i, s in enumerate(c["scans"]):
            assert g.add_scans([s]) == i
    else:
        assert g.add_scans(c["scans"]) == 0
    replay(g, c)
    return g


def replay(g, c):
    st = GC.reference(c)
    info = g.build(c["poses"][:c["build"]], GC.pres(c, c["build"]))
    same_cells(g, st[0], info, c["name"] + " build:")
    for k, (n, first) in enumerate(c["extends"]):
        info = g.extend(c["poses"][:n], first, GC.pres(c, n))
        same_cells(g, st[k + 1], info, f"{c['name']} extend {k}:")


SMALL = [c["name"] for c in CASES if c["name"] not in ("long_scaled", "long_fine") and not c["name"].startswith("extend_")
         and "ray" not in c and c["name"] not in GC.TIES and not c["name"].startswith("range_")]


@pytest.mark.parametrize("name", SMALL)
def test_case_equals_the_reference(capi, name):
    run(capi, BY_NAME[name]).close()


@pytest.mark.parametrize("name", ["long_scaled", "long_fine"])
def test_long_rays_equal_the_reference_however_the_scans_arrive(capi, name):
    c = BY_NAME[name]
    g = run(capi, c)
    first = (g.counts(), g.read(), g.info())
    replay(g, c)                                                               # a second time on the same handle
    assert g.info() == first[2]
    g.close()
    b = run(capi, c, one_by_one=True)                                          # the scans added one per call
    (h, p), grid = b.counts(), b.read()
    assert np.array_equal(h, first[0][0]) and np.array_equal(p, first[0][1]) and np.array_equal(grid, first[1]) and b.info() == first[2]
    b.close()


def test_long_rays_in_reverse_scan_order(capi):
    """the same scans stored in the opposite order fill every tile's list the other way round: integer counts, the same grid"""
    c = BY_NAME["long_scaled"]
    r = dict(c, scans=c["scans"][::-1])
    g = capi.Grid(**c["cfg"])
    g.add_scans(r["scans"])
    info = g.build(c["poses"])
    same_cells(g, GC.reference(c)[0], info, "long_scaled reversed:")
    g.close()


@pytest.mark.parametrize("name", [c["name"] for c in GC.directed_cases()])
def test_directed_ray(capi, name):
    c = BY_NAME[name]
    g = run(capi, c)
    h, p = g.counts()
    x0, y0, x1, y1 = c["ray"]
    cells = c["cells"]
    if cells is not None:                                                      # stated by hand, on the device result itself
        want = np.zeros((300, 300), np.uint32)
        for x, y in cells:
            want[y, x] = 1
        assert not differences("passes against the hand-stated cells", p, want)
    assert int(p.max(initial=0)) <= 1
    inside = 0 <= x1 < 300 and 0 <= y1 < 300
    assert int(h.sum()) == int(inside) == g.info()["hits"] and (not inside or h[y1, x1] == 1)
    if 0 <= x0 < 300 and 0 <= y0 < 300:
        assert p[y0, x0] == 1
    grid = g.read()
    assert ((grid == -1) == (p == 0)).all() and ((grid == 100) == (h == 1)).all()
    g.close()


@pytest.mark.parametrize("name", list(GC.TIES))
def test_classification_tie_by_hand(capi, name):
    hits, passes, _, want = GC.TIES[name]
    g = run(capi, BY_NAME[name])
    x, y = GC.TIE_CELL
    h, p = g.counts()
    assert (h[y, x], p[y, x]) == (hits, passes) and g.read()[y, x] == want
    g.close()


@pytest.mark.parametrize("name", list(GC.THRESHOLD_RANGES))
def test_range_threshold_by_hand(capi, name):
    _, valid, hit = GC.THRESHOLD_RANGES[name]
    g = run(capi, BY_NAME["range_" + name])
    i = g.info()
    assert (i["valid_beams"], i["hits"], int(g.counts()[0].sum())) == (valid, hit, hit)
    g.close()


@pytest.mark.parametrize("name", [c["name"] for c in GC.extend_cases()])
def test_extend_case(capi, name):
    c = BY_NAME[name]
    g = capi.Grid(**c["cfg"])
    g.add_scans(c["scans"])
    st = GC.reference(c)
    info = g.build(c["poses"][:c["build"]])
    same_cells(g, st[0], info, name + " build:")
    before = (g.counts(), g.read())
    for k, (n, first) in enumerate(c["extends"]):
        info = g.extend(c["poses"][:n], first)
        same_cells(g, st[k + 1], info, f"{name} extend {k}:")
    if name == "extend_nothing":                                               # nothing changed, grid bytes included
        (h, p), grid = g.counts(), g.read()
        assert np.array_equal(h, before[0][0]) and np.array_equal(p, before[0][1]) and np.array_equal(grid, before[1])
        assert (info["scans"], info["valid_beams"], info["hits"], info["off_grid"]) == (0, 0, 0, 0)
    if name == "extend_known_free_only":
        (h, p), grid = g.counts(), g.read()
        assert np.array_equal(h, before[0][0]) and int((p != before[0][1]).sum()) == int((grid != before[1]).sum()) > 0
    if name == "extend_twice":                                                 # equals one projection of everything on that geometry
        r = GR.GridReference(**c["cfg"])
        r.add_scans(c["scans"])
        r.use_geometry(GC.full_cfg(c), st[0].geom)
        r.extend(c["poses"], 0)
        same(g, r)
    g.close()
