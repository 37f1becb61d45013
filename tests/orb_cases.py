"""The ORB configurations away from the defaults that tests/test_orb_reference.py characterises on the restatement (no GPU) and
tests/test_orb_configs_gpu.py then holds the device to, bit for bit.  A case is a name, an image, a config and, where it needs
them, a mask and a pattern; the restatement's result for a case is computed once per process."""
import numpy as np

import orb_reference as R
import orb_scenes as S

ONE = dict(grid_rows=1, grid_cols=1, n_levels=1, edge_threshold=19)


def scene(w, h):
    return S.rectangles(w, h, seed=1000 + w)


def _cases():
    c = {}

    def add(name, img, cfg, mask=None, pattern=None):
        c[name] = dict(name=name, img=img, cfg=cfg, mask=mask, pattern=pattern)

    d = S.dots(130, 120)
    for t in (254, 253):
        add("dots_t%d" % t, d, dict(ONE, fast_threshold=t))
        add("inverse_dots_t%d" % t, 255 - d, dict(ONE, fast_threshold=t))
    for t in (1, 5, 40):
        add("rect160_t%d" % t, scene(160, 152), dict(fast_threshold=t))
    add("scale2", scene(400, 360), dict(scale_factor=2.0, n_levels=3, edge_threshold=19, number_of_features=40))
    add("scale105", scene(200, 190), dict(scale_factor=1.05, n_levels=8, edge_threshold=19))
    add("scale15", scene(203, 187), dict(scale_factor=1.5, n_levels=4, edge_threshold=19, grid_rows=1, grid_cols=2))
    add("grid8", scene(360, 355), dict(grid_rows=8, grid_cols=8, n_levels=1, edge_threshold=19))
    add("grid8_share0", scene(360, 355), dict(grid_rows=8, grid_cols=8, n_levels=1, edge_threshold=19, number_of_features=63))
    add("last_level0", scene(240, 220), dict(scale_factor=2.0, n_levels=3, edge_threshold=19, grid_rows=1, grid_cols=1, number_of_features=1))
    add("pattern15", S.framed(scene(163, 157)), dict(ONE), pattern=S.pattern15())
    add("pattern13", S.framed(scene(163, 157)), dict(ONE))
    add("satellites", S.satellites()[0], dict(ONE, fast_threshold=210))
    fm = dict(n_levels=3, scale_factor=1.5, edge_threshold=19)
    add("fine_mask", scene(240, 200), fm, mask=S.fine_mask(240, 200))
    add("fine_mask200", scene(240, 200), fm, mask=S.fine_mask(240, 200, hi=200))
    add("half_mask3", scene(240, 200), fm, mask=S.half_mask(240, 200))
    add("no_mask3", scene(240, 200), fm)
    return c


CASES = _cases()
PATTERN = S.pattern()
_cache = {}


def pattern_of(case):
    return case["pattern"] if case["pattern"] is not None else PATTERN


def reference(name):
    """-> (the restatement's result, its info) for a case, computed once"""
    if name not in _cache:
        case, info = CASES[name], {}
        _cache[name] = (R.extract(case["img"], pattern_of(case), mask=case["mask"], info=info, **case["cfg"]), info)
    return _cache[name]
