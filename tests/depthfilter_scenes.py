"""Seeded scenes for the depth-filter tests and tests/diag/depthfilter_timing.py: the laser-line tests' room for depth, and synthetic
grey images to guide the filter with."""
import numpy as np

import laserline_scenes as LS


def guide(width=640, height=480, seed=0, kind="blocks"):
    """mono8 guide image.  blocks: a ramp, rectangles of other grey levels and +-3 of noise (edges and smooth parts);
    noise: uniform 0..255; flat: one grey level; extremes: 0 and 255 side by side in a checkerboard"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "flat":
        return np.full((height, width), 128, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (height, width)).astype(np.uint8)
    if kind == "extremes":
        y, x = np.mgrid[:height, :width]
        return (((x + y) % 2) * 255).astype(np.uint8)
    assert kind == "blocks"
    y, x = np.mgrid[:height, :width]
    g = 60.0 + 100.0 * x / max(width - 1, 1) + 30.0 * y / max(height - 1, 1)
    for _ in range(6):
        x0, y0 = int(rng.integers(0, max(width, 1))), int(rng.integers(0, max(height, 1)))
        g[y0:y0 + max(height // 3, 1), x0:x0 + max(width // 4, 1)] = float(rng.integers(0, 256))
    g += rng.integers(-3, 4, (height, width))
    return np.clip(np.round(g), 0, 255).astype(np.uint8)


def depth(width=640, height=480, seed=0, u16=False, nans=0.01, **room):
    """the laser-line tests' room; of its NaN holes (f32) only the share `nans` stays NaN, the others become 0: the filter
    erases the 7 x 7 square around every NaN, and one hole in twenty as NaN would leave little else"""
    d = LS.room(width, height, seed=seed, u16=u16, **room)
    if not u16:
        rng = np.random.default_rng(2000 + seed)
        d[np.isnan(d) & (rng.random(d.shape) >= nans)] = 0.0
    return d


def scene(width=640, height=480, seed=0, u16=False, kind="blocks", T=None, group=None, **room):
    """-> (the image dict Laserline.pack_images takes, its guide)"""
    return LS.image(depth(width, height, seed, u16, **room), T, group=group), guide(width, height, seed, kind)
