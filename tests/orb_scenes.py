"""Seeded mono8 images, masks and the sampling pattern for the ORB tests.  The scenes are random rectangles under a small box blur:
rectangle corners are what FAST finds, the blur gives them a spread of scores.  The pattern is drawn from a seeded generator - the
library ships none and the reference's table is program text that stays out of this repository."""
import numpy as np


def pattern(seed=7):
    """512 points (x, y) int8, every coordinate in [-13, 13]"""
    return np.random.default_rng(seed).integers(-13, 14, size=(512, 2)).astype(np.int8)


def box3(img):
    """3 x 3 box mean, edges replicated, integer"""
    p = np.pad(img.astype(np.int64), 1, mode="edge")
    h, w = img.shape
    s = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
    return ((s + 4) // 9).astype(np.uint8)


def rectangles(w, h, seed, n=None, blurred=True):
    """n random rectangles (default: one per 150 pixels) of random grey on mid grey"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 110, np.uint8)
    if w == 0 or h == 0:
        return img
    for _ in range(n if n is not None else max(w * h // 150, 4)):
        rw, rh = int(rng.integers(3, 24)), int(rng.integers(3, 24))
        x, y = int(rng.integers(-4, w)), int(rng.integers(-4, h))
        img[max(y, 0):y + rh, max(x, 0):x + rw] = int(rng.integers(0, 256))
    return box3(img) if blurred else img


def squares(w, h, pitch=8, lo=40, mid=150, hi=210):
    """identical 3 x 3 squares with a brighter centre on a regular grid: the centre is a strict 3 x 3 maximum of the FAST score (a
    plain square's pixels tie with their neighbours and none survives the suppression), and every square scores the same"""
    img = np.full((h, w), lo, np.uint8)
    for y in range(4, h - 4, pitch):
        for x in range(4, w - 4, pitch):
            img[y - 1:y + 2, x - 1:x + 2] = mid
            img[y, x] = hi
    return img


def saturated(w, h, seed):
    """only 0 and 255"""
    return np.where(rectangles(w, h, seed, blurred=False) > 110, 255, 0).astype(np.uint8)


def half_mask(w, h):
    """zero on the far side of a slanted line through the image centre: the edge crosses the cell borders of a 2 x 2 grid"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where(3 * (x - w // 2) + (y - h // 2) < 0, 255, 0).astype(np.uint8)
