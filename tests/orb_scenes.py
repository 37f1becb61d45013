"""Seeded mono8 images, masks and the sampling pattern for the ORB tests.  The scenes are random rectangles under a small box blur:
rectangle corners are what FAST finds, the blur gives them a spread of scores.  Beside them, constructed scenes whose scores, angles
and mask levels are known in advance (dots, satellites, framed, fine_mask).  The pattern is drawn from a seeded generator - the
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


def pattern15(seed=11):
    """512 points (x, y) int8 over the whole admitted range [-15, 15]; the first eight are its corners and axis ends, which a
    rotation by 45 degrees carries 21 pixels from the keypoint: past an edge of 19"""
    p = np.random.default_rng(seed).integers(-15, 16, size=(512, 2)).astype(np.int8)
    p[:8] = [(15, 15), (15, -15), (-15, 15), (-15, -15), (15, 0), (-15, 0), (0, 15), (0, -15)]
    return p


def framed(img, seed=13, width=4):
    """the image with its outer `width` pixels replaced by noise over the whole grey range.  With an edge of 19 no FAST circle and no
    orientation patch (radius 15) reaches a frame of 4, so keypoints and angles are the plain image's; a descriptor read that leaves
    the image by 1 to 3 pixels comes back, reflected, to frame pixel 1 to 3 - where a clamp would read pixel 0, an unrelated value"""
    rng = np.random.default_rng(seed)
    out = img.copy()
    noise = rng.integers(0, 256, img.shape).astype(np.uint8)
    inner = np.zeros(img.shape, bool)
    inner[width:img.shape[0] - width, width:img.shape[1] - width] = True
    out[~inner] = noise[~inner]
    return out


DOT_PITCH, DOT_FIRST = 9, 4


def dots(w, h):
    """single pixels on a 9-pixel lattice on black, alternately 255 and 254 like a chess board: no circle of radius 3 holds two of
    them, so the first kind scores exactly 254 (0 < 255 - t up to t = 254), the second 253, and nothing else scores at all.
    255 - dots(w, h) gives the same scores from the darker side."""
    img = np.zeros((h, w), np.uint8)
    for j, y in enumerate(range(DOT_FIRST, h, DOT_PITCH)):
        for i, x in enumerate(range(DOT_FIRST, w, DOT_PITCH)):
            img[y, x] = 255 if (i + j) % 2 == 0 else 254
    return img


SATELLITE_PITCH, SATELLITE_FIRST = 48, 30
SATELLITE_OFFSETS = [None, (10, 0), (-10, 0), (0, 10), (0, -10), (7, 7), (-7, 7), (-7, -7), (7, -7), (12, 5)]     # (dx, dy)


def satellites():
    """-> (image, [(x, y, offset)]): isolated 255 pixels on a 48-pixel lattice on black, each with at most one 3 x 3 block of
    value 200 centred at a fixed offset inside its own orientation patch (radius 15) and outside every other dot's.  The block is the
    patch's only other mass, so the moments are m10 = 1800 dx, m01 = 1800 dy: on an axis one of them is exactly 0, on a diagonal they
    are equal, without a block both are 0.  The block's own pixels score below 200 and tie with one another."""
    cols, rows = 4, 3
    w, h = 2 * SATELLITE_FIRST + (cols - 1) * SATELLITE_PITCH, 2 * SATELLITE_FIRST + (rows - 1) * SATELLITE_PITCH
    img = np.zeros((h, w), np.uint8)
    where = []
    for k, off in enumerate(SATELLITE_OFFSETS):
        x, y = SATELLITE_FIRST + k % cols * SATELLITE_PITCH, SATELLITE_FIRST + k // cols * SATELLITE_PITCH
        img[y, x] = 255
        if off is not None:
            img[y + off[1] - 1:y + off[1] + 2, x + off[0] - 1:x + off[0] + 2] = 200
        where.append((x, y, off))
    return img, where


def fine_mask(w, h, hi=1):
    """values in {0, hi}: hi on the near side of half_mask's slanted line, a chess board of 3 x 3 fields of 0 and hi on the far
    side.  The fields are finer than a pyramid step can follow, so a resized level holds zeros and non-zeros where no
    nearest-neighbour rule puts them, and with hi > 1 values in between.  hi = 1 is the smallest value that is not 0."""
    y, x = np.mgrid[0:h, 0:w]
    board = np.where((x // 3 + y // 3) % 2 == 0, hi, 0)
    return np.where(3 * (x - w // 2) + (y - h // 2) < 0, hi, board).astype(np.uint8)
