"""NumPy restatement of the ORB contract in include/uzl_mi355x.h ("ORB keypoints, descriptors and binary GIST from grey images"),
written from that text alone, step by step, every cast explicit.  f32 values are numpy.float32 throughout (numpy rounds every
operation on its own, so nothing is fused); integers are int64 where the contract's int32 cannot overflow.  The FAST score is found
by the definition - t = 0, 1, 2, ... is tried for every pixel until it stops being a corner - and shares no shortcut with the
kernel's arc minima.  Nothing here is fast; the tests compute each expected result once."""
import math

import numpy as np

F32 = np.float32
F64 = np.float64

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3)]                                            # step 4: (dx, dy)
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]      # step 7
BLUR_K = [18, 34, 49, 55, 49, 34, 18]                                    # step 10
DEFAULTS = dict(number_of_features=300, grid_rows=2, grid_cols=2, n_levels=2, scale_factor=1.2, edge_threshold=31, fast_threshold=5)


def rnd(x):
    """cvRound: the f32 value widened to f64, rounded half to even"""
    return np.rint(np.asarray(x, F32).astype(F64)).astype(np.int64)


def reflect101(p, n):
    p = np.array(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def level_scale(scale_factor, l):
    return F32(math.pow(float(F32(scale_factor)), float(l)))


def level_size(w, h, scale_factor, l):
    if l == 0:
        return int(w), int(h)
    s = F32(1.0) / level_scale(scale_factor, l)
    return int(rnd(F32(w) * s)), int(rnd(F32(h) * s))


# ---------------------------------------------------------------------------------------------- step 3
def resize_taps(dn, sn):
    d = np.arange(dn, dtype=F64)
    scale = F64(1.0) / (F64(dn) / F64(sn))
    f = ((d + F64(0.5)) * scale - F64(0.5)).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    lo = s < 0
    s[lo] = 0; f[lo] = F32(0)
    hi = s >= sn - 1
    s[hi] = sn - 1; f[hi] = F32(0)
    s1 = np.minimum(s + 1, sn - 1)
    w0 = np.clip(rnd((F32(1) - f) * F32(2048)), -32768, 32767)
    w1 = np.clip(rnd(f * F32(2048)), -32768, 32767)
    return s, s1, w0, w1


def resize(src, dw, dh):
    sh, sw = src.shape
    if dw == 0 or dh == 0:
        return np.zeros((dh, dw), np.uint8)
    x0, x1, a0, a1 = resize_taps(dw, sw)
    y0, y1, b0, b1 = resize_taps(dh, sh)
    S = src.astype(np.int64)
    h = S[:, x0] * a0[None, :] + S[:, x1] * a1[None, :]
    h0, h1 = h[y0, :], h[y1, :]
    d = (((b0[:, None] * (h0 >> 4)) >> 16) + ((b1[:, None] * (h1 >> 4)) >> 16) + 2) >> 2
    return np.clip(d, 0, 255).astype(np.uint8)


def pyramid(img, n_levels, scale_factor):
    """step 2: level l from level l - 1, its size from level 0's"""
    h, w = img.shape
    out = [img]
    for l in range(1, n_levels):
        lw, lh = level_size(w, h, scale_factor, l)
        out.append(resize(out[-1], lw, lh))
    return out


# ---------------------------------------------------------------------------------------------- step 4
def is_corner(ring, centre, t):
    """ring: (16, N) int, centre: (N) int -> (N) bool: 9 cyclically contiguous ring pixels all > centre + t or all < centre - t"""
    out = np.zeros(centre.shape, bool)
    for b in (ring > centre + t, ring < centre - t):
        run = b.copy()
        for s in range(1, 9):
            run &= np.roll(b, -s, axis=0)
        out |= run.any(axis=0)
    return out


def fast_scores(img):
    """score(p) = the largest t >= 0 at which p is a corner, by trying every t in turn; 0 outside [3, n - 3) and where none"""
    H, W = img.shape
    score = np.zeros((H, W), np.int64)
    if H < 7 or W < 7:
        return score
    I = img.astype(np.int64)
    ys, xs = np.mgrid[3:H - 3, 3:W - 3]
    ys, xs = ys.ravel(), xs.ravel()
    ring = np.stack([I[ys + dy, xs + dx] for dx, dy in CIRCLE])
    centre = I[ys, xs]
    for t in range(0, 256):
        ok = is_corner(ring, centre, t)
        if not ok.any():
            break
        ys, xs, ring, centre = ys[ok], xs[ok], ring[:, ok], centre[ok]
        score[ys, xs] = t                               # a corner at t: the score is at least t
    return score


def fast_keypoints(img, mask, threshold):
    """-> x, y, score of the keypoints of step 4, in no particular order"""
    s = fast_scores(img)
    H, W = s.shape
    p = np.pad(s, 1)
    best = np.zeros_like(s)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                best = np.maximum(best, p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
    keep = (s >= threshold) & (s > best)
    if mask is not None:
        keep &= mask != 0
    y, x = np.nonzero(keep)
    return x, y, s[y, x]


# ---------------------------------------------------------------------------------------------- steps 6, 7
def n_per_level(nfeatures, scale_factor, n_levels):
    factor = F32(1.0 / float(F32(scale_factor)))
    d = F32(nfeatures) * (F32(1) - factor) / (F32(1) - F32(math.pow(float(factor), float(n_levels))))
    out, total = [], 0
    for _ in range(n_levels - 1):
        out.append(int(rnd(d)))
        total += out[-1]
        d = F32(d * factor)
    out.append(max(nfeatures - total, 0))
    return out


def retain_best(response, n):
    """-> bool mask: everything when at most n remain; else every response >= the n-th largest (ties all kept)"""
    response = np.asarray(response)
    if len(response) <= n:
        return np.ones(len(response), bool)
    if n <= 0:
        return np.zeros(len(response), bool)
    c = np.sort(response)[::-1][n - 1]
    return response >= c


def fast_atan2(y, x):
    y, x = F32(y), F32(x)
    scale = F32(180.0 / math.pi)
    p1, p3, p5, p7 = F32(0.9997878412794807) * scale, F32(-0.3258083974640975) * scale, F32(0.1555786518463281) * scale, \
        F32(-0.04432655554792128) * scale
    eps = F32(2.220446049250313e-16)                                     # (float)DBL_EPSILON
    ax, ay = abs(x), abs(y)
    if ax >= ay:
        c = ay / (ax + eps)
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    else:
        c = ax / (ay + eps)
        c2 = c * c
        a = F32(90) - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    if x < 0:
        a = F32(180) - a
    if y < 0:
        a = F32(360) - a
    assert a.dtype == F32
    return a


def ic_angle(img, x, y):
    m01 = m10 = 0
    for dy in range(-15, 16):
        d = UMAX[abs(dy)]
        row = img[y + dy, x - d:x + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * row).sum())
        m01 += dy * int(row.sum())
    return fast_atan2(F32(m01), F32(m10))


# ---------------------------------------------------------------------------------------------- steps 9, 10
def cos_sin(x):
    """f64, arithmetic only: octant reduction and fixed polynomials (the recipe of csrc/orb_types.hpp)"""
    x = float(x)
    k = float(np.rint(x * 0.63661977236758138243))
    r = (x - k * 1.57079632673412561417) - k * 6.07710050650619224932e-11
    z = r * r
    sp = r + r * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
         z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))))
    cp = 1.0 - 0.5 * z + z * z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
         z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))))
    q = int(k - 4.0 * math.floor(k * 0.25))
    return [(cp, sp), (-sp, cp), (-cp, -sp), (sp, -cp)][q]


def blur(img):
    H, W = img.shape
    if H == 0 or W == 0:
        return img.copy()
    I = img.astype(np.int64)
    K = np.array(BLUR_K, np.int64)
    cols = reflect101(np.arange(-3, W + 3), W)
    rows = reflect101(np.arange(-3, H + 3), H)
    P = I[rows][:, cols]
    hs = sum(K[k] * P[:, k:k + W] for k in range(7))
    vs = sum(K[k] * hs[k:k + H, :] for k in range(7))
    return np.minimum((vs + 32768) >> 16, 255).astype(np.uint8)


def pattern_reads(cx, cy, angle, pattern):
    """step 9: the row and the column at which each of the 512 pattern points is read from level position (cx, cy)"""
    rad = F32(angle) * F32(math.pi / 180.0)
    c, s = cos_sin(float(rad))
    a, b = F32(c), F32(s)
    P = np.asarray(pattern, np.int8).reshape(512, 2)
    px, py = P[:, 0].astype(F32), P[:, 1].astype(F32)
    return cy + rnd(px * b + py * a), cx + rnd(px * a - py * b)


def reads_outside(shape, cx, cy, angle, pattern):
    """how many of a descriptor's 512 reads fall outside its level image (and so take the unblurred, reflected branch of step 9)"""
    H, W = shape
    row, col = pattern_reads(cx, cy, angle, pattern)
    return int(((row < 0) | (row >= H) | (col < 0) | (col >= W)).sum())


def describe(blurred, raw, cx, cy, angle, pattern):
    """one descriptor at level position (cx, cy): 32 bytes"""
    H, W = raw.shape
    row, col = pattern_reads(cx, cy, angle, pattern)
    inside = (row >= 0) & (row < H) & (col >= 0) & (col < W)
    val = np.where(inside, blurred[np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)], raw[reflect101(row, H), reflect101(col, W)]).astype(np.int64)
    bits = (val[0::2] < val[1::2]).astype(np.uint8)                      # bit k of the descriptor: points 2k, 2k + 1
    return np.packbits(bits.reshape(32, 8), axis=1, bitorder="little").reshape(32)


# ---------------------------------------------------------------------------------------------- the whole
def cut(response, n):
    """steps 6 and 8 as a number: the smallest response a cut to n keeps - the n-th largest when more than n remain, 256 (above every
    response) when n is 0 and something remains, 0 (below every response) when nothing is cut"""
    response = np.asarray(response)
    if len(response) <= n:
        return 0
    if n <= 0:
        return 256
    return int(np.sort(response)[::-1][n - 1])


def detect_cell(cell, mask, cfg, info=None):
    """steps 2-8 for one cell -> list of (u, v, response, angle, octave) in cell coordinates (f32), after the cell's cut.  With info,
    info["stages"] gets one dict for the cell: levels and masks (the pyramids of step 2), candidates (per level x, y, score after
    steps 4-5) and cut (per level the smallest response steps 6 and 8 keep: the larger of the level's cut and the cell's)"""
    L, sf, edge = cfg["n_levels"], cfg["scale_factor"], cfg["edge_threshold"]
    n_l = n_per_level(2 * cfg["number_of_features"], sf, L)
    levels = pyramid(cell, L, sf)
    masks = pyramid(mask, L, sf) if mask is not None else [None] * L
    found = []
    stage = dict(levels=levels, masks=masks, candidates=[], cut=[])
    for l in range(L):
        img = levels[l]
        h, w = img.shape
        x, y, s = fast_keypoints(img, masks[l], cfg["fast_threshold"])
        if w <= 2 * edge or h <= 2 * edge:
            keep = np.zeros(len(x), bool)
        else:
            keep = (x >= edge) & (x < w - edge) & (y >= edge) & (y < h - edge)
        x, y, s = x[keep], y[keep], s[keep]
        if info is not None:
            info.setdefault("level_candidates", []).append((l, len(x), n_l[l]))
        stage["candidates"].append((x.astype(np.int64), y.astype(np.int64), s.astype(np.int64)))
        stage["cut"].append(cut(s, n_l[l]))
        keep = retain_best(s, n_l[l])
        scale = level_scale(sf, l)
        for xx, yy, ss in zip(x[keep], y[keep], s[keep]):
            u, v = F32(xx), F32(yy)
            if l > 0:
                u, v = u * scale, v * scale
            found.append((u, v, F32(ss), ic_angle(img, int(xx), int(yy)), l))
    n_cell = cfg["number_of_features"] // (cfg["grid_rows"] * cfg["grid_cols"])
    if info is not None:
        info.setdefault("cell_candidates", []).append((len(found), n_cell))
        cell_cut = cut([f[2] for f in found], n_cell)
        stage["cut"] = [max(c, cell_cut) for c in stage["cut"]]
        info.setdefault("stages", []).append(stage)
    keep = retain_best([f[2] for f in found], n_cell)
    return [f for f, k in zip(found, keep) if k]


def extract(img, pattern, mask=None, **cfg):
    """steps 1-10 for one image -> dict(u, v, response, angle: f32; octave: i32; desc: u8 (n, 32)) in the contract's order.  A dict
    passed as info=... comes back with the stages: per cell, row by row, what detect_cell reports; pyramid and blurred, the levels of
    the whole image of steps 9-10; outside, per keypoint the number of pattern points its descriptor read outside its level image"""
    cfg = dict(DEFAULTS, **cfg)
    info = cfg.pop("info", None)
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    gr, gc, edge = cfg["grid_rows"], cfg["grid_cols"], cfg["edge_threshold"]
    kps = []
    if H and W:
        for i in range(gr):
            for j in range(gc):
                y0, y1, x0, x1 = i * H // gr, (i + 1) * H // gr, j * W // gc, (j + 1) * W // gc
                cell_mask = mask[y0:y1, x0:x1] if mask is not None else None
                for u, v, r, a, o in detect_cell(img[y0:y1, x0:x1], cell_mask, cfg, info):
                    kps.append((o, -float(r), float(v + F32(y0)), float(u + F32(x0)), u + F32(x0), v + F32(y0), r, a))
    kps = [k for k in kps if edge <= int(rnd(k[4])) < W - edge and edge <= int(rnd(k[5])) < H - edge]
    kps.sort(key=lambda k: k[:4])
    n = len(kps)
    out = dict(u=np.array([k[4] for k in kps], F32), v=np.array([k[5] for k in kps], F32), response=np.array([k[6] for k in kps], F32),
               angle=np.array([k[7] for k in kps], F32), octave=np.array([k[0] for k in kps], np.int32), desc=np.zeros((n, 32), np.uint8))
    if n or (info is not None and H and W):
        raw = pyramid(img, cfg["n_levels"], cfg["scale_factor"])
        blurred = [blur(r) for r in raw]
        if info is not None:
            info.update(pyramid=raw, blurred=blurred, outside=[])
        for i, k in enumerate(kps):
            o = k[0]
            s = F32(1.0) / level_scale(cfg["scale_factor"], o)
            cx, cy = int(rnd(k[4] * s)), int(rnd(k[5] * s))
            out["desc"][i] = describe(blurred[o], raw[o], cx, cy, k[7], pattern)
            if info is not None:
                info["outside"].append(reads_outside(raw[o].shape, cx, cy, k[7], pattern))
    return out


def gist(img, angle_deg, pattern):
    """step 11 -> 32 bytes"""
    img = np.asarray(img, np.uint8)
    if img.size == 0:
        return np.zeros(32, np.uint8)
    small = resize(img, 63, 63)
    return describe(blur(small), small, 31, 31, F32(angle_deg), pattern)
